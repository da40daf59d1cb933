// fill_adj.hip — read adjudication of the contested fills: the alternatives round (fill_alt.hip) names, for a closed gap,
// a rival contig of the winner's level whose fill differs from the winner's.  This round places the gap's own pool on both fills, each
// between the same flank context (the LOCUS LC + F + RC), and lets every row vote for the locus it fits strictly better.  Definition and
// host twin: gappadder_amd/fill_adjudication.py::adjudicate_host (equal byte for byte); the ABI: gf_fill_adjudicate_dev,
// include/gapfill_hip.h.
//
// One workgroup of PL_THREADS threads per contested gap, grid-stride over the gaps; an uncontested gap gets its zero record and is left
// at once.  The launch is set up by fill_round_setup and pl_place_setup.  A contested gap runs two phases over ONE staged locus each:
//   fills    both fills located again by the alternatives' rule (fill_alt_dev.hpp: alt_candidate, every wave for itself, all with the
//            same answer) and compared with what the gf_fill_alt record states; a difference is a MISMATCH
//   phase W  the winner's locus staged into fill_place.hpp's LDS layout (adj_stage_locus: pl_stage_contig's loop over an accessor, so
//            that no locus is ever written to memory), pl_build_index, then pl_stage_rows + pl_place_row over the pool a batch at a
//            time; each row's best key and strand bit go to d_place_scratch (4 bytes a row, written and read back by the same thread)
//   phase R  the same for the rival's locus; each row's key is compared with its stored word and the row classified; the seven counters
//            are summed per wave with ballots (wave-uniform registers), once per wave into LDS, and thread 0 writes the record
// Two phases with a word per row keep the static LDS at one locus and one index (47 728 bytes, three workgroups on a CU); both loci at once would take two of each
// (about 84 KB, one workgroup).
// The skip verdicts (LONG before any staging, NON_ACGT behind the barrier of either stage) are the same in all threads, so every barrier
// is reached by the whole workgroup.
#include <cstring>

#include "fill_alt_dev.hpp"
#include "fill_place.hpp"
#include "fill_round.hpp"
#include "gf_internal.hpp"

namespace gf {

static_assert(sizeof(gf_fill_adj) == 48, "gf_fill_adj");
constexpr uint32_t AJ_WGS_PER_CU = 3;       // workgroups the static LDS lets a CU hold
constexpr uint32_t AJ_NONE = EMPTY32;        // the scratch word of a row without an accepted pair; else key << 1 | strand

struct AdjParams {
    PlPlaceArgs place;
    FillRoundArgs round;
    // what alt_candidate reads (fill_alt_dev.hpp)
    ContigList list;
    const uint8_t *anc_s, *anc_l;
    uint32_t n_gaps, a_s, a_l;
    const gf_fill_alt* alt;
    const uint8_t* flank_text;       // [n_gaps][2][C]
    const uint16_t* flank_len;       // [n_gaps][2]
    uint32_t* scratch;
    uint32_t C, min_votes, ratio;
    gf_fill_adj* out;
};

// a locus: byte x of LC + F + RC
struct AdjLocus {
    const uint8_t *lc, *rc;
    uint32_t n_l, n_r;
    AltFill F;
    __device__ __forceinline__ uint32_t size() const { return n_l + F.len + n_r; }
    __device__ __forceinline__ uint8_t at(uint32_t x) const {
        return x < n_l ? lc[x] : x < n_l + F.len ? F.at(x - n_l) : rc[x - n_l - F.len];
    }
};

// pl_stage_contig over the locus' accessor: word w of either array holds the bases 16 w - PL_LEAD .. + 15 of the locus / of its reverse
// complement; the index is cleared.  Returns nonzero in a thread that met a byte other than A, C, G, T.  The caller's barrier ends it
__device__ __forceinline__ uint32_t adj_stage_locus(const AdjLocus& T, uint32_t n, uint32_t* s_fwd, uint32_t* s_rc, uint32_t* s_idx) {
    const uint32_t t = threadIdx.x;
    uint32_t bad = 0;
    for (uint32_t w = t; w < PL_CTG_WORDS; w += PL_THREADS) {
        uint32_t vf = 0, vr = 0;
        const int32_t x0 = (int32_t)(16 * w) - (int32_t)PL_LEAD;
        if (x0 + 16 > 0 && x0 < (int32_t)n) {
            for (int32_t b = 0; b < 16; ++b) {
                const int32_t x = x0 + b;
                if (x < 0 || x >= (int32_t)n) continue;
                const uint32_t cf = base_code4(T.at((uint32_t)x)), cr = base_code4(T.at(n - 1 - (uint32_t)x));
                bad |= cf >> 2;
                vf |= (cf & 3u) << (30 - 2 * b);
                vr |= (3u - (cr & 3u)) << (30 - 2 * b);
            }
        }
        s_fwd[w] = bswap32(vf);
        s_rc[w] = bswap32(vr);
    }
    for (uint32_t i = t; i < PL_SLOTS / 2; i += PL_THREADS) s_idx[i] = 0;
    return bad;
}

__global__ __launch_bounds__(PL_THREADS) void fill_adj_kernel(AdjParams P) {
    __shared__ uint32_t s_idx[PL_SLOTS / 2];
    __shared__ uint32_t s_fwd[PL_CTG_WORDS];
    __shared__ uint32_t s_rc[PL_CTG_WORDS];
    __shared__ uint32_t s_rows[PL_ROW_WORDS];
    __shared__ uint32_t s_acc[8];                // votes_w, votes_r, votes_w_s0, votes_r_s0, ties, unplaced, only; a byte that is no base
    const uint32_t t = threadIdx.x, lane = t & 63;
    const uint32_t n_list = contig_list_end(P.list);
    for (uint32_t g = blockIdx.x; g < P.n_gaps; g += gridDim.x) {
        gf_fill_adj rec;
        memset(&rec, 0, sizeof(rec));
        const gf_fill_alt a = P.alt[g];
        if (!(a.flags & GF_FA_F_HAS_RIVAL) || (a.flags & GF_FA_F_LOST)) {
            if (t == 0) P.out[g] = rec;
            continue;
        }
        // ---- both fills again (every wave scans for itself: the same answer in all of them)
        const unsigned long long word = P.round.gap_best[g];
        bool ok = word != 0 && pick_word_unpack(word).contig == a.contig && a.contig < n_list && a.rival < n_list;
        gf_contig cw, cr;
        AltCand kw, kr;
        if (ok) {
            cw = P.list.contigs[a.contig];
            cr = P.list.contigs[a.rival];
            ok = cw.gap == g && cr.gap == g;
        }
        ok = ok && alt_candidate(P, cw, lane, &kw) && kw.strand == ((a.flags & GF_FA_F_REVERSE) ? 1u : 0u) && kw.span == a.fill_len;
        ok = ok && alt_candidate(P, cr, lane, &kr) && kr.strand == ((a.flags & GF_FA_F_RIVAL_REVERSE) ? 1u : 0u) && kr.span == a.rival_len;
        if (!ok) {
            if (t == 0) {
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_AJ_SEEN, 1u);
                atomicAdd(P.round.stats + GF_AJ_MISMATCH, 1u);
            }
            continue;
        }
        AdjLocus T;
        T.lc = P.flank_text + (uint64_t)g * 2 * P.C;
        T.rc = T.lc + P.C;
        T.n_l = P.flank_len[2 * g] < P.C ? P.flank_len[2 * g] : P.C;
        T.n_r = P.flank_len[2 * g + 1] < P.C ? P.flank_len[2 * g + 1] : P.C;
        T.F = {P.list.seq + cw.seq_off, kw.start, kw.span, kw.strand};
        const AltFill Fr = {P.list.seq + cr.seq_off, kr.start, kr.span, kr.strand};
        const uint32_t nw = T.size(), nr = T.n_l + Fr.len + T.n_r;
        const FillRows rows = fill_gap_rows(P.round, g);
        rec.contig = a.contig;
        rec.rival = a.rival;
        rec.locus_w = nw;
        rec.locus_r = nr;
        rec.flags = (uint8_t)((a.dist == GF_FA_DIST_FAR ? GF_AJ_F_RIVAL_FAR : 0) | (rows.r0 == rows.r1 ? GF_AJ_F_NO_ROWS : 0));
        if (nw > PL_MAX || nr > PL_MAX) {        // (nothing staged; the same in all threads)
            if (t == 0) {
                rec.flags |= GF_AJ_F_LONG;
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_AJ_SEEN, 1u);
                atomicAdd(P.round.stats + GF_AJ_SKIPPED_LONG, 1u);
            }
            continue;
        }
        __syncthreads();                         // (the previous gap's record is written from s_acc, its last rows are placed)
        if (t < 8) s_acc[t] = 0;
        __syncthreads();
        uint32_t v_w = 0, v_r = 0, v_w0 = 0, v_r0 = 0, v_tie = 0, v_un = 0, v_only = 0;   // of this wave (uniform over its lanes)
        bool skipped = false;
        for (uint32_t phase = 0; phase < 2; ++phase) {
            if (phase) T.F = Fr;
            const uint32_t n = phase ? nr : nw;
            // ---- stage, or skip
            if (adj_stage_locus(T, n, s_fwd, s_rc, s_idx)) atomicOr(&s_acc[7], 1u);
            __syncthreads();
            if (s_acc[7]) {                      // (the same in all threads)
                skipped = true;
                break;
            }
            // ---- index
            pl_build_index(s_fwd, s_idx, n, P.place.s);
            __syncthreads();
            // ---- place; phase R: classify
            for (uint64_t row0 = rows.r0; row0 < rows.r1; row0 += P.place.batch_rows) {
                const uint32_t nb = rows.r1 - row0 < P.place.batch_rows ? (uint32_t)(rows.r1 - row0) : P.place.batch_rows;
                const uint32_t mis = pl_stage_rows(P.place, row0, nb, s_rows);
                uint32_t here = AJ_NONE, there = AJ_NONE;
                if (t < nb) {
                    const uint32_t* nm = P.place.nmask ? P.place.nmask + (row0 + t) * P.place.nmw : nullptr;
                    const PlPlacement pm = pl_place_row(P.place, s_rows, (mis + t * P.place.rb) * 8, nm, s_fwd, s_rc, s_idx, n);
                    here = pm.cnt ? (pm.key << 1) | pm.strand : AJ_NONE;
                    if (phase) there = P.scratch[row0 + t];
                    else P.scratch[row0 + t] = here;
                }
                if (phase) {                     // here: on the rival's locus; there: on the winner's
                    const bool live = t < nb;
                    const uint32_t key_r = here >> 1, key_w = there >> 1;      // (AJ_NONE >> 1 is above every key)
                    const bool for_w = live && key_w < key_r, for_r = live && key_r < key_w;
                    v_w += (uint32_t)__popcll(__ballot(for_w));
                    v_r += (uint32_t)__popcll(__ballot(for_r));
                    v_w0 += (uint32_t)__popcll(__ballot(for_w && !(there & 1u)));
                    v_r0 += (uint32_t)__popcll(__ballot(for_r && !(here & 1u)));
                    v_tie += (uint32_t)__popcll(__ballot(live && key_w == key_r && here != AJ_NONE));
                    v_un += (uint32_t)__popcll(__ballot(live && here == AJ_NONE && there == AJ_NONE));
                    v_only += (uint32_t)__popcll(__ballot((for_w && here == AJ_NONE) || (for_r && there == AJ_NONE)));
                }
                __syncthreads();                 // (the rows are read: the next batch, the next stage or the next gap overwrites them)
            }
        }
        if (skipped) {
            if (t == 0) {
                rec.flags |= GF_AJ_F_NON_ACGT;
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_AJ_SEEN, 1u);
                atomicAdd(P.round.stats + GF_AJ_SKIPPED_NON_ACGT, 1u);
            }
            continue;
        }
        if (lane == 0) {
            if (v_w) atomicAdd(&s_acc[0], v_w);
            if (v_r) atomicAdd(&s_acc[1], v_r);
            if (v_w0) atomicAdd(&s_acc[2], v_w0);
            if (v_r0) atomicAdd(&s_acc[3], v_r0);
            if (v_tie) atomicAdd(&s_acc[4], v_tie);
            if (v_un) atomicAdd(&s_acc[5], v_un);
            if (v_only) atomicAdd(&s_acc[6], v_only);
        }
        __syncthreads();
        if (t == 0) {
            const uint64_t vw = s_acc[0], vr = s_acc[1];
            rec.votes_w = s_acc[0];
            rec.votes_r = s_acc[1];
            rec.votes_w_s0 = s_acc[2];
            rec.votes_r_s0 = s_acc[3];
            rec.ties = s_acc[4];
            rec.unplaced = s_acc[5];
            rec.only = s_acc[6];
            rec.verdict = (uint8_t)(vw >= P.min_votes && vw >= P.ratio * vr   ? GF_AJ_KEEP
                                    : vr >= P.min_votes && vr >= P.ratio * vw ? GF_AJ_SWITCH
                                                                              : GF_AJ_UNDECIDED);
            P.out[g] = rec;
            atomicAdd(P.round.stats + GF_AJ_SEEN, 1u);
            atomicAdd(P.round.stats + GF_AJ_ADJUDICATED, 1u);
            atomicAdd(P.round.stats + (rec.verdict == GF_AJ_KEEP ? GF_AJ_N_KEEP : rec.verdict == GF_AJ_SWITCH ? GF_AJ_N_SWITCH : GF_AJ_N_UNDECIDED), 1u);
            atomicAdd((unsigned long long*)(P.round.stats + GF_AJ_VOTES_W), (unsigned long long)vw);
            atomicAdd((unsigned long long*)(P.round.stats + GF_AJ_VOTES_R), (unsigned long long)vr);
            atomicAdd((unsigned long long*)(P.round.stats + GF_AJ_TIES), (unsigned long long)s_acc[4]);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_adjudicate_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                                      int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                      const void* d_gap_best, int anchor_long, int anchor_short, const void* d_alt, const void* d_flank_text,
                                      const void* d_flank_len, void* d_place_scratch, int seed, int max_mismatch, int min_overlap, int context,
                                      int min_votes, int ratio, void* d_adj, void* d_stats) {
    AdjParams P;
    memset(&P, 0, sizeof(P));
    int own = pl_place_setup(d_pool_packed, d_nmask_or_null, read_len, seed, max_mismatch, min_overlap, &P.place);
    // (a missing argument first, then the placement rule, then the round's own three)
    if (!d_alt || !d_flank_text || !d_flank_len || (pool_rows && !d_place_scratch)) own = GF_E_INVAL;
    else if (own == GF_OK && (context < min_overlap || context > GF_AJ_MAX_CONTEXT || min_votes < 1 || ratio < 2 || ratio > GF_AJ_MAX_RATIO))
        own = GF_E_INVAL;
    const FillRoundIn in = {d_pool_packed, d_pool_off, pool_rows, read_len, d_contigs, d_n_contigs, contig_cap, d_seq, d_gap_best, nullptr,
                            anchor_long, anchor_short, d_adj, d_stats};
    size_t blocks;
    const int rc = fill_round_setup(ctx, in, own, GF_AJ_WORDS, AJ_WGS_PER_CU, &P.round, &blocks);
    if (rc || !blocks) return rc;
    P.list = P.round.body.list;
    P.anc_s = anchor_short ? P.round.body.anc_s : P.round.body.anc_l;   // (alt_candidate: the short or only length, the long one or null)
    P.anc_l = anchor_short ? P.round.body.anc_l : nullptr;
    P.a_s = (uint32_t)(anchor_short ? anchor_short : anchor_long);
    P.a_l = (uint32_t)anchor_long;
    P.n_gaps = P.round.n_gaps;
    P.alt = (const gf_fill_alt*)d_alt;
    P.flank_text = (const uint8_t*)d_flank_text;
    P.flank_len = (const uint16_t*)d_flank_len;
    P.scratch = (uint32_t*)d_place_scratch;
    P.C = (uint32_t)context;
    P.min_votes = (uint32_t)min_votes;
    P.ratio = (uint32_t)ratio;
    P.out = (gf_fill_adj*)d_adj;
    LaunchTimer tm(ctx, GF_KERNEL_ADJ);
    hipLaunchKernelGGL(fill_adj_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
