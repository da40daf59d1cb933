// fill_pileup.hip — per-base pile-up of the closed gaps: the reads of a gap's own pool are placed without gaps on the gap's winning contig
// (the polish's rule), every column of the CONTIG takes their votes per base and read strand, the eight counters of every column go to a
// track, and one record per gap sums up the weak columns of the fill (gf_fill_pileup_dev, include/gapfill_hip.h; definition and host
// twin: gappadder_amd/pileup.py).  The reference has no such stage.
//
// One workgroup of 256 threads per closed gap, grid-stride over the gaps.  A gap is opened by fill_round.hpp (open / mismatch / ok, the
// body [b0, b1) of fill_body.hpp, the gap's pool rows); the launch is set up by fill_round_setup and pl_place_setup.  Per gap:
//   stage, index   fill_place.hpp (pl_stage_or_skip: a long or non-ACGT contig gets its flag and n_cols, no track)
//   place    the pool's rows a batch at a time, one row per thread, ONCE: a row's result — status, strand, diagonal on the contig as
//            stored + PS_BIAS (fill_pair_word.hpp) — goes to one u32 of the context's scratch array (global memory: a pool has no row
//            bound); written and read by the same workgroup, so workgroup scope is enough
//   vote     PU_VCHUNK contig columns per pass, eight u32 counters a column (fill_vote.hpp; LDS atomics).  The index is dead by then: the
//            counters take its LDS.  A pass reads the rows' words, and the packed bases of the rows that reach its columns, from global
//   emit     per column, from the finished counters: the track entry (eight u16, saturated; ONE 16-byte vector store), and for a body
//            column its classes — integer comparisons, independent of the order of the atomics.  A wave's low flags go to LDS as one
//            64-bit ballot; thread 0 walks the pass's 16 ballot words in ascending column order and carries (run length, its start)
//            into the next pass, so a run across a pass boundary is one run and the smallest column wins a tie
// Everything written to global memory is a plain C++ store or an atomicAdd of a vector lane.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md §23; no scratch, static LDS below 49 KB.
#include <cstring>

#include "fill_body.hpp"
#include "fill_pair_word.hpp"
#include "fill_place.hpp"
#include "fill_round.hpp"
#include "fill_vote.hpp"
#include "gf_internal.hpp"

namespace gf {

#ifdef GF_PU_REPLACE
// The comparison build of DESIGN.md §23 (make EXTRA_CXXFLAGS=-DGF_PU_REPLACE), not the library's: no placement words — every vote pass
// places the pool again, as fill_polish.hip does —, so the index lives through the passes and the counters get 16 KB of their own
constexpr bool PU_REPLACE = true;
constexpr uint32_t PU_VCHUNK = 512, PU_WGS_PER_CU = 2;
#else
constexpr bool PU_REPLACE = false;
constexpr uint32_t PU_VCHUNK = 1024, PU_WGS_PER_CU = 3;                      // columns of a vote pass: 8 counters each = the index's LDS
static_assert(PU_VCHUNK * 8 == PL_SLOTS / 2, "pile-up geometry");
#endif
static_assert(PU_VCHUNK % PL_THREADS == 0 && PL_THREADS % 64 == 0, "pile-up geometry");
enum { PU_A_BAD, PU_A_PLACED, PU_A_AMBIGUOUS, PU_A_UNCOVERED, PU_A_THIN, PU_A_CONTESTED, PU_A_MINORITY, PU_A_ONE_STRAND, PU_A_N };

struct PuParams {
    PlPlaceArgs place;
    FillRoundArgs round;
    uint32_t min_depth, min_agree;
    uint32_t* scratch;           // a placement word per pool row
    gf_fill_pileup* out;
    uint4* track;                // or null: records only
    uint64_t track_cap;
};

__global__ __launch_bounds__(PL_THREADS) void fill_pileup_kernel(PuParams P) {
    __shared__ uint32_t s_idx[PL_SLOTS / 2];
    __shared__ uint32_t s_fwd[PL_CTG_WORDS];
    __shared__ uint32_t s_rc[PL_CTG_WORDS];
    __shared__ uint32_t s_rows[PL_ROW_WORDS];
    __shared__ unsigned long long s_low[PU_VCHUNK / 64];
    __shared__ uint32_t s_loc[2];
    __shared__ uint32_t s_acc[PU_A_N];
    __shared__ unsigned long long s_off, s_sum, s_min;
#ifdef GF_PU_REPLACE
    __shared__ uint32_t s_votes[PU_VCHUNK * 8];
#else
    uint32_t* s_votes = s_idx;
#endif
    const uint32_t t = threadIdx.x, L = P.place.L;
    const uint32_t n_list = contig_list_end(P.round.body.list);
    for (uint32_t g = blockIdx.x; g < P.round.n_gaps; g += gridDim.x) {
        gf_fill_pileup rec;
        memset(&rec, 0, sizeof(rec));
        const FillGap fg = fill_gap_open<PL_THREADS>(P.round, n_list, g, s_loc);        // (fill_round.hpp; the same in all threads)
        if (fg.state == FILL_GAP_OPEN) {
            if (t == 0) P.out[g] = rec;
            continue;
        }
        if (fg.state == FILL_GAP_MISMATCH) {
            if (t == 0) {
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_PU_MISMATCH, 1u);
            }
            continue;
        }
        const uint32_t n = fg.fb.c.length;
        const char* ctg = P.round.body.list.seq + fg.fb.c.seq_off;
        const uint32_t b0 = (uint32_t)fg.fb.b0, b1 = (uint32_t)fg.fb.b1, n_cols = b1 - b0;
        if (t < PU_A_N) s_acc[t] = 0;
        if (t == 0) {
            s_sum = 0;
            s_min = ~0ull;
        }
        __syncthreads();
        // ---- stage, or skip (fill_place.hpp)
        const uint32_t skip = pl_stage_or_skip(ctg, n, s_fwd, s_rc, s_idx, &s_acc[PU_A_BAD], GF_PU_F_LONG, GF_PU_F_NON_ACGT);
        if (skip) {
            if (t == 0) {
                rec.flags = skip;
                rec.n_cols = n_cols;
                P.out[g] = rec;
                atomicAdd(P.round.stats + (skip == GF_PU_F_LONG ? GF_PU_SKIPPED_LONG : GF_PU_SKIPPED_NON_ACGT), 1u);
            }
            continue;
        }
        if (t == 0 && P.track) s_off = atomicAdd((unsigned long long*)(P.round.stats + GF_PU_ENTRIES), (unsigned long long)n);
        // ---- index
        pl_build_index(s_fwd, s_idx, n, P.place.s);
        const FillRows rows = fill_gap_rows(P.round, g);
        const uint64_t r0 = rows.r0, r1 = rows.r1;
        __syncthreads();
        // ---- place: one pass over the pool, a word per row
        if constexpr (!PU_REPLACE) {
            uint32_t placed = 0, ambiguous = 0;
            for (uint64_t row0 = r0; row0 < r1; row0 += P.place.batch_rows) {
                const uint32_t nb = r1 - row0 < P.place.batch_rows ? (uint32_t)(r1 - row0) : P.place.batch_rows;
                const uint32_t mis = pl_stage_rows(P.place, row0, nb, s_rows);
                if (t < nb) {
                    const uint32_t* nm = P.place.nmask ? P.place.nmask + (row0 + t) * P.place.nmw : nullptr;
                    const PlPlacement pm = pl_place_row(P.place, s_rows, (mis + t * P.place.rb) * 8, nm, s_fwd, s_rc, s_idx, n);
                    // strand 1: the row as stored lies at D on the reverse complement = its reverse complement at n - D - L on the contig
                    const int32_t d = pm.strand ? (int32_t)n - pm.D - (int32_t)L : pm.D;
                    placed += pm.cnt == 1;
                    ambiguous += pm.cnt > 1;
                    P.scratch[row0 + t] = pm.cnt == 0 ? 0u : pm.cnt > 1 ? PS_AMBIGUOUS : PS_PLACED | (pm.strand ? PS_STRAND : 0u) | (uint32_t)(d + (int32_t)PS_BIAS);
                }
                __syncthreads();                 // (the staged rows are read: the next batch replaces them)
            }
            if (placed) atomicAdd(&s_acc[PU_A_PLACED], placed);
            if (ambiguous) atomicAdd(&s_acc[PU_A_AMBIGUOUS], ambiguous);
        }
        __threadfence_block();
        __syncthreads();                         // (every row's word is in the scratch array; the index is dead)
        const uint64_t off = P.track ? s_off : 0;
        const bool fits = P.track && off + n <= P.track_cap;
        uint4* outp = P.track + off;
        uint32_t run = 0, run_col = 0, best_run = 0, best_col = 0;                      // (thread 0: the run of low columns that is open)
        // ---- vote and emit: PU_VCHUNK contig columns per pass
        for (uint32_t c_lo = 0; c_lo < n; c_lo += PU_VCHUNK) {
            const uint32_t c_hi = n - c_lo < PU_VCHUNK ? n : c_lo + PU_VCHUNK;
            for (uint32_t i = t; i < PU_VCHUNK * 8; i += PL_THREADS) s_votes[i] = 0;
            __syncthreads();
            if constexpr (PU_REPLACE) {
                for (uint64_t row0 = r0; row0 < r1; row0 += P.place.batch_rows) {
                    const uint32_t nb = r1 - row0 < P.place.batch_rows ? (uint32_t)(r1 - row0) : P.place.batch_rows;
                    const uint32_t mis = pl_stage_rows(P.place, row0, nb, s_rows);
                    if (t < nb) {
                        const uint32_t* nm = P.place.nmask ? P.place.nmask + (row0 + t) * P.place.nmw : nullptr;
                        const PlPlacement pm = pl_place_row(P.place, s_rows, (mis + t * P.place.rb) * 8, nm, s_fwd, s_rc, s_idx, n);
                        if (c_lo == 0 && pm.cnt) atomicAdd(&s_acc[pm.cnt == 1 ? PU_A_PLACED : PU_A_AMBIGUOUS], 1u);
                        if (pm.cnt == 1)
                            fill_vote_row<true>(s_votes, c_lo, c_hi, n, L, pm.strand, pm.D, (const uint8_t*)s_rows + mis + t * P.place.rb, nm);
                    }
                    __syncthreads();             // (the staged rows are read: the next batch replaces them)
                }
            } else
            for (uint64_t r = r0 + t; r < r1; r += PL_THREADS) {
                const uint32_t w = P.scratch[r];
                if (!(w & PS_PLACED)) continue;
                const uint32_t strand = (w & PS_STRAND) ? 1u : 0u;
                const int32_t d = (int32_t)(w & 0xFFFFu) - (int32_t)PS_BIAS;
                if (d >= (int32_t)c_hi || d + (int32_t)L <= (int32_t)c_lo) continue;
                fill_vote_row<true>(s_votes, c_lo, c_hi, n, L, strand, strand ? (int32_t)n - d - (int32_t)L : d, P.place.pool + r * P.place.rb,
                                    P.place.nmask ? P.place.nmask + r * P.place.nmw : nullptr);
            }
            __syncthreads();
            uint32_t c_unc = 0, c_thin = 0, c_con = 0, c_min = 0, c_one = 0;
            unsigned long long sum = 0, least = ~0ull;
            for (uint32_t k = 0; k < PU_VCHUNK; k += PL_THREADS) {                      // (every lane of a wave, for the ballot)
                const uint32_t j = c_lo + k + t;
                bool low = false;
                if (j < c_hi) {
                    const uint32_t* v = s_votes + (j - c_lo) * 8;
                    const uint32_t f0 = v[0], f1 = v[1], f2 = v[2], f3 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
                    if (fits) {
                        const uint32_t S = 65535u;
                        uint4 e;
                        e.x = (f0 < S ? f0 : S) | (f1 < S ? f1 : S) << 16;
                        e.y = (f2 < S ? f2 : S) | (f3 < S ? f3 : S) << 16;
                        e.z = (q0 < S ? q0 : S) | (q1 < S ? q1 : S) << 16;
                        e.w = (q2 < S ? q2 : S) | (q3 < S ? q3 : S) << 16;
                        outp[j] = e;
                    }
                    if (j >= b0 && j < b1) {
                        const uint32_t cur = stream32(s_fwd, 2 * (PL_LEAD + j)) >> 30;
                        const uint32_t fs = f0 + f1 + f2 + f3, qs = q0 + q1 + q2 + q3, depth = fs + qs;
                        const uint32_t a0 = f0 + q0, a1 = f1 + q1, a2 = f2 + q2, a3 = f3 + q3;
                        const uint32_t agree = cur == 0 ? a0 : cur == 1 ? a1 : cur == 2 ? a2 : a3;
                        uint32_t alt = 0;
                        if (cur != 0 && a0 > alt) alt = a0;
                        if (cur != 1 && a1 > alt) alt = a1;
                        if (cur != 2 && a2 > alt) alt = a2;
                        if (cur != 3 && a3 > alt) alt = a3;
                        const bool deep = depth >= P.min_depth;
                        const bool unc = depth == 0, thin = !unc && !deep;
                        const bool con = deep && 100ull * agree < (unsigned long long)P.min_agree * depth;
                        c_unc += unc;
                        c_thin += thin;
                        c_con += con;
                        c_min += alt > agree;
                        c_one += deep && (fs == 0 || qs == 0);
                        sum += depth;
                        const unsigned long long key = ((unsigned long long)depth << 32) | (j - b0);
                        least = key < least ? key : least;
                        low = unc || thin || con;
                    }
                }
                const unsigned long long mask = __ballot(low);
                if ((t & 63u) == 0) s_low[(k + t) >> 6] = mask;
            }
            if (c_unc) atomicAdd(&s_acc[PU_A_UNCOVERED], c_unc);
            if (c_thin) atomicAdd(&s_acc[PU_A_THIN], c_thin);
            if (c_con) atomicAdd(&s_acc[PU_A_CONTESTED], c_con);
            if (c_min) atomicAdd(&s_acc[PU_A_MINORITY], c_min);
            if (c_one) atomicAdd(&s_acc[PU_A_ONE_STRAND], c_one);
            if (sum) atomicAdd(&s_sum, sum);
            if (least != ~0ull) atomicMin(&s_min, least);
            __syncthreads();                     // (the votes are read: the next pass clears them; the ballots are written)
            if (t == 0) {
                // bit p of word w: column c_lo + 64 w + p is a low body column.  A column outside the body is never low: it ends a run
                for (uint32_t w = 0; w < PU_VCHUNK / 64; ++w) {
                    const unsigned long long m = s_low[w];
                    uint32_t p = 0;
                    while (p < 64) {
                        const unsigned long long x = m >> p;
                        if (x & 1ull) {
                            const unsigned long long y = ~x;                            // (its bits from 64 - p on are set)
                            const uint32_t ones = y ? (uint32_t)__builtin_ctzll(y) : 64u;
                            if (!run) run_col = c_lo + 64 * w + p - b0;
                            run += ones;
                            p += ones;
                            if (p < 64) {        // the run ends inside this word
                                if (run > best_run) { best_run = run; best_col = run_col; }
                                run = 0;
                            }
                        } else {
                            if (run > best_run) { best_run = run; best_col = run_col; }
                            run = 0;
                            p += x ? (uint32_t)__builtin_ctzll(x) : 64u - p;
                        }
                    }
                }
            }
        }
        if (t == 0) {
            if (run > best_run) { best_run = run; best_col = run_col; }
            const uint32_t n_low = s_acc[PU_A_UNCOVERED] + s_acc[PU_A_THIN] + s_acc[PU_A_CONTESTED];
            rec.off = fits ? off : 0;
            rec.len = fits ? n : 0;
            rec.flags = P.track && !fits ? (uint32_t)GF_PU_F_OVERFLOW : 0u;
            rec.n_cols = n_cols;
            rec.n_uncovered = s_acc[PU_A_UNCOVERED];
            rec.n_thin = s_acc[PU_A_THIN];
            rec.n_contested = s_acc[PU_A_CONTESTED];
            rec.n_minority = s_acc[PU_A_MINORITY];
            rec.n_one_strand = s_acc[PU_A_ONE_STRAND];
            rec.low_run = best_run;
            rec.low_run_col = best_col;
            if (n_cols) {
                rec.min_depth_seen = (uint32_t)(s_min >> 32);
                rec.min_depth_col = (uint32_t)s_min;
            }
            rec.depth_sum = s_sum;
            rec.reads_placed = s_acc[PU_A_PLACED];
            rec.reads_ambiguous = s_acc[PU_A_AMBIGUOUS];
            P.out[g] = rec;
            atomicAdd(P.round.stats + GF_PU_GAPS, 1u);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PU_PLACED), (unsigned long long)rec.reads_placed);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PU_AMBIGUOUS), (unsigned long long)rec.reads_ambiguous);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PU_LOW), (unsigned long long)n_low);
            if (P.track && !fits) atomicAdd(P.round.stats + GF_PU_OVERFLOW, 1u);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_pileup_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                                  int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                  const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                                  int min_overlap, int min_depth, int min_agree, void* d_records, void* d_track_or_null, size_t track_cap_entries,
                                  void* d_stats) {
    if ((track_cap_entries && !d_track_or_null) || ((uintptr_t)d_track_or_null & 15u)) return GF_E_INVAL;       // (whole 16-byte entries)
    PuParams P;
    memset(&P, 0, sizeof(P));
    int own = pl_place_setup(d_pool_packed, d_nmask_or_null, read_len, seed, max_mismatch, min_overlap, &P.place);
    if (min_depth < 1 || min_agree < 1 || min_agree > 100) own = GF_E_UNSUPPORTED;
    const FillRoundIn in = {d_pool_packed, d_pool_off, pool_rows, read_len, d_contigs, d_n_contigs, contig_cap, d_seq, d_gap_best, d_ctg_pick_or_null,
                            anchor_long, anchor_short, d_records, d_stats};
    size_t blocks;
    int rc = fill_round_setup(ctx, in, own, GF_PU_WORDS, PU_WGS_PER_CU, &P.round, &blocks);      // (workgroups the static LDS lets a CU hold)
    if (rc || !blocks) return rc;
    if ((rc = ensure(ctx, ctx->pu_place, 4 * pool_rows))) return rc;
    P.min_depth = (uint32_t)min_depth;
    P.min_agree = (uint32_t)min_agree;
    P.scratch = (uint32_t*)ctx->pu_place.p;
    P.out = (gf_fill_pileup*)d_records;
    P.track = (uint4*)d_track_or_null;
    P.track_cap = track_cap_entries;
    LaunchTimer tm(ctx, GF_KERNEL_PILEUP);
    hipLaunchKernelGGL(fill_pileup_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
