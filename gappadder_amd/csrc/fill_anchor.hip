// fill_anchor.hip — anchored pair span of the closed gaps: a mate the tagger found anchored in a flank of the gap, at its DRAFT coordinate,
// next to the placement of the other mate on the gap's winning contig (gf_fill_pairs_anchored_dev, include/gapfill_hip.h; definition and
// host twin: gappadder_amd/pair_anchors.py).  Runs behind gf_fill_pairs_dev of the same library: the rows' placement words
// (fill_pair_word.hpp) are an input, nothing is staged, indexed or placed here.  The reference has no such stage.
//   anchor_scatter_kernel   one tagger hit per thread, grid-stride: the filters, the mate's row by binary search of the gap's id slice
//                           (ps_order), a 64-bit atomicMin of (A0 << 1 | strand) into that row's anchor word — the caller's array, cleared
//                           to "none" on the stream before —; the drops are counted in LDS and added to the statistics once per workgroup
//   fill_anchor_kernel      one workgroup of 256 threads per closed gap, grid-stride.  A gap is opened by fill_round.hpp; a contig
//                           fill_pairs_kernel skipped (longer than PL_MAX, or a byte that base_code4 does not know: its stage's test) is
//                           skipped here — its scratch words are stale.  pair: a row per thread and turn, the anchor's virtual placement
//                           from the gap table and the body, the class of the pair in per-thread counters, and for an in-range pair LDS
//                           atomics into two difference arrays of n + 1 entries: the cover (i32) and the sum of insert - is_mean (i64).
//                           scan: §17's chunked prefix sum over both arrays; min / first argmin / zero count of the cover, and the columns
//                           with the smallest and the largest mean deviation by a workgroup reduction that compares means by
//                           cross-multiplication in 64 bits (|dev| < 2^20, a pool below 2^21 rows) and gives a tie to the smaller column
// Integer results, independent of the order of the atomics.  Everything written to global memory is a plain C++ store or an atomic of a
// vector lane.  Resources: DESIGN.md §20; the difference arrays take 96 KB of LDS: one workgroup per CU.
#include <cstring>

#include "fill_body.hpp"
#include "fill_pair_word.hpp"
#include "fill_round.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr unsigned long long PA_NONE = ~0ull;
enum { PA_S_KEPT, PA_S_CLIPPED, PA_S_IN_GAP, PA_S_SECONDARY, PA_S_ABSENT, PA_S_OTHER, PA_S_N };      // in the order of the statistics words
static_assert(GF_PA_KEPT + PA_S_OTHER == GF_PA_DROP_OTHER && GF_PA_KEPT + PA_S_ABSENT == GF_PA_ABSENT, "the scatter's counters are the words 4..9");
enum { PA_A_BAD, PA_A_ANCHORED, PA_A_PLACED, PA_A_PROPER, PA_A_MISORIENTED, PA_A_IN_RANGE, PA_A_SHORT, PA_A_LONG, PA_A_LEFT, PA_A_SPAN,
       PA_A_ZERO, PA_A_EVAL, PA_A_N };

struct PaScatterParams {
    const gf_alnrec* recs;
    uint64_t n_recs;
    const gf_taghit* hits;
    const uint32_t* n_hits;
    uint32_t hit_cap;
    const gf_gap* gaps;
    FillRoundArgs round;         // (pool_off, pool_rows, n_gaps, stats)
    const uint32_t* ids;
    unsigned long long* anchor;
};

struct PaParams {
    FillRoundArgs round;
    const unsigned long long* anchor;
    const uint32_t* scratch;
    const gf_gap* gaps;
    int64_t lo, hi, is_mean;     // lo, hi: is_mean -/+ z * is_sd
    uint32_t L, min_pairs;
    gf_fill_anchors* out;
};

__global__ __launch_bounds__(PL_THREADS) void anchor_scatter_kernel(PaScatterParams P) {
    __shared__ uint32_t s_cnt[PA_S_N];
    const uint32_t t = threadIdx.x;
    if (t < PA_S_N) s_cnt[t] = 0;
    __syncthreads();
    const uint32_t n = *P.n_hits < P.hit_cap ? *P.n_hits : P.hit_cap;
    for (uint64_t i = (uint64_t)blockIdx.x * PL_THREADS + t; i < n; i += (uint64_t)gridDim.x * PL_THREADS) {
        const gf_taghit h = P.hits[i];
        uint32_t what = PA_S_OTHER;
        do {
            if (h.to_mate != 1 || (h.kind != GF_KIND_DISCORDANT && h.kind != GF_KIND_UNMAP) || h.rec >= P.n_recs || h.gap >= P.round.n_gaps) break;
            const gf_alnrec A = P.recs[h.rec];
            if (A.clipflag) {                    // (the leftmost base is unknown: the record carries no CIGAR)
                what = PA_S_CLIPPED;
                break;
            }
            if (A.flag & (0x100u | 0x800u)) {
                what = PA_S_SECONDARY;
                break;
            }
            const uint32_t own = (uint32_t)A.read;
            if ((A.flag & 4u) || own == 0xFFFFFFFFu || A.pos == 0) break;
            const gf_gap G = P.gaps[h.gap];
            const uint32_t A0 = A.pos - 1;
            if (A0 >= G.start && A0 < G.end) {
                what = PA_S_IN_GAP;
                break;
            }
            const FillRows rows = fill_gap_rows(P.round, h.gap);
            const uint32_t id = own ^ 1u, want = ps_order(id);
            uint64_t a = rows.r0, b = rows.r1;   // the first row of the slice whose order is not below `want`
            while (a < b) {
                const uint64_t m = a + ((b - a) >> 1);
                if (ps_order(P.ids[m]) < want) a = m + 1;
                else b = m;
            }
            if (a >= rows.r1 || P.ids[a] != id) {
                what = PA_S_ABSENT;
                break;
            }
            atomicMin(&P.anchor[a], ((unsigned long long)A0 << 1) | ((A.flag >> 4) & 1u));
            what = PA_S_KEPT;
        } while (false);
        atomicAdd(&s_cnt[what], 1u);
    }
    __syncthreads();
    if (t < PA_S_N && s_cnt[t]) atomicAdd(P.round.stats + GF_PA_KEPT + t, s_cnt[t]);
}

// does the candidate (sum s, n pairs, column c) replace the holder (hs, hn, hc) as the smallest (SIGN = 1) / largest (SIGN = -1) mean?
// Means are compared by cross-multiplication; the products stay inside 64 bits (see above).  An equal mean: the smaller column
template <int SIGN>
__device__ __forceinline__ bool pa_better(long long s, uint32_t n, uint32_t c, long long hs, uint32_t hn, uint32_t hc) {
    if (!n) return false;
    if (!hn) return true;
    const long long x = s * (long long)hn, y = hs * (long long)n;
    return x == y ? c < hc : SIGN > 0 ? x < y : x > y;
}

__global__ __launch_bounds__(PL_THREADS) void fill_anchor_kernel(PaParams P) {
    __shared__ long long s_dev[PL_MAX + 1];
    __shared__ int32_t s_cov[PL_MAX + 1];
    __shared__ long long s_psum[PL_THREADS];
    __shared__ int32_t s_part[PL_THREADS];
    __shared__ long long s_es[2][PL_THREADS];    // the extremes' reduction: [0] the smallest mean, [1] the largest
    __shared__ uint32_t s_en[2][PL_THREADS], s_ec[2][PL_THREADS];
    __shared__ uint32_t s_loc[2];
    __shared__ uint32_t s_acc[PA_A_N];
    __shared__ unsigned long long s_span, s_devsum, s_min;
    const uint32_t t = threadIdx.x;
    const int64_t L = P.L;
    const uint32_t n_list = contig_list_end(P.round.body.list);
    for (uint32_t g = blockIdx.x; g < P.round.n_gaps; g += gridDim.x) {
        gf_fill_anchors rec;
        memset(&rec, 0, sizeof(rec));
        const FillGap fg = fill_gap_open<PL_THREADS>(P.round, n_list, g, s_loc);        // (fill_round.hpp; the same in all threads)
        if (fg.state == FILL_GAP_OPEN) {
            if (t == 0) P.out[g] = rec;
            continue;
        }
        if (fg.state == FILL_GAP_MISMATCH) {
            if (t == 0) {
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_PA_MISMATCH, 1u);
            }
            continue;
        }
        const uint32_t n = fg.fb.c.length, rev = fg.fb.rev;
        const char* ctg = P.round.body.list.seq + fg.fb.c.seq_off;
        const int64_t b0 = fg.fb.b0, b1 = fg.fb.b1;
        const FillRows rows = fill_gap_rows(P.round, g);
        rec.rows = (uint32_t)(rows.r1 - rows.r0);
        if (t < PA_A_N) s_acc[t] = 0;
        if (t == 0) {
            s_span = 0;
            s_devsum = 0;
            s_min = ~0ull;
        }
        __syncthreads();
        // ---- skip what fill_pairs_kernel skipped (pl_stage_or_skip: the length, then base_code4 of every byte); clear the differences
        const bool is_long = n > PL_MAX;
        if (!is_long) {
            uint32_t bad = 0;
            for (uint32_t i = t; i < n; i += PL_THREADS) bad |= base_code4((uint8_t)ctg[i]) >> 2;
            if (bad) atomicOr(&s_acc[PA_A_BAD], 1u);
            for (uint32_t i = t; i <= n; i += PL_THREADS) {
                s_cov[i] = 0;
                s_dev[i] = 0;
            }
        }
        __syncthreads();
        const uint32_t skip = is_long ? GF_PS_F_LONG : s_acc[PA_A_BAD] ? GF_PS_F_NON_ACGT : 0u;
        if (skip) {
            if (t == 0) {
                rec.flags = skip;
                P.out[g] = rec;
                atomicAdd(P.round.stats + (skip == GF_PS_F_LONG ? GF_PA_SKIPPED_LONG : GF_PA_SKIPPED_NON_ACGT), 1u);
            }
            continue;
        }
        // ---- pair: the anchor word and the placement word of every row
        {
            const gf_gap G = P.gaps[g];
            uint32_t c_anchored = 0, c_placed = 0, c_proper = 0, c_mis = 0, c_in = 0, c_short = 0, c_long = 0, c_left = 0, c_span = 0;
            long long sum = 0, dsum = 0;
            for (uint64_t i = rows.r0 + t; i < rows.r1; i += PL_THREADS) {
                const unsigned long long a = P.anchor[i];
                if (a == PA_NONE) continue;
                ++c_anchored;
                const uint32_t w = P.scratch[i];
                if (!(w & PS_PLACED)) continue;
                ++c_placed;
                const int64_t A0 = (int64_t)(a >> 1);
                const uint32_t sA = (uint32_t)a & 1u, str_a = rev ? 1u - sA : sA, str_b = (w & PS_STRAND) ? 1u : 0u;
                const bool left = A0 < (int64_t)G.start;
                const int64_t col = !rev ? (left ? b0 - ((int64_t)G.start - A0) : b1 + (A0 - (int64_t)G.end))
                                         : (left ? b1 + ((int64_t)G.start - A0) - L : b0 - (A0 - (int64_t)G.end) - L);
                const int64_t d = (int64_t)(w & 0xFFFFu) - (int64_t)PS_BIAS;
                const int64_t df = str_a ? d : col, dr = str_a ? col : d;
                if (str_a == str_b || df > dr) {
                    ++c_mis;
                    continue;
                }
                ++c_proper;
                const int64_t end = dr + L, insert = end - df;
                const bool in = insert > P.lo && insert < P.hi;
                if (in) ++c_in;
                else if (insert <= P.lo) ++c_short;
                else ++c_long;
                if (df <= b0 && b1 <= end) {
                    ++c_span;
                    sum += insert;
                }
                if (in) {
                    const long long dev = insert - P.is_mean;
                    c_left += left;
                    dsum += dev;
                    const uint32_t x0 = df <= 0 ? 0u : df < (int64_t)n ? (uint32_t)df : n, x1 = end <= 0 ? 0u : end < (int64_t)n ? (uint32_t)end : n;
                    atomicAdd(&s_cov[x0], 1);
                    atomicAdd(&s_cov[x1], -1);
                    atomicAdd((unsigned long long*)&s_dev[x0], (unsigned long long)dev);
                    atomicAdd((unsigned long long*)&s_dev[x1], (unsigned long long)-dev);
                }
            }
            if (c_anchored) atomicAdd(&s_acc[PA_A_ANCHORED], c_anchored);
            if (c_placed) atomicAdd(&s_acc[PA_A_PLACED], c_placed);
            if (c_proper) atomicAdd(&s_acc[PA_A_PROPER], c_proper);
            if (c_mis) atomicAdd(&s_acc[PA_A_MISORIENTED], c_mis);
            if (c_in) {
                atomicAdd(&s_acc[PA_A_IN_RANGE], c_in);
                atomicAdd(&s_devsum, (unsigned long long)dsum);
            }
            if (c_short) atomicAdd(&s_acc[PA_A_SHORT], c_short);
            if (c_long) atomicAdd(&s_acc[PA_A_LONG], c_long);
            if (c_left) atomicAdd(&s_acc[PA_A_LEFT], c_left);
            if (c_span) {
                atomicAdd(&s_acc[PA_A_SPAN], c_span);
                atomicAdd(&s_span, (unsigned long long)sum);
            }
        }
        __syncthreads();
        // ---- scan: thread t owns the columns [t * chunk, t * chunk + chunk) below b1 (an odd chunk, as in fill_pairs_kernel)
        if (b1 > b0) {
            const uint32_t e1 = (uint32_t)b1, e0 = (uint32_t)b0;
            const uint32_t chunk = ((e1 + PL_THREADS - 1) / PL_THREADS) | 1u;
            const uint32_t c0 = t * chunk < e1 ? t * chunk : e1, c1 = c0 + chunk < e1 ? c0 + chunk : e1;
            int32_t own = 0;
            long long own_s = 0;
            for (uint32_t c = c0; c < c1; ++c) {
                own += s_cov[c];
                own_s += s_dev[c];
            }
            s_part[t] = own;
            s_psum[t] = own_s;
            __syncthreads();
            for (uint32_t o = 1; o < PL_THREADS; o <<= 1) {
                const int32_t v = t >= o ? s_part[t - o] : 0;
                const long long vs = t >= o ? s_psum[t - o] : 0;
                __syncthreads();
                s_part[t] += v;
                s_psum[t] += vs;
                __syncthreads();
            }
            int32_t run = s_part[t] - own;       // the cover and the deviation sum of the column before c0
            long long run_s = s_psum[t] - own_s;
            uint32_t zeros = 0, n_eval = 0;
            unsigned long long best = ~0ull;
            long long mn_s = 0, mx_s = 0;
            uint32_t mn_n = 0, mx_n = 0, mn_c = 0, mx_c = 0;
            for (uint32_t c = c0; c < c1; ++c) {
                run += s_cov[c];
                run_s += s_dev[c];
                if (c < e0) continue;
                const unsigned long long key = ((unsigned long long)(uint32_t)run << 32) | c;
                best = key < best ? key : best;
                zeros += run == 0;
                if ((uint32_t)run < P.min_pairs) continue;
                ++n_eval;
                if (pa_better<1>(run_s, (uint32_t)run, c, mn_s, mn_n, mn_c)) {
                    mn_s = run_s;
                    mn_n = (uint32_t)run;
                    mn_c = c;
                }
                if (pa_better<-1>(run_s, (uint32_t)run, c, mx_s, mx_n, mx_c)) {
                    mx_s = run_s;
                    mx_n = (uint32_t)run;
                    mx_c = c;
                }
            }
            if (best != ~0ull) atomicMin(&s_min, best);
            if (zeros) atomicAdd(&s_acc[PA_A_ZERO], zeros);
            if (n_eval) atomicAdd(&s_acc[PA_A_EVAL], n_eval);
            s_es[0][t] = mn_s;
            s_en[0][t] = mn_n;
            s_ec[0][t] = mn_c;
            s_es[1][t] = mx_s;
            s_en[1][t] = mx_n;
            s_ec[1][t] = mx_c;
            __syncthreads();
            for (uint32_t o = PL_THREADS / 2; o; o >>= 1) {
                if (t < o) {
                    if (pa_better<1>(s_es[0][t + o], s_en[0][t + o], s_ec[0][t + o], s_es[0][t], s_en[0][t], s_ec[0][t])) {
                        s_es[0][t] = s_es[0][t + o];
                        s_en[0][t] = s_en[0][t + o];
                        s_ec[0][t] = s_ec[0][t + o];
                    }
                    if (pa_better<-1>(s_es[1][t + o], s_en[1][t + o], s_ec[1][t + o], s_es[1][t], s_en[1][t], s_ec[1][t])) {
                        s_es[1][t] = s_es[1][t + o];
                        s_en[1][t] = s_en[1][t + o];
                        s_ec[1][t] = s_ec[1][t + o];
                    }
                }
                __syncthreads();
            }
        }
        if (t == 0) {
            rec.n_anchored = s_acc[PA_A_ANCHORED];
            rec.n_placed = s_acc[PA_A_PLACED];
            rec.n_proper = s_acc[PA_A_PROPER];
            rec.n_misoriented = s_acc[PA_A_MISORIENTED];
            rec.n_in_range = s_acc[PA_A_IN_RANGE];
            rec.n_short = s_acc[PA_A_SHORT];
            rec.n_long = s_acc[PA_A_LONG];
            rec.n_left = s_acc[PA_A_LEFT];
            rec.n_span = s_acc[PA_A_SPAN];
            rec.span_insert_sum = (int64_t)s_span;
            rec.dev_sum = (int64_t)s_devsum;
            rec.n_cols = (uint32_t)(b1 - b0);
            if (b1 > b0) {
                rec.min_cover = (uint32_t)(s_min >> 32);
                rec.min_col = (uint32_t)s_min;
                rec.n_unspanned = s_acc[PA_A_ZERO];
                rec.n_eval = s_acc[PA_A_EVAL];
                if (rec.n_eval) {
                    rec.dev_min_col = s_ec[0][0];
                    rec.dev_min_n = s_en[0][0];
                    rec.dev_min_sum = s_es[0][0];
                    rec.dev_max_col = s_ec[1][0];
                    rec.dev_max_n = s_en[1][0];
                    rec.dev_max_sum = s_es[1][0];
                }
            }
            P.out[g] = rec;
            atomicAdd(P.round.stats + GF_PA_GAPS, 1u);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PA_ANCHORED), (unsigned long long)rec.n_anchored);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PA_PLACED), (unsigned long long)rec.n_placed);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PA_PROPER), (unsigned long long)rec.n_proper);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PA_IN_RANGE), (unsigned long long)rec.n_in_range);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PA_SPAN), (unsigned long long)rec.n_span);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_pairs_anchored_dev(gf_ctx* ctx, const void* d_pool_off, const void* d_pool_read_ids, size_t pool_cap_rows, int read_len,
                                          const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                          const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short,
                                          const void* d_place_scratch, const void* d_recs, size_t n_recs, const void* d_taghits,
                                          const void* d_n_taghits, size_t hit_cap, int is_mean, int is_sd, int z, int min_pairs, void* d_anchor,
                                          void* d_rec, void* d_stats) {
    if (pool_cap_rows && (!d_pool_read_ids || !d_place_scratch || !d_anchor)) return GF_E_INVAL;
    if (hit_cap && (!d_taghits || !d_n_taghits || (n_recs && !d_recs))) return GF_E_INVAL;
    if (hit_cap > 0xFFFFFFFFull) return GF_E_INVAL;
    const int own = (z < 1 || is_sd < 0 || min_pairs < 1 || (int64_t)z * is_sd >= (1ll << 20)) ? GF_E_UNSUPPORTED : GF_OK;
    // (the round reads no pool rows: the ids stand where the setup wants a pool with rows to be there)
    const FillRoundIn in = {d_pool_read_ids, d_pool_off, pool_cap_rows, read_len, d_contigs, d_n_contigs, contig_cap, d_seq, d_gap_best,
                            d_ctg_pick_or_null, anchor_long, anchor_short, d_rec, d_stats};
    PaParams P;
    memset(&P, 0, sizeof(P));
    size_t blocks;
    const int rc = fill_round_setup(ctx, in, own, GF_PA_WORDS, 1, &P.round, &blocks);   // 1: the difference arrays take most of a CU's LDS
    if (rc || !blocks) return rc;
    if (!ctx->d_gaps) return GF_E_STATE;
    P.anchor = (const unsigned long long*)d_anchor;
    P.scratch = (const uint32_t*)d_place_scratch;
    P.gaps = ctx->d_gaps;
    P.lo = (int64_t)is_mean - (int64_t)z * is_sd;
    P.hi = (int64_t)is_mean + (int64_t)z * is_sd;
    P.is_mean = is_mean;
    P.L = (uint32_t)read_len;
    P.min_pairs = (uint32_t)min_pairs;
    P.out = (gf_fill_anchors*)d_rec;
    LaunchTimer tm(ctx, GF_KERNEL_ANCHORS);
    if (pool_cap_rows) GF_HIP(ctx, hipMemsetAsync(d_anchor, 0xFF, 8 * pool_cap_rows, ctx->stream));
    if (hit_cap) {       // (without pool rows every target is absent: neither the ids nor the anchor words are touched)
        PaScatterParams S;
        memset(&S, 0, sizeof(S));
        S.recs = (const gf_alnrec*)d_recs;
        S.n_recs = n_recs;
        S.hits = (const gf_taghit*)d_taghits;
        S.n_hits = (const uint32_t*)d_n_taghits;
        S.hit_cap = (uint32_t)hit_cap;
        S.gaps = ctx->d_gaps;
        S.round = P.round;
        S.ids = (const uint32_t*)d_pool_read_ids;
        S.anchor = (unsigned long long*)d_anchor;
        const size_t want = (hit_cap + PL_THREADS - 1) / PL_THREADS, most = (size_t)ctx->n_cu * 8;
        hipLaunchKernelGGL(anchor_scatter_kernel, dim3((unsigned)(want < most ? want : most)), dim3(PL_THREADS), 0, ctx->stream, S);
        GF_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(fill_anchor_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
