// fill_pairs.hip — pair-span check of the closed gaps: the rows of ONE library's pool are placed without gaps on the gap's winning contig,
// the two mates of every pair are put together, and the record says how the pairs' inserts and their physical coverage fit the
// library's insert size (gf_fill_pairs_dev, include/gapfill_hip.h; definition and host twin: gappadder_amd/pair_span.py).
// The reference has no such stage.
//
// One workgroup of 256 threads per closed gap, grid-stride over the gaps.  A gap is opened by fill_round.hpp (open / mismatch / ok, the
// body [b0, b1) of fill_body.hpp, the gap's pool rows); the staging, the index and the placement of a row are fill_place.hpp's, and the
// launch is set up by fill_round_setup and pl_place_setup.  Per gap:
//   stage, index   fill_place.hpp (pl_stage_or_skip: a long or non-ACGT contig gets its flag and `rows`)
//   place    the pool's rows a batch at a time, one row per thread; a row's result — status, strand, diagonal on the contig as stored +
//            PS_BIAS — goes to one u32 of the caller's scratch array (global memory: a pool has no row bound).  ONE pass over the pool
//   pair     after a workgroup barrier (the scratch words are written and read by the same workgroup: workgroup scope is enough) every
//            thread takes rows of mate side 0, finds the mate's row by binary search of r ^ 1 in the gap's id slice — per gap the rows are
//            ordered by (mate side, pair), gf_build_pools_dev's contract —, classifies the pair, and adds +1 / -1 to a difference array
//            of n + 1 i32 for every in-range pair.  The index is dead by then: the array takes its LDS.  Counters: LDS atomics
//   scan     a workgroup prefix sum of the difference array up to b1 (a chunk of columns per thread, the chunks' sums scanned), then
//            min / first argmin / zero count over the body: integer results, independent of the order of the atomics
// Everything written to global memory is a plain C++ store or an atomicAdd of a vector lane.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md §17; no scratch, static LDS below 49 KB.
#include <cstring>

#include "fill_body.hpp"
#include "fill_pair_word.hpp"
#include "fill_place.hpp"
#include "fill_round.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t PS_IDX_WORDS = PL_MAX + 4;                                // the index's PL_SLOTS / 2 words, then the n + 1 differences
static_assert(PS_IDX_WORDS >= PL_SLOTS / 2 && PS_IDX_WORDS >= PL_MAX + 1, "pair-span geometry");      // (the placement word: fill_pair_word.hpp)
enum { PS_A_BAD, PS_A_COMPLETE, PS_A_PLACED, PS_A_PROPER, PS_A_MISORIENTED, PS_A_IN_RANGE, PS_A_SHORT, PS_A_LONG, PS_A_SPAN, PS_A_ZERO, PS_A_N };

struct PsParams {
    PlPlaceArgs place;
    FillRoundArgs round;         // (pool_off, pool_rows: the library's pool)
    const uint32_t* ids;
    const uint64_t* head_off;    // NULL, or offsets whose differences are the rows at the head of every slice that are ordered by (mate side, pair)
    int64_t lo, hi;              // is_mean -/+ z * is_sd
    uint32_t* scratch;
    gf_fill_pairs* out;
};

// the row of read `id` in ids[a, b) — ordered by (mate side, pair), or by_id: by read id — or b
__device__ __forceinline__ uint64_t ps_find(const uint32_t* ids, uint64_t a, uint64_t b, uint32_t id, bool by_id) {
    const uint64_t end = b;
    const uint32_t want = by_id ? id : ps_order(id);
    while (a < b) {
        const uint64_t m = a + ((b - a) >> 1);
        if ((by_id ? ids[m] : ps_order(ids[m])) < want) a = m + 1;
        else b = m;
    }
    return a < end && ids[a] == id ? a : end;
}

__global__ __launch_bounds__(PL_THREADS) void fill_pairs_kernel(PsParams P) {
    __shared__ uint32_t s_idx[PS_IDX_WORDS];
    __shared__ uint32_t s_fwd[PL_CTG_WORDS];
    __shared__ uint32_t s_rc[PL_CTG_WORDS];
    __shared__ uint32_t s_rows[PL_ROW_WORDS];
    __shared__ int32_t s_part[PL_THREADS];
    __shared__ uint32_t s_loc[2];
    __shared__ uint32_t s_acc[PS_A_N];
    __shared__ unsigned long long s_sum, s_min;
    int32_t* s_diff = (int32_t*)s_idx;
    const uint32_t t = threadIdx.x, L = P.place.L;
    const uint32_t n_list = contig_list_end(P.round.body.list);
    for (uint32_t g = blockIdx.x; g < P.round.n_gaps; g += gridDim.x) {
        gf_fill_pairs rec;
        memset(&rec, 0, sizeof(rec));
        const FillGap fg = fill_gap_open<PL_THREADS>(P.round, n_list, g, s_loc);        // (fill_round.hpp; the same in all threads)
        if (fg.state == FILL_GAP_OPEN) {
            if (t == 0) P.out[g] = rec;
            continue;
        }
        if (fg.state == FILL_GAP_MISMATCH) {
            if (t == 0) {
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_PS_MISMATCH, 1u);
            }
            continue;
        }
        const uint32_t n = fg.fb.c.length;
        const char* ctg = P.round.body.list.seq + fg.fb.c.seq_off;
        const uint32_t b0 = (uint32_t)fg.fb.b0, b1 = (uint32_t)fg.fb.b1;
        const FillRows rows = fill_gap_rows(P.round, g);
        const uint64_t r0 = rows.r0, r1 = rows.r1;
        rec.rows = (uint32_t)(r1 - r0);
        if (t < PS_A_N) s_acc[t] = 0;
        if (t == 0) {
            s_sum = 0;
            s_min = ~0ull;
        }
        __syncthreads();
        // ---- stage, or skip (fill_place.hpp)
        const uint32_t skip = pl_stage_or_skip(ctg, n, s_fwd, s_rc, s_idx, &s_acc[PS_A_BAD], GF_PS_F_LONG, GF_PS_F_NON_ACGT);
        if (skip) {
            if (t == 0) {
                rec.flags = skip;
                P.out[g] = rec;
                atomicAdd(P.round.stats + (skip == GF_PS_F_LONG ? GF_PS_SKIPPED_LONG : GF_PS_SKIPPED_NON_ACGT), 1u);
            }
            continue;
        }
        // ---- index
        pl_build_index(s_fwd, s_idx, n, P.place.s);
        __syncthreads();
        // ---- place: one pass, a word per row
        for (uint64_t row0 = r0; row0 < r1; row0 += P.place.batch_rows) {
            const uint32_t nb = r1 - row0 < P.place.batch_rows ? (uint32_t)(r1 - row0) : P.place.batch_rows;
            const uint32_t mis = pl_stage_rows(P.place, row0, nb, s_rows);
            if (t < nb) {
                const uint32_t* nm = P.place.nmask ? P.place.nmask + (row0 + t) * P.place.nmw : nullptr;
                const PlPlacement pm = pl_place_row(P.place, s_rows, (mis + t * P.place.rb) * 8, nm, s_fwd, s_rc, s_idx, n);
                // strand 1: the row as stored lies at D on the reverse complement = its reverse complement at n - D - L on the contig
                const int32_t d = pm.strand ? (int32_t)n - pm.D - (int32_t)L : pm.D;
                P.scratch[row0 + t] = pm.cnt == 0 ? 0u : pm.cnt > 1 ? PS_AMBIGUOUS : PS_PLACED | (pm.strand ? PS_STRAND : 0u) | (uint32_t)(d + (int32_t)PS_BIAS);
            }
            __syncthreads();                     // (the staged rows are read: the next batch replaces them)
        }
        for (uint32_t i = t; i <= n; i += PL_THREADS) s_diff[i] = 0;                    // (the index is dead)
        __threadfence_block();
        __syncthreads();                         // (every row's word is in the scratch array, the differences are clear)
        // ---- pair
        {
            uint32_t c_complete = 0, c_placed = 0, c_proper = 0, c_mis = 0, c_in = 0, c_short = 0, c_long = 0, c_span = 0;
            long long sum = 0;
            // [r0, rh): ordered by (mate side, pair); [rh, r1): pairs appended behind them, ordered by read id (a closing pool's recruits)
            const uint64_t rh = P.head_off ? min(r1, r0 + (P.head_off[g + 1] - P.head_off[g])) : r1;
            for (uint64_t i = r0 + t; i < r1; i += PL_THREADS) {
                const uint32_t id = P.ids[i];
                if (id & 1u) continue;
                if (i >= rh && ps_find(P.ids, r0, rh, id, false) < rh) continue;       // a read met twice counts at its first row
                uint64_t a = ps_find(P.ids, r0, rh, id ^ 1u, false);
                if (a >= rh) a = ps_find(P.ids, rh, r1, id ^ 1u, true);                // (the mate's first row as well)
                if (a >= r1) continue;
                ++c_complete;
                const uint32_t w0 = P.scratch[i], w1 = P.scratch[a];
                if (!(w0 & w1 & PS_PLACED)) continue;
                ++c_placed;
                const int32_t d0 = (int32_t)(w0 & 0xFFFFu) - (int32_t)PS_BIAS, d1 = (int32_t)(w1 & 0xFFFFu) - (int32_t)PS_BIAS;
                const int32_t df = (w0 & PS_STRAND) ? d1 : d0, dr = (w0 & PS_STRAND) ? d0 : d1;
                if (!((w0 ^ w1) & PS_STRAND) || df > dr) {
                    ++c_mis;
                    continue;
                }
                ++c_proper;
                const int32_t end = dr + (int32_t)L;
                const long long insert = (long long)end - df;
                const bool in = insert > P.lo && insert < P.hi;
                if (in) ++c_in;
                else if (insert <= P.lo) ++c_short;
                else ++c_long;
                if (df <= (int32_t)b0 && (int32_t)b1 <= end) {
                    ++c_span;
                    sum += insert;
                }
                if (in) {
                    atomicAdd(&s_diff[df > 0 ? df : 0], 1);
                    atomicAdd(&s_diff[end < (int32_t)n ? end : (int32_t)n], -1);
                }
            }
            if (c_complete) atomicAdd(&s_acc[PS_A_COMPLETE], c_complete);
            if (c_placed) atomicAdd(&s_acc[PS_A_PLACED], c_placed);
            if (c_proper) atomicAdd(&s_acc[PS_A_PROPER], c_proper);
            if (c_mis) atomicAdd(&s_acc[PS_A_MISORIENTED], c_mis);
            if (c_in) atomicAdd(&s_acc[PS_A_IN_RANGE], c_in);
            if (c_short) atomicAdd(&s_acc[PS_A_SHORT], c_short);
            if (c_long) atomicAdd(&s_acc[PS_A_LONG], c_long);
            if (c_span) {
                atomicAdd(&s_acc[PS_A_SPAN], c_span);
                atomicAdd(&s_sum, (unsigned long long)sum);
            }
        }
        __syncthreads();
        // ---- scan: thread t owns the columns [t * chunk, t * chunk + chunk) below b1 (an odd chunk: no LDS bank is taken twice)
        if (b1 > b0) {
            const uint32_t chunk = ((b1 + PL_THREADS - 1) / PL_THREADS) | 1u;
            const uint32_t c0 = t * chunk < b1 ? t * chunk : b1, c1 = c0 + chunk < b1 ? c0 + chunk : b1;
            int32_t own = 0;
            for (uint32_t c = c0; c < c1; ++c) own += s_diff[c];
            s_part[t] = own;
            __syncthreads();
            for (uint32_t o = 1; o < PL_THREADS; o <<= 1) {
                const int32_t v = t >= o ? s_part[t - o] : 0;
                __syncthreads();
                s_part[t] += v;
                __syncthreads();
            }
            int32_t run = s_part[t] - own;       // the cover of the column before c0
            uint32_t zeros = 0;
            unsigned long long best = ~0ull;
            for (uint32_t c = c0; c < c1; ++c) {
                run += s_diff[c];
                if (c < b0) continue;
                const unsigned long long key = ((unsigned long long)(uint32_t)run << 32) | c;
                best = key < best ? key : best;
                zeros += run == 0;
            }
            if (best != ~0ull) atomicMin(&s_min, best);
            if (zeros) atomicAdd(&s_acc[PS_A_ZERO], zeros);
            __syncthreads();
        }
        if (t == 0) {
            rec.pairs_complete = s_acc[PS_A_COMPLETE];
            rec.pairs_placed = s_acc[PS_A_PLACED];
            rec.n_proper = s_acc[PS_A_PROPER];
            rec.n_misoriented = s_acc[PS_A_MISORIENTED];
            rec.n_in_range = s_acc[PS_A_IN_RANGE];
            rec.n_short = s_acc[PS_A_SHORT];
            rec.n_long = s_acc[PS_A_LONG];
            rec.n_span = s_acc[PS_A_SPAN];
            rec.span_insert_sum = (int64_t)s_sum;
            rec.n_cols = b1 - b0;
            if (b1 > b0) {
                rec.min_cover = (uint32_t)(s_min >> 32);
                rec.min_col = (uint32_t)s_min;
                rec.n_unspanned = s_acc[PS_A_ZERO];
            }
            P.out[g] = rec;
            atomicAdd(P.round.stats + GF_PS_GAPS, 1u);
            if (rec.n_unspanned) atomicAdd(P.round.stats + GF_PS_UNSPANNED, 1u);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PS_COMPLETE), (unsigned long long)rec.pairs_complete);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PS_PLACED), (unsigned long long)rec.pairs_placed);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PS_PROPER), (unsigned long long)rec.n_proper);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PS_IN_RANGE), (unsigned long long)rec.n_in_range);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PS_SPAN), (unsigned long long)rec.n_span);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_pairs_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, const void* d_pool_read_ids,
                                 size_t pool_cap_rows, int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                 const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                                 int min_overlap, int is_mean, int is_sd, int z, void* d_place_scratch, void* d_rec, void* d_stats) {
    return gf_fill_pairs_split_dev(ctx, d_pool_packed, d_nmask_or_null, d_pool_off, d_pool_read_ids, pool_cap_rows, nullptr, read_len, d_contigs,
                                   d_n_contigs, contig_cap, d_seq, d_gap_best, d_ctg_pick_or_null, anchor_long, anchor_short, seed, max_mismatch,
                                   min_overlap, is_mean, is_sd, z, d_place_scratch, d_rec, d_stats);
}

extern "C" int gf_fill_pairs_split_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, const void* d_pool_read_ids,
                                 size_t pool_cap_rows, const void* d_head_off_or_null, int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                 const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                                 int min_overlap, int is_mean, int is_sd, int z, void* d_place_scratch, void* d_rec, void* d_stats) {
    if (pool_cap_rows && (!d_pool_read_ids || !d_place_scratch)) return GF_E_INVAL;
    PsParams P;
    memset(&P, 0, sizeof(P));
    int own = pl_place_setup(d_pool_packed, d_nmask_or_null, read_len, seed, max_mismatch, min_overlap, &P.place);
    if (z < 1 || is_sd < 0) own = GF_E_UNSUPPORTED;
    const FillRoundIn in = {d_pool_packed, d_pool_off, pool_cap_rows, read_len, d_contigs, d_n_contigs, contig_cap, d_seq, d_gap_best,
                            d_ctg_pick_or_null, anchor_long, anchor_short, d_rec, d_stats};
    size_t blocks;
    const int rc = fill_round_setup(ctx, in, own, GF_PS_WORDS, 3, &P.round, &blocks);   // 3: workgroups the static LDS lets a CU hold
    if (rc || !blocks) return rc;
    P.ids = (const uint32_t*)d_pool_read_ids;
    P.head_off = (const uint64_t*)d_head_off_or_null;
    P.lo = (int64_t)is_mean - (int64_t)z * is_sd;
    P.hi = (int64_t)is_mean + (int64_t)z * is_sd;
    P.scratch = (uint32_t*)d_place_scratch;
    P.out = (gf_fill_pairs*)d_rec;
    LaunchTimer tm(ctx, GF_KERNEL_PAIRS);
    hipLaunchKernelGGL(fill_pairs_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
