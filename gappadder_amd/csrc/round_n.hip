// round_n.hip — recruitment rounds 2 and later of the device step ("Repeated rounds"): round 1 (round2.hip) run again with
// the contigs the round before appended, until a round grows no gap.
//   table    the (k-mer, gap) table of the contigs [*d_first, n): round r reads only what round r - 1 appended.  One wave per contig; a
//            lane rolls the forward and the reverse k-mer along a run of RN_RUN positions (k - 1 + RN_RUN bases read instead of
//            k * RN_RUN).  The inserts are latency-bound random atomics, so what counts is how many lanes have one in flight: short
//            runs and a wave per contig keep most lanes of a few-hundred-base contig busy (a workgroup per contig with runs of 32 left
//            one lane in eighteen working and ran at half the speed of round 1's kernel).  The insert is round 1's (round2_dev.hpp)
//   carry    the distinct keys of the round before to the front of the key buffer, their per-gap counts to prev_cnt, their total into the
//            new round's HITS word: the recruitment (round 1's entry, unchanged) appends behind them
//   pools    round 1's, except that a gap gets a pool only when it is open and its count grew, and that both copies skip gaps without one
//   gate     every kernel here reads *d_live first (the round before's GROWN word; round 1's WITH) and returns when it is 0; the rocprim
//            sort and scans in between cannot be gated, so they write to the context's scratch and gated kernels carry the results on
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gf_internal.hpp"
#include "round2_dev.hpp"

namespace gf {

namespace {

constexpr uint32_t RN_RUN = 8;      // k-mer positions a lane rolls through before it starts again k - 1 bases back

__device__ __forceinline__ bool rn_live(const uint32_t* live) { return !live || *live != 0u; }

__global__ __launch_bounds__(256) void rn_clear_table_kernel(uint64_t* tab, uint64_t words, const uint32_t* live) {
    if (!rn_live(live)) return;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) tab[i] = 0;
}

// one wave per contig, one lane per run of RN_RUN k-mer positions
__global__ __launch_bounds__(256) void rn_table_kernel(const gf_contig* ctg, const uint32_t* d_n, uint64_t ctg_cap, const char* seq,
                                                       const uint64_t* best, uint64_t n_gaps, int k, const uint32_t* d_first, R2Slot* tab,
                                                       uint32_t log2, uint32_t* stats, const uint32_t* live) {
    if (!rn_live(live)) return;
    const uint64_t n1 = min((uint64_t)*d_n, ctg_cap);
    const int kb = 2 * k;
    const uint64_t mhi = kb >= 128 ? ~0ull : (kb > 64 ? (1ull << (kb - 64)) - 1 : 0ull);
    const uint64_t mlo = kb >= 64 ? ~0ull : (1ull << kb) - 1;
    const int sh = 128 - kb;    // left alignment
    uint32_t mine = 0;
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    for (uint64_t c = (uint64_t)*d_first + (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); c < n1; c += (uint64_t)gridDim.x * waves) {
        const gf_contig C = ctg[c];
        if (C.gap >= n_gaps || best[C.gap] != 0 || C.length < (uint32_t)k) continue;    // (uniform in the wave)
        const char* s = seq + C.seq_off;
        const uint32_t npos = C.length - (uint32_t)k + 1;
        for (uint32_t p0 = lane * RN_RUN; p0 < npos; p0 += 64u * RN_RUN) {
            const uint32_t end = min(p0 + RN_RUN, npos) + (uint32_t)k - 1;      // bases [p0, end), end <= length
            uint64_t fhi = 0, flo = 0, rhi = 0, rlo = 0;
            uint32_t run = 0;
            for (uint32_t i = p0; i < end; ++i) {
                const char ch = s[i];
                const uint64_t b = base_code(ch);
                fhi = ((fhi << 2) | (flo >> 62)) & mhi;
                flo = ((flo << 2) | b) & mlo;
                rlo = (rlo >> 2) | (rhi << 62);
                rhi >>= 2;
                if (kb - 2 >= 64) rhi |= (3u - b) << (kb - 2 - 64);
                else rlo |= (3u - b) << (kb - 2);
                run = r2_acgt(ch) ? run + 1 : 0;
                if (run < (uint32_t)k) continue;        // (run >= k implies i >= p0 + k - 1: the window lies in this thread's bases)
                const bool rev = rhi < fhi || (rhi == fhi && rlo < flo);
                const uint64_t chi = rev ? rhi : fhi, clo = rev ? rlo : flo;
                K128 v;
                if (sh == 0) { v.hi = chi; v.lo = clo; }
                else if (sh < 64) { v.hi = (chi << sh) | (clo >> (64 - sh)); v.lo = clo << sh; }
                else if (sh == 64) { v.hi = clo; v.lo = 0; }
                else { v.hi = clo << (sh - 64); v.lo = 0; }
                ++mine;
                r2_insert(tab, log2, v, C.gap, stats + R2_TAB_FULL);
            }
        }
    }
    if (mine) atomicAdd(stats + R2_KMERS, mine);
}

// the round before's distinct keys (flag / uidx / cnt as its pools call left them) to the front of the key buffer
__global__ __launch_bounds__(256) void rn_carry_kernel(unsigned long long* keys, const unsigned long long* sorted, uint64_t key_cap, uint64_t n_gaps,
                                                       const uint32_t* flag, const uint32_t* uidx, const uint32_t* cnt, uint32_t* prev_cnt,
                                                       const uint32_t* prev_stats, uint32_t* stats, const uint32_t* d_n, const uint32_t* np_in,
                                                       uint32_t* np_out, uint32_t n_lib, unsigned long long* snap, const uint32_t* live) {
    const uint64_t t0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    if (*live == 0u) {
        if (t0 == 0) {
            stats[R2_FIRST] = *d_n;
            stats[R2_GATED] = 1;
            for (uint32_t l = 0; l < n_lib; ++l) np_out[l] = 0;      // the recruitment of a gated round has no candidates
        }
        return;
    }
    const uint64_t total = min((uint64_t)prev_stats[R2_UNIQUE], key_cap);
    for (uint64_t i = t0; i < key_cap; i += stride) {
        if (flag[i]) {
            const uint64_t j = uidx[i];         // (j < total <= i: a slot the tail fill below leaves alone)
            if (j < total) {
                const unsigned long long x = sorted[i];
                keys[j] = x;
                if (snap) snap[j] = x;
            }
        }
        if (i >= total) keys[i] = R2_EMPTY_KEY;
    }
    for (uint64_t g = t0; g < n_gaps; g += stride) prev_cnt[g] = cnt[g];
    if (t0 == 0) {
        stats[R2_HITS] = (uint32_t)total;
        for (uint32_t l = 0; l < n_lib; ++l) np_out[l] = np_in[l];
    }
}

__global__ __launch_bounds__(256) void rn_zero_kernel(uint32_t* p, uint64_t n, const uint32_t* live) {
    if (!rn_live(live)) return;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) p[i] = 0;
}

// s: the sorted keys in the scratch; they go on to `out`, with their unique flags and the per-gap counts
__global__ __launch_bounds__(256) void rn_mark_kernel(const unsigned long long* s, uint64_t n, uint64_t n_gaps, unsigned long long* out, uint32_t* flag,
                                                      uint32_t* cnt, const uint32_t* live) {
    if (!rn_live(live)) return;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long x = s[i];
        const bool u = x != R2_EMPTY_KEY && key_gap(x) < n_gaps && (i == 0 || s[i - 1] != x);
        out[i] = x;
        flag[i] = u;
        if (u) atomicAdd(cnt + key_gap(x), 1u);
    }
}

// scan: the flags' exclusive scan in the scratch; it goes on to uidx, and every gap's first unique index to start
__global__ __launch_bounds__(256) void rn_start_kernel(const unsigned long long* s, uint64_t n, const uint32_t* flag, const uint32_t* scan,
                                                       uint32_t* uidx, uint32_t* start, const uint32_t* live) {
    if (!rn_live(live)) return;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t u = scan[i];
        uidx[i] = u;
        if (flag[i] && (i == 0 || key_gap(s[i - 1]) != key_gap(s[i]))) start[key_gap(s[i])] = u;      // (a flagged key's gap is < n_gaps)
    }
}

__global__ __launch_bounds__(256) void rn_sizes_kernel(const uint64_t* asm_off, const uint64_t* best, uint64_t n_gaps, const uint32_t* cnt,
                                                       const uint32_t* prev_cnt, uint64_t* rows, uint32_t* stats, const uint32_t* live) {
    if (!rn_live(live)) return;
    uint32_t tried = 0, with = 0, uni = 0, fresh = 0, grown = 0;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g <= n_gaps; g += (uint64_t)gridDim.x * blockDim.x) {
        if (g == n_gaps) { rows[g] = 0; continue; }
        const uint32_t c = cnt[g], p = prev_cnt[g];
        const bool open = best[g] == 0, grew = open && c > p;
        tried += open;
        with += c != 0;
        uni += c;
        fresh += open && c > p ? c - p : 0u;
        grown += grew;
        rows[g] = grew ? (asm_off[g + 1] - asm_off[g]) + 2ull * c : 0ull;
    }
    if (tried) atomicAdd(stats + R2_TRIED, tried);
    if (with) atomicAdd(stats + R2_WITH, with);
    if (uni) atomicAdd(stats + R2_UNIQUE, uni);
    if (fresh) atomicAdd(stats + R2_NEW, fresh);
    if (grown) atomicAdd(stats + R2_GROWN, grown);
}

// scan: the rows' exclusive scan in the scratch; the offsets are it, or all zero when the total is beyond the pool capacity
__global__ __launch_bounds__(256) void rn_offsets_kernel(const uint64_t* scan, uint64_t n_gaps, uint64_t pool_cap, uint64_t* off, uint32_t* stats,
                                                         const uint32_t* live) {
    if (!rn_live(live)) return;
    const uint64_t tot = scan[n_gaps];
    const bool ovf = tot > pool_cap;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g <= n_gaps; g += (uint64_t)gridDim.x * blockDim.x) off[g] = ovf ? 0ull : scan[g];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[R2_ROWS] = (uint32_t)tot;
        stats[R2_ROWS + 1] = (uint32_t)(tot >> 32);
        stats[R2_POOL_OVF] = ovf;
    }
}

// one workgroup per gap with a pool: its round-1 rows to the pool's head
__global__ __launch_bounds__(256) void rn_copy_round1_kernel(const uint8_t* asm_pool, const uint64_t* asm_off, const uint64_t* rows, const uint64_t* off,
                                                             uint32_t rb, uint8_t* pool, const uint32_t* stats, const uint32_t* live) {
    if (!rn_live(live)) return;
    const uint32_t g = blockIdx.x;
    if (!rows[g] || stats[R2_POOL_OVF]) return;
    const uint64_t n = (asm_off[g + 1] - asm_off[g]) * rb;
    const uint8_t* src = asm_pool + asm_off[g] * rb;
    uint8_t* dst = pool + off[g] * rb;
    for (uint64_t b = threadIdx.x; b < n; b += blockDim.x) dst[b] = src[b];
}

// every distinct pair of a gap with a pool: its two rows behind the gap's round-1 rows (a key of a gap without a pool has no row to go to)
__global__ __launch_bounds__(256) void rn_copy_recruits_kernel(const unsigned long long* s, uint64_t n, const uint32_t* flag, const uint32_t* uidx,
                                                               const uint32_t* start, const uint64_t* asm_off, const uint64_t* rows, const uint64_t* off,
                                                               LibRows libs, uint32_t rb, uint8_t* pool, const uint32_t* stats, const uint32_t* live) {
    if (!rn_live(live) || stats[R2_POOL_OVF]) return;
    const uint64_t per = 2ull * rb;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n * per; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = t / per, b = t - i * per;
        if (!flag[i]) continue;
        const unsigned long long x = s[i];
        const uint32_t g = key_gap(x), lib = (uint32_t)(x >> 36) & (GF_R2_MAX_LIBS - 1);
        if (!rows[g] || !libs.reads[lib]) continue;
        const uint64_t pair = x & ((1ull << 36) - 1);
        const uint64_t row = off[g] + (asm_off[g + 1] - asm_off[g]) + 2ull * (uidx[i] - start[g]);      // < off[g] + rows[g] <= pool_cap
        pool[row * rb + b] = libs.reads[lib][2 * pair * rb + b];
    }
}

size_t rn_align(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace
}  // namespace gf

using namespace gf;

extern "C" {

int gf_contig_kmer_table_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                  const void* d_gap_best, size_t n_gaps, int k, const void* d_first, void* d_table, int log2_slots, void* d_stats,
                                  const void* d_live_or_null) {
    if (!ctx || !d_contigs || !d_n_contigs || !d_seq || !d_gap_best || !d_first || !d_table || !d_stats) return GF_E_INVAL;
    if (k < 16 || k > 64 || log2_slots < 4 || log2_slots > 32 || n_gaps >= (1ull << 24) - 1) return GF_E_UNSUPPORTED;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    const uint64_t words = 3ull << log2_slots;
    hipLaunchKernelGGL(rn_clear_table_kernel, dim3(r2_grid(ctx, words)), dim3(256), 0, ctx->stream, (uint64_t*)d_table, words,
                       (const uint32_t*)d_live_or_null);
    hipLaunchKernelGGL(rn_table_kernel, dim3((unsigned)ctx->n_cu * 8), dim3(256), 0, ctx->stream, (const gf_contig*)d_contigs,
                       (const uint32_t*)d_n_contigs, (uint64_t)contig_cap, (const char*)d_seq, (const uint64_t*)d_gap_best, (uint64_t)n_gaps, k,
                       (const uint32_t*)d_first, (R2Slot*)d_table, (uint32_t)log2_slots, (uint32_t*)d_stats, (const uint32_t*)d_live_or_null);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_round_carry_dev(gf_ctx* ctx, void* d_keys, const void* d_keys_sorted, size_t key_cap, size_t n_gaps, const void* d_work, void* d_prev_cnt,
                       const void* d_prev_stats, void* d_stats, const void* d_n_contigs, const void* d_n_pairs, void* d_n_pairs_live, int n_lib,
                       void* d_snapshot_or_null, const void* d_live) {
    if (!ctx || !d_keys || !d_keys_sorted || !d_work || !d_prev_cnt || !d_prev_stats || !d_stats || !d_n_contigs || !d_n_pairs || !d_n_pairs_live ||
        !d_live)
        return GF_E_INVAL;
    if (n_lib < 1 || n_lib > GF_R2_MAX_LIBS || n_gaps == 0 || n_gaps >= (1ull << 24) - 1 || key_cap == 0 || key_cap > 0xFFFFFFFFull)
        return GF_E_UNSUPPORTED;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t* flag = (const uint32_t*)d_work;     // gf_round2_pools_dev's / gf_round_pools_dev's layout of d_work
    const uint32_t* uidx = flag + key_cap;
    const uint32_t* cnt = uidx + key_cap;
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    hipLaunchKernelGGL(rn_carry_kernel, dim3(r2_grid(ctx, std::max(key_cap, n_gaps))), dim3(256), 0, ctx->stream, (unsigned long long*)d_keys,
                       (const unsigned long long*)d_keys_sorted, (uint64_t)key_cap, (uint64_t)n_gaps, flag, uidx, cnt, (uint32_t*)d_prev_cnt,
                       (const uint32_t*)d_prev_stats, (uint32_t*)d_stats, (const uint32_t*)d_n_contigs, (const uint32_t*)d_n_pairs,
                       (uint32_t*)d_n_pairs_live, (uint32_t)n_lib, (unsigned long long*)d_snapshot_or_null, (const uint32_t*)d_live);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_round_pools_dev(gf_ctx* ctx, void* d_keys, void* d_keys_sorted, size_t key_cap, const void* const* d_lib_reads, int n_lib, int read_len,
                       const void* d_asm_pool, const void* d_asm_off, const void* d_gap_best, size_t n_gaps, const void* d_prev_cnt, void* d_work,
                       void* d_rows, void* d_pool, size_t pool_cap, void* d_stats, const void* d_live_or_null) {
    if (!ctx || !d_keys || !d_keys_sorted || !d_lib_reads || !d_asm_off || !d_gap_best || !d_prev_cnt || !d_work || !d_rows || !d_stats ||
        (pool_cap && !d_pool) || read_len < 1)
        return GF_E_INVAL;
    if (n_lib < 1 || n_lib > GF_R2_MAX_LIBS || n_gaps == 0 || n_gaps >= (1ull << 24) - 1 || key_cap == 0 || key_cap > 0xFFFFFFFFull)
        return GF_E_UNSUPPORTED;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    LibRows libs{};
    for (int l = 0; l < n_lib; ++l) {
        if (!d_lib_reads[l]) return GF_E_INVAL;
        libs.reads[l] = (const uint8_t*)d_lib_reads[l];
    }
    const uint32_t rb = (uint32_t)gf_packed_read_bytes(read_len);
    const uint32_t* live = (const uint32_t*)d_live_or_null;
    unsigned long long* keys = (unsigned long long*)d_keys;
    unsigned long long* sorted = (unsigned long long*)d_keys_sorted;
    uint32_t* flag = (uint32_t*)d_work;                 // [key_cap] unique flags
    uint32_t* uidx = flag + key_cap;                    // [key_cap] their exclusive scan
    uint32_t* cnt = uidx + key_cap;                     // [n_gaps] distinct recruited pairs per gap, all rounds so far
    uint32_t* start = cnt + n_gaps;                     // [n_gaps] the gap's first index in the unique list
    uint64_t* sizes = (uint64_t*)d_rows;                // [n_gaps + 1] this round's rows per gap
    uint64_t* off = sizes + n_gaps + 1;                 // [n_gaps + 1] their exclusive scan: the pool offsets
    uint32_t* st = (uint32_t*)d_stats;
    size_t t_sort = 0, t_scan32 = 0, t_scan64 = 0;
    GF_HIP(ctx, rocprim::radix_sort_keys(nullptr, t_sort, keys, sorted, key_cap, 0, 64, ctx->stream));
    GF_HIP(ctx, rocprim::exclusive_scan(nullptr, t_scan32, flag, uidx, 0u, key_cap, rocprim::plus<uint32_t>(), ctx->stream));
    GF_HIP(ctx, rocprim::exclusive_scan(nullptr, t_scan64, sizes, off, (uint64_t)0, n_gaps + 1, rocprim::plus<uint64_t>(), ctx->stream));
    // the scratch: rocprim's own, then what its calls write (an ungated call must not touch the caller's buffers)
    const size_t o_sorted = rn_align(std::max(t_sort, std::max(t_scan32, t_scan64)) + 64), o_off = o_sorted + rn_align(8 * key_cap),
                 o_scan = o_off + rn_align(8 * (n_gaps + 1)), total = o_scan + rn_align(4 * key_cap);
    int rc;
    if ((rc = ensure(ctx, ctx->r2_tmp, total))) return rc;
    char* tmp = (char*)ctx->r2_tmp.p;
    unsigned long long* t_sorted = (unsigned long long*)(tmp + o_sorted);
    uint64_t* t_off = (uint64_t*)(tmp + o_off);
    uint32_t* t_uidx = (uint32_t*)(tmp + o_scan);
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    GF_HIP(ctx, rocprim::radix_sort_keys(tmp, t_sort, keys, t_sorted, key_cap, 0, 64, ctx->stream));
    const unsigned gk = r2_grid(ctx, key_cap), gg = r2_grid(ctx, n_gaps + 1);
    hipLaunchKernelGGL(rn_zero_kernel, dim3(gg), dim3(256), 0, ctx->stream, cnt, (uint64_t)2 * n_gaps, live);
    hipLaunchKernelGGL(rn_mark_kernel, dim3(gk), dim3(256), 0, ctx->stream, t_sorted, (uint64_t)key_cap, (uint64_t)n_gaps, sorted, flag, cnt, live);
    GF_HIP(ctx, rocprim::exclusive_scan(tmp, t_scan32, flag, t_uidx, 0u, key_cap, rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(rn_start_kernel, dim3(gk), dim3(256), 0, ctx->stream, t_sorted, (uint64_t)key_cap, flag, t_uidx, uidx, start, live);
    hipLaunchKernelGGL(rn_sizes_kernel, dim3(gg), dim3(256), 0, ctx->stream, (const uint64_t*)d_asm_off, (const uint64_t*)d_gap_best, (uint64_t)n_gaps,
                       cnt, (const uint32_t*)d_prev_cnt, sizes, st, live);
    GF_HIP(ctx, rocprim::exclusive_scan(tmp, t_scan64, sizes, t_off, (uint64_t)0, n_gaps + 1, rocprim::plus<uint64_t>(), ctx->stream));
    hipLaunchKernelGGL(rn_offsets_kernel, dim3(gg), dim3(256), 0, ctx->stream, t_off, (uint64_t)n_gaps, (uint64_t)pool_cap, off, st, live);
    if (pool_cap) {
        hipLaunchKernelGGL(rn_copy_round1_kernel, dim3((unsigned)n_gaps), dim3(256), 0, ctx->stream, (const uint8_t*)d_asm_pool, (const uint64_t*)d_asm_off,
                           sizes, off, rb, (uint8_t*)d_pool, st, live);
        hipLaunchKernelGGL(rn_copy_recruits_kernel, dim3(r2_grid(ctx, key_cap * 2ull * rb)), dim3(256), 0, ctx->stream, sorted, (uint64_t)key_cap, flag,
                           uidx, start, (const uint64_t*)d_asm_off, sizes, off, libs, rb, (uint8_t*)d_pool, st, live);
    }
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // extern "C"
