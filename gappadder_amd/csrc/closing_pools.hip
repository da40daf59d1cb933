// closing_pools.hip — the closing pools of the device step: after the last recruitment round, for every CLOSED gap the
// rows the step's first assembly saw followed by the reads of every pair recruited for the gap, in (library, pair) order, each pair once —
// the pool the closing round assembled from, rebuilt for the rounds that look at the closed fills.  An open gap gets an empty pool.
//   bounds   per gap the first and one past the last index, in the distinct-key list, of its keys (of the one library, with a filter): read
//            off the sorted keys and the flag scan the last pools call left (round2.hip / round_n.hip: flag, uidx), no atomics
//   sizes    rows per closed gap = source rows + 2 * keys; rocprim's exclusive scan; the offsets, or all zero beyond the capacity
//   gather   a workgroup per gap copies its source rows, masks and ids as one contiguous block; half a wave per distinct key copies the
//            pair's two rows (adjacent in the library: 2 * row bytes from a 4-byte-aligned address), its masks and its ids.  Rows are 38
//            bytes at 150 bases, so a block starts on an even byte: dwords where source and destination agree mod 4, else halfwords
// Memory-bound copies; no kernel here writes a row with an atomic.
#include <rocprim/device/device_scan.hpp>

#include "gf_internal.hpp"
#include "round2_dev.hpp"

namespace gf {

namespace {

struct CpLibs {
    const uint8_t* reads[GF_R2_MAX_LIBS];
    const uint32_t* nmask[GF_R2_MAX_LIBS];
};

enum : uint32_t { CP_ROWS = 0 /* u64 */, CP_GAPS = 2, CP_RECRUITED = 3, CP_OVF = 4 };

// the group a key's run is counted in: its gap, or its (gap, library)
__device__ __forceinline__ unsigned long long cp_group(unsigned long long x, int filter) { return filter < 0 ? x >> 40 : x >> 36; }

template <typename T>
__device__ __forceinline__ void cp_copy_as(uint8_t* dst, const uint8_t* src, uint64_t n, uint32_t lane, uint32_t lanes) {
    const uint64_t head = min(n, (uint64_t)((sizeof(T) - ((uintptr_t)dst & (sizeof(T) - 1))) & (sizeof(T) - 1)));
    for (uint64_t b = lane; b < head; b += lanes) dst[b] = src[b];
    const uint64_t units = (n - head) / sizeof(T);
    const T* s = (const T*)(src + head);
    T* d = (T*)(dst + head);
    for (uint64_t u = lane; u < units; u += lanes) d[u] = s[u];
    for (uint64_t b = head + units * sizeof(T) + lane; b < n; b += lanes) dst[b] = src[b];
}

// n bytes by `lanes` lanes, in the widest unit of 4, 2, 1 bytes at which source and destination are aligned alike
__device__ __forceinline__ void cp_copy(uint8_t* dst, const uint8_t* src, uint64_t n, uint32_t lane, uint32_t lanes) {
    const uintptr_t x = (uintptr_t)dst ^ (uintptr_t)src;
    if ((x & 3u) == 0) cp_copy_as<uint32_t>(dst, src, n, lane, lanes);
    else if ((x & 1u) == 0) cp_copy_as<uint16_t>(dst, src, n, lane, lanes);
    else cp_copy_as<uint8_t>(dst, src, n, lane, lanes);
}

// first[g], end[g] (zeroed before): the run of gap g's keys (of library `filter`) in the distinct list; closed gaps only
__global__ __launch_bounds__(256) void cp_bounds_kernel(const unsigned long long* s, uint64_t n, uint64_t n_gaps, const uint32_t* flag,
                                                        const uint32_t* uidx, const uint64_t* best, int filter, uint32_t* first, uint32_t* end) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long x = s[i];
        const uint32_t g = key_gap(x);
        if (x == R2_EMPTY_KEY || g >= n_gaps || best[g] == 0) continue;
        if (filter >= 0 && (int)((x >> 36) & (GF_R2_MAX_LIBS - 1)) != filter) continue;
        const unsigned long long grp = cp_group(x, filter);
        if (i == 0 || cp_group(s[i - 1], filter) != grp) first[g] = uidx[i];                       // (the first of a run is a distinct key)
        if (i + 1 == n || cp_group(s[i + 1], filter) != grp) end[g] = uidx[i] + flag[i];         // (distinct keys up to and with i)
    }
}

__global__ __launch_bounds__(256) void cp_sizes_kernel(const uint64_t* src_off, const uint64_t* best, uint64_t n_gaps, const uint32_t* first,
                                                       const uint32_t* end, uint64_t* rows, uint32_t* stats) {
    uint32_t gaps = 0, recruited = 0;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g <= n_gaps; g += (uint64_t)gridDim.x * blockDim.x) {
        if (g == n_gaps || best[g] == 0) { rows[g] = 0; continue; }
        const uint64_t r = (src_off[g + 1] - src_off[g]) + 2ull * (end[g] - first[g]);
        rows[g] = r;
        gaps += r != 0;
        recruited += 2u * (end[g] - first[g]);
    }
    if (gaps) atomicAdd(stats + CP_GAPS, gaps);
    if (recruited) atomicAdd(stats + CP_RECRUITED, recruited);
}

// scan: the rows' exclusive scan; the offsets are it, or all zero when the total is beyond the capacity
__global__ __launch_bounds__(256) void cp_offsets_kernel(const uint64_t* scan, uint64_t n_gaps, uint64_t pool_cap, uint64_t* off, uint32_t* stats) {
    const uint64_t tot = scan[n_gaps];
    const bool ovf = tot > pool_cap;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g <= n_gaps; g += (uint64_t)gridDim.x * blockDim.x) off[g] = ovf ? 0ull : scan[g];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[CP_ROWS] = (uint32_t)tot;
        stats[CP_ROWS + 1] = (uint32_t)(tot >> 32);
        stats[CP_OVF] = ovf;
        if (ovf) stats[CP_GAPS] = stats[CP_RECRUITED] = 0;       // (every pool is left empty)
    }
}

// a workgroup per closed gap: its source rows, their masks (zero where the source has none), ids and library to the pool's head
__global__ __launch_bounds__(256) void cp_gather_source_kernel(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_nmask,
                                                               const uint32_t* src_ids, uint32_t src_lib, const uint64_t* best, uint64_t n_gaps,
                                                               const uint64_t* off, uint32_t rb, uint32_t mw, uint8_t* pool, uint32_t* nmask,
                                                               uint32_t* ids, uint8_t* lib, const uint32_t* stats) {
    if (stats[CP_OVF]) return;
    for (uint64_t g = blockIdx.x; g < n_gaps; g += gridDim.x) {
        if (best[g] == 0) continue;
        const uint64_t s0 = src_off[g], n = src_off[g + 1] - s0, d0 = off[g];      // (d0 + n <= off[g + 1] <= pool_cap)
        cp_copy(pool + d0 * rb, src + s0 * rb, n * rb, threadIdx.x, blockDim.x);
        if (nmask)
            for (uint64_t w = threadIdx.x; w < n * mw; w += blockDim.x) nmask[d0 * mw + w] = src_nmask ? src_nmask[s0 * mw + w] : 0u;
        if (ids)
            for (uint64_t r = threadIdx.x; r < n; r += blockDim.x) ids[d0 + r] = src_ids ? src_ids[s0 + r] : 0xFFFFFFFFu;
        if (lib)
            for (uint64_t r = threadIdx.x; r < n; r += blockDim.x) lib[d0 + r] = (uint8_t)src_lib;
    }
}

// half a wave per distinct key of a closed gap: the pair's two rows behind the gap's source rows, with masks, ids and library
__global__ __launch_bounds__(256) void cp_gather_recruits_kernel(const unsigned long long* s, uint64_t n, uint64_t n_gaps, const uint32_t* flag,
                                                                 const uint32_t* uidx, const uint32_t* first, const uint64_t* src_off,
                                                                 const uint64_t* best, int filter, const uint64_t* off, CpLibs libs, uint32_t rb,
                                                                 uint32_t mw, uint8_t* pool, uint32_t* nmask, uint32_t* ids, uint8_t* lib,
                                                                 const uint32_t* stats) {
    if (stats[CP_OVF]) return;
    const uint32_t lane = threadIdx.x & 31u;
    const uint64_t groups = ((uint64_t)gridDim.x * blockDim.x) >> 5;
    for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 5; i < n; i += groups) {
        if (!flag[i]) continue;                                   // (a flagged key is not the empty key and its gap is < n_gaps)
        const unsigned long long x = s[i];
        const uint32_t g = key_gap(x), l = (uint32_t)(x >> 36) & (GF_R2_MAX_LIBS - 1);
        if (best[g] == 0 || (filter >= 0 && (int)l != filter) || !libs.reads[l]) continue;
        const uint64_t pair = x & ((1ull << 36) - 1);
        // first[g] <= uidx[i] < end[g], so the two rows lie in [off[g], off[g + 1])
        const uint64_t row = off[g] + (src_off[g + 1] - src_off[g]) + 2ull * (uidx[i] - first[g]);
        cp_copy(pool + row * rb, libs.reads[l] + 2 * pair * rb, 2ull * rb, lane, 32u);
        if (nmask)
            for (uint32_t w = lane; w < 2u * mw; w += 32u) nmask[row * mw + w] = libs.nmask[l] ? libs.nmask[l][2 * pair * mw + w] : 0u;
        if (ids && lane < 2u) ids[row + lane] = (uint32_t)(2 * pair + lane);
        if (lib && lane < 2u) lib[row + lane] = (uint8_t)l;
    }
}

}  // namespace
}  // namespace gf

using namespace gf;

extern "C" {

size_t gf_closing_pools_work_words(size_t n_gaps) { return 2 * n_gaps + 4 * (n_gaps + 1) + 2; }

int gf_closing_pools_dev(gf_ctx* ctx, const void* d_keys_sorted, const void* d_round_work, size_t key_cap, const void* const* d_lib_reads,
                         const void* const* d_lib_nmask_or_null, int n_lib, int lib_filter, int read_len, const void* d_src_pool,
                         const void* d_src_off, const void* d_src_nmask_or_null, const void* d_src_ids_or_null, int src_lib, const void* d_gap_best,
                         size_t n_gaps, void* d_work, void* d_off, void* d_pool, size_t pool_cap, void* d_nmask_or_null, void* d_ids_or_null,
                         void* d_lib_or_null, void* d_stats) {
    if (!ctx || !d_keys_sorted || !d_round_work || !d_lib_reads || !d_src_off || !d_gap_best || !d_work || !d_off || !d_stats ||
        (pool_cap && (!d_pool || !d_src_pool)) || read_len < 1)
        return GF_E_INVAL;
    if (n_lib < 1 || n_lib > GF_R2_MAX_LIBS || lib_filter < -1 || lib_filter >= n_lib || n_gaps == 0 || n_gaps >= (1ull << 24) - 1 || key_cap == 0 ||
        key_cap > 0xFFFFFFFFull)
        return GF_E_UNSUPPORTED;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    CpLibs libs{};
    for (int l = 0; l < n_lib; ++l) {
        if (!d_lib_reads[l]) return GF_E_INVAL;
        libs.reads[l] = (const uint8_t*)d_lib_reads[l];
        libs.nmask[l] = d_lib_nmask_or_null ? (const uint32_t*)d_lib_nmask_or_null[l] : nullptr;
    }
    const uint32_t rb = (uint32_t)gf_packed_read_bytes(read_len), mw = (uint32_t)((read_len + 31) / 32);
    const unsigned long long* sorted = (const unsigned long long*)d_keys_sorted;
    const uint32_t* flag = (const uint32_t*)d_round_work;       // gf_round2_pools_dev's / gf_round_pools_dev's layout of their d_work
    const uint32_t* uidx = flag + key_cap;
    uint32_t* first = (uint32_t*)d_work;                        // [n_gaps] a gap's first index in the distinct list
    uint32_t* end = first + n_gaps;                             // [n_gaps] one past its last
    uint64_t* sizes = (uint64_t*)(end + n_gaps + (n_gaps & 1)); // [n_gaps + 1] rows per gap (8-byte aligned: 2 * n_gaps words, + 1 when odd)
    uint64_t* scan = sizes + n_gaps + 1;                        // [n_gaps + 1] their exclusive scan
    const uint64_t* best = (const uint64_t*)d_gap_best;
    const uint64_t* src_off = (const uint64_t*)d_src_off;
    uint32_t* st = (uint32_t*)d_stats;
    size_t t_scan = 0;
    GF_HIP(ctx, rocprim::exclusive_scan(nullptr, t_scan, sizes, scan, (uint64_t)0, n_gaps + 1, rocprim::plus<uint64_t>(), ctx->stream));
    int rc;
    if ((rc = ensure(ctx, ctx->r2_tmp, t_scan + 64))) return rc;
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    GF_HIP(ctx, hipMemsetAsync(st, 0, 4 * GF_CP_WORDS, ctx->stream));
    GF_HIP(ctx, hipMemsetAsync(first, 0, 8 * n_gaps, ctx->stream));
    const unsigned gk = r2_grid(ctx, key_cap), gg = r2_grid(ctx, n_gaps + 1);
    hipLaunchKernelGGL(cp_bounds_kernel, dim3(gk), dim3(256), 0, ctx->stream, sorted, (uint64_t)key_cap, (uint64_t)n_gaps, flag, uidx, best, lib_filter,
                       first, end);
    hipLaunchKernelGGL(cp_sizes_kernel, dim3(gg), dim3(256), 0, ctx->stream, src_off, best, (uint64_t)n_gaps, first, end, sizes, st);
    GF_HIP(ctx, rocprim::exclusive_scan(ctx->r2_tmp.p, t_scan, sizes, scan, (uint64_t)0, n_gaps + 1, rocprim::plus<uint64_t>(), ctx->stream));
    hipLaunchKernelGGL(cp_offsets_kernel, dim3(gg), dim3(256), 0, ctx->stream, scan, (uint64_t)n_gaps, (uint64_t)pool_cap, (uint64_t*)d_off, st);
    if (pool_cap) {
        hipLaunchKernelGGL(cp_gather_source_kernel, dim3((unsigned)std::min<uint64_t>(n_gaps, (uint64_t)ctx->n_cu * 16)), dim3(256), 0, ctx->stream,
                           (const uint8_t*)d_src_pool, src_off, (const uint32_t*)d_src_nmask_or_null, (const uint32_t*)d_src_ids_or_null,
                           (uint32_t)src_lib, best, (uint64_t)n_gaps, (const uint64_t*)d_off, rb, mw, (uint8_t*)d_pool, (uint32_t*)d_nmask_or_null,
                           (uint32_t*)d_ids_or_null, (uint8_t*)d_lib_or_null, st);
        hipLaunchKernelGGL(cp_gather_recruits_kernel, dim3(r2_grid(ctx, key_cap * 32ull)), dim3(256), 0, ctx->stream, sorted, (uint64_t)key_cap,
                           (uint64_t)n_gaps, flag, uidx, first, src_off, best, lib_filter, (const uint64_t*)d_off, libs, rb, mw, (uint8_t*)d_pool,
                           (uint32_t*)d_nmask_or_null, (uint32_t*)d_ids_or_null, (uint8_t*)d_lib_or_null, st);
    }
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // extern "C"
