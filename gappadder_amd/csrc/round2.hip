// round2.hip — the reference's second assembly round inside the device step (assemble_gaps.py:328-368, collect_both_unmapped_reads.py):
// for every gap the first pick leaves open, the pairs whose mates are BOTH unmapped (FLAG & 12 == 12) and that share a canonical k-mer
// with the gap's round-1 contigs are appended to the gap's pool, and the gap is assembled and picked again.  The predicate is the CLI's
// (collect_both_unmapped_reads.kmer_recruit_unmapped): at least one canonical k-mer in common, k-mers touching a non-ACGT contig base or an
// N-masked read base do not count, a hit recruits the read and its mate.
//   candidates  one bit per pair (atomicOr: a pair is listed once however many of its records carry the flags) -> pair ids
//   table       open addressing on (k-mer, gap): the probe sequence starts at the k-mer's hash, so every gap of a k-mer lies on one chain
//               that a look-up walks to the first empty slot.  A slot is claimed by one CAS on its state word (0 empty, 1 being written,
//               2 written); an inserter that meets a slot in state 1 reads it again in its next loop turn (no spin inside a branch: the
//               writing lane of the same wave finishes in the same turn)
//   recruit     one thread per candidate read: rolling forward / reverse 128-bit k-mers, the N mask as a run length, look-ups; the last
//               four gaps a read emitted are skipped locally, the rest is deduplicated by the sort
//   pools       keys gap << 40 | library << 36 | pair, radix-sorted: (gap, library, pair) order = the round-2 pool order after the gap's
//               round-1 rows; unique flags + scan give every recruited pair its row
//   append      round-2 contigs (assembled into buffers of their own) go after the round-1 contigs of the step's list
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gf_internal.hpp"
#include "round2_dev.hpp"

namespace gf {

namespace {

__global__ __launch_bounds__(256) void r2_candidates_kernel(const uint32_t* recs, uint64_t n_recs, uint64_t n_reads, uint32_t* bits,
                                                            uint32_t* out, uint64_t cap, uint32_t* n_out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_recs; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t* r = recs + 8 * i;
        if ((r[5] & 12u) != 12u) continue;                       // FLAG (low 16 bits of word 5): both mates unmapped
        const uint64_t read = (uint64_t)r[6] | ((uint64_t)r[7] << 32);
        if ((read | 1ull) >= n_reads) continue;                  // (a record of a read this array does not hold, or a mate beyond its end)
        const uint32_t pair = (uint32_t)(read >> 1), bit = 1u << (pair & 31);
        if (atomicOr(bits + (pair >> 5), bit) & bit) continue;
        const uint32_t j = atomicAdd(n_out, 1u);
        if (j < cap) out[j] = pair;
    }
}

__global__ __launch_bounds__(256) void r2_table_kernel(const gf_contig* ctg, const uint32_t* d_n, uint64_t ctg_cap, const char* seq,
                                                       const uint64_t* best, uint64_t n_gaps, int k, R2Slot* tab, uint32_t log2,
                                                       uint32_t* stats) {
    const uint64_t n1 = min((uint64_t)*d_n, ctg_cap);
    uint32_t mine = 0;
    for (uint64_t c = blockIdx.x; c < n1; c += gridDim.x) {
        const gf_contig C = ctg[c];
        if (C.gap >= n_gaps || best[C.gap] != 0 || C.length < (uint32_t)k) continue;    // (uniform in the block)
        const char* s = seq + C.seq_off;
        for (uint32_t p = threadIdx.x; p + k <= C.length; p += blockDim.x) {
            K128 v{0, 0};
            bool ok = true;
            for (int j = 0; j < k; ++j) {
                const char ch = s[p + j];
                ok = ok && r2_acgt(ch);
                const uint64_t b = base_code(ch);
                if (j < 32) v.hi |= b << (62 - 2 * j);
                else v.lo |= b << (62 - 2 * (j - 32));
            }
            if (!ok) continue;
            ++mine;
            r2_insert(tab, log2, canonical(v, k), C.gap, stats + R2_TAB_FULL);
        }
    }
    if (mine) atomicAdd(stats + R2_KMERS, mine);
}

// right-aligned 128-bit k-mer arithmetic of the rolling recruitment
struct R128 {
    uint64_t hi, lo;
};
__device__ __forceinline__ bool r128_less(const R128& a, const R128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

__global__ __launch_bounds__(256) void r2_recruit_kernel(const uint8_t* reads, const uint32_t* nmask, uint32_t L, uint32_t rb, uint32_t nmw,
                                                         const uint32_t* pairs, const uint32_t* d_np, uint64_t pair_cap, uint32_t lib, int k,
                                                         const R2Slot* tab, uint32_t log2, unsigned long long* keys, uint64_t key_cap,
                                                         uint32_t* stats) {
    const uint64_t np = min((uint64_t)*d_np, pair_cap);
    const uint32_t mask = (uint32_t)((1ull << log2) - 1);
    const int kb = 2 * k;
    const uint64_t mhi = kb >= 128 ? ~0ull : (kb > 64 ? (1ull << (kb - 64)) - 1 : 0ull);
    const uint64_t mlo = kb >= 64 ? ~0ull : (1ull << kb) - 1;
    const int sh = 128 - kb;    // left alignment
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < 2 * np; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t pair = pairs[t >> 1], read = 2 * pair + (t & 1);
        const uint8_t* row = reads + read * rb;
        const uint32_t* mrow = nmask ? nmask + read * nmw : nullptr;
        R128 f{0, 0}, r{0, 0};
        uint32_t run = 0, seen[4] = {~0u, ~0u, ~0u, ~0u}, ns = 0;
        uint32_t byte = 0;
        for (uint32_t i = 0; i < L; ++i) {
            if ((i & 3) == 0) byte = row[i >> 2];
            const uint64_t b = (byte >> (6 - 2 * (i & 3))) & 3u;
            const bool masked = mrow && ((mrow[i >> 5] >> (i & 31)) & 1u);
            f.hi = ((f.hi << 2) | (f.lo >> 62)) & mhi;
            f.lo = ((f.lo << 2) | b) & mlo;
            r.lo = (r.lo >> 2) | (r.hi << 62);
            r.hi >>= 2;
            if (kb - 2 >= 64) r.hi |= (3u - b) << (kb - 2 - 64);
            else r.lo |= (3u - b) << (kb - 2);
            run = masked ? 0 : run + 1;
            if (run < (uint32_t)k) continue;
            const R128 c = r128_less(r, f) ? r : f;
            K128 v;
            if (sh == 0) { v.hi = c.hi; v.lo = c.lo; }
            else if (sh < 64) { v.hi = (c.hi << sh) | (c.lo >> (64 - sh)); v.lo = c.lo << sh; }
            else if (sh == 64) { v.hi = c.lo; v.lo = 0; }
            else { v.hi = c.lo << (sh - 64); v.lo = 0; }
            uint32_t pos = hash_kmer(v, (int)log2);
            for (uint64_t probes = 0; probes <= mask; ++probes) {
                const R2Slot& s = tab[pos];
                if (s.state == 0u) break;
                if (s.hi == v.hi && s.lo == v.lo) {
                    const uint32_t g = s.gap;
                    if (g != seen[0] && g != seen[1] && g != seen[2] && g != seen[3]) {
                        seen[ns & 3] = g;
                        ++ns;
                        const uint32_t j = atomicAdd(stats + R2_HITS, 1u);
                        if (j < key_cap) keys[j] = ((unsigned long long)g << 40) | ((unsigned long long)lib << 36) | pair;
                    }
                }
                pos = (pos + 1) & mask;
            }
        }
    }
}

__global__ __launch_bounds__(256) void r2_mark_kernel(const unsigned long long* s, uint64_t n, uint64_t n_gaps, uint32_t* flag, uint32_t* cnt) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long x = s[i];
        const bool u = x != R2_EMPTY_KEY && key_gap(x) < n_gaps && (i == 0 || s[i - 1] != x);
        flag[i] = u;
        if (u) atomicAdd(cnt + key_gap(x), 1u);
    }
}

__global__ __launch_bounds__(256) void r2_start_kernel(const unsigned long long* s, uint64_t n, uint64_t n_gaps, const uint32_t* flag,
                                                       const uint32_t* uidx, uint32_t* start) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (flag[i] && (i == 0 || key_gap(s[i - 1]) != key_gap(s[i]))) start[key_gap(s[i])] = uidx[i];
}

__global__ __launch_bounds__(256) void r2_sizes_kernel(const uint64_t* asm_off, const uint64_t* best, uint64_t n_gaps, const uint32_t* cnt,
                                                       uint64_t* rows, uint32_t* stats) {
    uint32_t tried = 0, with = 0, uni = 0;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g <= n_gaps; g += (uint64_t)gridDim.x * blockDim.x) {
        if (g == n_gaps) { rows[g] = 0; continue; }
        const uint32_t c = cnt[g];
        tried += best[g] == 0;
        with += c != 0;
        uni += c;
        rows[g] = c ? (asm_off[g + 1] - asm_off[g]) + 2ull * c : 0ull;
    }
    if (tried) atomicAdd(stats + R2_TRIED, tried);
    if (with) atomicAdd(stats + R2_WITH, with);
    if (uni) atomicAdd(stats + R2_UNIQUE, uni);
}

__global__ void r2_total_kernel(const uint64_t* off, uint64_t n_gaps, uint64_t pool_cap, uint32_t* stats) {
    const uint64_t tot = off[n_gaps];
    stats[R2_ROWS] = (uint32_t)tot;
    stats[R2_ROWS + 1] = (uint32_t)(tot >> 32);
    stats[R2_POOL_OVF] = tot > pool_cap;
}

__global__ __launch_bounds__(256) void r2_clear_off_kernel(uint64_t* off, uint64_t n_gaps, const uint32_t* stats) {
    if (!stats[R2_POOL_OVF]) return;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g <= n_gaps; g += (uint64_t)gridDim.x * blockDim.x) off[g] = 0;
}

// one workgroup per gap: its round-1 rows to the head of its round-2 pool
__global__ __launch_bounds__(256) void r2_copy_round1_kernel(const uint8_t* asm_pool, const uint64_t* asm_off, const uint32_t* cnt, const uint64_t* off,
                                                             uint32_t rb, uint8_t* pool, const uint32_t* stats) {
    const uint32_t g = blockIdx.x;
    if (!cnt[g] || stats[R2_POOL_OVF]) return;
    const uint64_t n = (asm_off[g + 1] - asm_off[g]) * rb;
    const uint8_t* src = asm_pool + asm_off[g] * rb;
    uint8_t* dst = pool + off[g] * rb;
    for (uint64_t b = threadIdx.x; b < n; b += blockDim.x) dst[b] = src[b];
}

// every recruited pair: its two rows (adjacent in the library: reads 2p, 2p + 1) behind the gap's round-1 rows
__global__ __launch_bounds__(256) void r2_copy_recruits_kernel(const unsigned long long* s, uint64_t n, const uint32_t* flag, const uint32_t* uidx,
                                                               const uint32_t* start, const uint64_t* asm_off, const uint64_t* off, LibRows libs,
                                                               uint32_t rb, uint8_t* pool, const uint32_t* stats) {
    if (stats[R2_POOL_OVF]) return;
    const uint64_t per = 2ull * rb;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < n * per; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = t / per, b = t - i * per;
        if (!flag[i]) continue;
        const unsigned long long x = s[i];
        const uint32_t g = key_gap(x), lib = (uint32_t)(x >> 36) & (GF_R2_MAX_LIBS - 1);
        const uint64_t pair = x & ((1ull << 36) - 1);
        if (!libs.reads[lib]) continue;
        const uint64_t row = off[g] + (asm_off[g + 1] - asm_off[g]) + 2ull * (uidx[i] - start[g]);
        pool[row * rb + b] = libs.reads[lib][2 * pair * rb + b];
    }
}

__global__ __launch_bounds__(256) void r2_append_kernel(gf_contig* dst, const uint32_t* d_n1, uint64_t dst_cap, char* dst_seq, const uint64_t* d_s1,
                                                        uint64_t dst_seq_cap, const gf_contig* src, const uint32_t* d_n2, uint64_t src_cap,
                                                        const char* src_seq, const uint64_t* d_s2, uint64_t src_seq_cap) {
    const uint64_t n1 = *d_n1, s1 = *d_s1, n2 = *d_n2, s2 = *d_s2;
    if (n2 > src_cap || s2 > src_seq_cap || n1 + n2 > dst_cap || s1 + s2 > dst_seq_cap) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n2; i += stride) {
        gf_contig c = src[i];
        c.seq_off += s1;
        dst[n1 + i] = c;
    }
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < s2; i += stride) dst_seq[s1 + i] = src_seq[i];
}

__global__ void r2_append_counts_kernel(uint32_t* d_n1, uint64_t dst_cap, uint64_t* d_s1, uint64_t dst_seq_cap, const uint32_t* d_n2, uint64_t src_cap,
                                        const uint64_t* d_s2, uint64_t src_seq_cap, uint32_t* stats) {
    const uint64_t n1 = *d_n1, s1 = *d_s1, n2 = *d_n2, s2 = *d_s2;
    stats[R2_FIRST] = (uint32_t)n1;
    if (n2 > src_cap || s2 > src_seq_cap || n1 + n2 > dst_cap || s1 + s2 > dst_seq_cap) {
        stats[R2_APPEND_ERR] = 1;
        stats[R2_N2] = (uint32_t)n2;
        return;
    }
    *d_n1 = (uint32_t)(n1 + n2);
    *d_s1 = s1 + s2;
    stats[R2_N2] = (uint32_t)n2;
}

}  // namespace
}  // namespace gf

using namespace gf;

extern "C" {

int gf_both_unmapped_reads_dev(gf_ctx* ctx, const void* d_recs, size_t n_recs, size_t n_reads, void* d_pair_bits, void* d_pairs, size_t cap,
                               void* d_n_pairs) {
    if (!ctx || (n_recs && !d_recs) || !d_n_pairs || (n_reads && !d_pair_bits) || (cap && !d_pairs)) return GF_E_INVAL;
    if (n_reads > (1ull << 33)) return GF_E_UNSUPPORTED;     // (pair ids are 32-bit)
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(d_n_pairs, 0, 4, ctx->stream));
    if (!n_reads || !n_recs) return GF_OK;
    GF_HIP(ctx, hipMemsetAsync(d_pair_bits, 0, ((n_reads / 2 + 31) / 32) * 4, ctx->stream));
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    hipLaunchKernelGGL(r2_candidates_kernel, dim3(r2_grid(ctx, n_recs)), dim3(256), 0, ctx->stream, (const uint32_t*)d_recs, (uint64_t)n_recs,
                       (uint64_t)n_reads, (uint32_t*)d_pair_bits, (uint32_t*)d_pairs, (uint64_t)cap, (uint32_t*)d_n_pairs);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_contig_kmer_table_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, const void* d_gap_best,
                             size_t n_gaps, int k, void* d_table, int log2_slots, void* d_stats) {
    if (!ctx || !d_contigs || !d_n_contigs || !d_seq || !d_gap_best || !d_table || !d_stats) return GF_E_INVAL;
    if (k < 16 || k > 64 || log2_slots < 4 || log2_slots > 32 || n_gaps >= (1ull << 24) - 1) return GF_E_UNSUPPORTED;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(d_table, 0, (size_t)sizeof(R2Slot) << log2_slots, ctx->stream));
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    hipLaunchKernelGGL(r2_table_kernel, dim3((unsigned)ctx->n_cu * 8), dim3(256), 0, ctx->stream, (const gf_contig*)d_contigs,
                       (const uint32_t*)d_n_contigs, (uint64_t)contig_cap, (const char*)d_seq, (const uint64_t*)d_gap_best, (uint64_t)n_gaps, k,
                       (R2Slot*)d_table, (uint32_t)log2_slots, (uint32_t*)d_stats);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_recruit_by_contigs_dev(gf_ctx* ctx, const void* d_reads, const void* d_nmask_or_null, size_t n_reads, int read_len, const void* d_pairs,
                              const void* d_n_pairs, size_t pair_cap, int lib, int k, const void* d_table, int log2_slots, void* d_keys,
                              size_t key_cap, void* d_stats) {
    if (!ctx || !d_n_pairs || !d_table || !d_stats || (key_cap && !d_keys) || (pair_cap && (!d_pairs || !d_reads))) return GF_E_INVAL;
    if (k < 16 || k > 64 || read_len < 1 || log2_slots < 4 || log2_slots > 32 || lib < 0 || lib >= GF_R2_MAX_LIBS) return GF_E_UNSUPPORTED;
    if (!pair_cap || read_len < k) return GF_OK;
    (void)n_reads;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    LaunchTimer tm(ctx, GF_KERNEL_SCREEN);
    hipLaunchKernelGGL(r2_recruit_kernel, dim3(r2_grid(ctx, 2 * (uint64_t)pair_cap)), dim3(256), 0, ctx->stream, (const uint8_t*)d_reads,
                       (const uint32_t*)d_nmask_or_null, (uint32_t)read_len, (uint32_t)gf_packed_read_bytes(read_len), (uint32_t)((read_len + 31) / 32),
                       (const uint32_t*)d_pairs, (const uint32_t*)d_n_pairs, (uint64_t)pair_cap, (uint32_t)lib, k, (const R2Slot*)d_table,
                       (uint32_t)log2_slots, (unsigned long long*)d_keys, (uint64_t)key_cap, (uint32_t*)d_stats);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

size_t gf_round2_work_words(size_t key_cap, size_t n_gaps) { return 2 * key_cap + 2 * n_gaps + 2; }

int gf_round2_pools_dev(gf_ctx* ctx, void* d_keys, void* d_keys_sorted, size_t key_cap, const void* const* d_lib_reads, int n_lib, int read_len,
                        const void* d_asm_pool, const void* d_asm_off, const void* d_gap_best, size_t n_gaps, void* d_work, void* d_rows,
                        void* d_pool, size_t pool_cap, void* d_stats) {
    if (!ctx || !d_keys || !d_keys_sorted || !d_lib_reads || !d_asm_off || !d_gap_best || !d_work || !d_rows || !d_stats ||
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
    unsigned long long* keys = (unsigned long long*)d_keys;
    unsigned long long* sorted = (unsigned long long*)d_keys_sorted;
    uint32_t* flag = (uint32_t*)d_work;                 // [key_cap] unique flags
    uint32_t* uidx = flag + key_cap;                    // [key_cap] their exclusive scan
    uint32_t* cnt = uidx + key_cap;                     // [n_gaps] distinct recruited pairs per gap
    uint32_t* start = cnt + n_gaps;                     // [n_gaps] the gap's first index in the unique list
    uint64_t* sizes = (uint64_t*)d_rows;                // [n_gaps + 1] round-2 rows per gap
    uint64_t* off = sizes + n_gaps + 1;                 // [n_gaps + 1] their exclusive scan: the pool offsets
    uint32_t* st = (uint32_t*)d_stats;
    size_t t_sort = 0, t_scan32 = 0, t_scan64 = 0;
    GF_HIP(ctx, rocprim::radix_sort_keys(nullptr, t_sort, keys, sorted, key_cap, 0, 64, ctx->stream));
    GF_HIP(ctx, rocprim::exclusive_scan(nullptr, t_scan32, flag, uidx, 0u, key_cap, rocprim::plus<uint32_t>(), ctx->stream));
    GF_HIP(ctx, rocprim::exclusive_scan(nullptr, t_scan64, sizes, off, (uint64_t)0, n_gaps + 1, rocprim::plus<uint64_t>(), ctx->stream));
    int rc;
    if ((rc = ensure(ctx, ctx->r2_tmp, std::max(t_sort, std::max(t_scan32, t_scan64)) + 64))) return rc;
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    GF_HIP(ctx, rocprim::radix_sort_keys(ctx->r2_tmp.p, t_sort, keys, sorted, key_cap, 0, 64, ctx->stream));
    GF_HIP(ctx, hipMemsetAsync(cnt, 0, 2 * n_gaps * 4, ctx->stream));
    const unsigned gk = r2_grid(ctx, key_cap), gg = r2_grid(ctx, n_gaps + 1);
    hipLaunchKernelGGL(r2_mark_kernel, dim3(gk), dim3(256), 0, ctx->stream, sorted, (uint64_t)key_cap, (uint64_t)n_gaps, flag, cnt);
    GF_HIP(ctx, rocprim::exclusive_scan(ctx->r2_tmp.p, t_scan32, flag, uidx, 0u, key_cap, rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(r2_start_kernel, dim3(gk), dim3(256), 0, ctx->stream, sorted, (uint64_t)key_cap, (uint64_t)n_gaps, flag, uidx, start);
    hipLaunchKernelGGL(r2_sizes_kernel, dim3(gg), dim3(256), 0, ctx->stream, (const uint64_t*)d_asm_off, (const uint64_t*)d_gap_best, (uint64_t)n_gaps,
                       cnt, sizes, st);
    GF_HIP(ctx, rocprim::exclusive_scan(ctx->r2_tmp.p, t_scan64, sizes, off, (uint64_t)0, n_gaps + 1, rocprim::plus<uint64_t>(), ctx->stream));
    hipLaunchKernelGGL(r2_total_kernel, dim3(1), dim3(1), 0, ctx->stream, off, (uint64_t)n_gaps, (uint64_t)pool_cap, st);
    hipLaunchKernelGGL(r2_clear_off_kernel, dim3(gg), dim3(256), 0, ctx->stream, off, (uint64_t)n_gaps, st);
    if (pool_cap) {
        hipLaunchKernelGGL(r2_copy_round1_kernel, dim3((unsigned)n_gaps), dim3(256), 0, ctx->stream, (const uint8_t*)d_asm_pool, (const uint64_t*)d_asm_off,
                           cnt, off, rb, (uint8_t*)d_pool, st);
        hipLaunchKernelGGL(r2_copy_recruits_kernel, dim3(r2_grid(ctx, key_cap * 2ull * rb)), dim3(256), 0, ctx->stream, sorted, (uint64_t)key_cap, flag,
                           uidx, start, (const uint64_t*)d_asm_off, off, libs, rb, (uint8_t*)d_pool, st);
    }
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_contigs_append_dev(gf_ctx* ctx, void* d_contigs, void* d_n_contigs, size_t contig_cap, void* d_seq, void* d_seq_len, size_t seq_cap,
                          const void* d_src_contigs, const void* d_src_n, size_t src_cap, const void* d_src_seq, const void* d_src_seq_len,
                          size_t src_seq_cap, void* d_stats) {
    if (!ctx || !d_contigs || !d_n_contigs || !d_seq || !d_seq_len || !d_src_contigs || !d_src_n || !d_src_seq || !d_src_seq_len || !d_stats)
        return GF_E_INVAL;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    hipLaunchKernelGGL(r2_append_kernel, dim3((unsigned)ctx->n_cu * 4), dim3(256), 0, ctx->stream, (gf_contig*)d_contigs, (const uint32_t*)d_n_contigs,
                       (uint64_t)contig_cap, (char*)d_seq, (const uint64_t*)d_seq_len, (uint64_t)seq_cap, (const gf_contig*)d_src_contigs,
                       (const uint32_t*)d_src_n, (uint64_t)src_cap, (const char*)d_src_seq, (const uint64_t*)d_src_seq_len, (uint64_t)src_seq_cap);
    hipLaunchKernelGGL(r2_append_counts_kernel, dim3(1), dim3(1), 0, ctx->stream, (uint32_t*)d_n_contigs, (uint64_t)contig_cap, (uint64_t*)d_seq_len,
                       (uint64_t)seq_cap, (const uint32_t*)d_src_n, (uint64_t)src_cap, (const uint64_t*)d_src_seq_len, (uint64_t)src_seq_cap,
                       (uint32_t*)d_stats);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // extern "C"
