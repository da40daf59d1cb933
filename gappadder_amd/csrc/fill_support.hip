// fill_support.hip — read support of the closed gaps: how the reads of a gap's own pool back the k-mers of the sequence the pick is
// about to insert (gf_fill_support_dev, include/gapfill_hip.h; definition and host twin: gappadder_amd/read_support.py).
// The reference has no such check: it writes whatever the first anchored contig carries.
//
// One workgroup of 256 threads per closed gap, grid-stride over the gaps.  A gap is opened by fill_round.hpp: open / mismatch / ok, the
// gap's pool rows and its body [b0, b1) on the winning contig — from the contig's gf_ctg_pick (align / gapped) or from re-locating the
// exact anchors by pick.hip's rule (fill_body.hpp); the launch is set up by fill_round_setup.  The evaluated windows (every k-window
// with a body base) are taken in chunks of FS_CHUNK, and per chunk:
//   build    the chunk's contig bytes are staged in LDS; every window's canonical k-mer goes into an exact-key open-addressed table in
//            LDS (FS_SLOTS = 2 x FS_CHUNK slots: load <= 1/2).  A slot is claimed by a 32-bit CAS on its OWNER word (window + 1); keys
//            are compared through the owners' keys, which lie in the first FS_CHUNK entries of the — still unused — key arrays; after a
//            barrier every owner writes its key (from registers) into its slot and zeroes the slot's counter.  No sentinel key: any
//            128-bit value is a legal key (k = 64 has a canonical k-mer of all ones in the high word)
//   count    the pool's packed rows are staged a batch at a time (aligned dword loads; the batch is one contiguous byte range; a loop of
//            its own, not fill_place.hpp's pl_stage_rows: this row buffer is FS_ROW_WORDS long and takes 6 zero tail words, not 8) and the
//            batch's read windows are dealt to the threads: stream_kmer / stream_kmer64, canonical, hash_kmer, probe; a hit is one LDS
//            atomicAdd, a miss — most windows — ends at the first free slot
//   reduce   every window looks its counter up (its slot stayed in a register); n_zero, n_below, min, max, sum by wave reduction and
//            LDS atomics; the zero run from 4-window segment summaries that thread 0 joins in order, the open run carried into the next
//            chunk
// A fill longer than a chunk costs one more pass over the pool per chunk, never a result.  Static LDS: 52.1 KB (k > 32: three workgroups per CU) / 36.1 KB (four).
#include <cstring>

#include "fill_body.hpp"
#include "fill_round.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t FS_THREADS = 256, FS_CHUNK = 1024, FS_PER = FS_CHUNK / FS_THREADS;
constexpr int FS_LOG2 = 11;
constexpr uint32_t FS_SLOTS = 1u << FS_LOG2, FS_SLOT_MASK = FS_SLOTS - 1;
constexpr uint32_t FS_ROW_BYTES = 2000, FS_ROW_WORDS = FS_ROW_BYTES / 4 + 8;   // a batch of rows (a row has at most 250 bytes) + misalignment + over-read
static_assert(FS_SLOTS == 2 * FS_CHUNK && FS_PER == 4, "fill support geometry");

struct FsParams {
    const uint8_t* pool;
    const uint32_t* nmask;       // or null
    FillRoundArgs round;
    uint32_t rb, L, nmw, batch_rows;
    uint32_t k, min_count;
    gf_fill_support* out;
};

template <bool W>
__global__ __launch_bounds__(FS_THREADS) void fill_support_kernel(FsParams P) {
    __shared__ uint64_t s_hi[FS_SLOTS];
    __shared__ uint64_t s_lo[W ? FS_SLOTS : 1];
    __shared__ uint32_t s_cnt[FS_SLOTS];
    __shared__ uint32_t s_own[FS_SLOTS];        // build + count: owner window + 1, 0 = free; reduce: the chunk's supports
    __shared__ uint32_t s_rows[FS_ROW_WORDS];
    __shared__ uint8_t s_ctg[FS_CHUNK + 64];
    __shared__ uint32_t s_seg[FS_THREADS];
    __shared__ uint32_t s_loc[2];
    __shared__ uint32_t s_acc[4];               // n_zero, n_below, min, max
    __shared__ unsigned long long s_sum;
    const uint32_t t = threadIdx.x, lane = t & 63, k = P.k;
    const uint32_t n = contig_list_end(P.round.body.list);
    const uint32_t nwin = P.L >= k ? P.L - k + 1 : 0;
    for (uint32_t g = blockIdx.x; g < P.round.n_gaps; g += gridDim.x) {
        gf_fill_support rec;
        rec.n_windows = rec.n_zero = rec.n_below = rec.min = rec.max = rec.zero_run = 0;
        rec.sum = 0;
        // ---- open / mismatch / ok, the body [b0, b1) on the winning contig, the gap's rows (fill_round.hpp; the same in all threads)
        const FillGap fg = fill_gap_open<FS_THREADS>(P.round, n, g, s_loc);
        if (fg.state == FILL_GAP_OPEN) {
            if (t == 0) P.out[g] = rec;
            continue;
        }
        if (fg.state == FILL_GAP_MISMATCH) {
            if (t == 0) {
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_FS_MISMATCH, 1u);
            }
            continue;
        }
        const gf_contig c = fg.fb.c;
        const char* s = P.round.body.list.seq + c.seq_off;
        const int64_t b0 = fg.fb.b0, b1 = fg.fb.b1;
        const FillRows rows = fill_gap_rows(P.round, g);
        const uint64_t r0 = rows.r0, r1 = rows.r1;
        int64_t w_lo = b0 - (int64_t)k + 1, w_hi = (b1 > b0 ? b1 : b0) - 1;
        if (w_lo < 0) w_lo = 0;
        if (w_hi > (int64_t)c.length - (int64_t)k) w_hi = (int64_t)c.length - (int64_t)k;
        const uint32_t n_windows = w_hi >= w_lo ? (uint32_t)(w_hi - w_lo + 1) : 0u;
        if (t == 0) {
            s_acc[0] = s_acc[1] = s_acc[3] = 0;
            s_acc[2] = EMPTY32;
            s_sum = 0;
        }
        uint32_t run = 0, best = 0;              // thread 0: the open zero run at the end of the last chunk, the longest so far
        for (uint32_t w0 = 0; w0 < n_windows; w0 += FS_CHUNK) {
            const uint32_t nw = n_windows - w0 < FS_CHUNK ? n_windows - w0 : FS_CHUNK;
            const char* cs = s + w_lo + w0;
            __syncthreads();                     // (the previous chunk's reduce)
            for (uint32_t i = t; i < nw + k - 1; i += FS_THREADS) s_ctg[i] = (uint8_t)cs[i];
            for (uint32_t i = t; i < FS_SLOTS; i += FS_THREADS) s_own[i] = 0;
            __syncthreads();
            // ---- build: keys of this thread's windows (window t + 256 j), parked in the key arrays' first FS_CHUNK entries
            K128 key[FS_PER];
            uint32_t slot[FS_PER];
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t j = 0; j < FS_PER; ++j) {
                const uint32_t i = t + j * FS_THREADS;
                slot[j] = EMPTY32;
                key[j].hi = key[j].lo = 0;
                if (i >= nw) continue;
                uint64_t hi = 0, lo = 0;
                bool good = true;
                for (uint32_t b = 0; b < k; ++b) {
                    const uint32_t code = base_code4(s_ctg[i + b]);
                    good = good && code < 4;
                    if (b < 32) hi |= (uint64_t)(code & 3) << (62 - 2 * b);
                    else lo |= (uint64_t)(code & 3) << (62 - 2 * (b - 32));
                }
                if (!good) continue;             // a byte that is no base: support 0, no table entry
                if constexpr (W) {
                    key[j] = canonical(K128{hi, lo}, (int)k);
                } else {
                    key[j].hi = canonical64(hi, (int)k);
                }
                slot[j] = 0;                     // (marks the window as keyed until the claim below sets its slot)
                s_hi[i] = key[j].hi;
                if constexpr (W) s_lo[i] = key[j].lo;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t j = 0; j < FS_PER; ++j) {
                if (slot[j] == EMPTY32) continue;
                const uint32_t i = t + j * FS_THREADS;
                uint32_t h = hash_kmer(key[j], FS_LOG2);
                for (;;) {
                    const uint32_t o = atomicCAS(&s_own[h], 0u, i + 1);
                    if (o == 0) { mine |= 1u << j; break; }
                    if (s_hi[o - 1] == key[j].hi && (!W || s_lo[W ? o - 1 : 0] == key[j].lo)) break;
                    h = (h + 1) & FS_SLOT_MASK;
                }
                slot[j] = h;
            }
            __syncthreads();                     // every claim is made: the parked keys are no longer read
#pragma unroll
            for (uint32_t j = 0; j < FS_PER; ++j) {
                if (!(mine >> j & 1u)) continue;
                s_hi[slot[j]] = key[j].hi;
                if constexpr (W) s_lo[slot[j]] = key[j].lo;
                s_cnt[slot[j]] = 0;
            }
            __syncthreads();
            // ---- count: the pool's rows, a batch at a time
            for (uint64_t row0 = r0; row0 < r1 && nwin; row0 += P.batch_rows) {
                const uint32_t nb = r1 - row0 < P.batch_rows ? (uint32_t)(r1 - row0) : P.batch_rows;
                const uint8_t* gp = P.pool + row0 * P.rb;
                const uint32_t mis = (uint32_t)((uintptr_t)gp & 3u);
                const uint32_t* gw = (const uint32_t*)(gp - mis);
                const uint32_t n_words = (mis + nb * P.rb + 3) >> 2;
                for (uint32_t w = t; w < n_words; w += FS_THREADS) s_rows[w] = gw[w];
                if (t < 6) s_rows[n_words + t] = 0;
                __syncthreads();
                const uint32_t total = nb * nwin;
                for (uint32_t idx = t; idx < total; idx += FS_THREADS) {
                    const uint32_t r = idx / nwin, p = idx - r * nwin;
                    if (P.nmask && row_window_masked(P.nmask + (row0 + r) * P.nmw, P.nmw, p, k)) continue;
                    const uint32_t bit = (mis + r * P.rb) * 8 + 2 * p;
                    K128 q;
                    if constexpr (W) {
                        q = canonical(stream_kmer(s_rows, bit, (int)k), (int)k);
                    } else {
                        q.hi = canonical64(stream_kmer64(s_rows, bit, (int)k), (int)k);
                        q.lo = 0;
                    }
                    uint32_t h = hash_kmer(q, FS_LOG2);
                    while (s_own[h] != 0) {
                        if (s_hi[h] == q.hi && (!W || s_lo[W ? h : 0] == q.lo)) {
                            atomicAdd(&s_cnt[h], 1u);
                            break;
                        }
                        h = (h + 1) & FS_SLOT_MASK;
                    }
                }
                __syncthreads();
            }
            // ---- reduce
            uint32_t sup[FS_PER];
            uint32_t nz = 0, nbl = 0, mn = EMPTY32, mx = 0;
            unsigned long long sum = 0;
#pragma unroll
            for (uint32_t j = 0; j < FS_PER; ++j) {
                sup[j] = slot[j] == EMPTY32 ? 0u : s_cnt[slot[j]];
                if (t + j * FS_THREADS < nw) {
                    nz += sup[j] == 0;
                    nbl += sup[j] < P.min_count;
                    mn = sup[j] < mn ? sup[j] : mn;
                    mx = sup[j] > mx ? sup[j] : mx;
                    sum += sup[j];
                }
            }
            __syncthreads();                     // (the table's owner words have been read for the last time)
#pragma unroll
            for (uint32_t j = 0; j < FS_PER; ++j) s_own[t + j * FS_THREADS] = sup[j];
            for (int d = 32; d >= 1; d >>= 1) {
                nz += __shfl_xor(nz, d);
                nbl += __shfl_xor(nbl, d);
                const uint32_t m2 = __shfl_xor(mn, d), x2 = __shfl_xor(mx, d);
                mn = m2 < mn ? m2 : mn;
                mx = x2 > mx ? x2 : mx;
                sum += __shfl_xor(sum, d);
            }
            if (lane == 0) {
                atomicAdd(&s_acc[0], nz);
                atomicAdd(&s_acc[1], nbl);
                atomicMin(&s_acc[2], mn);
                atomicMax(&s_acc[3], mx);
                atomicAdd(&s_sum, sum);
            }
            __syncthreads();
            {   // windows 4t .. 4t + 3 of the chunk: leading zeros, trailing zeros, longest zero run, windows present
                uint32_t pre = 0, suf = 0, lng = 0, len = 0, cur = 0;
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t i = 4 * t + j;
                    if (i >= nw) break;
                    ++len;
                    cur = s_own[i] == 0 ? cur + 1 : 0;
                    lng = cur > lng ? cur : lng;
                    if (cur == len) pre = cur;
                }
                suf = cur;
                s_seg[t] = pre | (suf << 8) | (lng << 16) | (len << 24);
            }
            __syncthreads();
            if (t == 0) {
                for (uint32_t q = 0; q < FS_THREADS; ++q) {
                    const uint32_t v = s_seg[q], pre = v & 255u, suf = (v >> 8) & 255u, lng = (v >> 16) & 255u, len = v >> 24;
                    if (!len) break;
                    if (pre == len) {
                        run += len;
                    } else {
                        best = run + pre > best ? run + pre : best;
                        best = lng > best ? lng : best;
                        run = suf;
                    }
                    best = run > best ? run : best;
                }
            }
        }
        __syncthreads();
        if (t == 0) {
            rec.n_windows = n_windows;
            if (n_windows) {
                rec.n_zero = s_acc[0];
                rec.n_below = s_acc[1];
                rec.min = s_acc[2];
                rec.max = s_acc[3];
                rec.zero_run = best;
                rec.sum = s_sum;
            }
            P.out[g] = rec;
            atomicAdd(P.round.stats + GF_FS_GAPS, 1u);
            atomicAdd((unsigned long long*)(P.round.stats + GF_FS_WINDOWS), (unsigned long long)n_windows);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_support_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                                   int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                   const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int k, int min_count,
                                   void* d_support, void* d_stats) {
    if (min_count < 0) return GF_E_INVAL;
    const FillRoundIn in = {d_pool_packed, d_pool_off, pool_rows, read_len, d_contigs, d_n_contigs, contig_cap, d_seq, d_gap_best, d_ctg_pick_or_null,
                            anchor_long, anchor_short, d_support, d_stats};
    FsParams P;
    memset(&P, 0, sizeof(P));
    size_t blocks;
    // workgroups the static LDS lets a CU hold: 3 with the wide table, 4 with the narrow one
    const int rc = fill_round_setup(ctx, in, k < 16 || k > 64 ? GF_E_UNSUPPORTED : GF_OK, GF_FS_WORDS, k > 32 ? 3 : 4, &P.round, &blocks);
    if (rc || !blocks) return rc;
    P.pool = (const uint8_t*)d_pool_packed;
    P.nmask = (const uint32_t*)d_nmask_or_null;
    P.rb = (uint32_t)gf_packed_read_bytes(read_len);
    P.L = (uint32_t)read_len;
    P.nmw = (uint32_t)((read_len + 31) / 32);
    P.batch_rows = FS_ROW_BYTES / P.rb;
    P.k = (uint32_t)k;
    P.min_count = (uint32_t)min_count;
    P.out = (gf_fill_support*)d_support;
    LaunchTimer tm(ctx, GF_KERNEL_SUPPORT);
    if (k > 32)
        hipLaunchKernelGGL(fill_support_kernel<true>, dim3((unsigned)blocks), dim3(FS_THREADS), 0, ctx->stream, P);
    else
        hipLaunchKernelGGL(fill_support_kernel<false>, dim3((unsigned)blocks), dim3(FS_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
