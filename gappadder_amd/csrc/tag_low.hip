// tag_low.hip — the second hop's look-up.
//
// low_mapq_kernel restates collect_discordant_low_mapq_reads.py:4-84: MAPQ==0 records, focal_region[p] = the
// LAST discordant mate position q (sorted file order) with q-199 <= p <= q+299, one hit per row of q.
#include <cstring>

#include "tag_dev.hpp"

namespace gf {

// largest index uq in [first, hi) with upos[uq] <= lim, or `first - 1` when there is none: upos ascends inside a scaffold and the positions
// (mates of chimeric pairs) are spread evenly, so the search starts from the interpolated place and gallops — three or four loads instead
// of the seventeen of a bisection over 1.7e5 positions (the second hop was 0.55 ms of look-ups into an L2-resident array)
__device__ __forceinline__ uint32_t hop_upper(const uint32_t* upos, uint32_t first, uint32_t hi, uint64_t lim) {
    if (first >= hi) return first - 1;
    uint32_t lo = first;                       // invariant: everything below lo is <= lim, everything from hi on is > lim
    const uint32_t p0 = upos[first], p1 = upos[hi - 1];
    if ((uint64_t)p0 > lim) return first - 1;
    if ((uint64_t)p1 <= lim) return hi - 1;
    uint32_t g = first + (uint32_t)(((lim - p0) * (uint64_t)(hi - 1 - first)) / (uint64_t)(p1 - p0));   // p0 <= lim < p1
    if ((uint64_t)upos[g] <= lim) {
        lo = g + 1;
        for (uint32_t st = 1; lo < hi; st <<= 1) {         // gallop up
            const uint32_t t = lo + st - 1 < hi - 1 ? lo + st - 1 : hi - 1;
            if ((uint64_t)upos[t] <= lim) lo = t + 1; else { hi = t; break; }
        }
    } else {
        hi = g;
        for (uint32_t st = 1; lo < hi; st <<= 1) {         // gallop down
            const uint32_t t = hi > lo + st ? hi - st : lo;
            if ((uint64_t)upos[t] > lim) hi = t; else { lo = t + 1; break; }
        }
    }
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)upos[mid] <= lim) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__global__ __launch_bounds__(256) void low_mapq_kernel(LowParams P) {
    __shared__ gf_taghit whits[4][WHCAP];
    WaveHits hb{whits[threadIdx.x >> 6], 0};
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t n_half = 2 * P.n;
    const uint64_t chunk = 64ull * TAG_UNROLL;
    const uint4* src = reinterpret_cast<const uint4*>(P.recs);
    for (uint64_t h0 = wave * chunk; h0 < n_half; h0 += n_waves * chunk) {
        uint4 v[TAG_UNROLL];
#pragma unroll
        for (int u = 0; u < TAG_UNROLL; ++u) {
            const uint64_t h = h0 + 64ull * u + lane;
            v[u] = h < n_half ? src[h] : make_uint4(0, 0xFFFFFFFFu, 0, 0xFFFFFFFFu);
        }
#pragma unroll
        for (int u = 0; u < TAG_UNROLL; ++u) {
            const uint64_t h = h0 + 64ull * u + lane;
            const uint32_t nb_y = __shfl_down(v[u].y, 1);  // flag | mapq<<16 | clip<<24 of the even lane's record
            uint32_t row = 0, row_end = 0;
            if (!(lane & 1) && h < n_half) {
                const uint32_t pos = v[u].x, ref = v[u].w, mapq = (nb_y >> 16) & 0xFF;
                if (mapq == 0 && ref < P.n_scaffolds) {
                    const uint32_t first = P.scaf_off[ref];
                    const uint32_t uq = hop_upper(P.upos, first, P.scaf_off[ref + 1], (uint64_t)pos + 199);  // largest q <= pos+199
                    if (uq + 1 > first) {
                        if ((uint64_t)P.upos[uq] + 299 >= pos) {
                            row = P.urow[uq];
                            row_end = P.urow[uq + 1];
                        }
                    }
                }
            }
            emit_rows(row, row_end, (uint32_t)(h >> 1), hb, P.out, P.cap, P.n_out);
        }
    }
    if (hb.n) flush_wave_hits(hb, P.out, P.cap, P.n_out);
}

// second hop over the compacted list (2 % of the records, 12 B each) instead of a second pass over every record
__global__ __launch_bounds__(256) void low_mapq_compact_kernel(LowParams P) {
    __shared__ gf_taghit whits[4][WHCAP];
    WaveHits hb{whits[threadIdx.x >> 6], 0};
    const uint32_t n = *P.n_low < P.low_cap ? *P.n_low : P.low_cap;
    const uint32_t n_round = (n + 63) & ~63u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += gridDim.x * blockDim.x) {
        uint32_t row = 0, row_end = 0, rec = 0;
        if (i < n) {
            const gf_lowrec e = P.low[i];
            rec = e.rec;
            // 99 % of the MAPQ-0 records lie near no row of the table: one look-up in a hashed bit map of the rows' neighbourhoods (built
            // with the table: 2^22 bits, a twelfth set at C4) spares them the search — a chain of eight dependent loads that set the
            // kernel's pace (0.57 ms for 18 M records).  A bit shared by chance only sends a record through the search it would have
            // made anyway.
            bool near = e.ref < P.n_scaffolds;
            if (near && P.near_bits) {
                const uint32_t b = hop_near_bit(e.ref, e.pos >> HOP_NEAR_SHIFT);
                near = (P.near_bits[b >> 5] >> (b & 31)) & 1u;
            }
            if (near) {
                const uint32_t first = P.scaf_off[e.ref];
                const uint32_t uq = hop_upper(P.upos, first, P.scaf_off[e.ref + 1], (uint64_t)e.pos + 199);  // largest q <= pos+199
                if (uq + 1 > first) {
                    if ((uint64_t)P.upos[uq] + 299 >= e.pos) {
                        row = P.urow[uq];
                        row_end = P.urow[uq + 1];
                    }
                }
            }
        }
        emit_rows(row, row_end, rec, hb, P.out, P.cap, P.n_out);
    }
    if (hb.n) flush_wave_hits(hb, P.out, P.cap, P.n_out);
}

// the look-up itself: over the compacted MAPQ-0 list where there is one (d_low), over all n records otherwise
static int launch_look_up(gf_ctx* ctx, const void* d_recs, size_t n, const void* d_low, const void* d_n_low, size_t low_cap, const uint32_t* upos,
                          const uint32_t* urow, const uint32_t* soff, const uint32_t* near_bits, void* d_out, size_t cap, void* d_n_out) {
    LowParams P;
    P.recs = (const gf_alnrec*)d_recs;
    P.n = n;
    P.low = (const gf_lowrec*)d_low;
    P.n_low = (const uint32_t*)d_n_low;
    P.low_cap = (uint32_t)low_cap;
    P.upos = upos;
    P.urow = urow;
    P.scaf_off = soff;
    P.n_scaffolds = ctx->n_scaffolds;
    P.out = (gf_taghit*)d_out;
    P.cap = (uint32_t)cap;
    P.n_out = (uint32_t*)d_n_out;
    P.near_bits = near_bits;
    {
        LaunchTimer tm(ctx, GF_KERNEL_LOWMAPQ);
        if (d_low)
            hipLaunchKernelGGL(low_mapq_compact_kernel, dim3(stream_grid(ctx->n_cu, std::max<size_t>(low_cap, 1))), dim3(256), 0, ctx->stream, P);
        else
            hipLaunchKernelGGL(low_mapq_kernel, dim3(stream_grid(ctx->n_cu, n)), dim3(256), 0, ctx->stream, P);
    }
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int launch_low_mapq(gf_ctx* ctx, const void* d_recs, size_t n, const gf_dpos* table, size_t n_rows, void* d_out,
                    size_t cap, void* d_n_out, const void* d_low, const void* d_n_low, size_t low_cap) {
    if (n >= 0xFFFFFFFFull || cap > 0xFFFFFFFFull || n_rows >= 0xFFFFFFFFull || low_cap > 0xFFFFFFFFull) return GF_E_INVAL;
    if (ctx->n_scaffolds == 0) return GF_E_STATE;
    GF_HIP(ctx, hipMemsetAsync(d_n_out, 0, 4, ctx->stream));
    if ((n == 0 && !d_low) || n_rows == 0) return GF_OK;
    // host: unique positions per scaffold + row offsets (the table is tiny next to the record stream); the device copy
    // is cached and re-used while the caller passes the same rows (a pipeline calls this once per batch of records)
    const bool cached = ctx->low_rows.size() == n_rows * 4 && ctx->table.p &&
                        memcmp(ctx->low_rows.data(), table, n_rows * sizeof(gf_dpos)) == 0;
    if (!cached) {
        std::vector<uint32_t> upos, urow, soff(ctx->n_scaffolds + 1, 0);
        uint32_t cur_s = 0;
        for (size_t r = 0; r < n_rows; ++r) {
            if (r) {
                const gf_dpos &a = table[r - 1], &b = table[r];
                if (a.mate_scaffold > b.mate_scaffold || (a.mate_scaffold == b.mate_scaffold && a.mate_pos > b.mate_pos))
                    return GF_E_INVAL;  // must be sorted (run_multi_threads_discordant.py:103)
            }
            if (table[r].mate_scaffold >= ctx->n_scaffolds) return GF_E_INVAL;
            if (r == 0 || table[r].mate_scaffold != table[r - 1].mate_scaffold || table[r].mate_pos != table[r - 1].mate_pos) {
                while (cur_s < table[r].mate_scaffold) soff[++cur_s] = (uint32_t)upos.size();
                upos.push_back(table[r].mate_pos);
                urow.push_back((uint32_t)r);
            }
        }
        urow.push_back((uint32_t)n_rows);
        while (cur_s < ctx->n_scaffolds) soff[++cur_s] = (uint32_t)upos.size();
        const size_t b1 = upos.size() * 4, b2 = urow.size() * 4, b3 = soff.size() * 4;
        int rc;
        if ((rc = ensure(ctx, ctx->table, b1 + b2 + b3 + 64))) return rc;
        uint8_t* base = (uint8_t*)ctx->table.p;
        GF_HIP(ctx, hipMemcpyAsync(base, upos.data(), b1, hipMemcpyHostToDevice, ctx->stream));
        GF_HIP(ctx, hipMemcpyAsync(base + b1, urow.data(), b2, hipMemcpyHostToDevice, ctx->stream));
        GF_HIP(ctx, hipMemcpyAsync(base + b1 + b2, soff.data(), b3, hipMemcpyHostToDevice, ctx->stream));
        GF_HIP(ctx, hipStreamSynchronize(ctx->stream));  // host vectors go out of scope
        ctx->low_rows.assign((const uint32_t*)table, (const uint32_t*)table + n_rows * 4);
        ctx->low_b1 = b1;
        ctx->low_b2 = b2;
    }
    const uint32_t* tab = (const uint32_t*)ctx->table.p;
    return launch_look_up(ctx, d_recs, n, d_low, d_n_low, low_cap, tab, tab + ctx->low_b1 / 4, tab + (ctx->low_b1 + ctx->low_b2) / 4, nullptr, d_out, cap, d_n_out);
}

// second hop over the compacted MAPQ-0 list with look-up arrays that already live on the device (hop.hip builds them);
// *d_n_out was zeroed by the kernel that built the look-up arrays
int launch_low_mapq_devtable(gf_ctx* ctx, const void* d_low, const void* d_n_low, size_t low_cap, const uint32_t* upos, const uint32_t* urow,
                             const uint32_t* soff, const uint32_t* near_bits, void* d_out, size_t cap, void* d_n_out) {
    return launch_look_up(ctx, nullptr, 0, d_low, d_n_low, low_cap, upos, urow, soff, near_bits, d_out, cap, d_n_out);
}

}  // namespace gf
