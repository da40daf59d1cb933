// gap_span.hip — gap size from the gap-spanning read pairs (gf_gap_span_dev; definition and host twin: gappadder_amd/gap_span.py,
// DESIGN.md §21).
//
// A second streaming pass of the tagger's kind over one library: the 8-byte key column (or, without one, the first half of every
// 32-byte record) is streamed with 16-byte loads, several in flight; (scaffold, POS) is tested against the tagger's coarse bin map for
// the library's dist2, staged in LDS; what passes waits, 12 bytes each, in a queue per wave and is sifted 64 at a time through the fine
// map where one exists; only then is the 32-byte record fetched.  The back end walks the gaps whose LEFT window holds the record, from
// bin_first, decides candidate and class per (record, gap), and reduces into the gap's 64-byte record with integer atomics whose result
// nobody reads: coordinate-sorted records put the lanes of a wave on one gap, so the lanes that agree on the gap are combined first
// (ballots for the six class counts; butterflies for the sum, the sum of squares, min and max of the accepted) and ONE lane sends them.
// While the pass runs, tlen_min holds 2^31 - min (0 = nothing yet: the call clears the records with zeros); the closing kernel over the
// gaps turns it back, sets the flag, and adds the gaps' counters up into the statistics words — so the totals cost no atomic per
// candidate at all, and one per counter and workgroup of the closing kernel.
#include "gf_internal.hpp"

namespace gf {

struct SpanParams {
    const uint4* recs;        // 32-byte records as two 16-byte halves: {pos, mate_pos, tlen, ref}, {mate_ref, flag | mapq << 16 | clip << 24, read}
    const uint2* keys;        // KEYS: {pos, ref | (mapq == 0) << 31} per record, n + 1 entries
    uint64_t n;
    const gf_gap* gaps;
    const uint32_t* scaf_off;
    uint32_t n_scaffolds;
    int32_t read_len, dist2, lo, hi, min_mapq;
    const uint32_t* bin_bits;   // the tagger's map for dist2 (tag_map.hip, ensure_bin_map): bits, offsets, first gap per bin
    const uint32_t* bin_off;
    const uint32_t* bin_first;
    uint32_t bin_shift, bin_words, off_words;
    const uint32_t* fine_bits;
    const uint32_t* fine_off;
    uint32_t fine_shift;
    gf_gap_span* out;
};

struct SpanCand { uint32_t pos, ref, rec; };
constexpr uint32_t SPANQ = 96;       // per wave: < 64 waiting + what one step adds
constexpr int SPAN_UNROLL = 8;       // 16-byte loads in flight per lane behind the chunk at work
constexpr uint32_t SPAN_MIN_BIAS = 0x80000000u;
enum { GS_C_MULTI, GS_C_CLIPPED, GS_C_LOWQ, GS_C_LOW, GS_C_HIGH, GS_C_ACCEPTED, GS_C_N };

__device__ __forceinline__ void span_wave_sync() {   // LDS hand-off between the lanes of ONE wave
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t wave_add32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_add64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// the candidates of one walk step into their gaps' records: per distinct gap among the lanes one round, one lane sends
__device__ __forceinline__ void span_reduce(gf_gap_span* out, bool cand, uint32_t g, int cls, uint32_t tlen) {
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(cand);
    while (rem) {
        const int lead = __ffsll((long long)rem) - 1;
        const uint32_t g0 = __shfl(g, lead);
        const bool mine = cand && g == g0;
        const unsigned long long mb = __ballot(mine);
        rem &= ~mb;
        uint32_t cnt[GS_C_N];
#pragma unroll
        for (int c = 0; c < GS_C_N; ++c) cnt[c] = (uint32_t)__popcll(__ballot(mine && cls == c));
        uint32_t s = 0, mn = 0, mx = 0;
        unsigned long long sq = 0;
        if (cnt[GS_C_ACCEPTED]) {      // (wave-uniform)
            const bool acc = mine && cls == GS_C_ACCEPTED;
            s = wave_add32(acc ? tlen : 0u);                                        // tlen < 2^20: 64 of them fit 32 bits
            sq = wave_add64(acc ? (unsigned long long)tlen * tlen : 0ull);
            mn = wave_max32(acc ? SPAN_MIN_BIAS - tlen : 0u);
            mx = wave_max32(acc ? tlen : 0u);
        }
        if ((int)lane == lead) {
            gf_gap_span* r = out + g0;
            atomicAdd(&r->n_cand, (uint32_t)__popcll(mb));
            if (cnt[GS_C_MULTI]) atomicAdd(&r->n_multi, cnt[GS_C_MULTI]);
            if (cnt[GS_C_CLIPPED]) atomicAdd(&r->n_clipped, cnt[GS_C_CLIPPED]);
            if (cnt[GS_C_LOWQ]) atomicAdd(&r->n_lowq, cnt[GS_C_LOWQ]);
            if (cnt[GS_C_LOW]) atomicAdd(&r->n_low, cnt[GS_C_LOW]);
            if (cnt[GS_C_HIGH]) atomicAdd(&r->n_high, cnt[GS_C_HIGH]);
            if (cnt[GS_C_ACCEPTED]) {
                atomicAdd(&r->n, cnt[GS_C_ACCEPTED]);
                atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum), (unsigned long long)s);
                atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_sq), sq);
                atomicMax(&r->tlen_min, mn);
                atomicMax(&r->tlen_max, mx);
            }
        }
    }
}

// one record per lane (live: the lane has one; its key said pos, ref with ref < n_scaffolds and POS inside the scaffold's bins): the
// record's own tests, then the walk over the gaps whose left window holds it
__device__ __forceinline__ void span_search(const SpanParams& P, const uint32_t* boff, bool live, uint32_t pos, uint32_t ref, uint4 a, uint4 b) {
    const uint32_t flag = b.y & 0xFFFFu, mapq = (b.y >> 16) & 0xFFu, clip = b.y >> 24;
    const int32_t tl = (int32_t)a.z;
    live = live && a.x == pos && a.w == ref && b.x == ref && (flag & 1u) && !(flag & (4u | 8u | 0x100u | 0x800u)) && !(flag & 0x10u) &&
           (flag & 0x20u) && pos >= 1 && a.y >= 1 && tl > 0;
    const int64_t A0 = (int64_t)pos - 1, M0 = (int64_t)a.y - 1, M1 = A0 + tl;
    live = live && M0 < M1;
    uint32_t g = 0, g_beg = 0, g_end = 0;
    if (live) {
        g_beg = P.scaf_off[ref];
        g_end = P.scaf_off[ref + 1];
        g = P.bin_first[boff[ref] + (pos >> P.bin_shift)];     // the first gap whose window reaches the record's bin
        if (g < g_beg) g = g_beg;
    }
    for (;;) {
        gf_gap gp = {};
        if (live && g < g_end) gp = P.gaps[g];
        const bool more = live && g < g_end && (int64_t)gp.start - P.dist2 < (int64_t)pos;   // start - A0 <= dist2; starts ascend
        live = more;
        if (!__any(more)) break;
        bool cand = false;
        int cls = GS_C_N;
        if (more) {
            cand = A0 + P.read_len <= (int64_t)gp.start && (int64_t)gp.end <= M0;
            if (cand) {
                bool multi = false;
                if (g > g_beg) multi = (int64_t)P.gaps[g - 1].end > A0;
                if (!multi && g + 1 < g_end) multi = (int64_t)P.gaps[g + 1].start < M1;
                cls = multi ? GS_C_MULTI : clip ? GS_C_CLIPPED : (int32_t)mapq < P.min_mapq ? GS_C_LOWQ : tl < P.lo ? GS_C_LOW : tl > P.hi ? GS_C_HIGH
                                                                                                                                        : GS_C_ACCEPTED;
            }
        }
        span_reduce(P.out, cand, g, cls, (uint32_t)tl);
        if (more) ++g;
    }
}

// the last min(64, cand_n) queued keys: fine map, the record's fetch, the search
__device__ __forceinline__ void span_sift(const SpanParams& P, const uint32_t* boff, SpanCand* wcand, uint32_t& cand_n) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t base = cand_n > 64 ? cand_n - 64 : 0;
    bool live = base + lane < cand_n;
    SpanCand c = {};
    if (live) {
        c = wcand[base + lane];
        if (P.fine_bits) {
            const uint32_t f0 = P.fine_off[c.ref], fi = c.pos >> P.fine_shift, fb = f0 + fi;
            live = fi < P.fine_off[c.ref + 1] - f0 && ((P.fine_bits[fb >> 5] >> (fb & 31)) & 1u);
        }
    }
    span_wave_sync();
    cand_n = base;
    if (!__any(live)) return;
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (live) {
        a = P.recs[2 * (uint64_t)c.rec];
        b = P.recs[2 * (uint64_t)c.rec + 1];
    }
    span_search(P, boff, live, c.pos, c.ref, a, b);
}

// a key per lane against the coarse map; what passes is queued
__device__ __forceinline__ void span_offer(const SpanParams& P, const uint32_t* bins, const uint32_t* boff, SpanCand* wcand, uint32_t& cand_n,
                                           bool valid, uint32_t pos, uint32_t ref, uint32_t rec) {
    const uint32_t lane = threadIdx.x & 63;
    bool live = valid && ref < P.n_scaffolds;
    if (live) {
        const uint32_t b0 = boff[ref], nbin = boff[ref + 1] - b0, bi = pos >> P.bin_shift;
        live = bi < nbin && ((bins[(b0 + bi) >> 5] >> ((b0 + bi) & 31)) & 1u);
    }
    const unsigned long long cb = __ballot(live);
    if (!cb) return;
    const uint32_t cnt = (uint32_t)__popcll(cb);
    if (cand_n + cnt > SPANQ) span_sift(P, boff, wcand, cand_n);       // (cand_n < 64 on entry: one sift makes room)
    if (live) wcand[cand_n + __popcll(cb & ((1ull << lane) - 1))] = SpanCand{pos, ref, rec};
    cand_n += cnt;
    span_wave_sync();
    if (cand_n >= 64) span_sift(P, boff, wcand, cand_n);
}

// NW waves per workgroup; the coarse map (and, when they are few, the scaffold offsets) staged in LDS once per workgroup.  KEYS: the
// stream is the key column, two records per 16-byte load; otherwise the first half of every record, one per load.
template <int NW, bool KEYS>
__global__ __launch_bounds__(64 * NW) void gap_span_kernel(SpanParams P) {
    extern __shared__ uint32_t span_bins[];
    __shared__ SpanCand candq[NW][SPANQ];
    for (uint32_t i = threadIdx.x; i < P.bin_words + P.off_words; i += blockDim.x) span_bins[i] = P.bin_bits[i];   // (bits, then offsets: one array)
    const uint32_t* bins = span_bins;
    const uint32_t* boff = P.off_words ? span_bins + P.bin_words : P.bin_off;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    SpanCand* wcand = candq[threadIdx.x >> 6];
    uint32_t cand_n = 0;   // wave-uniform
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* src = reinterpret_cast<const u32x4*>(KEYS ? (const void*)P.keys : (const void*)P.recs);
    const uint64_t n_ld = KEYS ? (P.n + 1) / 2 : P.n;             // 16-byte loads in all
    const uint64_t stride = KEYS ? 1 : 2;                         // ... and their distance in 16-byte units
    const uint64_t chunk = 64ull * SPAN_UNROLL;
    u32x4 kn[SPAN_UNROLL];
#pragma unroll
    for (int u = 0; u < SPAN_UNROLL; ++u) {
        const uint64_t h = wave * chunk + 64ull * u + lane;
        kn[u] = h < n_ld ? __builtin_nontemporal_load(src + h * stride) : u32x4{0u, 0x7FFFFFFFu, 0u, 0x7FFFFFFFu};
    }
    for (uint64_t h0 = wave * chunk; h0 < n_ld; h0 += n_waves * chunk) {
        u32x4 v[SPAN_UNROLL];
#pragma unroll
        for (int u = 0; u < SPAN_UNROLL; ++u) v[u] = kn[u];
#pragma unroll
        for (int u = 0; u < SPAN_UNROLL; ++u) {
            const uint64_t h = h0 + n_waves * chunk + 64ull * u + lane;
            kn[u] = h < n_ld ? __builtin_nontemporal_load(src + h * stride) : u32x4{0u, 0x7FFFFFFFu, 0u, 0x7FFFFFFFu};
        }
#pragma unroll
        for (int u = 0; u < SPAN_UNROLL; ++u) {
            const uint64_t h = h0 + 64ull * u + lane;
            if constexpr (KEYS) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const uint64_t rec = 2 * h + half;
                    const uint32_t pos = half ? v[u].z : v[u].x, w = half ? v[u].w : v[u].y;
                    span_offer(P, bins, boff, wcand, cand_n, rec < P.n, pos, w & 0x7FFFFFFFu, (uint32_t)rec);
                }
            } else {
                span_offer(P, bins, boff, wcand, cand_n, h < P.n, v[u].x, v[u].w, (uint32_t)h);     // ('*': ref 0xFFFFFFFF, beyond n_scaffolds)
            }
        }
    }
    while (cand_n) span_sift(P, boff, wcand, cand_n);
}

// per gap: tlen_min back from its biased form, the flag; the gaps' counters added up into the statistics words
__global__ __launch_bounds__(256) void gap_span_finish_kernel(gf_gap_span* rec, uint32_t n_gaps, uint32_t* stats) {
    __shared__ unsigned long long tot[8];
    if (threadIdx.x < 8) tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_gaps; g += gridDim.x * blockDim.x) {
        gf_gap_span* r = rec + g;
        const uint32_t n = r->n;
        if (n) {
            r->tlen_min = SPAN_MIN_BIAS - r->tlen_min;
            r->flags = GF_GS_F_PAIRS;
            v[7] += 1;
        }
        v[0] += r->n_cand; v[1] += n; v[2] += r->n_multi; v[3] += r->n_clipped; v[4] += r->n_lowq; v[5] += r->n_low; v[6] += r->n_high;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned long long s = wave_add64(v[i]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot[i], s);
    }
    __syncthreads();
    if (threadIdx.x < 7 && tot[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + threadIdx.x, tot[threadIdx.x]);
    if (threadIdx.x == 7 && tot[7]) atomicAdd(stats + GF_GS_GAPS_WITH_PAIRS, (uint32_t)tot[7]);
}

int launch_gap_span(gf_ctx* ctx, const void* d_recs, const void* d_keys, size_t n, int read_len, int is_mean, int is_sd, int z, int shift,
                    int min_mapq, void* d_rec, void* d_stats) {
    if (z < 1 || shift < 0 || is_mean < 0 || is_sd < 0 || read_len < 1 || min_mapq < 0 || min_mapq > 255) return GF_E_UNSUPPORTED;
    const int64_t hi = (int64_t)is_mean + (int64_t)z * is_sd + shift, d2 = (int64_t)is_mean + 3ll * is_sd;
    if (hi >= (1 << 20) || d2 >= (1 << 20)) return GF_E_UNSUPPORTED;
    if (!ctx->d_gaps || ctx->gaps.empty()) return GF_E_STATE;
    if (n >= 0xFFFFFFFFull || ctx->gaps.size() >= (1ull << 27)) return GF_E_INVAL;
    const uint32_t n_gaps = (uint32_t)ctx->gaps.size();
    zero_regions(ctx, ZeroList{{(uint32_t*)d_rec, (uint32_t*)d_stats, nullptr, nullptr}, {n_gaps * (uint32_t)(sizeof(gf_gap_span) / 4), GF_GS_WORDS, 0, 0}});
    GF_HIP(ctx, hipGetLastError());
    if (n == 0) return GF_OK;
    SpanParams P;
    P.recs = (const uint4*)d_recs;
    P.keys = (const uint2*)d_keys;
    P.n = n;
    P.gaps = ctx->d_gaps;
    P.scaf_off = ctx->d_scaf_off;
    P.n_scaffolds = ctx->n_scaffolds;
    P.read_len = read_len;
    P.dist2 = (int32_t)d2;
    P.lo = (int32_t)((int64_t)is_mean - (int64_t)z * is_sd - shift);
    P.hi = (int32_t)hi;
    P.min_mapq = min_mapq;
    P.out = (gf_gap_span*)d_rec;
    gf_ctx::TagMap* M = nullptr;
    int rc = ensure_bin_map(ctx, P.dist2, &M);      // the tagger's own map for this library
    if (rc) return rc;
    P.bin_bits = (const uint32_t*)M->map.p;
    P.bin_off = P.bin_bits + M->words;
    P.bin_first = P.bin_off + ctx->n_scaffolds + 1;
    P.bin_shift = M->shift;
    P.bin_words = M->words;
    P.off_words = ctx->n_scaffolds + 1 <= 2048 ? ctx->n_scaffolds + 1 : 0;
    P.fine_bits = M->fine_words ? (const uint32_t*)M->fine.p : nullptr;
    P.fine_off = P.fine_bits ? P.fine_bits + M->fine_words : nullptr;
    P.fine_shift = M->fine_shift;
    const size_t map_bytes = (size_t)M->words * 4;
    const bool big_map = map_bytes > 32 * 1024;      // the 64-KiB map: one 16-wave workgroup per CU, as the tagger runs it
    const size_t static_lds = (big_map ? 16 : 4) * SPANQ * sizeof(SpanCand) + 64, lds_max = 160 * 1024;
    if (static_lds + map_bytes + (size_t)P.off_words * 4 > lds_max) P.off_words = 0;
    const size_t lds_map = map_bytes + (size_t)P.off_words * 4;
    if (static_lds + lds_map > lds_max) return GF_E_UNSUPPORTED;
    const unsigned grid = big_map ? (unsigned)std::max<size_t>(1, std::min<size_t>((n + 1023) / 1024, (size_t)ctx->n_cu))
                                  : (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)ctx->n_cu * 8));
    {
        LaunchTimer tm(ctx, GF_KERNEL_GAPSPAN);
        if (d_keys) {
            if (big_map) hipLaunchKernelGGL((gap_span_kernel<16, true>), dim3(grid), dim3(1024), lds_map, ctx->stream, P);
            else hipLaunchKernelGGL((gap_span_kernel<4, true>), dim3(grid), dim3(256), lds_map, ctx->stream, P);
        } else {
            if (big_map) hipLaunchKernelGGL((gap_span_kernel<16, false>), dim3(grid), dim3(1024), lds_map, ctx->stream, P);
            else hipLaunchKernelGGL((gap_span_kernel<4, false>), dim3(grid), dim3(256), lds_map, ctx->stream, P);
        }
        GF_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(gap_span_finish_kernel, dim3(std::max(1u, std::min((n_gaps + 255) / 256, 256u))), dim3(256), 0, ctx->stream,
                           (gf_gap_span*)d_rec, n_gaps, (uint32_t*)d_stats);
    }
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // namespace gf
