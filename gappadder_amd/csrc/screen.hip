// screen.hip — flank-k-mer screen of packed reads (north_star: "canonical k-mer extract/hash ... of streamed
// reads, flank-k-mer lookup to tag reads").  Predicate shape of IsReadContainingFreqKmers
// (ContigsCompactor-v0.2.0/ContigsMerger/KmerUtils.cpp:215-241) applied per gap on canonical k-mers.
//
// Filter (streams every read once; probes only ceil((L-15)/(k-15)) 16-mers per read, because any k-mer shared with a flank
// contains one of them; emits candidate read ids) — plan_screen below picks the form:
//   screen_filter_pipe_kernel  small key sets: coarse bitmap in LDS -> level-1 bitmap in L2 -> exact 16-mer set, software-pipelined
//   pf4_* (screen_pf4.hip)     large key sets: the probes sorted into 256 buckets, a bucket's slice of the level-1 bitmap in LDS
//   screen_filter_kernel       no LDS level (everything else)
// Verification of the candidates (exact): screen_verify.hip.
// This file: the plain and the pipelined kernel, the probe geometry, the plan of a screen call and launch_screen, which runs it.
#include "screen_dev.hpp"

namespace gf {

// PU = probes issued back-to-back before their results are consumed
template <int PU>
__global__ __launch_bounds__(256) void screen_filter_kernel(FilterParams P) {
    extern __shared__ uint32_t tile[];  // TILE_READS * rb bytes + 16 B pad
    // candidates are buffered per workgroup and appended to the global list with ONE atomic per ~768 of them:
    // a single global counter serialises returning atomics at ~11 ns each (MI355X_MICROARCH.md "dequeue" row)
    constexpr uint32_t CBUF = 1024;
    __shared__ uint32_t cbuf[CBUF];
    __shared__ uint32_t cbuf_n, cbuf_base;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63;
    if (tid == 0) cbuf_n = 0;
    const uint32_t tile_bytes = TILE_READS * P.rb;
    const uint64_t total_bytes = P.n_reads * P.rb;
    const uint64_t n_tiles = (P.n_reads + TILE_READS - 1) / TILE_READS;
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
    const uint32_t smask = (1u << P.s_log2) - 1;
    constexpr uint32_t GROUP = (32 / PU) * PU;  // probes whose results fit one 32-bit mask

    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t byte0 = t * tile_bytes;
        const uint32_t nbytes = (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes);
        const uint32_t n16 = nbytes & ~15u;
        const uint8_t* src = P.reads + byte0;
        for (uint32_t i = tid * 16; i < n16; i += 256 * 16)
            *reinterpret_cast<uint4*>(tb + i) = *reinterpret_cast<const uint4*>(src + i);
        for (uint32_t i = n16 + tid; i < nbytes; i += 256) tb[i] = src[i];
        if (tid < 16) tb[nbytes + tid] = 0;
        __syncthreads();

        const uint64_t r = t * TILE_READS + tid;
        bool cand = false;
        if (r < P.n_reads) {
            const uint32_t bit0 = tid * P.rb * 8;
            for (uint32_t g0 = 0; g0 < P.np && !cand; g0 += GROUP) {
                const uint32_t g1 = g0 + GROUP < P.np ? g0 + GROUP : P.np;
                uint32_t mask = 0;
                for (uint32_t j0 = g0; j0 < g1; j0 += PU) {
                    uint32_t word[PU], hb[PU];
#pragma unroll
                    for (int u = 0; u < PU; ++u) {
                        const uint32_t j = j0 + u;
                        word[u] = 0;
                        hb[u] = 0;
                        if (j < g1) {
                            const uint32_t key = canon16(stream32(tile, bit0 + P.first2 + j * P.stride2));
                            const uint32_t h = hash_s16_bitmap(key, P.bm_log2);
                            hb[u] = (h & 31) | (hash_s16_bit2(key) << 8);   // both bits of the key in its word
                            word[u] = h;                                    // (the level-1 word replaces it below)
                        }
                    }
                    if (P.bitmap_mid) {   // big key sets: an L2-resident reduced bitmap first, the fabric only for what passes
                        uint32_t mw[PU];
#pragma unroll
                        for (int u = 0; u < PU; ++u) mw[u] = (j0 + u < g1) ? P.bitmap_mid[word[u] >> (P.bm_log2 - P.mid_log2 + 5)] : 0;
#pragma unroll
                        for (int u = 0; u < PU; ++u) {
                            const uint32_t c = word[u] >> (P.bm_log2 - P.mid_log2);
                            const bool pass = (j0 + u < g1) && ((mw[u] >> (c & 31)) & 1u);
                            word[u] = pass ? P.bitmap[word[u] >> 5] : 0u;
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < PU; ++u) word[u] = (j0 + u < g1) ? P.bitmap[word[u] >> 5] : 0u;
                    }
#pragma unroll
                    for (int u = 0; u < PU; ++u) {
                        const uint32_t both = (word[u] >> (hb[u] & 31)) & (word[u] >> (hb[u] >> 8));
                        mask |= (both & 1u) << (j0 - g0 + u);
                    }
                }
                // level 2: confirm each bitmap hit in the exact canonical-16-mer set
                while (mask && !cand) {
                    const uint32_t j = g0 + __ffs(mask) - 1;
                    mask &= mask - 1;
                    const uint32_t key = canon16(stream32(tile, bit0 + P.first2 + j * P.stride2));
                    uint32_t s = hash_s16_set(key, P.s_log2);
                    uint32_t v;
                    while ((v = P.sset[s]) != EMPTY32) {
                        if (v == key) { cand = true; break; }
                        s = (s + 1) & smask;
                    }
                }
            }
        }
        // wave ballot + prefix count compaction of candidate reads into the workgroup buffer
        const unsigned long long bal = __ballot(cand);
        if (bal) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&cbuf_n, (uint32_t)__popcll(bal));
            base = __shfl(base, 0);
            if (cand) cbuf[base + __popcll(bal & ((1ull << lane) - 1))] = (uint32_t)r;
        }
        __syncthreads();
        if (cbuf_n > CBUF - TILE_READS) {  // uniform: no room for another tile's worth -> flush
            const uint32_t n = cbuf_n;
            if (tid == 0) cbuf_base = atomicAdd(P.n_cand, n);
            __syncthreads();
            for (uint32_t i = tid; i < n; i += 256) P.cand[cbuf_base + i] = cbuf[i];
            __syncthreads();
            if (tid == 0) cbuf_n = 0;
            __syncthreads();
        }
    }
    __syncthreads();
    {
        const uint32_t n = cbuf_n;
        if (n) {
            if (tid == 0) cbuf_base = atomicAdd(P.n_cand, n);
            __syncthreads();
            for (uint32_t i = tid; i < n; i += 256) P.cand[cbuf_base + i] = cbuf[i];
        }
    }
}

constexpr uint32_t WOBUF = 96;   // candidates buffered per wave (LDS); flushed with one global atomic when >= 32

// ---- software-pipelined wave kernel ---------------------------------------------------------------------------------
// A wave that streams its tiles and probes them on the spot pays two dependent L2 round trips per 64-read tile (level-1 bitmap word, then the exact
// set), ~2.5 us a tile and wave whatever the probe count; with 11 waves per CU that chain, not bandwidth, set its floor
// (measured: 0.31 ms with no probes, 0.73 ms with one).  Here each wave keeps THREE tiles in flight in registers:
//   stage A (tile t)    stage the tile in LDS, scramble its NP 16-mers, test the coarse LDS bitmap, ISSUE the level-1 loads
//   stage B (tile t-1)  level-1 words have arrived: pick the (up to two) passing probes, ISSUE their exact-set loads
//   stage C (tile t-2)  exact-set slots have arrived: candidate or not, append
// so no iteration waits for a load issued in the same iteration.  A probe is carried as its scrambled key p = key * M
// (bijective): every bitmap index is a shift of p, and key = p * M^-1 when the exact set is consulted.  The exact set is
// read four consecutive slots at a time (linear probing, table padded by three wrap-around slots), which settles almost
// every lookup in one request; the leftovers (3rd+ passing probe of a lane, a run of four foreign keys) take a serial path.
template <int NP>
struct PipeW {   // stage A -> B: scrambled keys, level-1 words, coarse-pass bits of one tile
    uint32_t p[NP], w[NP], pm;
    uint32_t t;  // tile index, PIPE_NONE when empty (tiles < 2^26 since reads < 2^32)
};
struct PipeS {   // stage B -> C: the (up to two) exact-set lookups of one tile
    uint32_t key0, key1;
    u32x4 v0, v1;
    uint32_t fl;  // bit 0/1: lookup 0/1 in use, bit 2: already a candidate (slow path)
    uint32_t t;
};
constexpr uint32_t PIPE_NONE = 0xFFFFFFFFu;

template <int NCH, int NP, bool EXACT>   // EXACT: the launch has exactly NP probes per read (no per-probe np test)
__global__ __launch_bounds__(512) void screen_filter_pipe_kernel(FilterParams P, uint32_t slice_words) {
    static_assert(NCH >= 1, "whole 16-byte chunks per lane");
    extern __shared__ uint32_t sm[];  // [coarse bitmap][per wave: 64 reads + pad | WOBUF candidate ids]
    const uint32_t tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x, nw = nthr >> 6;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);   // wave index, kept scalar
    const uint32_t bm_words = 1u << (P.lds_log2 - 5);
    for (uint32_t i = tid * 4; i < bm_words; i += nthr * 4)
        *reinterpret_cast<uint4*>(sm + i) = *reinterpret_cast<const uint4*>(P.bitmap_lds + i);
    uint32_t* tile = sm + bm_words + w * (slice_words + WOBUF);
    uint32_t* obuf = tile + slice_words;
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
    uint32_t obuf_n = 0;   // wave-uniform
    const uint32_t tile_bytes = 64 * P.rb;
    const uint64_t total_bytes = P.n_reads * P.rb;
    const uint32_t n_tiles = (uint32_t)((P.n_reads + 63) / 64);
    const bool same = P.bm_log2 == P.lds_log2;
    const bool bytes_ok = ((P.stride2 | P.first2) & 7) == 0;
    const uint32_t sh_lds = 32 - P.lds_log2, sh_bm = 32 - P.bm_log2;
    const uint32_t l2mask = same ? 0u : ~3u;
    const void* dummy = P.bitmap_lds;   // >= 16 readable bytes
    u32x4 pfA[NCH], pfB[NCH];
    auto prefetch = [&](u32x4 (&pf)[NCH], uint32_t t) {   // always NCH loads
        uint32_t n16 = 0;
        const void* base = dummy;
        if (t < n_tiles) {
            const uint64_t byte0 = (uint64_t)t * tile_bytes;
            n16 = (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes) >> 4;
            if (n16) base = P.reads + byte0;
        }
        base = uniform_ptr(base);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t i = lane + c * 64;
            const uint32_t off = i < n16 ? i * 16 : 0u;
            if (P.stream_policy == 1) vm_load128_nt(pf[c], off, base);
            else if (P.stream_policy == 2) vm_load128_sc1(pf[c], off, base);
            else if (P.stream_policy == 3) vm_load128_sc01nt(pf[c], off, base);
            else vm_load128(pf[c], off, base);
        }
    };
    const uint32_t tstride = gridDim.x * nw;   // < 2^26
    uint32_t t = blockIdx.x * nw + w;
    auto next_tile = [&](uint32_t x, uint32_t steps) {   // x + steps * tstride, saturating at n_tiles
        const uint64_t y = (uint64_t)x + (uint64_t)steps * tstride;
        return y < n_tiles ? (uint32_t)y : n_tiles;
    };
    prefetch(pfA, t);
    prefetch(pfB, next_tile(t, 1));

    PipeW<NP> W0, W1;
    PipeS S0, S1;
    W0.t = W1.t = PIPE_NONE;
    S0.t = S1.t = PIPE_NONE;
    __syncthreads();   // coarse bitmap staged

    // Loads issued per step, in order: NP (level-1 words), 2 (exact-set slots), NCH (prefetch of the tile two steps on).
    // vmcnt retires in issue order; every wait below names how many loads were issued after the one it needs.
    //   prefetch issued at the end of step s-2   -> staged at the top of step s
    //   level-1 words issued in stage A of s-1   -> tested in stage B of step s
    //   exact-set slots issued in stage B of s-1 -> tested in stage C of step s
    constexpr int PER_STEP = NP + 2 + NCH;
    constexpr int YOUNGER_THAN_PF = PER_STEP;      // all of step s-1
    constexpr int YOUNGER_THAN_S = NCH + NP;       // prefetch of step s-1, stage A of step s
    static_assert(YOUNGER_THAN_PF + PER_STEP <= 63, "vmcnt is a 6-bit counter");
    uint32_t n_steps = 0;
    const uint32_t rbase = lane * P.rb;

    // one step: stage A on tile t (fills WA), stage C on SC and stage B on WB -> SB (both filled one step ago)
    auto step = [&](u32x4 (&pf)[NCH], PipeW<NP>& WA, PipeW<NP>& WB, PipeS& SB, PipeS& SC) {
        const bool have = t < n_tiles;
        if (n_steps >= 2) vm_wait<YOUNGER_THAN_PF>(); else vm_wait<0>();
        ++n_steps;
#pragma unroll
        for (int c = 0; c < NCH; ++c) vm_ready(pf[c]);
        if (have) {
            const uint64_t byte0 = (uint64_t)t * tile_bytes;
            const uint32_t nbytes = (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes);
            const uint32_t n16 = nbytes >> 4;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint32_t i = lane + c * 64;
                if (i < n16) *reinterpret_cast<u32x4*>(tb + i * 16) = pf[c];
            }
            if (nbytes & 15u) {   // only the very last tile of the array
                const uint8_t* src = P.reads + byte0;
                for (uint32_t i = n16 * 16 + lane; i < nbytes; i += 64) tb[i] = src[i];
            }
            if (lane < 16) tb[nbytes + lane] = 0;
        }
        wave_lds_sync();
        {
            const uint32_t en = (have && (uint64_t)t * 64 + lane < P.n_reads) ? 0xFFFFFFFFu : 0u;
            uint32_t bw[NP], w32[NP];
            // the uniform byte-aligned / bit-aligned choice is made ONCE around the unrolled loop, so that all NP tile reads
            // are issued back to back (a branch per probe put an s_waitcnt lgkmcnt(0) behind every single ds_read2)
            if (bytes_ok) {
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    const uint32_t jj = EXACT || (uint32_t)j < P.np ? (uint32_t)j : 0u;
                    w32[j] = stream32_bytes(tile, rbase + ((P.first2 + jj * P.stride2) >> 3));
                }
            } else {
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    const uint32_t jj = EXACT || (uint32_t)j < P.np ? (uint32_t)j : 0u;
                    w32[j] = stream32(tile, rbase * 8 + P.first2 + jj * P.stride2);
                }
            }
#pragma unroll
            for (int j = 0; j < NP; ++j) WA.p[j] = canon16(w32[j]) * S16_MUL;
#pragma unroll
            for (int j = 0; j < NP; ++j) bw[j] = sm[WA.p[j] >> (sh_lds + 5)];
            uint32_t pm = 0;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                uint32_t pass = (uint32_t)__builtin_amdgcn_sbfe((int)bw[j], WA.p[j] >> sh_lds, 1);   // 0 or all ones
                pass &= EXACT || (uint32_t)j < P.np ? en : 0u;
                pm |= pass & (1u << j);
                vm_load32(WA.w[j], (WA.p[j] >> (sh_bm + 3)) & (pass & l2mask), P.bitmap);   // offset 0 when idle
            }
            WA.pm = pm;
            WA.t = have ? t : PIPE_NONE;
            wave_lds_sync();   // all lanes are done with the slice before the next step overwrites it
        }
        // ---- everything issued up to stage B of the previous step has arrived
        vm_wait<YOUNGER_THAN_S>();
        // ---- stage C
        if (SC.t != PIPE_NONE) {
            vm_ready(SC.v0); vm_ready(SC.v1);
            const bool hit0 = SC.v0.x == SC.key0 || SC.v0.y == SC.key0 || SC.v0.z == SC.key0 || SC.v0.w == SC.key0;
            const bool hit1 = SC.v1.x == SC.key1 || SC.v1.y == SC.key1 || SC.v1.z == SC.key1 || SC.v1.w == SC.key1;
            const bool open0 = SC.v0.x == EMPTY32 || SC.v0.y == EMPTY32 || SC.v0.z == EMPTY32 || SC.v0.w == EMPTY32;
            const bool open1 = SC.v1.x == EMPTY32 || SC.v1.y == EMPTY32 || SC.v1.z == EMPTY32 || SC.v1.w == EMPTY32;
            const bool on0 = SC.fl & 1u, on1 = SC.fl & 2u;
            bool cand = (SC.fl & 4u) || (on0 && hit0) || (on1 && hit1);
            const bool walk0 = on0 && !hit0 && !open0, walk1 = on1 && !hit1 && !open1;
            if ((walk0 || walk1) && !cand) {   // rare: four foreign keys in a row
                if (walk0) cand = sset_walk(P, SC.key0, hash_s16_set(SC.key0, P.s_log2) + 4);
                if (walk1 && !cand) cand = sset_walk(P, SC.key1, hash_s16_set(SC.key1, P.s_log2) + 4);
            }
            const unsigned long long bal = __ballot(cand);
            if (bal) {
                const uint32_t cnt = (uint32_t)__popcll(bal);
                if (cand) obuf[obuf_n + __popcll(bal & ((1ull << lane) - 1))] = SC.t * 64 + lane;
                obuf_n += cnt;   // <= 31 + 64 <= WOBUF
                wave_lds_sync();
                if (obuf_n >= 32) {
                    uint32_t gb = 0;
                    if (lane == 0) gb = atomicAdd(P.n_cand, obuf_n);
                    gb = __shfl(gb, 0);
                    for (uint32_t i = lane; i < obuf_n; i += 64) P.cand[gb + i] = obuf[i];
                    obuf_n = 0;
                    wave_lds_sync();
                }
            }
            SC.t = PIPE_NONE;
        }
        // ---- stage B (always two loads)
        uint32_t p0 = 0, p1 = 0, fl = 0;
        if (WB.t != PIPE_NONE) {
#pragma unroll
            for (int j = 0; j < NP; ++j) vm_ready(WB.w[j]);
            uint32_t mask = 0;
#pragma unroll
            for (int j = 0; j < NP; ++j)   // both bits of the key in its word (index.hip sets two per key)
                mask |= (__builtin_amdgcn_ubfe(WB.w[j], WB.p[j] >> sh_bm, 1) & __builtin_amdgcn_ubfe(WB.w[j], WB.p[j], 1)) << j;
            mask = same ? WB.pm : (mask & WB.pm);
            const uint32_t m2 = mask & (mask - 1), m3 = m2 & (m2 - 1);
            const int j0 = __ffs(mask) - 1, j1 = __ffs(m2) - 1;   // -1 when absent
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                p0 = j0 == j ? WB.p[j] : p0;
                p1 = j1 == j ? WB.p[j] : p1;
            }
            fl = (mask ? 1u : 0u) | (m2 ? 2u : 0u);
            if (m3) {   // rare: third and later passing probes of a lane, looked up on the spot
                bool slow = false;
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    if (((m3 >> j) & 1u) && !slow) {
                        const uint32_t key = WB.p[j] * S16_MUL_INV;
                        slow = sset_walk(P, key, hash_s16_set(key, P.s_log2));
                    }
                }
                fl |= slow ? 4u : 0u;
            }
        }
        SB.fl = fl;
        SB.key0 = p0 * S16_MUL_INV; SB.key1 = p1 * S16_MUL_INV;
        vm_load128(SB.v0, (fl & 1u) ? hash_s16_set(SB.key0, P.s_log2) * 4 : 0u, P.sset);
        vm_load128(SB.v1, (fl & 2u) ? hash_s16_set(SB.key1, P.s_log2) * 4 : 0u, P.sset);
        SB.t = WB.t;
        WB.t = PIPE_NONE;
        prefetch(pf, next_tile(t, 2));
        t = next_tile(t, 1);
    };
    auto done = [&]() { return t >= n_tiles && W0.t == PIPE_NONE && W1.t == PIPE_NONE && S0.t == PIPE_NONE && S1.t == PIPE_NONE; };
    for (;;) {
        //   prefetch regs, A fills, B reads, B fills, C reads
        if (done()) break;
        step(pfA, W0, W1, S0, S1);
        if (done()) break;
        step(pfB, W1, W0, S1, S0);
    }
    vm_wait<0>();
    if (obuf_n) {
        uint32_t gb = 0;
        if (lane == 0) gb = atomicAdd(P.n_cand, obuf_n);
        gb = __shfl(gb, 0);
        for (uint32_t i = lane; i < obuf_n; i += 64) P.cand[gb + i] = obuf[i];
    }
}

// Probed 16-mers of a read: offsets first + j * stride, stride = k - 15.  A k-mer at offset p in [0, L - k] covers the 16-mer
// offsets [p, p + stride - 1], so the probes must start at first <= k - 16 and reach L - k: np = floor((L - k) / stride) + 1 of
// them do — one fewer than probing from offset 0 to the end of the read whenever (L - 16) mod stride < k - 16 (150-base reads:
// k = 51: 3 instead of 4, k = 41: 5 instead of 6, k = 31: 8 instead of 9).  first = the byte-aligned offset closest below k - 16
// that still reaches (the pipelined kernel fetches byte-aligned probes faster).
// The 256-bucket filter checks `ext` more bases behind every seed (Part4Params::ext): a k-mer must then contain the 16-mer AND
// those bases, so the stride is k - 15 - ext and first <= k - 16 - ext; ext = the most (<= 2) that leaves np as it is
// (150-base reads: k = 51: 2, stride 34; k = 41: 2; k = 31: 1).
ProbeSpots probe_geometry(int read_len, int k, bool ext_allowed) {
    const int stride = k - 15;
    int ext = 0;
    if (ext_allowed)
        for (int e = 2; e >= 1 && !ext; --e)
            if (stride - e >= 1 && (read_len - k) / (stride - e) == (read_len - k) / stride) ext = e;
    ProbeSpots g;
    g.ext = (uint32_t)ext;
    g.stride = (uint32_t)(stride - ext);
    g.np = (uint32_t)((read_len - k) / (int)g.stride + 1);
    g.first = (uint32_t)(k - 16 - ext);
    const int lo = (read_len - k) - (int)(g.np - 1) * (int)g.stride;
    const uint32_t al = g.first & ~3u;
    if ((int)al >= lo) g.first = al;
    return g;
}

// The pipelined kernel's instantiations: the kernel and the name rocprofv3 prints for it, in one entry (gf_screen_kernels reports the
// entry launched).  Five probe slots cover reads with fewer (EXACT = false: a test per slot); six to ten are unrolled exactly.
struct PipeKernel {
    uint32_t nch, npt;
    bool exact;
    void (*fn)(FilterParams, uint32_t);
    const char* name;
};
#define PIPE_K(N, Q, E) {N, Q, E, screen_filter_pipe_kernel<N, Q, E>, "screen_filter_pipe_kernel<" #N ", " #Q ", " #E ">"}
#define PIPE_K4(Q, E) PIPE_K(1, Q, E), PIPE_K(2, Q, E), PIPE_K(3, Q, E), PIPE_K(4, Q, E)
static const PipeKernel PIPE_KERNELS[] = {PIPE_K4(5, false), PIPE_K4(5, true), PIPE_K4(6, true), PIPE_K4(7, true), PIPE_K4(8, true), PIPE_K4(9, true), PIPE_K4(10, true)};
#undef PIPE_K4
#undef PIPE_K
static const PipeKernel* pipe_kernel(uint32_t nch, uint32_t npt, bool exact) {
    for (const PipeKernel& e : PIPE_KERNELS)
        if (e.nch == nch && e.npt == npt && e.exact == exact) return &e;
    return nullptr;
}

// What launch_screen will do for n_reads reads of read_len bases against index ix under the context's options (screen_variant: 0 =
// automatic; 9 / 13 force the plain / pipelined form, 16 / 17 the partitioned form with whole-line / unaligned stores, 18 = 16 without
// a probe column — the parity tests run every one of them on the same inputs).
static void plan_pf4(const gf_ctx* ctx_or_null, ScreenPlan& S, size_t n_reads);
ScreenPlan plan_screen(const gf_ctx* ctx, const FlankIndex& ix, size_t n_reads, int read_len) {
    ScreenPlan S = {};
    const int variant = ctx->screen_variant;
    const uint32_t rb = (uint32_t)((read_len + 3) / 4);
    const size_t tiles64 = (n_reads + 63) / 64;
    S.rb = rb;
    // is the 256-bucket partitioned filter eligible?  (Its geometry — bases checked behind a seed — holds wherever it is, also where
    // the pipelined kernel is then taken.)
    const bool pf4_ok = (variant == 16 || variant == 17 || variant == 18 || (variant == 0 && n_reads >= (1u << 20))) && ix.bm_log2 >= 27 &&
                        ix.bm_log2 <= 28 && rb <= 64 && ix.d_sgrp && pf4_scatter_lds_bytes(pf4_slice_words(rb)) <= 156 * 1024;
    S.pg = probe_geometry(read_len, ix.k, pf4_ok && ctx->screen_ext);
    const uint32_t np = S.pg.np;

    // the LDS pre-filter pays while the coarse bitmap is sparse enough to stop most probes before L2 and a handful of waves
    // fit next to it (long reads leave too few); the pipelined form covers up to 10 probes and 64 packed bytes per read
    const size_t w_bm_bytes = ix.d_bitmap_lds ? ((size_t)1 << ix.lds_log2) / 8 : 0;
    const size_t w_slice_words = ((size_t)64 * rb + 16 + 15) / 16 * 4;
    const size_t w_per_wave = (w_slice_words + WOBUF) * 4;
    const size_t w_nw = std::min<size_t>(16, (160 * 1024 - 512 - w_bm_bytes) / w_per_wave);
    const int nch = (rb + 15) / 16 <= 4 ? (int)((rb + 15) / 16) : 0;
    const bool lds_auto = ix.d_bitmap_lds && ix.lds_fill <= 0.6 && variant == 0 && w_nw >= 6;
    const bool lds_forced = variant == 13 && ix.d_bitmap_lds && w_nw >= 2;
    const bool pipe_ok = np >= 1 && np <= 10 && ix.lds_log2 >= 7 && nch >= 1;
    if ((lds_auto || lds_forced) && pipe_ok) {
        S.form = ScreenForm::pipe;
        S.nw = (uint32_t)std::min<size_t>(w_nw, 8);   // measured: 8 waves x 256 VGPRs beat 11 x 168
        S.nch = (uint32_t)nch;
        S.npt = std::max(5u, np);                     // probes per read, unrolled
        S.exact = np == S.npt;
        S.pipe = pipe_kernel(S.nch, S.npt, S.exact);
        S.pipe_grid = (unsigned)std::min<size_t>((tiles64 + S.nw - 1) / S.nw, ctx->n_cu);
        S.pipe_slice_words = w_slice_words;
        S.pipe_lds_bytes = w_bm_bytes + S.nw * w_per_wave;
        return S;
    }
    if (!pf4_ok) {
        S.form = ScreenForm::plain;
        return S;
    }
    plan_pf4(ctx, S, n_reads);
    return S;
}

// The partitioned filter (256 buckets, 4-byte pairs, see Part4Params) for S.rb and S.pg: the form of pass A, its parts and the workspace.
// Nothing here reads the index — what pass A leaves depends on the reads and these numbers alone, which is why a library may keep it
// (fill_parts_geom).  ctx null: the default options on a device of 256 CUs.
static void plan_pf4(const gf_ctx* ctx, ScreenPlan& S, size_t n_reads) {
    const int variant = ctx ? ctx->screen_variant : 0, n_cu = ctx ? ctx->n_cu : 256, writers = ctx ? ctx->screen_pf4_writers : 0,
              cap8_opt = ctx ? ctx->screen_pf4_cap8 : 0;
    const uint32_t rb = S.rb, np = S.pg.np;
    const size_t tiles64 = (n_reads + 63) / 64;
    S.bytes = ((2 * S.pg.first) & 7u) == 0 && ((2 * S.pg.stride) & 7u) == 0;
    S.slice_words = pf4_slice_words(rb);
    const size_t tiles_wg = (size_t)PF2_WAVES * PF2_TILES;      // tiles per workgroup and iteration
    // (the pair list carries the writer in 8 bits; an empty read set plans like one tile — nothing is launched for it)
    S.n_writers = (uint32_t)std::max<size_t>(std::min<size_t>(std::min<size_t>((tiles64 + tiles_wg - 1) / tiles_wg, (size_t)n_cu), 256), 1);
    if (writers > 0) S.n_writers = std::min(S.n_writers, (uint32_t)writers);   // tests: long parts on small inputs (several trips of pass B)
    S.tiles_wg = (uint32_t)tiles_wg;
    const size_t n_iter = (tiles64 + (size_t)S.n_writers * tiles_wg - 1) / ((size_t)S.n_writers * tiles_wg);
    const double pairs_w = (double)n_iter * tiles_wg * 64.0 * np;
    const double expect = pairs_w / PF2_NB;
    S.cap = ((uint32_t)(expect * 1.05 + 6.0 * std::sqrt(expect + 1.0) + 128.0) + 63u) & ~63u;
    // whole-line stores (pf4_scatter_lines_kernel) where all probes of a read make one or two groups, the open lines fit beside the tiles
    // and a line's index in `pairs` fits 32 bits (screen_variant 17: the unaligned form all the same)
    S.grp = np < PF2_GROUP ? (np ? np : 1u) : PF2_GROUP;   // probes per sorted group
    S.n_grp = (np + S.grp - 1) / S.grp;
    const bool lines = S.n_grp <= 2 && pf4_lines_lds_bytes(S.slice_words, S.grp) <= 160 * 1024 && variant != 17 &&
                       (uint64_t)PF2_NB * S.n_writers * (S.cap >> 5) + 1 < 0xFFFFFFFFull;
    S.form = lines ? ScreenForm::pf4_lines : ScreenForm::pf4_runs;
    // the library's probe column instead of its rows: only the whole-line form with all probes in one group (screen_variant 18: the rows all the same)
    S.col_ok = lines && S.n_grp == 1 && variant != 18;
    S.lds_a = lines ? pf4_lines_lds_bytes(S.slice_words, S.grp) : pf4_scatter_lds_bytes(S.slice_words);
    S.lds_a_col = pf4_lines_lds_bytes(0, S.grp);
    S.n_groups = (uint32_t)(n_iter * S.n_grp);
    S.gs = (S.n_groups + 1 + 15) & ~15u;
    S.cap8 = (uint32_t)(std::min<size_t>(std::max<size_t>((size_t)1 << 22, n_reads / 2), 0x7FFFFFFFu) / PF4_CHUNK * PF4_CHUNK);
    if (cap8_opt > 0) S.cap8 = (uint32_t)std::max(1, cap8_opt / (int)PF4_CHUNK) * PF4_CHUNK;   // tests: a short pair list (the serial path)
    S.plane = ((uint64_t)n_reads + 63) & ~(uint64_t)63;
    const size_t b_pairs = (size_t)PF2_NB * S.n_writers * S.cap * 4, b_cnt = ((size_t)PF2_NB * S.n_writers * 4 + 255 + 256) & ~(size_t)255,
                 b_seen = (((size_t)n_reads + 31) / 32 * 4 + 255) & ~(size_t)255, b_fill = (size_t)PF2_NB * S.n_writers * S.gs * 4,
                 b_c8 = ((size_t)S.cap8 * 12 + S.cap8 / PF4_CHUNK + 1 + 255) & ~(size_t)255;
    S.o_n_cand8 = b_cnt - 256;
    S.o_seen = b_cnt;
    S.o_cand8 = b_cnt + b_seen;
    S.o_cand8x = S.o_cand8 + (size_t)S.cap8 * 8;
    S.o_chunk_b = S.o_cand8 + (size_t)S.cap8 * 12;
    S.o_fills = S.o_cand8 + b_c8;
    S.o_pairs = S.o_fills + b_fill;
    S.ws_bytes = S.o_pairs + b_pairs + 1024;
    S.ws_bytes_resident = S.o_fills;
    S.zero_bytes = 256 + b_seen;
}

// ix: the flank index of k when the context has gaps (the column is then wanted only where the screen would stream it), or null
void fill_probe_geom(gf_ctx* ctx, const FlankIndex* ix, size_t n_reads, int read_len, int k, gf_probe_geom* g) {
    const ProbeSpots pg = probe_geometry(read_len, k, !ctx || ctx->screen_ext != 0);
    const uint32_t rb = (uint32_t)((read_len + 3) / 4);
    // a column pays where it is at most half the row; the column form of pass A takes up to four probes of reads the whole-line form
    // takes — and, with a context and an index, only where the plan of that screen says so
    g->reserved = 0;
    g->use = pg.np >= 1 && pg.np <= 4 && 2 * 4 * pg.np <= rb && rb <= 64 && pf4_lines_lds_bytes(pf4_slice_words(rb), pg.np) <= 160 * 1024 &&
             (!ctx || !ix || (n_reads < 0xFFFFFFFFull && plan_screen(ctx, *ix, n_reads, read_len).col_ok));
    g->n_reads = n_reads;
    g->read_len = (uint32_t)read_len;
    g->k = (uint32_t)k;
    g->first = pg.first;
    g->stride = pg.stride;
    g->np = pg.np;
    g->ext = pg.ext;
}

// What a library's resident parts depend on and whether they are kept (`use`): the probe geometry, and of the plan the numbers that
// shape pass A's output.  With an index the plan is the one the screen itself will make; without (no gaps yet, or no context) the one
// the partitioned filter would have.  Returns that plan: the build launches its pass A.
ScreenPlan fill_parts_geom(gf_ctx* ctx, const FlankIndex* ix, size_t n_reads, int read_len, int k, gf_screen_parts_geom* g) {
    fill_probe_geom(ctx, ix, n_reads, read_len, k, &g->probe);
    ScreenPlan S = {};
    if (n_reads < 0xFFFFFFFFull) {
        if (ctx && ix) S = plan_screen(ctx, *ix, n_reads, read_len);
        else {
            S.rb = (uint32_t)((read_len + 3) / 4);
            S.pg = probe_geometry(read_len, k, !ctx || ctx->screen_ext != 0);
            if (S.rb <= 64 && pf4_scatter_lds_bytes(pf4_slice_words(S.rb)) <= 156 * 1024) plan_pf4(ctx, S, n_reads);
        }
    }
    g->use = g->probe.use && S.col_ok && S.cap < (1u << 24);
    g->n_writers = S.n_writers;
    g->cap = S.cap;
    g->gs = S.gs;
    g->n_groups = S.n_groups;
    g->n_grp = S.n_grp;
    g->tiles_wg = S.tiles_wg;
    g->reserved = 0;
    return S;
}

// is the handed column one that pass A may stream for this plan: built for exactly this call's reads and geometry?
static bool column_fits(const ScreenPlan& S, int k, size_t n_reads, int read_len, const void* d_probes, const gf_probe_geom* built_for) {
    return S.col_ok && d_probes && built_for && built_for->use && built_for->n_reads == n_reads && built_for->read_len == (uint32_t)read_len &&
           built_for->k == (uint32_t)k && built_for->first == S.pg.first && built_for->stride == S.pg.stride && built_for->np == S.pg.np &&
           built_for->ext == S.pg.ext;
}

// are the handed parts what pass A of this plan would leave: built for exactly this call's reads, geometry and parts?
static bool parts_fit(const ScreenPlan& S, int k, size_t n_reads, int read_len, const void* d_parts, const gf_screen_parts_geom* b) {
    return d_parts && b && b->use && column_fits(S, k, n_reads, read_len, d_parts, &b->probe) && b->n_writers == S.n_writers && b->cap == S.cap &&
           b->gs == S.gs && b->n_groups == S.n_groups && b->n_grp == S.n_grp && b->tiles_wg == S.tiles_wg;
}

static FilterParams filter_params(const gf_ctx* ctx, const FlankIndex& ix, const ScreenPlan& S, const void* d_reads, size_t n_reads) {
    FilterParams F;
    F.reads = (const uint8_t*)d_reads;
    F.n_reads = n_reads;
    F.rb = S.rb;
    F.stride2 = 2 * S.pg.stride;
    F.first2 = 2 * S.pg.first;
    F.np = S.pg.np;
    F.bitmap = ix.d_bitmap;
    F.sset = ix.d_sset;
    F.bm_log2 = ix.bm_log2;
    F.s_log2 = ix.s_log2;
    F.cand = (uint32_t*)ctx->cand.p;
    F.n_cand = (uint32_t*)ctx->counters.p;
    F.bitmap_lds = ix.d_bitmap_lds;
    F.lds_log2 = ix.lds_log2;
    F.stream_policy = (uint32_t)ctx->screen_stream_policy;
    F.bitmap_mid = ix.mid_log2 ? ix.d_bitmap_mid : nullptr;
    F.mid_log2 = (uint32_t)ix.mid_log2;
    return F;
}

static int launch_filter_plain(gf_ctx* ctx, const ScreenPlan& S, const FilterParams& F) {
    const size_t n_tiles = ((size_t)F.n_reads + TILE_READS - 1) / TILE_READS;
    const unsigned grid = (unsigned)std::min<size_t>(n_tiles, (size_t)ctx->n_cu * 8);
    ctx->screen_kernels = "screen_filter_kernel<9>";
    LaunchTimer tm(ctx, GF_KERNEL_SCREEN);
    hipLaunchKernelGGL(screen_filter_kernel<9>, dim3(grid), dim3(256), TILE_READS * S.rb + 16, ctx->stream, F);
    return GF_OK;
}

// software-pipelined wave kernel (three tiles in flight per wave)
static int launch_filter_pipe(gf_ctx* ctx, const ScreenPlan& S, const FilterParams& F) {
    if (!S.pipe) return GF_E_UNSUPPORTED;   // (the plan takes this form only for chunk and probe counts the table holds)
    ctx->screen_kernels = S.pipe->name;
    LaunchTimer tm(ctx, GF_KERNEL_SCREEN);
    hipLaunchKernelGGL(S.pipe->fn, dim3(S.pipe_grid), dim3(S.nw * 64), S.pipe_lds_bytes, ctx->stream, F, (uint32_t)S.pipe_slice_words);
    return GF_OK;
}

// gf_stream_wait_after_filter: the peer's stream goes on once the filter pass has finished
static int wait_after_filter(gf_ctx* ctx, gf_ctx* waiter) {
    hipEvent_t ev;
    GF_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(waiter->stream, ev, 0);
    (void)hipEventDestroy(ev);
    if (e != hipSuccess) return set_hip_error(ctx, e, "gf_stream_wait_after_filter");
    return GF_OK;
}

int launch_screen(gf_ctx* ctx, const FlankIndex& ix, const void* d_reads, const void* d_nmask, size_t n_reads,
                  int read_len, int min_hits, void* d_out, size_t cap, void* d_n_out, const void* d_probes, const gf_probe_geom* built_for,
                  const void* d_parts, const gf_screen_parts_geom* parts_for) {
    // one-shot (gf_stream_wait_after_filter): taken here, so that no exit below leaves it armed for a later, unrelated pass
    gf_ctx* const waiter = ctx->after_filter;
    ctx->after_filter = nullptr;
    if (read_len < ix.k || read_len > 1000) return GF_E_INVAL;
    if (n_reads >= 0xFFFFFFFFull || cap > 0xFFFFFFFFull) return GF_E_INVAL;
    if ((read_len + 3) / 4 > 250) return GF_E_UNSUPPORTED;
    int rc;
    if ((rc = ensure(ctx, ctx->cand, std::max<size_t>(n_reads, 1) * 4))) return rc;
    if ((rc = ensure(ctx, ctx->counters, GF_COUNTER_BYTES))) return rc;
    // [0] n_cand [1] error overflow [2] [3] [4] the overflow lists of the verification passes
    zero_regions(ctx, ZeroList{{(uint32_t*)ctx->counters.p, (uint32_t*)d_n_out, nullptr, nullptr}, {5, 1, 0, 0}});
    if (n_reads == 0) return GF_OK;

    const ScreenPlan S = plan_screen(ctx, ix, n_reads, read_len);
    const FilterParams F = filter_params(ctx, ix, S, d_reads, n_reads);
    switch (S.form) {
        case ScreenForm::pipe: rc = launch_filter_pipe(ctx, S, F); break;
        case ScreenForm::plain: rc = launch_filter_plain(ctx, S, F); break;
        default:
            rc = launch_filter_pf4(ctx, ix, S, F, column_fits(S, ix.k, n_reads, read_len, d_probes, built_for) ? d_probes : nullptr,
                                   parts_fit(S, ix.k, n_reads, read_len, d_parts, parts_for) ? d_parts : nullptr);
            break;
    }
    if (rc) return rc;
    GF_HIP(ctx, hipGetLastError());
    if (waiter && (rc = wait_after_filter(ctx, waiter))) return rc;
    return launch_verify_passes(ctx, ix, S.pg, d_reads, d_nmask, n_reads, read_len, min_hits, d_out, cap, d_n_out);
}

// A library's resident parts: pass A alone into the caller's buffer (a set-up call: it waits for the stream once, to read how many pairs
// found their part full — any, and the parts are not kept)
int launch_parts_build(gf_ctx* ctx, const FlankIndex* ix, const void* d_reads, const void* d_probes, const gf_probe_geom* probes_for, size_t n_reads,
                       int read_len, int k, void* d_parts, gf_screen_parts_geom* built_for) {
    if (n_reads >= 0xFFFFFFFFull) return GF_E_INVAL;
    const ScreenPlan S = fill_parts_geom(ctx, ix, n_reads, read_len, k, built_for);
    if (n_reads == 0) built_for->use = 0;
    if (!built_for->use) return GF_OK;
    int rc;
    if ((rc = ensure(ctx, ctx->counters, GF_COUNTER_BYTES))) return rc;
    uint32_t* spills = (uint32_t*)ctx->counters.p + 5;   // ([0, 5): the screen's own)
    GF_HIP(ctx, hipMemsetAsync(spills, 0, 4, ctx->stream));
    FilterParams F = {};
    F.reads = (const uint8_t*)d_reads;
    F.n_reads = n_reads;
    F.rb = S.rb;
    F.stride2 = 2 * S.pg.stride;
    F.first2 = 2 * S.pg.first;
    F.np = S.pg.np;
    if ((rc = launch_pass_a_build(ctx, S, F, column_fits(S, k, n_reads, read_len, d_probes, probes_for) ? d_probes : nullptr, d_parts, spills))) return rc;
    GF_HIP(ctx, hipGetLastError());
    uint32_t n_spilled = 0;
    GF_HIP(ctx, hipMemcpyAsync(&n_spilled, spills, 4, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_spilled) built_for->use = 0;
    return GF_OK;
}

}  // namespace gf
