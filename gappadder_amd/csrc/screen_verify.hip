// screen_verify.hip — exact verification of the filter's candidates (VerifyParams: screen_dev.hpp):
//   screen_verify_ext_kernel   seed and extend against the packed flanks (min_hits == 1, no repeat mask)
//   screen_verify_kernel       every k-mer position through the k-mer -> gap table, per-gap position count >= min_hits
#include "screen_dev.hpp"

namespace gf {

struct __attribute__((packed, aligned(4))) Slots4 { uint32_t x, y, z, w; };

__device__ __forceinline__ uint32_t packed_word(const VerifyParams& P, uint64_t w) {
    if (w < P.n_words) return P.reads32[w];
    uint32_t v = 0;
    if (w == P.n_words) {
        const uint8_t* t = reinterpret_cast<const uint8_t*>(P.reads32 + P.n_words);
        for (uint32_t i = 0; i < P.tail_bytes; ++i) v |= (uint32_t)t[i] << (8 * i);
    }
    return v;
}

// read r of the packed array, re-aligned to a word boundary, into row[0 .. rw) (zero behind its rb bytes).  The words are fetched
// sixteen at a time before any is used: a lane's fetches are independent, one round of global latency per sixteen words (fetched and
// stored one by one, every word of a candidate cost the wave a round trip: 60 us per 64 candidates at C4)
__device__ __forceinline__ void stage_read(const VerifyParams& P, uint32_t* row, uint32_t rw, uint32_t r, bool active) {
    const uint64_t o = (uint64_t)r * P.rb;
    const uint64_t w0 = o >> 2;
    const uint32_t sh = (uint32_t)(o & 3) * 8;
    const uint32_t nw = (P.rb + 3) / 4;
    for (uint32_t i0 = 0; i0 < rw; i0 += 16) {
        uint32_t x[17];
#pragma unroll
        for (uint32_t t = 0; t < 17; ++t) x[t] = (active && i0 + t <= nw) ? packed_word(P, w0 + i0 + t) : 0u;
#pragma unroll
        for (uint32_t t = 0; t < 16; ++t) {
            const uint32_t i = i0 + t;
            if (i >= rw) break;
            uint32_t v = sh ? (x[t] >> sh) | (x[t + 1] << (32 - sh)) : x[t];
            if (i >= nw) v = 0;
            else if (i == nw - 1 && (P.rb & 3)) v &= (1u << ((P.rb & 3) * 8)) - 1;   // drop the next read's bytes
            row[i] = v;
        }
    }
}

// One wavefront per workgroup.  A wave takes 64 candidates at a time: lane j fetches candidate j's packed read
// into LDS (one round of global latency for 64 reads), then the whole wave verifies the candidates one by one —
// lane = k-mer position, two positions per lane in flight, one 16-B (32-B for k > 32) slot load per probe step.
template <bool WIDE>
__global__ __launch_bounds__(64) void screen_verify_kernel(VerifyParams P) {
    extern __shared__ uint32_t sm[];  // [64][rw] read words | list[list_cap]
    constexpr uint32_t OBUF = 128;    // hits buffered per wave: one global atomic per >= 64 hits (see filter kernel)
    __shared__ gf_hit obuf[OBUF];
    __shared__ uint32_t obuf_n;
    const uint32_t lane = threadIdx.x;
    if (lane == 0) obuf_n = 0;
    const uint32_t rw = (P.rb + 24) / 4 + 1;  // words per staged read, zero padded (stream_kmer reads past the end)
    uint32_t* list = sm + 64 * rw;
    const uint32_t n_cand = *P.n_cand;
    const uint32_t npos = P.read_len - P.k + 1;
    const uint32_t tmask = (1u << P.t_log2) - 1;
    const bool gate = P.sset != nullptr && P.np >= 1 && P.np <= 32;

    // 64 candidates per wave and pass.  (Measured: smaller batches on more concurrent waves are SLOWER — the pass is bound by
    // random 16-B table loads served from the Infinity Cache, not by wave count.)
    const uint32_t bsz = P.batch;
    for (uint32_t c0 = blockIdx.x * bsz; c0 < n_cand; c0 += gridDim.x * bsz) {
        const uint32_t nb = n_cand - c0 < bsz ? n_cand - c0 : bsz;
        const uint32_t my_r = lane < nb ? P.cand[c0 + lane] : 0;
        stage_read(P, sm + lane * rw, rw, my_r, lane < nb);   // my candidate's read
        __syncthreads();
        // Window gate.  A k-mer of the read can only equal a flank k-mer if the ONE probed 16-mer it contains
        // (offset first + q * stride, q = ceil((p - first) / stride) or 0; stride = k - 15) is a flank 16-mer.  Every lane looks its own
        // candidate's np aligned 16-mers up in the exact set (three lookups in flight, four slots per request), so the
        // table below is only consulted around real 16-mer hits: a chance candidate costs ~k-15 table reads, not L-k+1.
        uint32_t my_gate = 0xFFFFFFFFu;
        if (gate) {
            my_gate = 0;
            if (lane < nb) {
                const uint32_t* row = sm + lane * rw;
                for (uint32_t q0 = 0; q0 < P.np; q0 += 3) {
                    uint32_t key[3];
                    Slots4 v[3];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const uint32_t q = q0 + u < P.np ? q0 + u : P.np - 1;
                        key[u] = canon16(stream32(row, 2 * (P.first + q * P.stride)));
                        v[u] = *reinterpret_cast<const Slots4*>(P.sset + hash_s16_set(key[u], (int)P.s_log2));
                    }
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        if (q0 + u >= P.np) continue;
                        bool hit = v[u].x == key[u] || v[u].y == key[u] || v[u].z == key[u] || v[u].w == key[u];
                        const bool open = v[u].x == EMPTY32 || v[u].y == EMPTY32 || v[u].z == EMPTY32 || v[u].w == EMPTY32;
                        if (!hit && !open) {   // rare: four foreign keys in a row
                            uint32_t sl = hash_s16_set(key[u], (int)P.s_log2) + 4;
                            for (;;) {
                                const uint32_t x = P.sset[sl & ((1u << P.s_log2) - 1)];
                                if (x == key[u]) { hit = true; break; }
                                if (x == EMPTY32) break;
                                ++sl;
                            }
                        }
                        my_gate |= (uint32_t)hit << (q0 + u);
                    }
                }
            }
        }
        for (uint32_t j = 0; j < nb; ++j) {
            const uint32_t r = __shfl(my_r, j);
            const uint32_t gate_j = __shfl(my_gate, j);
            const uint32_t* rwp = sm + j * rw;
            uint32_t n = 0;  // (position, gap) matches of this read; wave-uniform, appended by ballot + prefix count
            for (uint32_t pp = 0; pp < npos; pp += 128) {
                K128 cn[2];
                uint32_t slot[2];
                bool act[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t p = pp + lane + 64 * u;
                    act[u] = p < npos;
                    if (gate && act[u]) act[u] = (gate_j >> (p <= P.first ? 0u : (p - P.first + P.stride - 1) / P.stride)) & 1u;
                    if (act[u] && P.nmask) {  // any N inside [p, p+k) ?
                        for (uint32_t q = p; q < p + P.k; ++q)
                            if ((P.nmask[(uint64_t)r * P.nmw + (q >> 5)] >> (q & 31)) & 1u) { act[u] = false; break; }
                    }
                    cn[u] = K128{0, 0};
                    slot[u] = 0;
                    if (act[u]) {
                        if (WIDE) cn[u] = canonical(stream_kmer(rwp, 2 * p, (int)P.k), (int)P.k);
                        else cn[u] = K128{canonical64(stream_kmer64(rwp, 2 * p, (int)P.k), (int)P.k), 0};   // k <= 32: one word
                        slot[u] = hash_kmer(cn[u], (int)P.t_log2);
                    }
                }
                // wave-uniform probe steps; finished lanes idle.  Two consecutive slots per step and position: the common chain
                // (one matching entry, then the EMPTY terminator) ends in ONE round trip — the kernel walks its 64 candidates
                // one after the other, so round trips per candidate set its pace
                while (__any(act[0] || act[1])) {
                    uint4 a[2][2], b[2][2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
#pragma unroll
                        for (int d = 0; d < 2; ++d) {
                            a[u][d] = make_uint4(0, 0, EMPTY32, 0);
                            b[u][d] = make_uint4(EMPTY32, 0, 0, 0);
                            if (act[u]) {
                                const uint64_t sl = (slot[u] + d) & tmask;
                                if (WIDE) { a[u][d] = P.table[2 * sl]; b[u][d] = P.table[2 * sl + 1]; }
                                else a[u][d] = P.table[sl];
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
#pragma unroll
                        for (int d = 0; d < 2; ++d) {
                            const uint32_t g = WIDE ? b[u][d].x : a[u][d].z;
                            bool eq = false;
                            if (act[u]) {
                                if (g == EMPTY32) act[u] = false;
                                else {
                                    eq = (((uint64_t)a[u][d].y << 32) | a[u][d].x) == cn[u].hi;
                                    if (WIDE) eq = eq && (((uint64_t)a[u][d].w << 32) | a[u][d].z) == cn[u].lo;
                                }
                            }
                            const unsigned long long bal = __ballot(eq);
                            if (bal) {
                                const uint32_t o = n + __popcll(bal & ((1ull << lane) - 1));
                                if (eq && o < P.list_cap) list[o] = g;
                                n += (uint32_t)__popcll(bal);
                            }
                        }
                        slot[u] = (slot[u] + 2) & tmask;
                    }
                }
            }
            __syncthreads();
            if (n > P.list_cap) {  // rare (repeat-rich flanks): defer this read to the large-list launch
                if (lane == 0) {
                    const uint32_t o = atomicAdd(P.overflow, 1u);
                    if (P.overflow_list) P.overflow_list[o] = r;
                }
                n = 0;
            }
            // distinct gaps and their position counts.  Up to 256 matches: entries held in registers, one wave
            // step per DISTINCT gap (ballot + popcount); longer lists (pass 2 only): quadratic scan in LDS.
            if (n <= 256) {
                uint32_t v[4];
                bool todo[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = lane + 64 * u;
                    todo[u] = i < n;
                    v[u] = todo[u] ? list[i] : 0;
                }
                while (true) {
                    const unsigned long long b0 = __ballot(todo[0]), b1 = __ballot(todo[1]), b2 = __ballot(todo[2]),
                                             b3 = __ballot(todo[3]);
                    if (!(b0 | b1 | b2 | b3)) break;
                    uint32_t g;
                    if (b0) g = __shfl(v[0], __ffsll((long long)b0) - 1);
                    else if (b1) g = __shfl(v[1], __ffsll((long long)b1) - 1);
                    else if (b2) g = __shfl(v[2], __ffsll((long long)b2) - 1);
                    else g = __shfl(v[3], __ffsll((long long)b3) - 1);
                    uint32_t cnt = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool m = todo[u] && v[u] == g;
                        cnt += (uint32_t)__popcll(__ballot(m));
                        if (m) todo[u] = false;
                    }
                    if (cnt >= P.min_hits) {
                        if (lane == 0) obuf[obuf_n] = gf_hit{g, r};
                        __syncthreads();
                        if (lane == 0) obuf_n = obuf_n + 1;
                        __syncthreads();
                    }
                    if (obuf_n >= OBUF - 64) {
                        const uint32_t nn = obuf_n;
                        uint32_t gb = 0;
                        if (lane == 0) gb = atomicAdd(P.n_out, nn);
                        gb = __shfl(gb, 0);
                        for (uint32_t q = lane; q < nn; q += 64)
                            if (gb + q < P.cap) P.out[gb + q] = obuf[q];
                        __syncthreads();
                        if (lane == 0) obuf_n = 0;
                        __syncthreads();
                    }
                }
            } else
            for (uint32_t i0 = 0; i0 < n; i0 += 64) {
                const uint32_t i = i0 + lane;
                bool emit = false;
                uint32_t g = 0;
                if (i < n) {
                    g = list[i];
                    uint32_t cnt = 0;
                    bool first = true;
                    for (uint32_t q = 0; q < n; ++q) {
                        if (list[q] == g) {
                            ++cnt;
                            if (q < i) first = false;
                        }
                    }
                    emit = first && cnt >= P.min_hits;
                }
                const unsigned long long bal = __ballot(emit);
                if (bal) {  // single wave per block: obuf_n is only touched here, in lock-step
                    const uint32_t base = obuf_n;
                    if (emit) obuf[base + __popcll(bal & ((1ull << lane) - 1))] = gf_hit{g, r};
                    __syncthreads();
                    if (lane == 0) obuf_n = base + (uint32_t)__popcll(bal);
                    __syncthreads();
                    if (obuf_n >= OBUF - 64) {
                        const uint32_t nn = obuf_n;
                        uint32_t gb = 0;
                        if (lane == 0) gb = atomicAdd(P.n_out, nn);
                        gb = __shfl(gb, 0);
                        for (uint32_t q = lane; q < nn; q += 64)
                            if (gb + q < P.cap) P.out[gb + q] = obuf[q];
                        __syncthreads();
                        if (lane == 0) obuf_n = 0;
                        __syncthreads();
                    }
                }
            }
            __syncthreads();
        }
        __syncthreads();
    }
    __syncthreads();
    if (obuf_n) {
        const uint32_t nn = obuf_n;
        uint32_t gb = 0;
        if (lane == 0) gb = atomicAdd(P.n_out, nn);
        gb = __shfl(gb, 0);
        for (uint32_t q = lane; q < nn; q += 64)
            if (gb + q < P.cap) P.out[gb + q] = obuf[q];
    }
}

// ---- seed-and-extend verification (min_hits == 1, no repeat mask) -----------------------------------------------------
// A read k-mer at offset p equals a flank k-mer (either strand) iff the ONE probed 16-mer inside it (read offset
// first + q * stride) equals the 16-mer at the corresponding flank position AND the exact match extends from that
// seed far enough to cover [p, p + k) inside the read, the flank's ACGT run and no read N.  So instead of hashing every
// k-mer of a candidate into the 16-B/slot k-mer table (tens of MB: every lookup a fabric request), each aligned 16-mer that
// is a flank 16-mer (exact set, 4 slots per request) is looked up in its occurrence list and the match is extended along
// the diagonal by XOR of 16-base words against the 2-bit packed flanks (0.15 MB at C2: L2/L1 resident):
//   hit(gap)  <=>  some seed/occurrence of that gap has  left_ext + 16 + right_ext >= k,
// extensions capped by k - 16, the read ends, the nearest read N, and the flank's room inside its ACGT run.
// Palindromic 16-mers are tried on both strands.  A candidate lists its gaps in LDS: VEXT_LIST entries in the first pass (64
// candidates per wave); the reads that hit more gaps than that — reads inside a repeat shared by many flanks — go through the
// overflow list to a second launch of this kernel with VEXT_LIST_BIG entries and a few candidates per wave, and only what outgrows
// that as well to the table kernel.  (Round 3 sent every overflow straight to the table kernel: on the planted-repeat workload,
// where 0.5 M reads hit 30-50 gaps each, that pass took 460 ms of a 475-ms step.)
constexpr uint32_t VEXT_STAGE = 1024;    // hits a wave collects in its slice of the staging buffer before one atomic appends them to the list
constexpr uint32_t VEXT_WALK_MAX = 96;   // occurrences one lane of the first pass walks for a (read, seed) before it hands the read to the long-list pass
constexpr uint32_t VEXT_LIST = 16, VEXT_LIST_BIG = 256, VEXT_BATCH_BIG = 8, VEXT_LIST_HUGE = 2048, VEXT_BATCH_HUGE = 2;   // (8 x 256 slots = 8 KiB per wave: a dozen waves per CU; the long list is a hash SET of gaps, full at 192)


__device__ __forceinline__ uint32_t fl32(const uint32_t* words, uint32_t base) {   // 16 bases from base offset `base`, MSB-first words
    const uint32_t d = base >> 4, sh = 2 * (base & 15);
    const uint64_t v = ((uint64_t)words[d] << 32) | words[d + 1];
    return (uint32_t)((v << sh) >> 32);
}

// 64 mask bits starting at bit `start` (may be negative or run past the row: those bits read 0)
__device__ __forceinline__ uint64_t nbits64(const uint32_t* m, int nmw, int start) {
    const int w0 = start >> 5;     // arithmetic shift: floor
    const uint32_t sh = (uint32_t)start & 31;
    uint32_t x[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int idx = w0 + t;
        x[t] = (idx >= 0 && idx < nmw) ? m[idx] : 0u;
    }
    const uint64_t lo = ((uint64_t)x[1] << 32) | x[0];
    return sh ? (lo >> sh) | ((uint64_t)x[2] << (64 - sh)) : lo;
}

__device__ __forceinline__ bool ext_hit(const uint32_t* row, uint32_t qs, const uint32_t* fw, uint32_t f, bool same, uint32_t capL,
                                        uint32_t capR, uint32_t k) {
    // row / fw point at base 0 of the read / flank; both have >= 4 readable words in front and zero padding behind
    uint32_t lext = 0, rext = 0;
    for (uint32_t c = 0; 16 * c < capL; ++c) {
        const uint32_t R = stream32(row - 4, 128 + 2 * (qs - 16 * (c + 1)));
        const uint32_t F = same ? fl32(fw - 4, 64 + f - 16 * (c + 1)) : revpairs32(~fl32(fw - 4, 64 + f + 16 + 16 * c));
        const uint32_t X = R ^ F;
        if (X == 0) { lext += 16; continue; }
        lext += (uint32_t)__builtin_ctz(X) >> 1;
        break;
    }
    lext = lext < capL ? lext : capL;
    for (uint32_t c = 0; 16 * c < capR; ++c) {
        const uint32_t R = stream32(row - 4, 128 + 2 * (qs + 16 + 16 * c));
        const uint32_t F = same ? fl32(fw - 4, 64 + f + 16 + 16 * c) : revpairs32(~fl32(fw - 4, 64 + f - 16 * (c + 1)));
        const uint32_t X = R ^ F;
        if (X == 0) { rext += 16; continue; }
        rext += (uint32_t)__builtin_clz(X) >> 1;
        break;
    }
    rext = rext < capR ? rext : capR;
    return lext + rext + 16 >= k;
}

__global__ __launch_bounds__(64) void screen_verify_ext_kernel(VerifyParams P) {
    extern __shared__ uint32_t sm[];   // rows [64][rwp] | nmask [64][nmw] | slots [64][np] | cnt [64] | lists [batch][vlist]
    constexpr uint32_t OBUF = 128;
    __shared__ gf_hit obuf[OBUF];
    __shared__ uint32_t obuf_n;
    const uint32_t lane = threadIdx.x;
    if (lane == 0) obuf_n = 0;
    // The hit list has ONE counter, and returning atomics on one address are served at 11-15 ns each: the LDS buffer (>= 64 hits)
    // empties into the wave's slice of a global staging buffer, and the slice joins the list a thousand hits at a time (C4: 3.8 M
    // hits per step were 47 000 atomics — half of the kernel's time on that counter's queue).
    gf_hit* const stage = P.stage + (size_t)blockIdx.x * VEXT_STAGE;
    uint32_t stage_n = 0;   // wave-uniform
    auto flush_stage = [&]() {
        uint32_t gb = 0;
        if (lane == 0) gb = atomicAdd(P.n_out, stage_n);
        gb = __shfl(gb, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wave's own stores are in L2; read them back from there (not from L1)
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(stage);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(P.out);
        static_assert(sizeof(gf_hit) == 8, "hits move as 64-bit words");
        for (uint32_t q = lane; q < stage_n; q += 64)
            if (gb + q < P.cap) dst[gb + q] = __hip_atomic_load(src + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stage_n = 0;
    };
    auto put_out = [&](uint32_t nn) {   // obuf[0, nn) -> staging slice
        if (stage_n + nn > VEXT_STAGE) flush_stage();
        for (uint32_t q = lane; q < nn; q += 64) stage[stage_n + q] = obuf[q];
        stage_n += nn;
    };
    const uint32_t rw = (P.rb + 24) / 4 + 1, rwp = rw + 4;
    const uint32_t nmw = P.nmask ? P.nmw : 0;
    uint32_t* rows = sm;
    uint32_t* nmr = rows + 64 * rwp;
    uint32_t* slots = nmr + 64 * nmw;
    uint32_t* cnt = slots + 64 * P.np;
    uint32_t* lists = cnt + 64;
    const uint32_t VL = P.vlist;
    const bool SET = VL > VEXT_LIST;   // (then a power of two)
    const uint32_t n_cand = *P.n_cand;
    const uint32_t W = P.k - 16;
    const uint32_t bsz = P.batch;
    __syncthreads();
    for (uint32_t c0 = blockIdx.x * bsz; c0 < n_cand; c0 += gridDim.x * bsz) {
        const uint32_t nb = n_cand - c0 < bsz ? n_cand - c0 : bsz;
        const uint32_t my_r = lane < nb ? P.cand[c0 + lane] : 0;
        {   // stage my candidate's read, re-aligned to a word boundary, behind 4 zero words
            uint32_t* row = rows + lane * rwp;
            row[0] = row[1] = row[2] = row[3] = 0;
            stage_read(P, row + 4, rw, my_r, lane < nb);
            for (uint32_t i = 0; i < nmw; ++i) nmr[lane * nmw + i] = lane < nb ? P.nmask[(uint64_t)my_r * P.nmw + i] : 0;
            cnt[lane] = 0;
            if (SET) for (uint32_t i = lane; i < bsz * VL; i += 64) lists[i] = EMPTY32;
        }
        __syncthreads();
        // exact-set lookup of every aligned 16-mer of my candidate: slot of the match, or EMPTY32
        if (lane < nb) {
            const uint32_t* row = rows + lane * rwp + 4;
            for (uint32_t q0 = 0; q0 < P.np; q0 += 3) {
                uint32_t key[3], h[3];
                Slots4 v[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const uint32_t q = q0 + u < P.np ? q0 + u : P.np - 1;
                    key[u] = canon16(stream32(row, 2 * (P.first + q * P.stride)));
                    h[u] = hash_s16_set(key[u], (int)P.s_log2);
                    v[u] = *reinterpret_cast<const Slots4*>(P.sset + h[u]);
                }
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    if (q0 + u >= P.np) continue;
                    uint32_t sl = EMPTY32;
                    if (v[u].x == key[u]) sl = h[u];
                    else if (v[u].y == key[u]) sl = h[u] + 1;
                    else if (v[u].z == key[u]) sl = h[u] + 2;
                    else if (v[u].w == key[u]) sl = h[u] + 3;
                    else if (v[u].x != EMPTY32 && v[u].y != EMPTY32 && v[u].z != EMPTY32 && v[u].w != EMPTY32) {
                        uint32_t s2 = h[u] + 4;   // rare: four foreign keys in a row
                        for (;;) {
                            const uint32_t x = P.sset[s2 & ((1u << P.s_log2) - 1)];
                            if (x == key[u]) { sl = s2; break; }
                            if (x == EMPTY32) break;
                            ++s2;
                        }
                    }
                    slots[lane * P.np + q0 + u] = sl == EMPTY32 ? EMPTY32 : (sl & ((1u << P.s_log2) - 1));
                }
            }
        }
        __syncthreads();
        // one work item per (candidate, aligned 16-mer)
        const uint32_t n_items = nb * P.np;
        // what the walks below need of an item: the seed's place in the read and how far an extension may run (wave-uniform in the long-list pass)
        struct Item { const uint32_t* row; uint32_t j, qs; bool ro, pal, ok; uint32_t baseL, baseR; };
        auto item_of = [&](uint32_t i) -> Item {
            Item it;
            it.j = i / P.np;
            const uint32_t q = i - it.j * P.np;
            it.row = rows + it.j * rwp + 4;
            it.qs = P.first + q * P.stride;
            const uint32_t w16 = stream32(it.row, 2 * it.qs);
            const uint32_t key = canon16(w16);
            it.ro = key != w16;
            it.pal = revpairs32(~key) == key;
            it.ok = true;
            uint32_t nl = 64, nr = 64;
            if (nmw) {
                const uint32_t* m = nmr + it.j * nmw;
                if (nbits64(m, (int)nmw, (int)it.qs) & 0xFFFFull) it.ok = false;      // an N inside the seed: no k-mer through it counts
                const uint64_t lb = nbits64(m, (int)nmw, (int)it.qs - 64), rbits = nbits64(m, (int)nmw, (int)it.qs + 16);
                nl = lb ? (uint32_t)__builtin_clzll(lb) : 64;
                nr = rbits ? (uint32_t)__builtin_ctzll(rbits) : 64;
            }
            it.baseL = W < it.qs ? W : it.qs;
            it.baseR = P.read_len - (it.qs + 16);
            it.baseL = it.baseL < nl ? it.baseL : nl;
            it.baseR = it.baseR < W ? it.baseR : W;
            it.baseR = it.baseR < nr ? it.baseR : nr;
            return it;
        };
        // one occurrence {flank, info} of the item's 16-mer: does a k-mer of the read through the seed equal the flank's there?
        auto occ_hits = [&](const Item& it, uint32_t fid, uint32_t info) -> bool {
            const uint32_t f = info & 0xFFFFu, lroom = (info >> 18) & 63u, rroom = (info >> 24) & 63u;
            const bool fo = (info >> 16) & 1u;
            const uint32_t* fw = P.fpk + P.foff[fid];
            bool hit = false;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const bool same = t == 0 ? (it.ro == fo) : (it.ro != fo);
                if (t == 1 && !it.pal) break;
                const uint32_t capL = it.baseL < (same ? lroom : rroom) ? it.baseL : (same ? lroom : rroom);
                const uint32_t capR = it.baseR < (same ? rroom : lroom) ? it.baseR : (same ? rroom : lroom);
                if (capL + capR + 16 < P.k) continue;
                hit = hit || ext_hit(it.row, it.qs, fw, f, same, capL, capR, P.k);
            }
            return hit;
        };
        if (SET) {
            // long-list pass: the reads here sit in repeats, their seeds' occurrence lists hold tens to hundreds of entries — ONE item at a
            // time, its occurrences spread over the lanes (a lane per (read, seed) walked such a list alone: 18 ms on the stress bench).  The
            // gap list is a hash set: one CAS claims a slot, so lanes cannot list a gap twice.
            for (uint32_t i = 0; i < n_items; ++i) {
                const uint32_t slot = slots[i];
                if (slot == EMPTY32) continue;
                const Item it = item_of(i);
                if (!it.ok) continue;
                uint32_t* lj = lists + it.j * VL;
                for (uint32_t oi0 = P.sval[slot];; oi0 += 64) {
                    const uint32_t oi = oi0 + lane;
                    const bool in = oi < P.n_occ;
                    const uint32_t fid = in ? P.occ[2 * (size_t)oi] : 0u, info = in ? P.occ[2 * (size_t)oi + 1] : (1u << 17);
                    const unsigned long long lastb = __ballot((info >> 17) & 1u);
                    const uint32_t n_here = lastb ? (uint32_t)__ffsll((long long)lastb) : 64u;      // lanes below belong to this 16-mer's list
                    if (lane < n_here) {
                        // a gap that is listed already needs no second proof: a low-complexity 16-mer stands at fifty offsets of the same
                        // flank, and the extension is a hundred instructions and four loads, the set look-up five
                        const uint32_t g = fid >> 1;
                        uint32_t hs = (g * 0x9E3779B1u) & (VL - 1);
                        bool listed = false;
                        for (uint32_t pr = 0; pr < VL; ++pr) {
                            const uint32_t x = lj[hs];
                            if (x == g) { listed = true; break; }
                            if (x == EMPTY32) break;
                            hs = (hs + 1) & (VL - 1);
                        }
                        if (!listed && occ_hits(it, fid, info)) {
                            for (uint32_t pr = 0;; ++pr) {      // (from the first free or foreign slot the look-up stopped at)
                                if (pr == VL) { cnt[it.j] = VL + 1; break; }
                                const uint32_t old = atomicCAS(&lj[hs], EMPTY32, g);
                                if (old == EMPTY32) { atomicAdd(&cnt[it.j], 1u); break; }
                                if (old == g) break;
                                hs = (hs + 1) & (VL - 1);
                            }
                        }
                    }
                    if (lastb) break;
                }
            }
        } else
        for (uint32_t i = lane; i < n_items; i += 64) {
            const uint32_t slot = slots[i];
            if (slot == EMPTY32) continue;
            const Item it = item_of(i);
            if (!it.ok) continue;
            const uint32_t j = it.j;
            uint32_t oi = P.sval[slot];
            for (uint32_t steps = 0;; ++steps) {
                if (steps == VEXT_WALK_MAX) { cnt[j] = VL + 1; break; }      // a long occurrence list (a 16-mer that stands in hundreds of flanks): the long-list pass walks it 64 entries at a time
                const uint32_t fid = P.occ[2 * (size_t)oi], info = P.occ[2 * (size_t)oi + 1];
                {
                    const uint32_t g = fid >> 1;
                    uint32_t* lj = lists + j * VL;
                    const uint32_t have = cnt[j] < VL ? cnt[j] : VL;
                    bool dup = false;
                    for (uint32_t e = 0; e < have; ++e) dup = dup || lj[e] == g;
                    if (!dup && occ_hits(it, fid, info)) {      // (a gap that is listed already needs no second proof)
                        const uint32_t e = atomicAdd(&cnt[j], 1u);
                        if (e < VL) lj[e] = g;
                    }
                }
                if (((info >> 17) & 1u) || cnt[j] > VL) break;      // (a list that has run over: the read goes to the long-list pass as a whole)
                ++oi;
            }
        }
        __syncthreads();
        // per candidate: distinct gaps -> hits (a list that ran over goes to the table kernel)
        {
            const uint32_t n = lane < nb ? cnt[lane] : 0;
            const bool over = SET ? n > VL - VL / 4 : n > VL;
            const unsigned long long ob = __ballot(over);
            if (ob) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(P.overflow, (uint32_t)__popcll(ob));
                base = __shfl(base, 0);
                if (over && P.overflow_list) P.overflow_list[base + __popcll(ob & ((1ull << lane) - 1))] = my_r;
            }
            const uint32_t* lj = lists + (lane < nb ? lane : 0) * VL;
            for (uint32_t d = 0; d < VL; ++d) {
                bool emit = !over && (SET ? n > 0 : d < n);
                uint32_t g = 0;
                if (emit) {
                    g = lj[d];
                    if (SET) emit = g != EMPTY32;
                    else for (uint32_t e = 0; e < d; ++e) emit = emit && lj[e] != g;
                }
                const unsigned long long bal = __ballot(emit);
                if (!bal) { if (!SET && !__any(d + 1 < n && !over)) break; else continue; }
                const uint32_t base = obuf_n;
                if (emit) obuf[base + __popcll(bal & ((1ull << lane) - 1))] = gf_hit{g, my_r};
                __syncthreads();
                if (lane == 0) obuf_n = base + (uint32_t)__popcll(bal);
                __syncthreads();
                if (obuf_n >= OBUF - 64) {
                    put_out(obuf_n);
                    __syncthreads();
                    if (lane == 0) obuf_n = 0;
                    __syncthreads();
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (obuf_n) put_out(obuf_n);
    if (stage_n) flush_stage();
}

int launch_verify_passes(gf_ctx* ctx, const FlankIndex& ix, const ProbeSpots& pg, const void* d_reads, const void* d_nmask, size_t n_reads,
                         int read_len, int min_hits, void* d_out, size_t cap, void* d_n_out) {
    const uint32_t rb = (uint32_t)((read_len + 3) / 4);
    uint32_t* d_cnt = (uint32_t*)ctx->counters.p;  // [0] n_cand [1] error overflow [2] [3] [4] the overflow lists of the passes below
    int rc;
    VerifyParams V;
    V.reads32 = (const uint32_t*)d_reads;
    V.n_words = ((uint64_t)n_reads * rb) / 4;
    V.tail_bytes = (uint32_t)(((uint64_t)n_reads * rb) & 3);
    V.nmask = (const uint32_t*)d_nmask;
    V.rb = rb;
    V.read_len = read_len;
    V.k = ix.k;
    V.nmw = (read_len + 31) / 32;
    V.cand = (const uint32_t*)ctx->cand.p;
    V.n_cand = d_cnt;
    V.table = (const uint4*)ix.d_table;
    V.t_log2 = ix.t_log2;
    V.min_hits = min_hits < 1 ? 1 : min_hits;
    V.sset = (ctx->screen_verify_gate || ctx->screen_verify_ext) ? ix.d_sset : nullptr;
    V.s_log2 = ix.s_log2;
    V.stride = pg.stride;
    V.np = pg.np;
    V.first = pg.first;
    V.batch = (uint32_t)std::min(64, std::max(1, ctx->screen_verify_batch));
    const uint32_t npos = read_len - ix.k + 1;
    V.out = (gf_hit*)d_out;
    V.cap = (uint32_t)cap;
    V.n_out = (uint32_t*)d_n_out;
    V.stage = nullptr;
    const unsigned grid2 = (unsigned)ctx->n_cu * 32;  // one wave per block, every wave slot of the chip
    auto launch_verify = [&](const VerifyParams& VP) {
        const size_t lds2 = (64 * ((rb + 24) / 4 + 1) + VP.list_cap) * 4;
        LaunchTimer tm(ctx, GF_KERNEL_VERIFY);
        if (ix.k > 32)
            hipLaunchKernelGGL(screen_verify_kernel<true>, dim3(grid2), dim3(64), lds2, ctx->stream, VP);
        else
            hipLaunchKernelGGL(screen_verify_kernel<false>, dim3(grid2), dim3(64), lds2, ctx->stream, VP);
    };
    // pass 1: small per-wave list (keeps every wave slot of the chip busy); reads that overflow it are queued
    if ((rc = ensure(ctx, ctx->cand2, std::max<size_t>(n_reads, 1) * 4))) return rc;
    V.list_cap = std::max<uint32_t>(256, 2 * npos);
    V.overflow = d_cnt + 2;
    V.overflow_list = (uint32_t*)ctx->cand2.p;
    V.sval = ix.d_sval; V.occ = ix.d_occ; V.fpk = ix.d_fpk; V.foff = ix.d_foff;
    V.n_occ = (uint32_t)ix.n_occ;
    V.vlist = VEXT_LIST;
    const bool use_ext = ctx->screen_verify_ext && V.min_hits == 1 && ix.max_gaps_per_kmer == 0 && ix.ext_ok && V.np >= 1 && V.np <= 32;
    if (use_ext) {
        if ((rc = ensure(ctx, ctx->verify_stage, (size_t)grid2 * VEXT_STAGE * sizeof(gf_hit)))) return rc;
        V.stage = (gf_hit*)ctx->verify_stage.p;
        // seed-and-extend kernel instead of the k-mer table (same hits; see screen_verify_ext_kernel)
        const size_t rwp = (rb + 24) / 4 + 1 + 4, nmw = d_nmask ? V.nmw : 0;
        {
            const size_t lds2 = (64 * (rwp + nmw + V.np + 1) + (size_t)V.batch * V.vlist) * 4;
            LaunchTimer tm(ctx, GF_KERNEL_VERIFY);
            hipLaunchKernelGGL(screen_verify_ext_kernel, dim3(grid2), dim3(64), lds2, ctx->stream, V);
        }
        // pass 2: the reads that hit more than VEXT_LIST gaps (repeats shared by many flanks), a few per wave with a long list each;
        // what outgrows that too is queued for the table kernel (the old candidate list is free by now)
        // ... and a third pass for the reads that hit more gaps than THAT set holds (a homopolymer run shared by hundreds of flanks): two
        // reads per wave, 2 048 slots each.  The lists alternate between the two candidate buffers.
        const uint32_t big_vl[2] = {VEXT_LIST_BIG, VEXT_LIST_HUGE}, big_batch[2] = {VEXT_BATCH_BIG, VEXT_BATCH_HUGE};
        uint32_t* bufs[2] = {(uint32_t*)ctx->cand2.p, (uint32_t*)ctx->cand.p};
        for (int ps = 0; ps < 2; ++ps) {
            V.cand = bufs[ps & 1];
            V.n_cand = d_cnt + 2 + ps;
            V.overflow = d_cnt + 3 + ps;
            V.overflow_list = bufs[(ps + 1) & 1];
            V.vlist = big_vl[ps];
            V.batch = big_batch[ps];
            const size_t lds2 = (64 * (rwp + nmw + V.np + 1) + (size_t)V.batch * V.vlist) * 4;
            LaunchTimer tm(ctx, GF_KERNEL_VERIFY);
            hipLaunchKernelGGL(screen_verify_ext_kernel, dim3(grid2), dim3(64), lds2, ctx->stream, V);
        }
        V.cand = bufs[0];
        V.n_cand = d_cnt + 4;
        V.batch = (uint32_t)std::min(64, std::max(1, ctx->screen_verify_batch));
    } else {
        launch_verify(V);
        V.cand = (const uint32_t*)ctx->cand2.p;
        V.n_cand = d_cnt + 2;
    }
    GF_HIP(ctx, hipGetLastError());
    // last pass: the queued reads through the k-mer table with a list as large as LDS allows; overflowing that is an error (d_cnt[1])
    size_t want = ix.max_gaps_per_kmer ? (size_t)npos * ix.max_gaps_per_kmer : 15000;
    V.list_cap = (uint32_t)std::min<size_t>(std::max<size_t>(want, 1024), 15000);
    V.overflow = d_cnt + 1;
    V.overflow_list = nullptr;
    launch_verify(V);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // namespace gf
