// screen_pf4.hip — the 256-bucket partitioned filter of the read screen (constants and Part4Params: screen_dev.hpp).
//   pass A   every probe of every read becomes a 4-byte pair in its bucket's part:
//     pf4_scatter_kernel        unaligned runs (more than eight probes per read; screen_variant 17)
//     pf4_scatter_lines_kernel  whole, aligned 128-byte lines
//     pf4_scatter_col_kernel    whole lines, the probes streamed from the library's probe column (read_probes_kernel builds one)
//   pass B   pf4_probe_kernel    a bucket's slice of the level-1 bitmap in LDS, the exact set for what passes
//   resolve  pf4_resolve_kernel  pairs found in the exact set -> their reads (`seen` bits)
//   list     pf4_list_kernel     `seen` -> the candidate list
// Pass A's output depends on the reads alone: launch_pass_a_build runs it once into a library's resident parts, and a screen handed
// parts that fit its plan starts at pass B (launch_filter_pf4).
#include "screen_dev.hpp"

namespace gf {

// do the bases right of the probe at bit offset `bit` of the read staged at `words` (bit offsets from the start of `words`) agree
// with what some flank has next to this 16-mer?  w16 = the read's 16-mer, key = its canonical form
template <typename P>
__device__ __forceinline__ bool pf4_ext_ok(P words, uint32_t bit, uint32_t w16, uint32_t key, uint32_t ext, uint32_t xw) {
    if (ext == 0) return true;
    const uint32_t nb = stream32(words, bit + 32) >> 28;          // the two bases behind the 16-mer: nearest << 2 | next
    const bool ro = key != w16;                                    // the read shows the reverse complement of the canonical form:
    const uint32_t code = ro ? nb ^ 15u : nb;                      // its right side is the canonical LEFT side, complemented
    const uint32_t mask = ro ? (xw & 0xFFFFu) : (xw >> 16);
    return ext >= 2 ? (mask >> code) & 1u : ((mask >> (code & 12u)) & 15u) != 0;
}

// does read r have an aligned 16-mer with scrambled key pk?  (slow path: bytes from global memory)
__device__ __forceinline__ bool pf4_read_has_key(const FilterParams& P, uint64_t r, uint32_t pk) {
    const uint8_t* rd = P.reads + r * P.rb;
    for (uint32_t j = 0; j < P.np; ++j) {
        const uint32_t bit = P.first2 + j * P.stride2, by = bit >> 3, sh = bit & 7;
        uint64_t v = 0;
        for (uint32_t q = 0; q < 5; ++q) v = (v << 8) | ((by + q < P.rb) ? rd[by + q] : 0);
        const uint32_t w16 = (uint32_t)((v << sh) >> 8);
        if (canon16(w16) * S16_MUL == pk) return true;
    }
    return false;
}
// octet (read >> 3) of the pair at position `pos` of part (b, w) with batch octet `oc`: the batch is the group g with
// fills[g] <= pos < fills[g + 1] — searched from the proportional guess (the fills grow almost linearly)
__device__ __forceinline__ uint32_t pf4_octet(const Part4Params& Q, uint32_t b, uint32_t w, uint32_t pos, uint32_t oc) {
    const uint32_t* F = Q.fills + ((size_t)b * Q.n_writers + w) * Q.gs;
    const uint32_t G = Q.n_groups, n = F[G];
    uint32_t lo = (uint32_t)((uint64_t)pos * G / (n ? n : 1u)), hi;
    if (lo >= G) lo = G - 1;
    if (F[lo] <= pos) {
        uint32_t st = 1;
        hi = lo + 1;
        while (hi < G && F[hi] <= pos) { lo = hi; st <<= 1; hi = lo + st < G ? lo + st : G; }
    } else {
        uint32_t st = 1;
        hi = lo;
        lo = hi > st ? hi - st : 0;
        while (lo > 0 && F[lo] > pos) { hi = lo; st <<= 1; lo = hi > st ? hi - st : 0; }
    }
    while (hi - lo > 1) {   // F[lo] <= pos < F[hi]
        const uint32_t mid = (lo + hi) >> 1;
        if (F[mid] <= pos) lo = mid; else hi = mid;
    }
    return (uint32_t)(((uint64_t)(lo / Q.n_grp) * Q.n_writers * Q.tiles_wg + (uint64_t)w * Q.tiles_wg) * 8) + oc;
}
// every read of an octet that can have produced the pair is marked a candidate — by one lane on its own (pair list full, or a
// part that ran full in pass A)
__device__ __forceinline__ void pf4_resolve_octet_serial(const Part4Params& Q, uint32_t octet, uint32_t pk) {
    const FilterParams& P = Q.F;
    for (uint32_t sub = 0; sub < 8; ++sub) {
        const uint64_t r = (uint64_t)octet * 8 + sub;
        if (r < P.n_reads && pf4_read_has_key(P, r, pk)) atomicOr(&Q.seen[r >> 5], 1u << (r & 31));
    }
}
// Measured on 112.5 M reads, k=51 (2^28-bit bitmap): 16 waves x 1 tile 2.47 ms, 16 x 2 tiles + alternating histograms 2.22 ms (longer
// runs per bucket: 32 pairs = 256 B); 8 waves x 2 tiles with the sort buffer overlaid on the tiles, three workgroups per CU: 2.68 ms
// (128-B runs, three times the parts); 16 x 3 tiles overlaid: 5.6 ms (36 scrambled keys per lane in registers spill).
// What bounds it (same launch, parts of the kernel switched off): loads without stores 1.34 ms, stores without loads 1.57 ms, both
// 2.25-2.37 ms = 8.2 GB at 3.5 TB/s.  Twelve producer waves sorting into one of two 6-byte-entry LDS buffers while four copier waves
// write the other buffer out (stores off every producer's path) took the same 2.377 ms, `nt` stores 2.82 ms, `sc1` stores 2.26 ms:
// the mix of a 4.3-GB read stream and 65 536 scattered 256-B write runs is what the memory system delivers at this rate.
// G = probes sorted per group: PF2_GROUP, or the read's whole probe count when that is smaller (k = 51: three — a fourth, dead probe
// slot costs every lane its instructions all the same)
template <uint32_t G, bool BYTES>   // BYTES: the probes start at byte boundaries: one byte permute fetches them
__global__ __launch_bounds__(64 * PF2_WAVES) void pf4_scatter_kernel(Part4Params Q, uint32_t slice_words) {
    extern __shared__ uint32_t sm[];   // [16 waves x PF2_TILES tiles][keys: BATCH x 4 B][octets: BATCH x 1 B][fill stage 256 x 17][hist 3 x 256][offs 258][written 2 x 256]
    const FilterParams& P = Q.F;
    constexpr uint32_t NT = 64 * PF2_WAVES;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t* tiles = sm + wv * PF2_TILES * slice_words;
    uint32_t* skey = sm + PF2_WAVES * PF2_TILES * slice_words;
    uint8_t* sidx = reinterpret_cast<uint8_t*>(skey + PF2_BATCH);
    uint32_t* stage = reinterpret_cast<uint32_t*>(sidx + PF2_BATCH);
    uint32_t* hist3 = stage + PF2_NB * (PF4_STAGE + 1);
    uint32_t* offs = hist3 + 3 * PF2_NB;
    uint32_t* written2 = offs + PF2_NB + 2;
    const uint32_t writer = blockIdx.x;
    const uint32_t tile_bytes = 64 * P.rb;
    const uint64_t total_bytes = P.n_reads * P.rb;
    const uint64_t n_tiles = (P.n_reads + 63) / 64;
    auto part = [&](uint32_t b) { return Q.pairs + ((size_t)b * Q.n_writers + writer) * Q.cap; };
    auto fill_row = [&](uint32_t b) { return Q.fills + ((size_t)b * Q.n_writers + writer) * Q.gs; };
    uint32_t* dummy = Q.pairs + (size_t)PF2_NB * Q.n_writers * Q.cap;   // 64 x 4 bytes behind the parts
    for (uint32_t i = tid; i < PF2_NB; i += NT) { written2[i] = 0; hist3[i] = 0; hist3[PF2_NB + i] = 0; hist3[2 * PF2_NB + i] = 0; }
    constexpr int NPF = 4;   // 64 reads x <= 64 B
    u32x4 pf[PF2_TILES][NPF];
    auto prefetch = [&](uint64_t t0) {
#pragma unroll
        for (uint32_t q = 0; q < PF2_TILES; ++q) {
            const uint64_t t = t0 + q;
            const bool on = t < n_tiles;
            const uint64_t byte0 = on ? t * tile_bytes : 0;
            const uint32_t nbytes = on ? (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes) : 0u;
            const void* base = uniform_ptr(nbytes >= 16 ? (const void*)(P.reads + byte0) : (const void*)Q.count);   // (idle: 16 bytes of the workspace)
#pragma unroll
            for (int c = 0; c < NPF; ++c) {
                const uint32_t i = lane + c * 64;
                vm_load128(pf[q][c], i < (nbytes >> 4) ? i * 16 : 0u, base);
            }
        }
    };
    const uint64_t t_step = (uint64_t)gridDim.x * PF2_WAVES * PF2_TILES;
    const uint64_t n_iter = (n_tiles + t_step - 1) / t_step;
    prefetch(((uint64_t)blockIdx.x * PF2_WAVES + wv) * PF2_TILES);
    uint32_t hsel = 0, wsel = 0, g = 0;
    uint32_t stores_since = 0;   // copy-out stores this wave has issued since its last prefetch (wave-uniform)
    __syncthreads();
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint64_t t0 = it * t_step + ((uint64_t)blockIdx.x * PF2_WAVES + wv) * PF2_TILES;
        const uint32_t octet0 = (uint32_t)((it * t_step + (uint64_t)blockIdx.x * PF2_WAVES * PF2_TILES) * 8);   // octet of batch index 0
        // this tile's loads were issued before the previous iteration's copy-out stores: those may stay in flight
        switch (stores_since < 12u ? stores_since : 12u) {
            case 0: vm_wait<0>(); break;   case 1: vm_wait<1>(); break;   case 2: vm_wait<2>(); break;   case 3: vm_wait<3>(); break;
            case 4: vm_wait<4>(); break;   case 5: vm_wait<5>(); break;   case 6: vm_wait<6>(); break;   case 7: vm_wait<7>(); break;
            case 8: vm_wait<8>(); break;   case 9: vm_wait<9>(); break;   case 10: vm_wait<10>(); break; case 11: vm_wait<11>(); break;
            default: vm_wait<12>(); break;
        }
#pragma unroll
        for (uint32_t q = 0; q < PF2_TILES; ++q)
#pragma unroll
            for (int c = 0; c < NPF; ++c) vm_ready(pf[q][c]);
        stores_since = 0;
#pragma unroll
        for (uint32_t q = 0; q < PF2_TILES; ++q) {
            const uint64_t t = t0 + q;
            if (t >= n_tiles) continue;
            uint8_t* tb = reinterpret_cast<uint8_t*>(tiles + q * slice_words);
            const uint64_t byte0 = t * tile_bytes;
            const uint32_t nbytes = (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes);
            const uint32_t n16 = nbytes & ~15u;
#pragma unroll
            for (int c = 0; c < NPF; ++c) {
                const uint32_t i = lane + c * 64;
                if (i < (n16 >> 4)) *reinterpret_cast<u32x4*>(tb + (uint64_t)i * 16) = pf[q][c];
            }
            for (uint32_t i = n16 + lane; i < nbytes; i += 64) tb[i] = P.reads[byte0 + i];
            if (lane < 16) tb[nbytes + lane] = 0;
        }
        wave_lds_sync();
        prefetch(t0 + t_step);
        const uint32_t bit0 = lane * P.rb * 8;
        for (uint32_t j0 = 0; j0 < P.np; j0 += G, ++g) {
            uint32_t* hist = hist3 + hsel * PF2_NB;        // all zero (start / zeroed during the copy-out before last)
            const uint32_t* written = written2 + wsel * PF2_NB;
            uint32_t pk[PF2_TILES][G], rank[PF2_TILES][G];
#pragma unroll
            for (uint32_t q = 0; q < PF2_TILES; ++q) {
                const bool live = t0 + q < n_tiles && (t0 + q) * 64 + lane < P.n_reads;
#pragma unroll
                for (uint32_t u = 0; u < G; ++u) {
                    const bool on = live && j0 + u < P.np;
                    pk[q][u] = on ? canon16(BYTES ? stream32_bytes(tiles + q * slice_words, (bit0 + P.first2 + (j0 + u) * P.stride2) >> 3) : stream32(tiles + q * slice_words, bit0 + P.first2 + (j0 + u) * P.stride2)) * S16_MUL : 0u;
                    rank[q][u] = on ? atomicAdd(&hist[pk[q][u] >> (32 - PF2_NB_LOG2)], 1u) : EMPTY32;
                }
            }
            __syncthreads();
            if (wv == 0) {   // exclusive scan of the 256 bins: four per lane
                uint32_t v[4], sum = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) { v[q] = hist[lane * 4 + q]; sum += v[q]; }
                uint32_t inc = sum;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t y = __shfl_up(inc, d);
                    if ((int)lane >= d) inc += y;
                }
                uint32_t run = inc - sum;
#pragma unroll
                for (int q = 0; q < 4; ++q) { offs[lane * 4 + q] = run; run += v[q]; }
                if (lane == 63) offs[PF2_NB] = inc;
            } else if (wv <= PF2_NB / 64) {   // the parts' fill before (history) and after this group
                const uint32_t i = tid - 64;
                const uint32_t w0 = written[i], w = w0 + hist[i];
                stage[i * (PF4_STAGE + 1) + (g % PF4_STAGE)] = w0;
                written2[(wsel ^ 1u) * PF2_NB + i] = w < Q.cap ? w : Q.cap;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t q = 0; q < PF2_TILES; ++q)
#pragma unroll
                for (uint32_t u = 0; u < G; ++u)
                    if (rank[q][u] != EMPTY32) {
                        const uint32_t at = offs[pk[q][u] >> (32 - PF2_NB_LOG2)] + rank[q][u];
                        skey[at] = pk[q][u];
                        sidx[at] = (uint8_t)((wv * PF2_TILES + q) * 8 + (lane >> 3));
                    }
            __syncthreads();
            const uint32_t n_pairs = offs[PF2_NB];
            const uint32_t hz = hsel == 0 ? 2 : hsel - 1;
            for (uint32_t i = tid; i < PF2_NB; i += NT) hist3[hz * PF2_NB + i] = 0;                  // the histogram of the group after next
            for (uint32_t i0 = 0; i0 < n_pairs; i0 += NT) {         // (whole waves stay in the loop: one store per wave and trip)
                const uint32_t i = i0 + tid;
                const bool valid = i < n_pairs;
                const uint32_t key = valid ? skey[i] : 0u;
                const uint32_t oc = valid ? (uint32_t)sidx[i] : 0u;
                const uint32_t b = key >> (32 - PF2_NB_LOG2);
                const uint32_t at = valid ? written[b] + (i - offs[b]) : 0u;
                const bool spill = valid && at >= Q.cap;
                {
                    uint32_t* dst = (valid && !spill) ? part(b) + at : dummy + lane;
                    const uint32_t e = (key << 8) | oc;
                    asm volatile("global_store_dword %0, %1, off" ::"v"(dst), "v"(e) : "memory");
                    ++stores_since;
                }
                if (spill && Q.spills) atomicAdd(Q.spills, 1u);   // (the parts alone are built: counted, the caller keeps none)
                else if (spill) {   // a part that is full (degenerate inputs): tested on the spot
                    const uint32_t h = key >> (32 - P.bm_log2);
                    const uint32_t wd = P.bitmap[h >> 5];
                    if ((wd >> (h & 31)) & (wd >> (key & 31)) & 1u) {
                        const uint32_t k16 = key * S16_MUL_INV;
                        if (sset_walk(P, k16, hash_s16_set(k16, P.s_log2))) pf4_resolve_octet_serial(Q, octet0 + oc, key);
                    }
                }
            }
            if ((g % PF4_STAGE) == PF4_STAGE - 1 || g + 1 == Q.n_groups) {   // the staged fill rows leave as 64-byte pieces
                const uint32_t g_lo = g - g % PF4_STAGE;
                for (uint32_t i = tid; i < PF2_NB * PF4_STAGE; i += NT) {
                    const uint32_t b = i / PF4_STAGE, j = i % PF4_STAGE;
                    if (g_lo + j <= g) fill_row(b)[g_lo + j] = stage[b * (PF4_STAGE + 1) + j];
                }
            }
            hsel = hsel == 2 ? 0 : hsel + 1;
            wsel ^= 1u;
        }
    }
    vm_wait<0>();   // the last prefetch (idle tiles) still targets this wave's registers
    __syncthreads();
    for (uint32_t i = tid; i < PF2_NB; i += NT) {
        const uint32_t w = written2[wsel * PF2_NB + i];
        Q.count[(size_t)i * Q.n_writers + writer] = w;
        fill_row(i)[Q.n_groups] = w;
    }
}

// ---- pass A with WHOLE-LINE stores.  The kernel above writes a bucket's pairs of one group (about 24 at k = 51) where the part's fill
// stands: 96-byte runs that start anywhere.  Measured with the same write pattern beside a read stream (tools/scratch/wbench.hip:
// 65 536 parts filled front to back, 8.2 GB read): unaligned 96-byte runs 2.96 ms (WRITE_SIZE 1.25 x the bytes), aligned 64-byte
// pieces 2.35 ms (1.33 x: the L2 line is 128 bytes), aligned 128-byte lines 2.21 ms with twice the bytes written — 0.2 ms over the
// read stream alone (1.98 ms).  So a bucket's pairs leave as whole, aligned 32-entry lines: what a group leaves over (< 32 entries
// per bucket) waits in an LDS line per bucket (`carry`, two per bucket: the line being filled, and the one that takes the group's
// tail while the filled line is on its way out) and is the head of the bucket's next line.  A pair's position in its part is still
// its generation order (T_old + rank), which is all pass B and the fill history need.
//   A new pair with position p_rel = c + rank relative to the open line (c = T_old & 31, total = c + the group's pairs):
//     p_rel < 32               -> the open line                          carry[sel][b][p_rel]
//     p_rel >= total & ~31     -> the tail: head of the next open line   carry[sel ^ 1][b][p_rel & 31]
//     otherwise                -> a whole line between the two           sent[offs[b] + p_rel - 32]   (few: ~24 pairs per bucket and group)
//   Between the ranks and the placement four waves prepare the buckets' words, one bucket per lane: c, sel, total (`desc`), the
//   fill history, the list of completed open lines (`lga` = line index in `pairs`, `lsrc` = where
//   the line stands in LDS), room in `sent` for the few buckets with whole lines between (an LDS counter: their order is free).
//   Copy-out: the listed lines leave, 32 lanes per line.
// A wave stages ONE tile at a time (its second tile waits in the prefetch registers until the first one's probes are taken): the
// 64 KiB of open lines fit for reads up to 160 bases.  All probes of a read are in one group (np <= 4).
// NG = groups per tile iteration: a read's G x NG probe slots are taken from the staged tile at once and sorted G at a time — k = 31 on
// 150-base reads has eight probes per read = two groups of four through the same branch-free machinery (before: pf4_scatter_kernel<4>,
// 16.1 ms per launch at C5 against this kernel's 9.8 ms for C4's three probes).  Probe slots beyond np (np < G x NG) are dead.
// COL: the probes come from the library's probe column (Part4Params::probes, defined in gf_internal.hpp) instead of the packed rows: a
// wave's 64 reads are 256 aligned, contiguous bytes of each probe's plane, loaded straight into registers one iteration ahead — no tile
// in LDS (slice_words == 0), no extraction, canonical form or scrambling per probe.  Everything behind the fetch is the same code.
template <uint32_t G, bool BYTES, uint32_t NG, bool COL>   // BYTES: the probes start at byte boundaries (k = 51, 31, ... at 2 bits per base): one byte permute fetches them
__device__ __forceinline__ void pf4_scatter_lines_body(const Part4Params& Q, uint32_t slice_words) {
    static_assert(!COL || NG == 1, "the column form takes all probes of a read as one group");
    extern __shared__ uint32_t sm[];   // [16 waves x 1 tile][sent][carry 2 x 256 x 32][fill stage 256 x (ST + 1)][hist 3 x 256][written 2 x 256][desc 256][offs 256][lga, lsrc: 2 x (256 + sent lines)][cnt 8]
    const FilterParams& P = Q.F;
    constexpr uint32_t NT = 64 * PF2_WAVES;
    constexpr uint32_t ST = pf4_stage_of(G), LN = PF4_LINE, LM = PF4_LINE - 1;
    constexpr uint32_t NSENT = G * PF2_WAVES * PF2_TILES * 64, NLINE = PF2_NB + NSENT / LN;
    constexpr uint32_t TMASK = 0x7FFFFFFFu;
    const uint32_t tid0 = threadIdx.x, wv = (uint32_t)__builtin_amdgcn_readfirstlane(tid0 >> 6);
    uint32_t tid = tid0, lane = tid0 & 63;
    uint32_t* tile = sm + wv * slice_words;
    uint32_t* sent = sm + PF2_WAVES * slice_words;
    uint32_t* carry = sent + NSENT;            // (behind `sent`: a pair's place is one index into both)
    uint32_t* stage = carry + 2 * PF2_NB * LN;
    uint32_t* hist3 = stage + PF2_NB * (ST + 1);
    uint32_t* written2 = hist3 + 3 * PF2_NB;   // generated so far (<= cap) | open line's carry buffer << 31
    uint32_t* desc = written2 + 2 * PF2_NB;    // per bucket FOUR words, see the bucket-word phase: where a pair of the group goes is base + its position, base one of three
    uint32_t* lga = desc + 4 * PF2_NB;             // lines that leave in this group: line index in `pairs` — [0, 256): completed open lines; behind: the lines of `sent`
    uint32_t* lsrc = lga + NLINE;              // ... and where the line stands in LDS (word index from `sent`)
    uint32_t* cnt = lsrc + NLINE;              // [g & 1] completed open lines, [2 + (g & 1)] words of `sent` taken
    const uint32_t writer = blockIdx.x;
    const uint32_t tile_bytes = 64 * P.rb;
    const uint64_t total_bytes = P.n_reads * P.rb;
    const uint64_t n_tiles = (P.n_reads + 63) / 64;
    const uint32_t cap_lines = Q.cap >> 5;     // (the capacity is a multiple of 64 entries; the host checked that every line index fits 32 bits)
    auto part = [&](uint32_t b) { return Q.pairs + ((size_t)b * Q.n_writers + writer) * Q.cap; };
    auto fill_row = [&](uint32_t b) { return Q.fills + ((size_t)b * Q.n_writers + writer) * Q.gs; };
    const uint32_t dummy_line = PF2_NB * Q.n_writers * cap_lines;   // 128 bytes behind the parts
    for (uint32_t i = tid; i < PF2_NB; i += NT) { written2[i] = 0; hist3[i] = 0; hist3[PF2_NB + i] = 0; hist3[2 * PF2_NB + i] = 0; }
    if (tid < 8) cnt[tid] = 0;
    constexpr int NPF = 4;   // 64 reads x <= 64 B
    u32x4 pf[PF2_TILES][NPF];
    uint32_t pc[PF2_TILES][G];   // COL: the tiles' column words
    auto prefetch_col = [&](uint64_t t, uint32_t q) {   // (the planes are padded to whole tiles: every lane of a live tile has a word)
        const bool on = t < n_tiles;
#pragma unroll
        for (uint32_t u = 0; u < G; ++u) {
            const void* base = uniform_ptr(on ? (const void*)(Q.probes + (uint64_t)u * Q.plane + t * 64) : (const void*)Q.count);
            vm_load32(pc[q][u], on ? lane * 4 : 0u, base);
        }
    };
    auto prefetch = [&](uint64_t t, uint32_t q) {
        const bool on = t < n_tiles;
        const uint64_t byte0 = on ? t * tile_bytes : 0;
        const uint32_t nbytes = on ? (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes) : 0u;
        const void* base = uniform_ptr(nbytes >= 16 ? (const void*)(P.reads + byte0) : (const void*)Q.count);   // (idle: 16 bytes of the workspace)
#pragma unroll
        for (int c = 0; c < NPF; ++c) {
            const uint32_t i = lane + c * 64;
            vm_load128(pf[q][c], i < (nbytes >> 4) ? i * 16 : 0u, base);
        }
    };
    const uint64_t t_step = (uint64_t)gridDim.x * PF2_WAVES * PF2_TILES;
    const uint64_t n_iter = (n_tiles + t_step - 1) / t_step;
#pragma unroll
    for (uint32_t q = 0; q < PF2_TILES; ++q) {
        if constexpr (COL) prefetch_col(((uint64_t)blockIdx.x * PF2_WAVES + wv) * PF2_TILES + q, q);
        else prefetch(((uint64_t)blockIdx.x * PF2_WAVES + wv) * PF2_TILES + q, q);
    }
    if constexpr (COL) {
        vm_wait<0>();
#pragma unroll
        for (uint32_t q = 0; q < PF2_TILES; ++q)
#pragma unroll
            for (uint32_t u = 0; u < G; ++u) vm_ready(pc[q][u]);
    }
    uint32_t hsel = 0, wsel = 0;
    uint32_t stores_since = 0;   // copy-out stores this wave has issued since its last prefetch (wave-uniform)
    __syncthreads();
    for (uint64_t it = 0; it < n_iter; ++it) {   // NG groups per iteration: g = it * NG + gi
        asm volatile("" : "+v"(tid), "+v"(lane));   // (opaque: what derives from them is computed where it is used, not kept in registers across the iteration)
        const uint64_t t0 = it * t_step + ((uint64_t)blockIdx.x * PF2_WAVES + wv) * PF2_TILES;
        const uint32_t octet0 = (uint32_t)((it * t_step + (uint64_t)blockIdx.x * PF2_WAVES * PF2_TILES) * 8);   // octet of batch index 0
        uint32_t pka[PF2_TILES][G * NG];      // the raw 16-mers of every probe slot of the iteration's tiles
        const uint32_t bit0 = lane * P.rb * 8;
        if constexpr (COL) {
            // this iteration's column words have arrived (awaited before the loop / at the end of the previous iteration); the next
            // iteration's are asked for now and have the whole iteration to come
#pragma unroll
            for (uint32_t q = 0; q < PF2_TILES; ++q)
#pragma unroll
                for (uint32_t u = 0; u < G; ++u) pka[q][u] = pc[q][u];
#pragma unroll
            for (uint32_t q = 0; q < PF2_TILES; ++q) prefetch_col(t0 + q + t_step, q);
        } else {
#pragma unroll
        for (uint32_t q = 0; q < PF2_TILES; ++q) {
            // tile q's loads were issued before the loads of the tiles behind it and the previous copy-out's stores: those may stay in flight
            vm_wait_range<(PF2_TILES - 1) * NPF, (PF2_TILES - 1) * NPF + 15>((uint32_t)__builtin_amdgcn_readfirstlane(stores_since) + (PF2_TILES - 1) * NPF);
#pragma unroll
            for (int c = 0; c < NPF; ++c) vm_ready(pf[q][c]);
            const uint64_t t = t0 + q;
            if (t < n_tiles) {
                uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
                const uint64_t byte0 = t * tile_bytes;
                const uint32_t nbytes = (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes);
                const uint32_t n16 = nbytes & ~15u;
#pragma unroll
                for (int c = 0; c < NPF; ++c) {
                    const uint32_t i = lane + c * 64;
                    if (i < (n16 >> 4)) *reinterpret_cast<u32x4*>(tb + (uint64_t)i * 16) = pf[q][c];
                }
                for (uint32_t i = n16 + lane; i < nbytes; i += 64) tb[i] = P.reads[byte0 + i];
                if (lane < 16) tb[nbytes + lane] = 0;
            }
            wave_lds_sync();
            prefetch(t + t_step, q);
#pragma unroll
            for (uint32_t u = 0; u < G * NG; ++u)     // (a slot beyond np reads inside the staged tile + pad all the same; its pair is never ranked)
                pka[q][u] = BYTES ? stream32_bytes(tile, (bit0 + P.first2 + (NG == 1 || u < P.np ? u : 0u) * P.stride2) >> 3)
                                  : stream32(tile, bit0 + P.first2 + (NG == 1 || u < P.np ? u : 0u) * P.stride2);
            wave_lds_sync();   // the tile's probes are taken (LDS operations of a wave execute in order): the next tile may take its place
        }
        }
        stores_since = 0;
#pragma unroll
      for (uint32_t gi = 0; gi < NG; ++gi) {
        const uint32_t g = (uint32_t)it * NG + gi;
        uint32_t* hist = hist3 + hsel * PF2_NB;        // all zero (start / zeroed during the copy-out before last)
        const uint32_t* written = written2 + wsel * PF2_NB;
        uint32_t pk[PF2_TILES][G], rank[PF2_TILES][G];
#pragma unroll
        for (uint32_t q = 0; q < PF2_TILES; ++q) {
            const bool live = t0 + q < n_tiles && (t0 + q) * 64 + lane < P.n_reads;
            // (with NG == 1 the kernel is launched with G == np — all probes of a read in one group —; a tile's probes share ONE execution
            // mask; the test against np below is the same for every lane)
            if (live) {
#pragma unroll
                for (uint32_t u = 0; u < G; ++u) {
                    if (NG == 1 || gi * G + u < P.np) {
                        pk[q][u] = COL ? pka[q][gi * G + u] : canon16(pka[q][gi * G + u]) * S16_MUL;
                        rank[q][u] = atomicAdd(&hist[pk[q][u] >> (32 - PF2_NB_LOG2)], 1u);
                    } else { pk[q][u] = 0u; rank[q][u] = EMPTY32; }
                }
            } else {
#pragma unroll
                for (uint32_t u = 0; u < G; ++u) { pk[q][u] = 0u; rank[q][u] = EMPTY32; }
            }
        }
        __syncthreads();
        if (wv >= 1 && wv <= PF2_NB / 64) {   // the buckets' words, one bucket per lane
            const uint32_t i = tid - 64, w = written[i], t_old = w & TMASK, sel = w >> 31, n_new = hist[i];
            const uint32_t room = Q.cap - t_old, ne = n_new < room ? n_new : room;   // (pairs beyond the part's capacity are not placed)
            const uint32_t c = t_old & LM, total = c + ne, full = total & ~LM;
            const bool done = total >= LN;
            stage[i * (ST + 1) + (g % ST)] = t_old;
            written2[(wsel ^ 1u) * PF2_NB + i] = (t_old + ne) | ((sel ^ (done ? 1u : 0u)) << 31);
            // A pair with position p_rel = c + rank goes to word base + p_rel of `sent`, base one of three by where p_rel lies (the
            // placement picks it with two compares): the open line (p_rel < 32), the whole lines between (< full; they start at `of`), the
            // tail = head of the next open line.  The four words leave and are fetched as ONE 16-byte LDS access; the fourth holds
            // c | full / 32 << 5 | the pairs that fit the part << 14 (a rank beyond it: the part is full, the pair is tested on the spot).
            const uint32_t of = full > LN ? atomicAdd(&cnt[2 + (g & 1u)], full - LN) : 0u;    // whole lines between the open line and the tail
            uint4 dv;
            dv.x = NSENT + sel * (PF2_NB * LN) + i * LN;
            dv.y = of - LN;
            dv.z = NSENT + (sel ^ 1u) * (PF2_NB * LN) + i * LN - full;
            dv.w = c | ((full >> 5) << 5) | (ne << 14);        // (full / 32 <= 257: nine bits; ne <= 8 192: fourteen)
            reinterpret_cast<uint4*>(desc)[i] = dv;
            const unsigned long long bal = __ballot(done);
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&cnt[g & 1u], (uint32_t)__popcll(bal));   // (the four waves' lists follow each other in any order)
            base = (uint32_t)__builtin_amdgcn_readfirstlane(base);
            if (done) {   // the open line leaves: from carry[sel][b] to position t_old & ~31 of the part
                const uint32_t at = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
                lga[at] = (i * Q.n_writers + writer) * cap_lines + (t_old >> 5);
                lsrc[at] = NSENT + sel * (PF2_NB * LN) + i * LN;
            }
        }
        __syncthreads();
        uint32_t spilled = 0, midm = 0;
        const uint32_t dummy_word = (uint32_t)((cnt + 7) - sent);   // (an unused counter word takes the entries of dead lanes and of pairs beyond a full part)
#pragma unroll
        for (uint32_t q = 0; q < PF2_TILES; ++q) {
            uint4 dv[G];
#pragma unroll
            for (uint32_t u = 0; u < G; ++u) dv[u] = reinterpret_cast<const uint4*>(desc)[pk[q][u] >> (32 - PF2_NB_LOG2)];   // the buckets' words first: independent LDS reads
#pragma unroll
            for (uint32_t u = 0; u < G; ++u) {   // straight-line: no branch per pair (the rare cases are collected as bit masks and handled behind the loop)
                const uint32_t key = pk[q][u], m = dv[u].w;
                const uint32_t p_rel = (m & LM) + rank[q][u];
                const bool ok = rank[q][u] < (m >> 14);                      // (a dead lane's rank is EMPTY32: never below)
                const bool lo = p_rel < LN, mid = !lo && (p_rel >> 5) < ((m >> 5) & 0x1FFu);   // (full is a multiple of 32)
                const uint32_t at = (lo ? dv[u].x : mid ? dv[u].y : dv[u].z) + p_rel;
                sent[ok ? at : dummy_word] = (key << 8) | ((wv * PF2_TILES + q) * 8 + (lane >> 3));
                if (!ok) spilled |= 1u << (q * G + u);
                if (ok && mid && (at & LM) == 0) midm |= 1u << (q * G + u);   // the first pair of a whole line between lists it
            }
        }
        if (midm) {   // (static indices: a dynamically indexed pk[][] would live in scratch memory)
#pragma unroll
            for (uint32_t x = 0; x < PF2_TILES * G; ++x)
                if ((midm >> x) & 1u) {
                    const uint32_t q = x / G, u = x % G, b = pk[q][u] >> (32 - PF2_NB_LOG2);
                    const uint4 d4 = reinterpret_cast<const uint4*>(desc)[b];
                    const uint32_t p_rel = (d4.w & LM) + rank[q][u], at = d4.y + p_rel;
                    lga[PF2_NB + (at >> 5)] = (b * Q.n_writers + writer) * cap_lines + (((written[b] & TMASK & ~LM) + p_rel) >> 5);
                    lsrc[PF2_NB + (at >> 5)] = at;
                }
        }
        if (spilled && Q.spills) {   // (the parts alone are built: counted, the caller keeps none)
#pragma unroll
            for (uint32_t x = 0; x < PF2_TILES * G; ++x)
                if (((spilled >> x) & 1u) && rank[x / G][x % G] != EMPTY32) atomicAdd(Q.spills, 1u);
        } else if (spilled) {   // a part that is full (degenerate inputs): its pair is tested on the spot
#pragma unroll
            for (uint32_t x = 0; x < PF2_TILES * G; ++x)
                if (((spilled >> x) & 1u) && rank[x / G][x % G] != EMPTY32) {
                    const uint32_t q = x / G, u = x % G, key = pk[q][u];
                    const uint32_t h = key >> (32 - P.bm_log2);
                    const uint32_t wd = P.bitmap[h >> 5];
                    if ((wd >> (h & 31)) & (wd >> (key & 31)) & 1u) {
                        const uint32_t k16 = key * S16_MUL_INV;
                        if (sset_walk(P, k16, hash_s16_set(k16, P.s_log2))) pf4_resolve_octet_serial(Q, octet0 + (wv * PF2_TILES + q) * 8 + (lane >> 3), key);
                    }
                }
        }
        __syncthreads();
        const uint32_t n_open = cnt[g & 1u], n_out = (n_open + (cnt[2 + (g & 1u)] >> 5)) * LN;
        if (tid < 2) cnt[2 * tid + ((g + 1) & 1u)] = 0;   // (the next group's)
        const uint32_t hz = hsel == 0 ? 2 : hsel - 1;
        for (uint32_t i = tid; i < PF2_NB; i += NT) hist3[hz * PF2_NB + i] = 0;                  // the histogram of the group after next
        // whole lines leave, eight lanes each (16 bytes per lane), two trips' LDS reads in flight.  Whole waves stay in the loop — one
        // store per wave and trip, lanes without a piece write behind the parts — so that the number of stores in flight is known.
        const uint32_t n_q = n_out >> 2;
        for (uint32_t i0 = 0; i0 < n_q; i0 += 2 * NT) {
            uint32_t ga[2], src[2];
            u32x4 e[2];
#pragma unroll
            for (uint32_t j = 0; j < 2; ++j) {
                const uint32_t i = i0 + j * NT + tid, ln = i >> 3;
                const bool valid = i < n_q;
                const uint32_t at = ln < n_open ? ln : PF2_NB + ln - n_open;
                ga[j] = valid ? lga[at] : dummy_line;
                src[j] = valid ? lsrc[at] + (tid & 7u) * 4 : 0u;
            }
#pragma unroll
            for (uint32_t j = 0; j < 2; ++j) e[j] = *reinterpret_cast<const u32x4*>(sent + src[j]);
#pragma unroll
            for (uint32_t j = 0; j < 2; ++j)
                if (i0 + j * NT < n_q) {
                    const uint32_t* dst = Q.pairs + (((size_t)ga[j] << 5) | ((tid & 7u) * 4));
                    asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(dst), "v"(e[j]) : "memory");
                    ++stores_since;
                }
        }
        if ((g % ST) == ST - 1 || g + 1 == Q.n_groups) {   // the staged fill rows leave as 64- (32-) byte pieces
            const uint32_t g_lo = g - g % ST;
            for (uint32_t i = tid; i < PF2_NB * ST; i += NT) {
                const uint32_t b = i / ST, j = i % ST;
                if (g_lo + j <= g) fill_row(b)[g_lo + j] = stage[b * (ST + 1) + j];
            }
        }
        hsel = hsel == 2 ? 0 : hsel + 1;
        wsel ^= 1u;
      }
        if constexpr (COL) {
            // The words asked for at the top of this iteration are awaited HERE, not at the top of the next one: a value that crosses the
            // loop edge may be copied to another register there, and a copy made before the data is in reads the register's old content
            // (seen: 4 of 86 456 hits lost).  Issued before this iteration's copy-out stores: those may stay in flight.
            vm_wait_range<0, 15>((uint32_t)__builtin_amdgcn_readfirstlane(stores_since));
#pragma unroll
            for (uint32_t q = 0; q < PF2_TILES; ++q)
#pragma unroll
                for (uint32_t u = 0; u < G; ++u) vm_ready(pc[q][u]);
        }
    }
    vm_wait<0>();   // the last prefetch (idle tiles) still targets this wave's registers
    __syncthreads();
    for (uint32_t t = tid; t < PF2_NB * LN; t += NT) {   // the open lines
        const uint32_t b = t >> 5, w = written2[wsel * PF2_NB + b], T = w & TMASK;
        if ((t & LM) < (T & LM)) part(b)[(T & ~LM) + (t & LM)] = carry[(w >> 31) * (PF2_NB * LN) + t];
    }
    for (uint32_t i = tid; i < PF2_NB; i += NT) {
        const uint32_t w = written2[wsel * PF2_NB + i] & TMASK;
        Q.count[(size_t)i * Q.n_writers + writer] = w;
        fill_row(i)[Q.n_groups] = w;
    }
}

template <uint32_t G, bool BYTES, uint32_t NG = 1>
__global__ __launch_bounds__(64 * PF2_WAVES) void pf4_scatter_lines_kernel(Part4Params Q, uint32_t slice_words) {
    pf4_scatter_lines_body<G, BYTES, NG, false>(Q, slice_words);
}
template <uint32_t G>
__global__ __launch_bounds__(64 * PF2_WAVES) void pf4_scatter_col_kernel(Part4Params Q) {
    pf4_scatter_lines_body<G, false, 1, true>(Q, 0u);
}

// ---- the probe column's stand-alone producer (gf_read_probes_dev): a tile of 256 rows staged in LDS, one read per lane, one
// coalesced store per probe plane
__global__ __launch_bounds__(256) void read_probes_kernel(const uint8_t* reads, uint64_t n_reads, uint32_t rb, uint32_t first2, uint32_t stride2,
                                                          uint32_t np, uint64_t plane, uint32_t* probes) {
    extern __shared__ uint32_t tile[];  // TILE_READS * rb bytes + 16 B pad
    const uint32_t tid = threadIdx.x;
    const uint32_t tile_bytes = TILE_READS * rb;
    const uint64_t total_bytes = n_reads * rb;
    const uint64_t n_tiles = (n_reads + TILE_READS - 1) / TILE_READS;
    uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t byte0 = t * tile_bytes;
        const uint32_t nbytes = (uint32_t)((total_bytes - byte0) < tile_bytes ? (total_bytes - byte0) : tile_bytes);
        const uint32_t n16 = nbytes & ~15u;
        const uint8_t* src = reads + byte0;
        for (uint32_t i = tid * 16; i < n16; i += 256 * 16)
            *reinterpret_cast<uint4*>(tb + i) = *reinterpret_cast<const uint4*>(src + i);
        for (uint32_t i = n16 + tid; i < nbytes; i += 256) tb[i] = src[i];
        if (tid < 16) tb[nbytes + tid] = 0;
        __syncthreads();
        const uint64_t r = t * TILE_READS + tid;
        if (r < plane)   // (the pad behind the last read, up to a whole 64-read tile, is zero)
            for (uint32_t j = 0; j < np; ++j)
                probes[(uint64_t)j * plane + r] = r < n_reads ? probe_word(stream32(tile, tid * rb * 8 + first2 + j * stride2)) : 0u;
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void pf4_probe_kernel(Part4Params Q) {
    extern __shared__ uint32_t sm[];   // [slice of the level-1 bitmap: 2^(bm_log2 - 8) bits][per wave: 2 x PF4_OBUF words of list entries | 2 x PF2_PEND words of pairs | PF4_OBUF ext words]
    const FilterParams& P = Q.F;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t slice_words = 1u << (P.bm_log2 - PF2_NB_LOG2 - 5);
    const uint32_t sh_w = 45 - P.bm_log2, sh_b1 = 40 - P.bm_log2;   // entry -> word of the slice / first bit inside the word (the second: entry bits 8..12)
    unsigned long long* obuf = reinterpret_cast<unsigned long long*>(sm + slice_words + wv * (3 * PF4_OBUF + 2 * PF2_PEND));
    unsigned long long* pend = obuf + PF4_OBUF;
    uint32_t* obx = reinterpret_cast<uint32_t*>(pend + PF2_PEND);
    uint32_t obuf_n = 0, pend_n = 0;   // wave-uniform
    const unsigned long long lt = (1ull << lane) - 1;
    for (uint32_t b = blockIdx.x; b < PF2_NB; b += gridDim.x) {
        // The pair list is reserved in CHUNKS of PF4_CHUNK entries per wave and bucket (a single global counter serialises returning
        // atomics at ~11 ns each: one atomic per 32-64 entries was 0.8 ms per 112.5 M reads, the whole pass); a chunk belongs to ONE
        // bucket (chunk_b), so an entry needs no bucket bits; what is left of a wave's last chunk is filled with the invalid entry ~0.
        uint32_t ch_at = 0, ch_end = 0;   // wave-uniform: this wave's chunk
        bool list_full = false;           // wave-uniform: a reservation came back beyond the list — no more reservations (the counter
                                          // then stops at most one chunk per wave beyond the capacity: it cannot wrap)
        auto flush = [&]() {
            uint32_t done = 0;
            while (done < obuf_n) {
                if (ch_at == ch_end) {
                    uint32_t gb = Q.cap8;
                    if (lane == 0 && !list_full) {
                        gb = atomicAdd(Q.n_cand8, PF4_CHUNK);
                        if (gb < Q.cap8) Q.chunk_b[gb / PF4_CHUNK] = (uint8_t)b;
                    }
                    ch_at = __shfl(gb, 0);
                    ch_end = ch_at + PF4_CHUNK;
                    list_full = ch_at >= Q.cap8;
                }
                const uint32_t room = ch_end - ch_at, m = obuf_n - done < room ? obuf_n - done : room;
                for (uint32_t q = lane; q < m; q += 64) {
                    const unsigned long long cp = obuf[done + q];
                    if (ch_at + q < Q.cap8) { Q.cand8[ch_at + q] = cp; Q.cand8x[ch_at + q] = obx[done + q]; }
                    else pf4_resolve_octet_serial(Q, pf4_octet(Q, b, (uint32_t)(cp >> 56), (uint32_t)(cp >> 32) & 0xFFFFFFu, (uint32_t)(cp >> 24) & 255u),
                                                  (b << 24) | ((uint32_t)cp & 0xFFFFFFu));
                }
                ch_at += m;
                done += m;
            }
            obuf_n = 0;
            wave_lds_sync();
        };
        // Exact-set look-up of the last min(64, pend_n) queued pairs {writer | position | batch octet | key bits}, one per lane, in TWO
        // steps: `ask` sends for the four slots at the key's home (one request), `take` — called before the next `ask`, a batch of
        // pairs later — reads the answer, so the wave streams on while the set answers (asked and taken in one go, the look-ups were
        // 0.24 of pass B's 0.91 ms per 675 M pairs: every 6 400 pairs a wave stood still for a round trip to the set).
        uint4 asked_v = make_uint4(EMPTY32, EMPTY32, EMPTY32, EMPTY32), asked_x = make_uint4(0, 0, 0, 0);   // the key's home group: four keys, their ext words
        unsigned long long asked_pr = 0;
        bool asked = false;           // this lane has a look-up in flight
        auto take = [&]() {
            bool cand = false;
            uint32_t xw = 0;
            if (asked) {
                const uint32_t key = ((b << 24) | ((uint32_t)asked_pr & 0xFFFFFFu)) * S16_MUL_INV;
                if (asked_v.x == key) { cand = true; xw = asked_x.x; }
                else if (asked_v.y == key) { cand = true; xw = asked_x.y; }
                else if (asked_v.z == key) { cand = true; xw = asked_x.z; }
                else if (asked_v.w == key) { cand = true; xw = asked_x.w; }
                else if (asked_v.x != EMPTY32 && asked_v.y != EMPTY32 && asked_v.z != EMPTY32 && asked_v.w != EMPTY32)   // rare: a full group of foreign keys
                    cand = pf4_sgrp_walk(Q, key, (hash_s16_set(key, P.s_log2) >> 2) + 1, xw);
            }
            asked = false;
            const unsigned long long bal = __ballot(cand);
            if (bal) {
                if (obuf_n + (uint32_t)__popcll(bal) > PF4_OBUF) flush();
                if (cand) { obuf[obuf_n + __popcll(bal & lt)] = asked_pr; obx[obuf_n + __popcll(bal & lt)] = xw; }
                obuf_n += (uint32_t)__popcll(bal);
                wave_lds_sync();
                if (obuf_n >= 32) flush();
            }
        };
        auto ask = [&]() {
            take();
            const uint32_t base = pend_n > 64 ? pend_n - 64 : 0;
            if (base + lane < pend_n) {
                asked_pr = pend[base + lane];
                const uint32_t key = ((b << 24) | ((uint32_t)asked_pr & 0xFFFFFFu)) * S16_MUL_INV;
                const uint4* G = reinterpret_cast<const uint4*>(Q.sgrp + (size_t)(hash_s16_set(key, P.s_log2) >> 2) * 8);   // 32 aligned bytes: one request
                asked_v = G[0];
                asked_x = G[1];
                asked = true;
            }
            pend_n = base;
            wave_lds_sync();
        };
        __syncthreads();
        for (uint32_t i = tid * 4; i < slice_words; i += 1024 * 4)
            *reinterpret_cast<uint4*>(sm + i) = *reinterpret_cast<const uint4*>(P.bitmap + (size_t)b * slice_words + i);
        __syncthreads();
        for (uint32_t w = wv; w < Q.n_writers; w += 16) {
            const uint32_t n = Q.count[(size_t)b * Q.n_writers + w];
            const uint32_t* src = Q.pairs + ((size_t)b * Q.n_writers + w) * Q.cap;
            constexpr int PB = 16;   // entries per lane and trip: four 16-byte loads (eight: 0.86 vs 0.81 ms per 675 M pairs) (lane = four consecutive entries of each 1 024-byte row)
            u32x4 nx4[PB / 4];
            // The pairs pass through ONCE (10.8 GB per launch at C4) and are loaded NON-TEMPORALLY, as the tagger loads its key stream: they do
            // not take the L2s' lines from the exact set's.  Measured at C4 (rocprofv3, 7 dispatches per build, all builds in one session):
            // 2.78 -> 2.41-2.44 ms per launch; the fetched bytes hardly move (15.4 -> 15.3 GB), so it is not the bytes that the time follows —
            // with the set laid out by bucket and an XCD working on two buckets at a time (tried, not kept) the fetches fell to 11.1 GB and
            // the time stayed 2.44 ms (2.50 without these loads): DESIGN.md §4.
            auto fetch = [&](uint32_t i0) {
#pragma unroll
                for (int c = 0; c < PB / 4; ++c) {
                    const uint32_t at = i0 + (c * 64 + lane) * 4;
                    nx4[c] = at < n ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + (at >> 2)) : u32x4{0, 0, 0, 0};   // (a part's capacity is a multiple of 64 entries)
                }
            };
            fetch(0);
            for (uint32_t i0 = 0; i0 < n; i0 += PB * 64) {
                uint32_t pr[PB];
#pragma unroll
                for (int c = 0; c < PB / 4; ++c) { pr[4 * c] = nx4[c].x; pr[4 * c + 1] = nx4[c].y; pr[4 * c + 2] = nx4[c].z; pr[4 * c + 3] = nx4[c].w; }
                if (i0 + PB * 64 < n) fetch(i0 + PB * 64);
                // both bits of every key in its word of the slice: the trip's sixteen LDS reads first (independent), then the tests.  An entry
                // is key bits << 8 | octet and the bucket's 8 bits are the same for the whole slice, so the word index is ONE shift of the
                // entry (its top bm_log2 - 13 bits: always inside the slice) and each bit index one bit-field extract — the pass is bound by
                // its vector instructions (PMC: 30 per pair), not by LDS or HBM
                uint32_t wd[PB], passm = 0;
#pragma unroll
                for (int u = 0; u < PB; ++u) wd[u] = sm[pr[u] >> sh_w];
                // (the pass is used with bitmaps of 2^27 / 2^28 bits: their keys carry a third bit, kmer_dev.hpp::hash_s16_bit3 — with it a
                //  third fewer pairs go on to the exact set, whose 128-byte lines were 6.8 of this pass's 17.6 GB at C4)
#pragma unroll
                for (int u = 0; u < PB; ++u) {
                    const uint32_t b1 = (pr[u] >> sh_b1) & 31u, b2 = (pr[u] >> 8) & 31u;
                    passm |= ((wd[u] >> b1) & (wd[u] >> b2) & (wd[u] >> s16_bit3_of(b1, b2)) & 1u) << u;
                }
                if (i0 + PB * 64 > n) {   // the part's last trip: entries behind its end do not count
                    uint32_t keep = 0;   // (per load its first min(4, n - at) entries: no sixteen mask constants in registers)
#pragma unroll
                    for (int c = 0; c < PB / 4; ++c) {
                        const uint32_t at = i0 + (c * 64 + lane) * 4, k = at >= n ? 0u : n - at < 4u ? n - at : 4u;
                        keep |= ((1u << k) - 1u) << (4 * c);
                    }
                    passm &= keep;
                }
                // The passing entries (1.2 % at C4: a dozen per trip, nearly all lanes none or one) leave lane by lane, lowest bit first: one
                // round per entry of the lane that holds most — two on average — where a ballot per entry SLOT ran sixteen rounds, nine of
                // them with a taker.  The entry is picked from its sixteen registers by the four bits of its index.
                for (;;) {
                    const bool has = passm != 0;
                    const unsigned long long bal = __ballot(has);
                    if (!bal) break;
                    const uint32_t u = has ? (uint32_t)__builtin_ctz(passm) : 0u;
                    // (bit-field inserts under an all-ones / all-zeros mask: written as `c ? a : b` the compiler makes a dynamically indexed
                    //  array of it — 128 bytes of scratch memory per lane)
                    const uint32_t m0 = 0u - (u & 1u), m1 = 0u - ((u >> 1) & 1u), m2 = 0u - ((u >> 2) & 1u), m3 = 0u - ((u >> 3) & 1u);
                    uint32_t s8[8], s4[4], s2[2];
#pragma unroll
                    for (int q = 0; q < 8; ++q) s8[q] = (pr[2 * q + 1] & m0) | (pr[2 * q] & ~m0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) s4[q] = (s8[2 * q + 1] & m1) | (s8[2 * q] & ~m1);
#pragma unroll
                    for (int q = 0; q < 2; ++q) s2[q] = (s4[2 * q + 1] & m2) | (s4[2 * q] & ~m2);
                    const uint32_t e = (s2[1] & m3) | (s2[0] & ~m3);
                    const uint32_t pos = i0 + ((u >> 2) * 64 + lane) * 4 + (u & 3);
                    if (has) pend[pend_n + __popcll(bal & lt)] = ((unsigned long long)w << 56) | ((unsigned long long)pos << 32) | ((e & 255u) << 24) | (e >> 8);
                    passm &= passm - 1u;
                    pend_n += (uint32_t)__popcll(bal);                    // < 64 + 64 <= PF2_PEND
                    wave_lds_sync();
                    if (pend_n >= 64) ask();
                }
            }
        }
        while (pend_n) ask();
        take();
        if (obuf_n) flush();
        for (uint32_t q = ch_at + lane; q < ch_end; q += 64)
            if (q < Q.cap8) Q.cand8[q] = ~0ull;
    }
}

// A pair that is in the exact set -> the reads it can have come from.  Its batch follows from its position in the part (the
// part's fill history), its octet from the entry; every read of the octet that has an aligned 16-mer with the pair's scrambled key
// IS a candidate: its bit in `seen` is set.  Eight lanes per pair (lane = read of the octet), eight pairs per lane group in flight;
// a read's aligned 16-mers are fetched with one unaligned 8-byte load each.
__global__ __launch_bounds__(256) void pf4_resolve_kernel(Part4Params Q) {
    extern __shared__ uint32_t sm[];   // per wave: 8 octets x (octet words rounded up to 4, + 4)
    const FilterParams& P = Q.F;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane & 7, slot = lane >> 3;
    const uint32_t ow = 2 * P.rb;                         // words per octet (8 reads x rb bytes; the octet starts 16-byte aligned)
    const uint32_t ow4 = (ow + 3) / 4;                    // 16-byte pieces
    const uint32_t row = ow4 * 4 + 4;
    uint32_t* stg = sm + (wv * 8 + slot) * row;
    const uint32_t n = *Q.n_cand8 < Q.cap8 ? *Q.n_cand8 : Q.cap8;
    const uint64_t total_bytes = P.n_reads * P.rb;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t e0 = wave * 64; e0 < n; e0 += n_waves * 64) {
        // lane = pair: its octet (one dependent chain of look-ups per lane, 64 in flight per wave) ...
        uint32_t my_octet = 0xFFFFFFFFu, my_pk = 0, my_xw = 0;
        {
            const uint64_t e = e0 + lane;
            const unsigned long long cp = e < n ? Q.cand8[e] : ~0ull;
            if (cp != ~0ull) {   // (~0: unused tail of a wave's chunk)
                const uint32_t b = Q.chunk_b[e / PF4_CHUNK];
                my_xw = Q.cand8x[e];
                my_pk = (b << 24) | ((uint32_t)cp & 0xFFFFFFu);
                my_octet = pf4_octet(Q, b, (uint32_t)(cp >> 56), (uint32_t)(cp >> 32) & 0xFFFFFFu, (uint32_t)(cp >> 24) & 255u);
            }
        }
        // ... then eight lanes per pair, eight pairs per round: the lanes stage the octet (8 reads, contiguous) in LDS with aligned
        // 16-byte loads, lane = read scrambles its own aligned 16-mers
        for (int u = 0; u < 8; ++u) {
            const uint32_t octet = __shfl(my_octet, u * 8 + slot), pk = __shfl(my_pk, u * 8 + slot), xw = __shfl(my_xw, u * 8 + slot);
            const bool valid = octet != 0xFFFFFFFFu;
            if (!__any(valid)) continue;
            const uint64_t byte0 = (uint64_t)octet * 8 * P.rb;
            for (uint32_t c = sub; c < ow4; c += 8) {
                uint4 v = make_uint4(0, 0, 0, 0);
                const uint64_t at = byte0 + (uint64_t)c * 16;
                if (valid) {
                    if (at + 16 <= total_bytes) v = *reinterpret_cast<const uint4*>(P.reads + at);
                    else {
                        uint32_t t[4] = {0, 0, 0, 0};
                        for (uint32_t q = 0; q < 16; ++q) if (at + q < total_bytes) t[q >> 2] |= (uint32_t)P.reads[at + q] << (8 * (q & 3));
                        v = make_uint4(t[0], t[1], t[2], t[3]);
                    }
                }
                *reinterpret_cast<uint4*>(stg + c * 4) = v;
            }
            wave_lds_sync();
            const uint64_t r = (uint64_t)octet * 8 + sub;
            bool hit = false;
            if (valid && r < P.n_reads)
                for (uint32_t j = 0; j < P.np && !hit; ++j) {
                    const uint32_t bit = sub * P.rb * 8 + P.first2 + j * P.stride2, w16 = stream32(stg, bit), key = canon16(w16);
                    hit = key * S16_MUL == pk && pf4_ext_ok(stg, bit, w16, key, Q.ext, xw);
                }
            if (hit) atomicOr(&Q.seen[r >> 5], 1u << (r & 31));
            wave_lds_sync();
        }
    }
}

// the candidate list = the reads whose `seen` bit is set: every workgroup compacts one contiguous slice of the bitmap (count, one
// global atomic for the slice, then write)
__global__ __launch_bounds__(256) void pf4_list_kernel(Part4Params Q) {
    __shared__ uint32_t s_w[4], s_base;
    const FilterParams& P = Q.F;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t n_words = (P.n_reads + 31) / 32;
    const uint64_t per = ((n_words + gridDim.x - 1) / gridDim.x + 255) & ~(uint64_t)255;   // whole 256-word rows per workgroup
    const uint64_t w0 = (uint64_t)blockIdx.x * per, w1 = w0 + per < n_words ? w0 + per : n_words;
    // pass 1: the slice's candidates (coalesced: thread t takes word t of every 256-word row)
    uint32_t c = 0;
    for (uint64_t i = w0 + tid; i < w1; i += 256) c += (uint32_t)__popc(Q.seen[i]);
    for (int d = 32; d; d >>= 1) c += __shfl_down(c, d);
    if (lane == 0) s_w[wv] = c;
    __syncthreads();
    if (tid == 0) {
        const uint32_t tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        s_base = tot ? atomicAdd(P.n_cand, tot) : 0u;
    }
    __syncthreads();
    uint32_t base = s_base;
    // pass 2 (the slice is in L2 now): row by row, a block scan of the words' popcounts places every read in read order
    for (uint64_t r0 = w0; r0 < w1; r0 += 256) {
        uint32_t v = r0 + tid < w1 ? Q.seen[r0 + tid] : 0u;
        const uint32_t n = (uint32_t)__popc(v);
        uint32_t inc = n;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d);
            if ((int)lane >= d) inc += y;
        }
        __syncthreads();                       // (the previous row's wave totals have been read)
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        uint32_t off = base + inc - n;
        for (uint32_t q = 0; q < wv; ++q) off += s_w[q];
        while (v) {
            const uint32_t bit = (uint32_t)__ffs(v) - 1;
            v &= v - 1;
            P.cand[off++] = (uint32_t)((r0 + tid) * 32 + bit);
        }
        base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
}

int launch_read_probes(gf_ctx* ctx, const FlankIndex* ix, const void* d_reads, size_t n_reads, int read_len, int k, void* d_probes, gf_probe_geom* geom) {
    fill_probe_geom(ctx, ix, n_reads, read_len, k, geom);
    if (n_reads == 0) return GF_OK;
    const uint32_t rb = (uint32_t)((read_len + 3) / 4);
    const uint64_t plane = ((uint64_t)n_reads + 63) & ~(uint64_t)63;
    const size_t n_tiles = (n_reads + TILE_READS - 1) / TILE_READS;
    hipLaunchKernelGGL(read_probes_kernel, dim3((unsigned)std::min<size_t>(n_tiles, (size_t)ctx->n_cu * 8)), dim3(256), TILE_READS * rb + 16, ctx->stream,
                       (const uint8_t*)d_reads, (uint64_t)n_reads, rb, 2 * geom->first, 2 * geom->stride, geom->np, plane, (uint32_t*)d_probes);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

// Pass A's instantiations: the kernel and the name rocprofv3 prints for it, in one entry (gf_screen_kernels reports the entry launched).
// The row forms take (Part4Params, slice_words), the column form Part4Params alone.
struct PassAKernel {
    ScreenForm form;
    bool col;
    uint32_t grp;
    bool bytes;     // (row forms)
    uint32_t ng;    // groups per tile iteration (whole-line forms)
    void (*rows)(Part4Params, uint32_t);
    void (*column)(Part4Params);
    const char* name;
};
#define PA_RUNS(G, B) {ScreenForm::pf4_runs, false, G, B, 0, pf4_scatter_kernel<G, B>, nullptr, "pf4_scatter_kernel<" #G "u, " #B ">"}
#define PA_LINES(G, B, NG) {ScreenForm::pf4_lines, false, G, B, NG, pf4_scatter_lines_kernel<G, B, NG>, nullptr, "pf4_scatter_lines_kernel<" #G "u, " #B ", " #NG "u>"}
#define PA_COL(G) {ScreenForm::pf4_lines, true, G, false, 1, nullptr, pf4_scatter_col_kernel<G>, "pf4_scatter_col_kernel<" #G "u>"}
static const PassAKernel PASS_A_KERNELS[] = {
    PA_RUNS(1, true), PA_RUNS(2, true), PA_RUNS(3, true), PA_RUNS(4, true), PA_RUNS(1, false), PA_RUNS(2, false), PA_RUNS(3, false), PA_RUNS(4, false),
    PA_LINES(1, true, 1), PA_LINES(2, true, 1), PA_LINES(3, true, 1), PA_LINES(4, true, 1),
    PA_LINES(1, false, 1), PA_LINES(2, false, 1), PA_LINES(3, false, 1), PA_LINES(4, false, 1),
    PA_LINES(4, true, 2), PA_LINES(4, false, 2),      // five to eight probes per read: two groups of four
    PA_COL(1), PA_COL(2), PA_COL(3), PA_COL(4),
};
#undef PA_RUNS
#undef PA_LINES
#undef PA_COL
static const PassAKernel* pass_a_kernel(const ScreenPlan& S, bool col) {
    for (const PassAKernel& e : PASS_A_KERNELS)
        if (e.form == S.form && e.col == col && e.grp == S.grp && (col || e.bytes == S.bytes) && (S.form == ScreenForm::pf4_runs || e.ng == S.n_grp)) return &e;
    return nullptr;
}

static void launch_pass_a(gf_ctx* ctx, const ScreenPlan& S, const PassAKernel* pa, const Part4Params& Q) {
    if (pa->column) hipLaunchKernelGGL(pa->column, dim3(Q.n_writers), dim3(64 * PF2_WAVES), S.lds_a_col, ctx->stream, Q);
    else hipLaunchKernelGGL(pa->rows, dim3(Q.n_writers), dim3(64 * PF2_WAVES), S.lds_a, ctx->stream, Q, (uint32_t)S.slice_words);
}

// the parts of a buffer laid out by parts_layout, as pass A writes and the later passes read them
static void point_at_parts(Part4Params& Q, const ScreenPlan& S, void* d_parts) {
    const PartsLayout L = parts_layout(S.n_writers, S.cap, S.gs);
    Q.count = (uint32_t*)d_parts;
    Q.fills = (uint32_t*)((uint8_t*)d_parts + L.o_fills);
    Q.pairs = (uint32_t*)((uint8_t*)d_parts + L.o_pairs);
}

int launch_pass_a_build(gf_ctx* ctx, const ScreenPlan& S, const FilterParams& F, const void* d_probes, void* d_parts, uint32_t* spills) {
    if (S.cap >= (1u << 24) || !spills) return GF_E_INVAL;
    Part4Params Q = {};   // (nothing of an index, no workspace: with `spills` set pass A touches the reads or the column and the parts alone)
    Q.F = F;
    Q.n_writers = S.n_writers;
    Q.cap = S.cap;
    point_at_parts(Q, S, d_parts);
    Q.gs = S.gs;
    Q.n_groups = S.n_groups;
    Q.n_grp = S.n_grp;
    Q.tiles_wg = S.tiles_wg;
    Q.probes = (const uint32_t*)d_probes;
    Q.plane = S.plane;
    Q.spills = spills;
    const PassAKernel* pa = pass_a_kernel(S, d_probes != nullptr);
    if (!pa) return GF_E_UNSUPPORTED;
    ctx->screen_kernels = pa->name;   // (the form the build took)
    launch_pass_a(ctx, S, pa, Q);
    return GF_OK;
}

int launch_filter_pf4(gf_ctx* ctx, const FlankIndex& ix, const ScreenPlan& S, const FilterParams& F, const void* d_probes, const void* d_parts) {
    if (S.cap >= (1u << 24)) return GF_E_INVAL;   // a position must fit 24 bits (2^32 reads stay far below)
    int rc;
    if ((rc = ensure(ctx, ctx->part_ws, d_parts ? S.ws_bytes_resident : S.ws_bytes))) return rc;
    uint8_t* ws = (uint8_t*)ctx->part_ws.p;
    Part4Params Q;
    Q.F = F;
    Q.n_writers = S.n_writers;
    Q.cap = S.cap;
    Q.pairs = (uint32_t*)(ws + S.o_pairs);
    Q.count = (uint32_t*)ws;
    Q.fills = (uint32_t*)(ws + S.o_fills);
    // a library's resident parts: pass B, resolve and list READ count, fills and pairs and write the workspace alone, so the buffer is
    // the same after any number of screens
    if (d_parts) point_at_parts(Q, S, const_cast<void*>(d_parts));
    Q.spills = nullptr;
    Q.gs = S.gs;
    Q.n_groups = S.n_groups;
    Q.n_grp = S.n_grp;
    Q.tiles_wg = S.tiles_wg;
    Q.seen = (uint32_t*)(ws + S.o_seen);
    Q.cand8 = (unsigned long long*)(ws + S.o_cand8);
    Q.chunk_b = (uint8_t*)(ws + S.o_chunk_b);
    Q.n_cand8 = (uint32_t*)(ws + S.o_n_cand8);
    Q.cap8 = S.cap8;
    Q.sgrp = ix.d_sgrp;
    Q.ext = S.pg.ext;
    Q.cand8x = (uint32_t*)(ws + S.o_cand8x);
    Q.probes = (const uint32_t*)d_probes;
    Q.plane = S.plane;
    GF_HIP(ctx, hipMemsetAsync(ws + S.o_n_cand8, 0, S.zero_bytes, ctx->stream));
    const PassAKernel* pa = d_parts ? nullptr : pass_a_kernel(S, d_probes != nullptr);
    if (!pa && !d_parts) return GF_E_UNSUPPORTED;   // (the plan's forms all have their entry)
    ctx->screen_kernels = (pa ? std::string(pa->name) + "," : std::string()) + "pf4_probe_kernel,pf4_resolve_kernel,pf4_list_kernel";
    LaunchTimer tm(ctx, GF_KERNEL_SCREEN);
    if (pa) launch_pass_a(ctx, S, pa, Q);
    const size_t lds_b = (((size_t)1 << (ix.bm_log2 - PF2_NB_LOG2 - 5)) + 16 * (3 * PF4_OBUF + 2 * PF2_PEND)) * 4;
    hipLaunchKernelGGL(pf4_probe_kernel, dim3((unsigned)std::min<size_t>(PF2_NB, (size_t)ctx->n_cu)), dim3(1024), lds_b, ctx->stream, Q);
    const size_t lds_r = (size_t)4 * 8 * (((2 * (size_t)S.rb + 3) / 4) * 4 + 4) * 4;
    hipLaunchKernelGGL(pf4_resolve_kernel, dim3((unsigned)ctx->n_cu * 8), dim3(256), lds_r, ctx->stream, Q);
    hipLaunchKernelGGL(pf4_list_kernel, dim3((unsigned)std::min<size_t>((size_t)ctx->n_cu * 4, ((size_t)F.n_reads + 32 * 256 - 1) / (32 * 256))), dim3(256), 0, ctx->stream, Q);
    ctx->screen_view = gf_screen_view{Q.count, Q.fills, Q.pairs, nullptr, nullptr, Q.n_writers, Q.cap, Q.gs, Q.n_groups};
    if (ctx->screen_keep_cand) {   // diagnostics: the verification passes reuse the candidate buffer, so the tests get a copy of it
        if ((rc = ensure(ctx, ctx->cand_keep, std::max<size_t>((size_t)F.n_reads, 1) * 4 + 16))) return rc;
        GF_HIP(ctx, hipMemcpyAsync(ctx->cand_keep.p, F.n_cand, 4, hipMemcpyDeviceToDevice, ctx->stream));
        GF_HIP(ctx, hipMemcpyAsync((uint8_t*)ctx->cand_keep.p + 16, F.cand, (size_t)F.n_reads * 4, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->screen_view.n_cand = (const uint32_t*)ctx->cand_keep.p;
        ctx->screen_view.cand = (const uint32_t*)((uint8_t*)ctx->cand_keep.p + 16);
    }
    return GF_OK;
}

}  // namespace gf
