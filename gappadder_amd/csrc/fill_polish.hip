// fill_polish.hip — consensus polish of the closed gaps: the reads of a gap's own pool are placed without gaps on the gap's winning
// contig, every column of the fill takes a vote, and the polished contig is written out with one record per gap (gf_fill_polish_dev,
// include/gapfill_hip.h; definition and host twin: gappadder_amd/polish.py).  The reference has no such stage.
//
// One workgroup of 256 threads per closed gap, grid-stride over the gaps.  The body [b0, b1) comes from fill_body.hpp, as in
// fill_support.hip.  Per gap:
//   stage    the contig, 2 bits a base, twice in LDS: as stored and reverse-complemented, each between PL_LEAD bases of padding, so
//            that a read that overhangs either end is compared without a branch (the overlap mask removes the padding).  A read as
//            stored on the reverse-complemented contig at diagonal D is the reverse-complemented read on the contig at n - D - L: no
//            read is ever reverse-complemented
//   index    an open-addressed multimap in LDS from the contig's s-mers to their positions: PL_SLOTS 16-bit slots (position + 1,
//            0 = free; load <= 1/2), claimed by a 32-bit CAS on the word that holds the slot; a key is compared through its position
//            (the contig's own bases), so there is no key array and no sentinel key
//   place    the pool's packed rows are staged a batch at a time, one row per thread: each of the floor(L / s) unmasked seeds per strand
//            is looked up (the stored window for strand 0, its reverse complement for strand 1), every hit gives a diagonal, which
//            is verified on the 2-bit words — XOR, pair-fold, popcount under the overlap and N masks — and counted once: only from
//            its FIRST clean seed inside the overlap (the earlier seeds are compared again).  Kept per row: the best key
//            (mismatches, then overlap) with its multiplicity and its diagonal
//   vote     a row with one best placement adds its unmasked bases to the columns' four counters (LDS atomics) — PL_VCHUNK body
//            columns per pass; a longer body costs another pass over the pool (the placement is computed again), never a result
//   decide   per column, integer comparisons of the four counters: independent of the order of the atomics.  The polished contig goes
//            to d_bases with byte stores, at an offset from the u64 counter in d_stats
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md §16; no scratch, static LDS below 64 KB.
#include <cstring>

#include "fill_body.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t PL_THREADS = 256, PL_MAX = GF_PL_MAX_CONTIG, PL_VCHUNK = 1024;
constexpr int PL_LOG2 = 14;
constexpr uint32_t PL_SLOTS = 1u << PL_LOG2, PL_SLOT_MASK = PL_SLOTS - 1;
constexpr uint32_t PL_LEAD = 1024;                                           // padding bases on either side of a staged contig (read_len <= 1000)
constexpr uint32_t PL_CTG_WORDS = (PL_LEAD + PL_MAX + PL_LEAD) / 16 + 2;     // 16 bases a word + the bit stream's over-read
constexpr uint32_t PL_ROW_BYTES = 9728, PL_ROW_WORDS = PL_ROW_BYTES / 4 + 10; // a batch of rows (256 rows of 150 bases) + misalignment + over-read
static_assert(PL_SLOTS >= 2 * PL_MAX && PL_MAX < 0xFFFFu && PL_LEAD % 16 == 0, "polish geometry");

struct PlParams {
    const uint8_t* pool;
    const uint32_t* nmask;       // or null
    const uint64_t* pool_off;
    uint64_t pool_rows;
    uint32_t rb, L, nmw, batch_rows;
    FillBodyArgs body;
    const uint32_t* n_contigs;
    uint32_t contig_cap;
    const char* seq;
    const unsigned long long* gap_best;
    uint32_t n_gaps, s, n_seeds, max_mm, min_ov, min_votes;
    gf_fill_polish* out;
    uint8_t* bases;
    uint64_t base_cap;
    uint32_t* stats;
};

__device__ __forceinline__ uint32_t pl_slot(const uint32_t* idx, uint32_t h) { return (idx[h >> 1] >> ((h & 1u) * 16)) & 0xFFFFu; }

// 32 bits -> the even bits of 64 (bit b -> bit 2 b)
__device__ __forceinline__ uint64_t pl_spread(uint32_t v) {
    uint64_t x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

__device__ __forceinline__ uint64_t pl_bits64(const uint32_t* words, uint32_t bit) {
    return ((uint64_t)stream32(words, bit) << 32) | stream32(words, bit + 32);
}

// mismatches of the row (bit offset rbit in s_rows, N-mask words nm or null) on the staged contig `ctg` at diagonal D, over the read
// positions [i0, i1); stops counting beyond `limit`
__device__ __forceinline__ uint32_t pl_mismatches(const uint32_t* s_rows, uint32_t rbit, const uint32_t* nm, const uint32_t* ctg, int32_t D,
                                                  uint32_t i0, uint32_t i1, uint32_t limit) {
    uint32_t mm = 0;
    for (uint32_t w = i0 >> 5; 32 * w < i1 && mm <= limit; ++w) {
        const uint32_t lo = i0 > 32 * w ? i0 - 32 * w : 0u, hi = i1 - 32 * w < 32u ? i1 - 32 * w : 32u;
        uint32_t vm = (hi == 32u ? 0xFFFFFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);       // bit b: read base 32 w + b is compared
        if (nm) vm &= ~nm[w];
        const uint64_t x = pl_bits64(s_rows, rbit + 64 * w) ^ pl_bits64(ctg, 2u * (uint32_t)((int32_t)PL_LEAD + D + (int32_t)(32 * w)));
        const uint64_t m = (x | (x >> 1)) & 0x5555555555555555ull;                            // base b of the word: bit 62 - 2 b
        mm += (uint32_t)__popcll(m & pl_spread(__brev(vm)));
    }
    return mm;
}

__global__ __launch_bounds__(PL_THREADS) void fill_polish_kernel(PlParams P) {
    __shared__ uint32_t s_idx[PL_SLOTS / 2];
    __shared__ uint32_t s_votes[PL_VCHUNK * 4];
    __shared__ uint32_t s_fwd[PL_CTG_WORDS];
    __shared__ uint32_t s_rc[PL_CTG_WORDS];
    __shared__ uint32_t s_rows[PL_ROW_WORDS];
    __shared__ uint32_t s_loc[2];
    __shared__ uint32_t s_acc[5];               // a byte that is no base, columns changed, columns uncovered, rows placed, rows ambiguous
    __shared__ unsigned long long s_off;
    const uint32_t t = threadIdx.x, s = P.s, L = P.L;
    const uint32_t n_list = *P.n_contigs < P.contig_cap ? *P.n_contigs : P.contig_cap;
    for (uint32_t g = blockIdx.x; g < P.n_gaps; g += gridDim.x) {
        const unsigned long long word = P.gap_best[g];
        gf_fill_polish rec;
        rec.off = 0;
        rec.len = rec.flags = rec.n_cols = rec.n_changed = rec.n_uncovered = rec.reads_placed = rec.reads_ambiguous = rec.reserved = 0;
        if (!word) {
            if (t == 0) P.out[g] = rec;
            continue;
        }
        const FillBody fb = fill_body<PL_THREADS>(P.body, n_list, g, word, s_loc);      // (the same in all threads)
        if (!fb.ok) {
            if (t == 0) {
                P.out[g] = rec;
                atomicAdd(P.stats + GF_PL_MISMATCH, 1u);
            }
            continue;
        }
        const uint32_t n = fb.c.length;
        const char* ctg = P.seq + fb.c.seq_off;
        const uint32_t b0 = (uint32_t)fb.b0, b1 = (uint32_t)fb.b1, n_cols = b1 - b0;
        const bool is_long = n > PL_MAX;
        __syncthreads();                         // (the previous gap's record is written)
        if (t == 0) {
            s_acc[0] = s_acc[1] = s_acc[2] = s_acc[3] = s_acc[4] = 0;
            s_off = atomicAdd((unsigned long long*)(P.stats + GF_PL_BASES), (unsigned long long)n);
        }
        __syncthreads();
        // ---- stage: word w of either array holds the bases 16 w - PL_LEAD .. + 15 of the contig / of its reverse complement
        if (!is_long) {
            uint32_t bad = 0;
            for (uint32_t w = t; w < PL_CTG_WORDS; w += PL_THREADS) {
                uint32_t vf = 0, vr = 0;
                const int32_t x0 = (int32_t)(16 * w) - (int32_t)PL_LEAD;
                if (x0 + 16 > 0 && x0 < (int32_t)n) {
                    for (int32_t b = 0; b < 16; ++b) {
                        const int32_t x = x0 + b;
                        if (x < 0 || x >= (int32_t)n) continue;
                        const uint32_t cf = base_code4((uint8_t)ctg[x]), cr = base_code4((uint8_t)ctg[n - 1 - (uint32_t)x]);
                        bad |= cf >> 2;
                        vf |= (cf & 3u) << (30 - 2 * b);
                        vr |= (3u - (cr & 3u)) << (30 - 2 * b);
                    }
                }
                s_fwd[w] = bswap32(vf);
                s_rc[w] = bswap32(vr);
            }
            for (uint32_t i = t; i < PL_SLOTS / 2; i += PL_THREADS) s_idx[i] = 0;
            if (bad) atomicOr(&s_acc[0], 1u);
        }
        __syncthreads();
        const uint64_t off = s_off;
        const bool fits = off + n <= P.base_cap;
        uint8_t* outp = P.bases + off;
        const uint32_t skip = is_long ? (uint32_t)GF_PL_F_LONG : s_acc[0] ? (uint32_t)GF_PL_F_NON_ACGT : 0u;
        if (skip) {                              // copied out unpolished
            if (fits)
                for (uint32_t i = t; i < n; i += PL_THREADS) outp[i] = (uint8_t)ctg[i];
            if (t == 0) {
                rec.off = fits ? off : 0;
                rec.len = fits ? n : 0;
                rec.flags = skip | (fits ? 0u : (uint32_t)GF_PL_F_OVERFLOW);
                rec.n_cols = n_cols;
                P.out[g] = rec;
                atomicAdd(P.stats + (is_long ? GF_PL_SKIPPED_LONG : GF_PL_SKIPPED_NON_ACGT), 1u);
                if (!fits) atomicAdd(P.stats + GF_PL_OVERFLOW, 1u);
            }
            continue;
        }
        // ---- index: every s-mer position into the first free slot from its hash on
        for (uint32_t p = t; p + s <= n; p += PL_THREADS) {
            const uint64_t key = stream_kmer64(s_fwd, 2 * (PL_LEAD + p), (int)s);
            uint32_t h = hash_kmer(K128{key, 0}, PL_LOG2);
            for (;;) {
                uint32_t* wp = &s_idx[h >> 1];
                const uint32_t sh = (h & 1u) * 16;
                uint32_t old = *wp;
                bool mine = false;
                while (((old >> sh) & 0xFFFFu) == 0) {
                    const uint32_t prev = atomicCAS(wp, old, old | ((p + 1) << sh));
                    if (prev == old) { mine = true; break; }
                    old = prev;
                }
                if (mine) break;
                h = (h + 1) & PL_SLOT_MASK;
            }
        }
        uint64_t r0 = P.pool_off[g], r1 = P.pool_off[g + 1];
        if (r1 > P.pool_rows) r1 = P.pool_rows;
        if (r0 > r1) r0 = r1;
        // ---- place, vote and decide: PL_VCHUNK body columns per pass (one pass for an empty body: the rows are still counted)
        for (uint32_t c_lo = b0, pass = 0; pass == 0 || c_lo < b1; c_lo += PL_VCHUNK, ++pass) {
            const uint32_t c_hi = b1 - c_lo < PL_VCHUNK ? b1 : c_lo + PL_VCHUNK;
            for (uint32_t i = t; i < PL_VCHUNK * 4; i += PL_THREADS) s_votes[i] = 0;
            __syncthreads();                     // (also: the index is built)
            for (uint64_t row0 = r0; row0 < r1; row0 += P.batch_rows) {
                const uint32_t nb = r1 - row0 < P.batch_rows ? (uint32_t)(r1 - row0) : P.batch_rows;
                const uint8_t* gp = P.pool + row0 * P.rb;
                const uint32_t mis = (uint32_t)((uintptr_t)gp & 3u);
                const uint32_t* gw = (const uint32_t*)(gp - mis);
                const uint32_t n_words = (mis + nb * P.rb + 3) >> 2;
                for (uint32_t w = t; w < n_words; w += PL_THREADS) s_rows[w] = gw[w];
                if (t < 8) s_rows[n_words + t] = 0;
                __syncthreads();
                if (t < nb) {
                    const uint32_t rbit = (mis + t * P.rb) * 8;
                    const uint32_t* nm = P.nmask ? P.nmask + (row0 + t) * P.nmw : nullptr;
                    uint32_t best = EMPTY32, cnt = 0, bstrand = 0;
                    int32_t bD = 0;
                    for (uint32_t strand = 0; strand < 2; ++strand) {
                        const uint32_t* A = strand ? s_rc : s_fwd;
                        for (uint32_t j = 0; j < P.n_seeds; ++j) {
                            const uint32_t ws = strand ? L - (j + 1) * s : j * s;
                            if (nm && row_window_masked(nm, P.nmw, ws, s)) continue;
                            const uint64_t kmer = stream_kmer64(s_rows, rbit + 2 * ws, (int)s);
                            const uint64_t key = strand ? revpairs64(~kmer) << (64 - 2 * s) : kmer;
                            uint32_t h = hash_kmer(K128{key, 0}, PL_LOG2);
                            for (uint32_t e; (e = pl_slot(s_idx, h)) != 0; h = (h + 1) & PL_SLOT_MASK) {
                                const uint32_t p = e - 1;
                                if (stream_kmer64(s_fwd, 2 * (PL_LEAD + p), (int)s) != key) continue;
                                const int32_t D = (strand ? (int32_t)(n - p - s) : (int32_t)p) - (int32_t)ws;
                                const uint32_t i0 = D < 0 ? (uint32_t)(-D) : 0u, i1 = (int32_t)L < (int32_t)n - D ? L : (uint32_t)((int32_t)n - D);
                                const uint32_t ov = i1 - i0;
                                if (ov < P.min_ov) continue;
                                bool seen = false;                   // an earlier seed of this strand that is clean on this diagonal has counted it
                                for (uint32_t j2 = 0; j2 < j && !seen; ++j2) {
                                    const uint32_t w2 = strand ? L - (j2 + 1) * s : j2 * s;
                                    if (w2 < i0 || w2 + s > i1 || (nm && row_window_masked(nm, P.nmw, w2, s))) continue;
                                    seen = stream_kmer64(s_rows, rbit + 2 * w2, (int)s) ==
                                           stream_kmer64(A, 2u * (uint32_t)((int32_t)PL_LEAD + D + (int32_t)w2), (int)s);
                                }
                                if (seen) continue;
                                const uint32_t mm = pl_mismatches(s_rows, rbit, nm, A, D, i0, i1, P.max_mm);
                                if (mm > P.max_mm) continue;
                                const uint32_t k2 = (mm << 12) | (4095u - ov);
                                if (k2 < best) {
                                    best = k2;
                                    cnt = 1;
                                    bstrand = strand;
                                    bD = D;
                                } else if (k2 == best) {
                                    ++cnt;
                                }
                            }
                        }
                    }
                    if (pass == 0 && cnt) atomicAdd(&s_acc[cnt == 1 ? 3 : 4], 1u);
                    if (cnt == 1 && c_hi > c_lo) {
                        // strand 0: read base i on column D + i; strand 1: its complement on column n - 1 - D - i
                        const int32_t i0 = bD < 0 ? -bD : 0, i1 = (int32_t)L < (int32_t)n - bD ? (int32_t)L : (int32_t)n - bD;
                        int32_t lo = bstrand ? (int32_t)n - bD - (int32_t)c_hi : (int32_t)c_lo - bD;
                        int32_t hi = bstrand ? (int32_t)n - bD - (int32_t)c_lo : (int32_t)c_hi - bD;
                        lo = lo > i0 ? lo : i0;
                        hi = hi < i1 ? hi : i1;
                        const uint8_t* rowb = (const uint8_t*)s_rows + mis + t * P.rb;
                        for (int32_t i = lo; i < hi; ++i) {
                            if (nm && ((nm[i >> 5] >> (i & 31)) & 1u)) continue;
                            const uint32_t code = (rowb[i >> 2] >> (6 - 2 * (i & 3))) & 3u;
                            const uint32_t col = bstrand ? n - 1 - (uint32_t)(bD + i) : (uint32_t)(bD + i);
                            atomicAdd(&s_votes[(col - c_lo) * 4 + (bstrand ? 3u - code : code)], 1u);
                        }
                    }
                }
                __syncthreads();
            }
            uint32_t changed = 0, uncovered = 0;
            for (uint32_t j = c_lo + t; j < c_hi; j += PL_THREADS) {
                const uint32_t* v = s_votes + (j - c_lo) * 4;
                const uint32_t v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
                const uint32_t cur = stream32(s_fwd, 2 * (PL_LEAD + j)) >> 30;
                uint32_t bb = 0, bv = v0;
                if (v1 > bv) { bb = 1; bv = v1; }
                if (v2 > bv) { bb = 2; bv = v2; }
                if (v3 > bv) { bb = 3; bv = v3; }
                const uint32_t vc = cur == 0 ? v0 : cur == 1 ? v1 : cur == 2 ? v2 : v3;
                const bool change = bv >= P.min_votes && bv > vc;
                const uint32_t now = change ? bb : cur;
                changed += change;
                uncovered += (v0 | v1 | v2 | v3) == 0;
                if (fits) outp[j] = (uint8_t)(now == 0 ? 'A' : now == 1 ? 'C' : now == 2 ? 'G' : 'T');
            }
            if (changed) atomicAdd(&s_acc[1], changed);
            if (uncovered) atomicAdd(&s_acc[2], uncovered);
            __syncthreads();                     // (the votes are read: the next pass clears them)
        }
        if (fits)
            for (uint32_t i = t; i < n; i += PL_THREADS)
                if (i < b0 || i >= b1) outp[i] = (uint8_t)ctg[i];
        if (t == 0) {
            rec.off = fits ? off : 0;
            rec.len = fits ? n : 0;
            rec.flags = fits ? 0u : (uint32_t)GF_PL_F_OVERFLOW;
            rec.n_cols = n_cols;
            rec.n_changed = s_acc[1];
            rec.n_uncovered = s_acc[2];
            rec.reads_placed = s_acc[3];
            rec.reads_ambiguous = s_acc[4];
            P.out[g] = rec;
            atomicAdd(P.stats + GF_PL_GAPS, 1u);
            atomicAdd((unsigned long long*)(P.stats + GF_PL_CHANGED), (unsigned long long)s_acc[1]);
            atomicAdd((unsigned long long*)(P.stats + GF_PL_PLACED), (unsigned long long)s_acc[3]);
            atomicAdd((unsigned long long*)(P.stats + GF_PL_AMBIGUOUS), (unsigned long long)s_acc[4]);
            if (!fits) atomicAdd(P.stats + GF_PL_OVERFLOW, 1u);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_polish_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                                  int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                  const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                                  int min_overlap, int min_votes, void* d_polish, void* d_bases, size_t base_cap, void* d_stats) {
    if (!ctx || !d_pool_off || (pool_rows && !d_pool_packed) || !d_contigs || !d_n_contigs || !d_seq || !d_gap_best || !d_polish || !d_stats ||
        (base_cap && !d_bases) || read_len < 1 || read_len > 1000 || contig_cap > 0x7FFFFFFFull)
        return GF_E_INVAL;
    if (!d_ctg_pick_or_null && (anchor_long < 8 || anchor_long > FB_ANCHOR_MAX || (anchor_short && (anchor_short < 8 || anchor_short >= anchor_long))))
        return GF_E_INVAL;
    if (seed < 12 || seed > 32 || max_mismatch < 0 || max_mismatch > 15 || min_overlap < seed || min_overlap > read_len || min_votes < 1 ||
        read_len / seed <= max_mismatch)
        return GF_E_UNSUPPORTED;
    const size_t ng = ctx->gaps.size();
    if (ctx->flank_left.size() != ng || ctx->flank_right.size() != ng) return GF_E_STATE;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(d_stats, 0, 4 * GF_PL_WORDS, ctx->stream));
    if (!ng) return GF_OK;
    PlParams P;
    memset(&P, 0, sizeof(P));
    int rc;
    if (!d_ctg_pick_or_null) {
        if ((rc = anchor_table_for(ctx, anchor_long, &P.body.anc_l))) return rc;
        if (anchor_short && (rc = anchor_table_for(ctx, anchor_short, &P.body.anc_s))) return rc;
        P.body.a_l = (uint32_t)anchor_long;
        P.body.a_s = (uint32_t)anchor_short;
    }
    P.pool = (const uint8_t*)d_pool_packed;
    P.nmask = (const uint32_t*)d_nmask_or_null;
    P.pool_off = (const uint64_t*)d_pool_off;
    P.pool_rows = pool_rows;
    P.rb = (uint32_t)gf_packed_read_bytes(read_len);
    P.L = (uint32_t)read_len;
    P.nmw = (uint32_t)((read_len + 31) / 32);
    P.batch_rows = PL_ROW_BYTES / P.rb < PL_THREADS ? PL_ROW_BYTES / P.rb : PL_THREADS;
    P.body.contigs = (const gf_contig*)d_contigs;
    P.body.seq = P.seq = (const char*)d_seq;
    P.body.ctg_pick = (const gf_ctg_pick*)d_ctg_pick_or_null;
    P.n_contigs = (const uint32_t*)d_n_contigs;
    P.contig_cap = (uint32_t)contig_cap;
    P.gap_best = (const unsigned long long*)d_gap_best;
    P.n_gaps = (uint32_t)ng;
    P.s = (uint32_t)seed;
    P.n_seeds = (uint32_t)(read_len / seed);
    P.max_mm = (uint32_t)max_mismatch;
    P.min_ov = (uint32_t)min_overlap;
    P.min_votes = (uint32_t)min_votes;
    P.out = (gf_fill_polish*)d_polish;
    P.bases = (uint8_t*)d_bases;
    P.base_cap = base_cap;
    P.stats = (uint32_t*)d_stats;
    const size_t resident = (size_t)ctx->n_cu * 2;                     // workgroups the static LDS lets a CU hold
    const size_t blocks = ng < resident ? ng : resident;
    LaunchTimer tm(ctx, GF_KERNEL_POLISH);
    hipLaunchKernelGGL(fill_polish_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
