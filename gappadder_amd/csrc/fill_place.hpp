// fill_place.hpp — the gapless placement of a gap's pool rows on its winning contig (gappadder_amd/polish.py: placements),
// one device copy for the rounds that place reads on a fill: fill_polish.hip (the vote) and fill_pairs.hip (the pair spans).  Host side,
// pl_place_setup checks the placement rule of a launch and fills PlPlaceArgs.  The device pieces, all but the last called by every
// thread of a workgroup of PL_THREADS threads:
//   pl_stage_contig   the contig, 2 bits a base, twice in LDS: as stored and reverse-complemented, each between PL_LEAD bases of padding, so
//                     that a read that overhangs either end is compared without a branch (the overlap mask removes the padding).  A read as
//                     stored on the reverse-complemented contig at diagonal D is the reverse-complemented read on the contig at n - D - L:
//                     no read is ever reverse-complemented.  Clears the index as well
//   pl_stage_or_skip  pl_stage_contig, its barrier, and what the round does with the contig: 0 (staged), the round's LONG flag (more than
//                     PL_MAX bases: nothing staged) or its NON_ACGT flag (a byte that is no base); what a skipped contig gets is the round's
//   pl_build_index    an open-addressed multimap in LDS from the contig's s-mers to their positions: PL_SLOTS 16-bit slots (position + 1,
//                     0 = free; load <= 1/2), claimed by a 32-bit CAS on the word that holds the slot; a key is compared through its position
//                     (the contig's own bases), so there is no key array and no sentinel key
//   pl_stage_rows     a batch of packed pool rows into LDS, one row per thread (ends on a workgroup barrier)
//   pl_place_row      each of the floor(L / s) unmasked seeds per strand is looked up (the stored window for strand 0, its reverse
//                     complement for strand 1), every hit gives a diagonal, which is verified on the 2-bit words — XOR, pair-fold, popcount
//                     under the overlap and N masks — and counted once: only from its FIRST clean seed inside the overlap (the earlier
//                     seeds are compared again).  Kept per row: the best key (mismatches, then overlap) with its multiplicity and diagonal
#pragma once
#include "fill_body.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t PL_THREADS = 256, PL_MAX = GF_PL_MAX_CONTIG;
constexpr int PL_LOG2 = 14;
constexpr uint32_t PL_SLOTS = 1u << PL_LOG2, PL_SLOT_MASK = PL_SLOTS - 1;
constexpr uint32_t PL_LEAD = 1024;                                           // padding bases on either side of a staged contig (read_len <= 1000)
constexpr uint32_t PL_CTG_WORDS = (PL_LEAD + PL_MAX + PL_LEAD) / 16 + 2;     // 16 bases a word + the bit stream's over-read
constexpr uint32_t PL_ROW_BYTES = 9728, PL_ROW_WORDS = PL_ROW_BYTES / 4 + 10; // a batch of rows (256 rows of 150 bases) + misalignment + over-read
static_assert(PL_SLOTS >= 2 * PL_MAX && PL_MAX < 0xFFFFu && PL_LEAD % 16 == 0, "placement geometry");

// the pool and the placement rule of one launch
struct PlPlaceArgs {
    const uint8_t* pool;
    const uint32_t* nmask;       // or null; rows aligned with the pool's
    uint32_t rb, L, nmw, batch_rows;
    uint32_t s, n_seeds, max_mm, min_ov;
};

// the rows of one batch a workgroup may take: what fits PL_ROW_BYTES, one row per thread at the most
inline uint32_t pl_batch_rows(uint32_t rb) { return PL_ROW_BYTES / rb < PL_THREADS ? PL_ROW_BYTES / rb : PL_THREADS; }

// The placement rule of a launch as the ABI entries receive it: GF_E_UNSUPPORTED for seed outside 12..32, max_mismatch outside 0..15,
// min_overlap outside seed..read_len or no more seeds than mismatches (then *A is untouched); else *A is filled and GF_OK returned
inline int pl_place_setup(const void* d_pool_packed, const void* d_nmask_or_null, int read_len, int seed, int max_mismatch, int min_overlap,
                          PlPlaceArgs* A) {
    if (seed < 12 || seed > 32 || max_mismatch < 0 || max_mismatch > 15 || min_overlap < seed || min_overlap > read_len ||
        read_len / seed <= max_mismatch)
        return GF_E_UNSUPPORTED;
    A->pool = (const uint8_t*)d_pool_packed;
    A->nmask = (const uint32_t*)d_nmask_or_null;
    A->rb = (uint32_t)gf_packed_read_bytes(read_len);
    A->L = (uint32_t)read_len;
    A->nmw = (uint32_t)((read_len + 31) / 32);
    A->batch_rows = pl_batch_rows(A->rb);
    A->s = (uint32_t)seed;
    A->n_seeds = (uint32_t)(read_len / seed);
    A->max_mm = (uint32_t)max_mismatch;
    A->min_ov = (uint32_t)min_overlap;
    return GF_OK;
}

// cnt accepted (strand, diagonal) pairs share the best key; strand and D are those of the first of them.  D is the diagonal on the array
// of its strand: on the contig as stored for strand 0, on its reverse complement for strand 1.  key: the best key itself, mismatches << 12
// | (4095 - overlap), EMPTY32 without a pair (fill_place_split.hpp goes on from it)
struct PlPlacement {
    uint32_t cnt, strand, key;
    int32_t D;
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

// stage: word w of either array holds the bases 16 w - PL_LEAD .. + 15 of the contig / of its reverse complement; the index is cleared.
// Returns nonzero in a thread that met a byte other than A, C, G, T.  The caller's barrier ends the stage
__device__ __forceinline__ uint32_t pl_stage_contig(const char* ctg, uint32_t n, uint32_t* s_fwd, uint32_t* s_rc, uint32_t* s_idx) {
    const uint32_t t = threadIdx.x;
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
    return bad;
}

// stage or skip: the contig of n bases is staged unless it is longer than PL_MAX; *s_bad — one word of LDS that is zero before the
// caller's last barrier — takes the stage's verdict.  Ends on a workgroup barrier.  Returns, the same in all threads, 0 or the flag the
// round gives a contig it does not place: f_long, f_non_acgt
__device__ __forceinline__ uint32_t pl_stage_or_skip(const char* ctg, uint32_t n, uint32_t* s_fwd, uint32_t* s_rc, uint32_t* s_idx, uint32_t* s_bad,
                                                     uint32_t f_long, uint32_t f_non_acgt) {
    const bool is_long = n > PL_MAX;
    if (!is_long && pl_stage_contig(ctg, n, s_fwd, s_rc, s_idx)) atomicOr(s_bad, 1u);
    __syncthreads();
    return is_long ? f_long : *s_bad ? f_non_acgt : 0u;
}

// index: every s-mer position into the first free slot from its hash on.  The caller's barrier ends the build
__device__ __forceinline__ void pl_build_index(const uint32_t* s_fwd, uint32_t* s_idx, uint32_t n, uint32_t s) {
    for (uint32_t p = threadIdx.x; p + s <= n; p += PL_THREADS) {
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
}

// the nb rows from pool row row0 on into s_rows; returns the byte offset of the first of them there.  Ends on a workgroup barrier
__device__ __forceinline__ uint32_t pl_stage_rows(const PlPlaceArgs& A, uint64_t row0, uint32_t nb, uint32_t* s_rows) {
    const uint32_t t = threadIdx.x;
    const uint8_t* gp = A.pool + row0 * A.rb;
    const uint32_t mis = (uint32_t)((uintptr_t)gp & 3u);
    const uint32_t* gw = (const uint32_t*)(gp - mis);
    const uint32_t n_words = (mis + nb * A.rb + 3) >> 2;
    for (uint32_t w = t; w < n_words; w += PL_THREADS) s_rows[w] = gw[w];
    if (t < 8) s_rows[n_words + t] = 0;
    __syncthreads();
    return mis;
}

// the placement of the staged row at bit offset rbit (N-mask words nm or null) on the contig of n bases staged in s_fwd / s_rc / s_idx
__device__ __forceinline__ PlPlacement pl_place_row(const PlPlaceArgs& A, const uint32_t* s_rows, uint32_t rbit, const uint32_t* nm,
                                                    const uint32_t* s_fwd, const uint32_t* s_rc, const uint32_t* s_idx, uint32_t n) {
    const uint32_t s = A.s, L = A.L;
    uint32_t best = EMPTY32, cnt = 0, bstrand = 0;
    int32_t bD = 0;
    for (uint32_t strand = 0; strand < 2; ++strand) {
        const uint32_t* C = strand ? s_rc : s_fwd;
        for (uint32_t j = 0; j < A.n_seeds; ++j) {
            const uint32_t ws = strand ? L - (j + 1) * s : j * s;
            if (nm && row_window_masked(nm, A.nmw, ws, s)) continue;
            const uint64_t kmer = stream_kmer64(s_rows, rbit + 2 * ws, (int)s);
            const uint64_t key = strand ? revpairs64(~kmer) << (64 - 2 * s) : kmer;
            uint32_t h = hash_kmer(K128{key, 0}, PL_LOG2);
            for (uint32_t e; (e = pl_slot(s_idx, h)) != 0; h = (h + 1) & PL_SLOT_MASK) {
                const uint32_t p = e - 1;
                if (stream_kmer64(s_fwd, 2 * (PL_LEAD + p), (int)s) != key) continue;
                const int32_t D = (strand ? (int32_t)(n - p - s) : (int32_t)p) - (int32_t)ws;
                const uint32_t i0 = D < 0 ? (uint32_t)(-D) : 0u, i1 = (int32_t)L < (int32_t)n - D ? L : (uint32_t)((int32_t)n - D);
                const uint32_t ov = i1 - i0;
                if (ov < A.min_ov) continue;
                bool seen = false;                   // an earlier seed of this strand that is clean on this diagonal has counted it
                for (uint32_t j2 = 0; j2 < j && !seen; ++j2) {
                    const uint32_t w2 = strand ? L - (j2 + 1) * s : j2 * s;
                    if (w2 < i0 || w2 + s > i1 || (nm && row_window_masked(nm, A.nmw, w2, s))) continue;
                    seen = stream_kmer64(s_rows, rbit + 2 * w2, (int)s) ==
                           stream_kmer64(C, 2u * (uint32_t)((int32_t)PL_LEAD + D + (int32_t)w2), (int)s);
                }
                if (seen) continue;
                const uint32_t mm = pl_mismatches(s_rows, rbit, nm, C, D, i0, i1, A.max_mm);
                if (mm > A.max_mm) continue;
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
    PlPlacement out;
    out.cnt = cnt;
    out.strand = bstrand;
    out.key = best;
    out.D = bD;
    return out;
}

}  // namespace gf
