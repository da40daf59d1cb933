// fill_place_split.hpp — the placement of a pool row on its gap's winning contig with at most ONE indel (gappadder_amd/polish_gapped.py:
// placements_gapped), on fill_place.hpp's staging, s-mer index and mismatch words; used by fill_polish_gapped.hip.
//
// A row is never reverse-complemented: strand 1 is the row as stored on the reverse-complemented contig (fill_place.hpp).  In that frame
// the definition's split candidate reads the same for both strands — a LEFT part [i0, x) on diagonal Da, gi inserted read bases, a RIGHT
// part [x + gi, i1) on diagonal Db, Db - Da = g - gi, x between the end of Da's leftmost clean seed and the start of Db's rightmost one less gi
// — but for the tie between equal mm(x): the definition takes the leftmost column of the stored contig, which is the smallest x for
// strand 0 and the LARGEST for strand 1.  plg_event maps breakpoint, column and inserted bases to stored orientation.
//   plg_place_row   1. the gapless candidates: pl_place_row itself (its best key and multiplicity are where the search goes on);  2. only when no
//                   gapless candidate costs less than two — a split costs its mismatches plus two, so it can neither beat nor tie one that
//                   does —, per strand every diagonal Da from its leftmost clean seed (the LDS index), against the 2 G diagonals Db within
//                   max_indel of it that the index gives for the seed windows right of that seed, each taken from the rightmost window that is clean on it.  mm(x) is taken
//                   once at the smallest x (two pl_mismatches) and then carried along x through the 32-base mismatch masks of the two
//                   diagonals (XOR, pair-fold, squeeze): +1 for a base the left part gains, -1 for one the right part loses
#pragma once
#include "fill_place.hpp"

namespace gf {

// One best candidate (cnt == 1): strand, the left diagonal D, the right diagonal D2 (== D: gapless) and the breakpoint x of a split
struct PlgPlacement {
    uint32_t cnt, strand, x;
    int32_t D, D2;
};

// the even bits of 64 -> 32 bits (bit 2 b -> bit b): pl_spread's inverse
__device__ __forceinline__ uint32_t plg_squeeze(uint64_t x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}

// bit b: read base base0 + b is unmasked and differs from the staged contig `ctg` on diagonal D (base0 + 31 < L + 32; no overlap mask:
// the caller asks inside the contig)
__device__ __forceinline__ uint32_t plg_diff32(const uint32_t* s_rows, uint32_t rbit, const uint32_t* nm, uint32_t nmw, const uint32_t* ctg,
                                               int32_t D, uint32_t base0) {
    const uint64_t x = pl_bits64(s_rows, rbit + 2 * base0) ^ pl_bits64(ctg, 2u * (uint32_t)((int32_t)PL_LEAD + D + (int32_t)base0));
    uint32_t m = __brev(plg_squeeze(x | (x >> 1)));
    if (nm) {
        const uint32_t w = base0 >> 5, sh = base0 & 31;
        const uint32_t lo = w < nmw ? nm[w] : 0u, hi = w + 1 < nmw ? nm[w + 1] : 0u;
        m &= ~(sh ? (lo >> sh) | (hi << (32 - sh)) : lo);
    }
    return m;
}

// the read's window [ws, ws + s) is unmasked, lies inside the contig of n bases on diagonal D and equals it
__device__ __forceinline__ bool plg_seed_on(const uint32_t* s_rows, uint32_t rbit, const uint32_t* nm, uint32_t nmw, const uint32_t* ctg, int32_t D,
                                            uint32_t ws, uint32_t s, uint32_t n) {
    const int32_t p = D + (int32_t)ws;
    if (p < 0 || p + (int32_t)s > (int32_t)n) return false;
    if (nm && row_window_masked(nm, nmw, ws, s)) return false;
    return stream_kmer64(s_rows, rbit + 2 * ws, (int)s) == stream_kmer64(ctg, 2u * (uint32_t)((int32_t)PL_LEAD + p), (int)s);
}

// the placement of the staged row at bit offset rbit (N-mask words nm or null) on the contig of n bases staged in s_fwd / s_rc / s_idx
__device__ __forceinline__ PlgPlacement plg_place_row(const PlPlaceArgs& A, uint32_t max_indel, const uint32_t* s_rows, uint32_t rbit,
                                                      const uint32_t* nm, const uint32_t* s_fwd, const uint32_t* s_rc, const uint32_t* s_idx,
                                                      uint32_t n) {
    const uint32_t s = A.s, L = A.L;
    const PlPlacement gapless = pl_place_row(A, s_rows, rbit, nm, s_fwd, s_rc, s_idx, n);
    uint32_t best = gapless.key;
    PlgPlacement out;
    out.cnt = gapless.cnt;
    out.strand = gapless.strand;
    out.x = 0;
    out.D = out.D2 = gapless.D;
    if ((best >> 12) < 2u || A.max_mm < 2u) return out;      // a gapless candidate of cost 0 or 1, or no room for an indel's two: no split can reach it
    for (uint32_t strand = 0; strand < 2; ++strand) {
        const uint32_t* C = strand ? s_rc : s_fwd;
        const uint32_t w_base = strand ? L - A.n_seeds * s : 0u;      // the seed windows of the row frame, ascending
        for (uint32_t j = 0; j < A.n_seeds; ++j) {
            const uint32_t ws = w_base + j * s;
            if (nm && row_window_masked(nm, A.nmw, ws, s)) continue;
            const uint64_t kmer = stream_kmer64(s_rows, rbit + 2 * ws, (int)s);
            const uint64_t key = strand ? revpairs64(~kmer) << (64 - 2 * s) : kmer;
            uint32_t h = hash_kmer(K128{key, 0}, PL_LOG2);
            for (uint32_t e; (e = pl_slot(s_idx, h)) != 0; h = (h + 1) & PL_SLOT_MASK) {
                const uint32_t p = e - 1;
                if (stream_kmer64(s_fwd, 2 * (PL_LEAD + p), (int)s) != key) continue;
                const int32_t D = (strand ? (int32_t)(n - p - s) : (int32_t)p) - (int32_t)ws;
                bool seen = false;               // a seed further left is clean on this diagonal: its pairs are counted from there
                for (uint32_t j2 = 0; j2 < j && !seen; ++j2) seen = plg_seed_on(s_rows, rbit, nm, A.nmw, C, D, w_base + j2 * s, s, n);
                if (seen) continue;
                const uint32_t i0 = D < 0 ? (uint32_t)(-D) : 0u;
                // ---- the split candidates (strand, D, D2): ws is D's leftmost clean seed
                const uint32_t x_lo = ws + s;
                // the right diagonals come from the index as well: every seed window right of D's leftmost is looked up, and a hit
                // within max_indel of D is taken from the RIGHTMOST window that is clean on it (a window further right is compared)
                for (uint32_t j2 = A.n_seeds; j2 > j + 1; --j2) {
                    const uint32_t ws2 = w_base + (j2 - 1) * s;
                    if (nm && row_window_masked(nm, A.nmw, ws2, s)) continue;
                    const uint64_t kmer2 = stream_kmer64(s_rows, rbit + 2 * ws2, (int)s);
                    const uint64_t key2 = strand ? revpairs64(~kmer2) << (64 - 2 * s) : kmer2;
                    uint32_t h2 = hash_kmer(K128{key2, 0}, PL_LOG2);
                    for (uint32_t e2; (e2 = pl_slot(s_idx, h2)) != 0; h2 = (h2 + 1) & PL_SLOT_MASK) {
                        const uint32_t p2 = e2 - 1;
                        const int32_t D2 = (strand ? (int32_t)(n - p2 - s) : (int32_t)p2) - (int32_t)ws2;
                        const int32_t dd = D2 - D;
                        if (dd == 0 || dd > (int32_t)max_indel || dd < -(int32_t)max_indel) continue;
                        if (stream_kmer64(s_fwd, 2 * (PL_LEAD + p2), (int)s) != key2) continue;
                        bool later = false;
                        for (uint32_t j3 = j2; j3 < A.n_seeds && !later; ++j3) later = plg_seed_on(s_rows, rbit, nm, A.nmw, C, D2, w_base + j3 * s, s, n);
                        if (later) continue;
                        const uint32_t gi = dd < 0 ? (uint32_t)(-dd) : 0u;
                        if (ws2 < x_lo + gi) continue;
                        const uint32_t x_hi = ws2 - gi;
                        const uint32_t i1 = (int32_t)L < (int32_t)n - D2 ? L : (uint32_t)((int32_t)n - D2);
                        const uint32_t ov = i1 - i0 - gi;
                        if (ov < A.min_ov) continue;
                        uint32_t mm = pl_mismatches(s_rows, rbit, nm, C, D, i0, x_lo, 0xFFFFu) +
                                      pl_mismatches(s_rows, rbit, nm, C, D2, x_lo + gi, i1, 0xFFFFu);
                        uint32_t bmm = EMPTY32, bx = 0;
                        for (uint32_t xb = x_lo; xb <= x_hi; xb += 32) {
                            const uint32_t gain = plg_diff32(s_rows, rbit, nm, A.nmw, C, D, xb);
                            const uint32_t lose = plg_diff32(s_rows, rbit, nm, A.nmw, C, D2, xb + gi);
                            const uint32_t nb = x_hi - xb < 31u ? x_hi - xb + 1 : 32u;
                            for (uint32_t b = 0; b < nb; ++b) {
                                const uint32_t x = xb + b;
                                const bool ok = !(gi && nm && row_window_masked(nm, A.nmw, x, gi));
                                if (ok && (mm < bmm || (strand && mm == bmm))) {
                                    bmm = mm;
                                    bx = x;
                                }
                                mm += ((gain >> b) & 1u) - ((lose >> b) & 1u);
                            }
                        }
                        if (bmm == EMPTY32 || bmm + 2u > A.max_mm) continue;
                        const uint32_t k2 = ((bmm + 2u) << 12) | (4095u - ov);
                        if (k2 < best) {
                            best = k2;
                            out.cnt = 1;
                            out.strand = strand;
                            out.D = D;
                            out.D2 = D2;
                            out.x = bx;
                        } else if (k2 == best) {
                            ++out.cnt;
                        }
                    }
                }
            }
        }
    }
    return out;
}

// The event of a split placement in stored orientation as the table's 64-bit key — column p (14 bits) << 38 | INS << 37 | length
// (5 bits) << 32 | the inserted bases as a base-4 number — so that the definition's order (p, DEL before INS, length, bases) is the
// keys' numeric order; no key is 0.  *p_out, *gd_out: the column and the deleted columns (0 for an insertion)
__device__ __forceinline__ unsigned long long plg_event(const PlgPlacement& pm, const uint32_t* s_rows, uint32_t rbit, uint32_t n,
                                                        uint32_t* p_out, uint32_t* gd_out) {
    const bool ins = pm.D2 < pm.D;
    const uint32_t len = (uint32_t)(ins ? pm.D - pm.D2 : pm.D2 - pm.D);
    const uint32_t gi = ins ? len : 0u;
    const uint32_t p = pm.strand ? (uint32_t)((int32_t)n - pm.D2 - (int32_t)pm.x - (int32_t)gi) : (uint32_t)(pm.D + (int32_t)pm.x);
    uint32_t num = 0;
    if (ins) {
        const uint32_t v = stream32(s_rows, rbit + 2 * pm.x) >> (32 - 2 * len);
        num = pm.strand ? revpairs32(~v << (32 - 2 * len)) : v;       // strand 1: the reverse complement of the row's bases
    }
    *p_out = p;
    *gd_out = ins ? 0u : len;
    return ((unsigned long long)p << 38) | ((unsigned long long)ins << 37) | ((unsigned long long)len << 32) | num;
}

}  // namespace gf
