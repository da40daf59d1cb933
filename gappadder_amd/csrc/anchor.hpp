// anchor.hpp — the exact anchors of the gaps' flanks as the device holds them, and the scan of one contig for them by one wave
// (DESIGN.md §19).  The table of one anchor length `a` (gf::anchor_table, pick.hip; built once per gf_set_gaps) has per gap ANCHOR_ROWS
// rows of ANCHOR_MAX bytes: the last `a` bases of the left flank, the first `a` of the right flank, the reverse complements of the two —
// each from byte 0 of its row, byte 0 == 0: the gap has no anchors of this length — and a flags row.  Read by pick.hip (the pick),
// pick_ext.hip (the extended fill) and fill_body.hpp (the re-location of a pick).
#pragma once
#include "gf_internal.hpp"

namespace gf {

enum : int { ANC_LEFT, ANC_RIGHT, ANC_RC_LEFT, ANC_RC_RIGHT, ANC_FLAGS, ANCHOR_ROWS };
constexpr int ANCHOR_MAX = 32, ANCHOR_ROW = ANCHOR_ROWS * ANCHOR_MAX;

// byte 0 of the flags row: the flank is exactly `a` bases long, so its hits are unclipped on both strands
constexpr uint32_t ANC_F_LEFT_WHOLE = 1, ANC_F_RIGHT_WHOLE = 2;

// the rows of gap `gap` in a table, and row `r` of them
template <typename B> GF_HD B* anchor_rows(B* table, uint64_t gap) { return table + gap * ANCHOR_ROW; }
template <typename B> GF_HD B* anchor_row(B* rows, int r) { return rows + r * ANCHOR_MAX; }

// does the gap have anchors of the table's length? (one test for both sides would do: the builder fills all four rows or none)
GF_HD bool anchor_rows_set(const uint8_t* rows) { return anchor_row(rows, ANC_LEFT)[0] != 0 && anchor_row(rows, ANC_RIGHT)[0] != 0; }
GF_HD uint32_t anchor_flags(const uint8_t* rows) { return anchor_row(rows, ANC_FLAGS)[0]; }

// One wave, ONE pass over the contig s[0 .. length) (length >= a >= 8) for the four patterns in `as`, a gap's rows of length a: a lane loads
// four bases at its position as one dword and compares them with the heads of the four patterns held in registers (1.5 % of the positions
// go on to the byte loop).  Pattern q (ANC_LEFT .. ANC_RC_RIGHT) is looked for when want[q & 1], its side, is set.  After the wave
// reduction every lane holds, per pattern q, any[q], and the leftmost / rightmost position mn[q] / mx[q].
// LONG: a second anchor length al > a at once — the short anchors are the inner ends of the long ones, so a long hit is a short hit that
// extends: with `alp` (the gap's rows of length al, or null for none) a short hit whose other al - a bases match as well is reported in
// [4 + q], at the position of the long pattern.  The arrays have 8 entries then, 4 otherwise.
template <bool LONG>
__device__ __forceinline__ void anchor_scan(const char* s, uint32_t length, const uint8_t* as, const uint8_t* alp, uint32_t a,
                                            uint32_t al, const bool* want, uint32_t lane, uint32_t* mn, uint32_t* mx, bool* any) {
    constexpr int NQ = LONG ? 8 : 4;
    const uint32_t ext = LONG && alp ? al - a : 0;
    uint32_t head[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint8_t* pat = anchor_row(as, q);
        head[q] = (uint32_t)pat[0] | ((uint32_t)pat[1] << 8) | ((uint32_t)pat[2] << 16) | ((uint32_t)pat[3] << 24);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) { mn[q] = EMPTY32; mx[q] = 0; any[q] = false; }
    const uint32_t last = length - a;
    for (uint32_t p = lane; p <= last; p += 64) {
        uint32_t w = 0;                                       // four bases at p (a >= 8: they exist)
#pragma unroll
        for (int b = 0; b < 4; ++b) w |= (uint32_t)(uint8_t)s[p + b] << (8 * b);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!want[q & 1] || w != head[q]) continue;
            const uint8_t* pat = anchor_row(as, q);
            uint32_t i = 4;
            while (i < a && (uint8_t)s[p + i] == pat[i]) ++i;
            if (i != a) continue;
            any[q] = true;
            mn[q] = p < mn[q] ? p : mn[q];
            mx[q] = p > mx[q] ? p : mx[q];
            if constexpr (LONG) {
                if (!alp) continue;
                // the long pattern around this short hit: the short one is its END for the left anchor and for revcomp(right), its
                // START for the right anchor and for revcomp(left)
                const uint8_t* lp = anchor_row(alp, q);
                const bool at_end = q == ANC_LEFT || q == ANC_RC_RIGHT;
                if (at_end ? p < ext : p + al > length) continue;
                const uint32_t p0 = at_end ? p - ext : p;
                bool ok = true;
                for (uint32_t j = 0; j < ext && ok; ++j) {
                    const uint32_t o = at_end ? j : a + j;
                    ok = (uint8_t)s[p0 + o] == lp[o];
                }
                if (!ok) continue;
                any[4 + q] = true;
                mn[4 + q] = p0 < mn[4 + q] ? p0 : mn[4 + q];
                mx[4 + q] = p0 > mx[4 + q] ? p0 : mx[4 + q];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {   // wave reductions
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t m2 = __shfl_xor(mn[q], d), x2 = __shfl_xor(mx[q], d);
            mn[q] = m2 < mn[q] ? m2 : mn[q];
            mx[q] = x2 > mx[q] ? x2 : mx[q];
        }
        any[q] = __ballot(any[q]) != 0;
    }
}

// The pick's pair of one level on one contig, from the scan's positions of that level (any / mn / mx of its four patterns), the level's
// flags `fl` and its anchor length a: span + 1, or 0 for no pair, and the strand of the hits (pick.hip, fill_alt.hip).
__device__ __forceinline__ uint32_t pick_span(const bool* any, const uint32_t* mn, const uint32_t* mx, uint32_t fl, uint32_t a, uint32_t* orient) {
    // forward: leftmost left anchor, rightmost right anchor;  reverse: leftmost revcomp(right), rightmost revcomp(left) (the oriented
    // contig is the reverse complement).  An unclipped flank's reverse hit is hidden by its forward hit.
    const bool lf = any[ANC_LEFT], rf = any[ANC_RIGHT], lr = any[ANC_RC_LEFT] && !((fl & ANC_F_LEFT_WHOLE) && lf),
               rr = any[ANC_RC_RIGHT] && !((fl & ANC_F_RIGHT_WHOLE) && rf);
    *orient = 0;
    if (lf && rf) return mx[ANC_RIGHT] >= mn[ANC_LEFT] + a ? mx[ANC_RIGHT] - (mn[ANC_LEFT] + a) + 1 : 0;
    if (lr && rr) { *orient = 1; return mx[ANC_RC_LEFT] >= mn[ANC_RC_RIGHT] + a ? mx[ANC_RC_LEFT] - (mn[ANC_RC_RIGHT] + a) + 1 : 0; }
    return 0;
}

}  // namespace gf
