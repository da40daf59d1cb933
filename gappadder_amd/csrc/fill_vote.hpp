// fill_vote.hpp — the votes of one placed pool row on a window of contig columns (gappadder_amd/polish.py, pileup.py: votes; DESIGN.md
// §16, §23).  fill_pileup.hip takes them per read strand over the whole contig (fill_vote_row<true>).  fill_vote_row<false> restates
// fill_polish.hip's unstranded vote loop for the follow-up that moves the polish here; until then nothing instantiates it and no test
// runs it.
#pragma once
#include "gf_internal.hpp"

namespace gf {

// The placed row (strand, D: PlPlacement's, D on the array of its strand; rowb: its packed bytes, LDS or global; nm: its N-mask words or
// null) on the contig of n bases adds each of its unmasked bases that falls on a column of [c_lo, c_hi) to that column's counters in
// `votes` (LDS atomics).  A column has 4 counters, indexed by the base as it reads on the stored contig — or, STRANDED, 8: those 4 for
// rows on strand 0, then 4 for rows on strand 1.
//   strand 0: read base i on column D + i; strand 1: its complement on column n - 1 - D - i
template <bool STRANDED>
__device__ __forceinline__ void fill_vote_row(uint32_t* votes, uint32_t c_lo, uint32_t c_hi, uint32_t n, uint32_t L, uint32_t strand, int32_t D,
                                              const uint8_t* rowb, const uint32_t* nm) {
    constexpr uint32_t PER_COL = STRANDED ? 8 : 4;
    const int32_t i0 = D < 0 ? -D : 0, i1 = (int32_t)L < (int32_t)n - D ? (int32_t)L : (int32_t)n - D;
    int32_t lo = strand ? (int32_t)n - D - (int32_t)c_hi : (int32_t)c_lo - D;
    int32_t hi = strand ? (int32_t)n - D - (int32_t)c_lo : (int32_t)c_hi - D;
    lo = lo > i0 ? lo : i0;
    hi = hi < i1 ? hi : i1;
    for (int32_t i = lo; i < hi; ++i) {
        if (nm && ((nm[i >> 5] >> (i & 31)) & 1u)) continue;
        const uint32_t code = (rowb[i >> 2] >> (6 - 2 * (i & 3))) & 3u;
        const uint32_t col = strand ? n - 1 - (uint32_t)(D + i) : (uint32_t)(D + i);
        atomicAdd(&votes[(col - c_lo) * PER_COL + (STRANDED && strand ? 4u : 0u) + (strand ? 3u - code : code)], 1u);
    }
}

}  // namespace gf
