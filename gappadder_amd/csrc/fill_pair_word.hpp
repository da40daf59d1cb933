// fill_pair_word.hpp — the placement word fill_pairs.hip leaves per pool row in the caller's scratch array, and the order of a gap's id
// slice: what fill_anchor.hip reads behind it.
#pragma once
#include "fill_place.hpp"

namespace gf {

// status (PS_PLACED / PS_AMBIGUOUS / 0: unplaced), strand, and the diagonal on the contig as stored + PS_BIAS in the low 16 bits
constexpr uint32_t PS_BIAS = 1024, PS_STRAND = 1u << 16, PS_PLACED = 1u << 17, PS_AMBIGUOUS = 2u << 17;
static_assert(PL_MAX + 2 * PS_BIAS < PS_STRAND, "pair-span geometry");

// the order of a gap's id slice: mate side, then pair
__device__ __forceinline__ uint32_t ps_order(uint32_t id) { return ((id & 1u) << 31) | (id >> 1); }

}  // namespace gf
