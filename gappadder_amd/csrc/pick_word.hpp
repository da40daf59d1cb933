// pick_word.hpp — the one codec of gap_best[g] on the device (the definition: the header of pick.hip; the host's codec: pipeline.decode_best /
// pick_index).  level << 56 | span + 1 (saturating) << 32 | (PICK_CONTIG_MAX - contig) << 1 | strand, 0 = no pick: an atomicMax over the
// words of a gap keeps the higher level, then the longer span, then the earlier contig.
#pragma once
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t PICK_SPAN_SAT = 0xFFFFFFu, PICK_CONTIG_MAX = 0x7FFFFFFFu;   // the span field has 24 bits, the contig field 31

struct PickWord { uint32_t level, span1, contig, reverse; };   // span1: the span field, span + 1 or PICK_SPAN_SAT

// span: bases between the two hits.  The only saturation: a span beyond the field still outranks every shorter one, it never wraps
GF_HD unsigned long long pick_word_pack(uint32_t level, uint64_t span, uint32_t contig, uint32_t reverse) {
    const uint64_t span1 = span + 1 < PICK_SPAN_SAT ? span + 1 : PICK_SPAN_SAT;
    return ((unsigned long long)level << 56) | (span1 << 32) | ((unsigned long long)(PICK_CONTIG_MAX - contig) << 1) | reverse;
}

GF_HD PickWord pick_word_unpack(unsigned long long word) {
    return {(uint32_t)(word >> 56), (uint32_t)(word >> 32) & PICK_SPAN_SAT, PICK_CONTIG_MAX - ((uint32_t)(word >> 1) & PICK_CONTIG_MAX), (uint32_t)word & 1u};
}

// does a located span (+ 1) agree with the word's field?  A saturated field stands for every span at least that long
GF_HD bool pick_word_span_matches(uint64_t span_plus_1, uint32_t field) {
    return field < PICK_SPAN_SAT ? span_plus_1 == field : span_plus_1 >= field;
}

// the gap's best word so far, and the count of closed gaps: the first word a gap receives closes it
__device__ __forceinline__ void pick_word_publish(unsigned long long* gap_best, uint32_t* n_closed, uint32_t gap, unsigned long long word) {
    if (atomicMax(gap_best + gap, word) == 0) atomicAdd(n_closed, 1u);
}

}  // namespace gf
