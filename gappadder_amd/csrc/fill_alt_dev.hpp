// fill_alt_dev.hpp — where the fill of a CANDIDATE lies on its contig and how it is read, oriented (candidate, fill), one
// device copy for the rounds that look at a gap's other contigs: fill_alt.hip (the alternatives) and fill_adj.hip (the adjudication).
// The launch parameters are a template argument: a struct with the contig list (`list`), the anchor tables of the short (or only) and
// the long length (`anc_s`, `anc_l` or null), their lengths (`a_s`, `a_l`) and `n_gaps`.
#pragma once
#include "anchor.hpp"
#include "contig_list.hpp"
#include "gf_internal.hpp"
#include "pick_word.hpp"

namespace gf {

// a candidate: the contig's own word as pick_anchor_kernel forms it (level, span, strand) and where its fill starts on the contig as stored
struct AltCand { uint32_t level, span, strand, start; };

// the whole wave scans contig c; false: pick_anchor_kernel publishes no word for it.  Every lane returns the same.
template <class Params>
__device__ __forceinline__ bool alt_candidate(const Params& P, const gf_contig& c, uint32_t lane, AltCand* o) {
    const uint32_t a = P.a_s, al = P.a_l;
    if (c.gap >= P.n_gaps || c.length < 2 * a) return false;
    const uint8_t* as = anchor_rows(P.anc_s, c.gap);
    if (!anchor_rows_set(as)) return false;
    const uint8_t* alp = P.anc_l ? anchor_rows(P.anc_l, c.gap) : nullptr;
    const bool has_long = alp && anchor_rows_set(alp) && c.length >= 2 * al;
    const bool want[2] = {true, true};
    uint32_t mn[8], mx[8];
    bool any[8];
    anchor_scan<true>(P.list.seq + c.seq_off, c.length, as, has_long ? alp : nullptr, a, al, want, lane, mn, mx, any);
    uint32_t orient = 0, best = 0;
    if (has_long) best = pick_span(any + 4, mn + 4, mx + 4, anchor_flags(alp), al, &orient);
    if (best) {
        *o = {al, best - 1, orient, (orient ? mn[4 + ANC_RC_RIGHT] : mn[4 + ANC_LEFT]) + al};
        return true;
    }
    best = pick_span(any, mn, mx, anchor_flags(as), a, &orient);
    if (!best) return false;
    *o = {a, best - 1, orient, (orient ? mn[ANC_RC_RIGHT] : mn[ANC_LEFT]) + a};
    return true;
}

// an oriented fill: byte x of it, read forward or complemented from the far end
struct AltFill {
    const char* s;                   // the contig
    uint32_t start, len, strand;
    __device__ __forceinline__ uint8_t at(uint32_t x) const { return (uint8_t)(strand ? base_comp(s[start + len - 1 - x]) : s[start + x]); }
};

}  // namespace gf
