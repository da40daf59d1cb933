// contig_list.hpp — the step's contig list as every consumer reads it.  The device counter can stand BEYOND the capacity of
// the record array (an overflowed producer keeps counting so that the step can raise; the records beyond were never written), so the valid
// records are [contig_list_begin, contig_list_end): the rule tests/test_gpu_contig_caps.py defends, written here once.
#pragma once
#include "gf_internal.hpp"

namespace gf {

struct ContigList {
    const gf_contig* contigs;
    const uint32_t* n_contigs;   // device counter
    uint32_t contig_cap;
    const char* seq;
    const uint32_t* first;       // or null: only the contigs from *first on (those a round appended)
};

// (the counter and the capacity alone: merge.hip's MgParams holds them as mutable pointers of its own)
__device__ __forceinline__ uint32_t contig_list_end(const uint32_t* n_contigs, uint32_t contig_cap) { return *n_contigs < contig_cap ? *n_contigs : contig_cap; }
__device__ __forceinline__ uint32_t contig_list_end(const ContigList& L) { return contig_list_end(L.n_contigs, L.contig_cap); }
__device__ __forceinline__ uint32_t contig_list_begin(const ContigList& L) { return L.first ? *L.first : 0u; }

// The largest capacity an entry accepts.  The two differ, as they always have: gf_pick_anchored*_dev take any 32-bit capacity, every
// other entry stops at the 31-bit contig field of the pick word (pick.hip).  Both are kept as they are.
constexpr size_t CONTIG_CAP_ANCHORED = 0xFFFFFFFFull, CONTIG_CAP_WORD = 0x7FFFFFFFull;

// Host side, the head of every entry over the list, in the order every such entry answers: GF_E_INVAL for a missing list argument or a
// capacity beyond cap_max; own_rc when it is not GF_OK — the entry's verdict on its own arguments, reached without touching ctx;
// GF_E_STATE when the context's flanks do not match its gaps; else *L.  What follows — hipSetDevice, zeroed statistics, GF_OK for an
// empty gap list — stays the entry's: the picks return before they touch the device, the others zero their statistics first.
inline int contig_list_view(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, size_t cap_max, const void* d_seq,
                            const void* d_first_or_null, int own_rc, ContigList* L) {
    if (!ctx || !d_contigs || !d_n_contigs || !d_seq || contig_cap > cap_max) return GF_E_INVAL;
    if (own_rc) return own_rc;
    if (ctx->flank_left.size() != ctx->gaps.size() || ctx->flank_right.size() != ctx->gaps.size()) return GF_E_STATE;
    *L = {(const gf_contig*)d_contigs, (const uint32_t*)d_n_contigs, (uint32_t)contig_cap, (const char*)d_seq, (const uint32_t*)d_first_or_null};
    return GF_OK;
}

}  // namespace gf
