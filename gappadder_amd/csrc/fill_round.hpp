// fill_round.hpp — what the rounds that look at a closed fill after the last pick of the step share around fill_body.hpp (fill_support.hip,
// fill_polish.hip, fill_pairs.hip): the arguments of every such launch (FillRoundArgs), how a workgroup opens a gap
// (fill_gap_open, fill_gap_rows) and — host side — the one setup of a launch (fill_round_setup, api.hip).  A rule about closed fills — what
// a mismatch is, how the pool slice is clamped, a new anchor mode — is written here or in fill_body.hpp, once.
#pragma once
#include "fill_body.hpp"
#include "gf_internal.hpp"

namespace gf {

// the arguments of a launch that every round reads the same way
struct FillRoundArgs {
    FillBodyArgs body;           // the contig list (body.list: the only copy), the picks
    const uint64_t* pool_off;    // the gaps' row ranges in the pool the round reads ...
    uint64_t pool_rows;          // ... and the rows of that pool array
    const unsigned long long* gap_best;
    uint32_t n_gaps;
    uint32_t* stats;             // the round's own statistics words
};

enum : uint32_t { FILL_GAP_OPEN, FILL_GAP_MISMATCH, FILL_GAP_OK };

struct FillGap {
    uint32_t state;              // FILL_GAP_*; fb is set for FILL_GAP_OK only
    FillBody fb;
};

struct FillRows {
    uint64_t r0, r1;
};

// the rows [r0, r1) of gap g in the round's pool, clamped to the pool array.  Apart from fill_gap_open, so that a kernel asks where it
// first needs them: held across fill_polish_kernel's stage and index they cost it 16 more spilled SGPRs
__device__ __forceinline__ FillRows fill_gap_rows(const FillRoundArgs& R, uint32_t g) {
    FillRows out;
    out.r0 = R.pool_off[g];
    out.r1 = R.pool_off[g + 1];
    if (out.r1 > R.pool_rows) out.r1 = R.pool_rows;
    if (out.r0 > out.r1) out.r0 = out.r1;
    return out;
}

// Gap g of the launch, called by every thread of a workgroup of THREADS threads (n_list: contig_list_end(R.body.list); s_loc: two words of LDS);
// every thread gets the same answer.  FILL_GAP_OPEN and FILL_GAP_MISMATCH: the caller writes its zero record (thread 0, no barrier)
// and, for a mismatch, counts it in its MISMATCH word — in a branch per state: one merged branch spills more.  FILL_GAP_OK: returns behind a workgroup barrier, so the record thread 0
// wrote for the workgroup's previous gap — from LDS the caller is about to reset — is written.  fill_body's exact branch goes through
// workgroup barriers of its own: the word of a gap is the same in all threads, so it is reached by all of them or by none.
template <uint32_t THREADS>
__device__ __forceinline__ FillGap fill_gap_open(const FillRoundArgs& R, uint32_t n_list, uint32_t g, uint32_t* s_loc) {
    FillGap out;
    const unsigned long long word = R.gap_best[g];
    if (!word) {
        out.state = FILL_GAP_OPEN;
        return out;
    }
    out.fb = fill_body<THREADS>(R.body, n_list, g, word, s_loc);
    if (!out.fb.ok) {
        out.state = FILL_GAP_MISMATCH;
        return out;
    }
    out.state = FILL_GAP_OK;
    __syncthreads();                             // (the previous gap's record is written)
    return out;
}

// ---- host side: the arguments the three ABI entries share, as they receive them (d_stats: u32[stats_words], zeroed by the setup)
struct FillRoundIn {
    const void *d_pool_packed, *d_pool_off;
    size_t pool_rows;
    int read_len;
    const void *d_contigs, *d_n_contigs;
    size_t contig_cap;
    const void *d_seq, *d_gap_best, *d_ctg_pick_or_null;
    int anchor_long, anchor_short;
    const void* d_records;
    void* d_stats;
};

// The one setup of a round's launch (api.hip).  In this order, which is the entries' order of old: GF_E_INVAL for a bad shared argument
// or anchor length; own_rc when it is not GF_OK — the entry's verdict on its own parameters, GF_E_UNSUPPORTED; GF_E_STATE without
// flanks; then the device, the statistics words zeroed on the stream, the exact anchors' tables (without a gf_ctg_pick array) and *R.
// *blocks: the workgroups to launch with wgs_per_cu of them resident on a CU — 0 when the context has no gaps: nothing to launch.
int fill_round_setup(gf_ctx* ctx, const FillRoundIn& in, int own_rc, uint32_t stats_words, uint32_t wgs_per_cu, FillRoundArgs* R, size_t* blocks);

}  // namespace gf
