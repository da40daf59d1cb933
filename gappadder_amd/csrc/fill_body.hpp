// fill_body.hpp — where the fill of a closed gap lies on its winning contig: the body [b0, b1) between the two flank hits of the pick
// word (gappadder_amd/read_support.py: locate).  One rule for the rounds that look at a fill after the last pick of the
// step — fill_support.hip, fill_polish.hip and fill_pairs.hip —, which reach it through fill_round.hpp's gap prologue (the latter two
// also use fill_place.hpp, which uses the window-mask helper below).  With a gf_ctg_pick per contig (the align and gapped modes) the body lies between the two
// alignments; without it the exact anchors (anchor.hpp) are re-located by pick.hip's rule at the anchor length the word carries, and a
// span that does not match the word's span field (pick_word.hpp) is a mismatch.
#pragma once
#include "anchor.hpp"
#include "contig_list.hpp"
#include "gf_internal.hpp"
#include "pick_word.hpp"

namespace gf {

// the assembly's window rule (assemble.hip window_masked): does the window [p, p + len) touch a masked base of the row?
__device__ __forceinline__ bool row_window_masked(const uint32_t* row, uint32_t nmw, uint32_t p, uint32_t len) {
    const uint32_t w = p >> 5, sh = p & 31;
    const uint64_t lo = (uint64_t)row[w] | ((uint64_t)(w + 1 < nmw ? row[w + 1] : 0u) << 32);
    const uint64_t hi = w + 2 < nmw ? row[w + 2] : 0u;
    const uint64_t a = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return (len >= 64 ? a : a & ((1ull << len) - 1)) != 0;
}

struct FillBodyArgs {
    ContigList list;             // (first: null)
    const gf_ctg_pick* ctg_pick; // or null: exact anchors
    const uint8_t* anc_l;        // exact: table of anchor length a_l, and of a_s (or null)
    const uint8_t* anc_s;
    uint32_t a_l, a_s;
};

struct FillBody {
    bool ok;                     // false: the contig does not carry the pick the word states
    uint32_t rev;                // the word's strand bit
    gf_contig c;                 // the winning contig (length 0 when the word names none)
    int64_t b0, b1;
};

// Called by every thread of a workgroup of THREADS threads with the same arguments (n: the contigs of the list); every thread gets the
// same answer.  s_loc: two words of LDS; the exact branch goes through workgroup barriers.
template <uint32_t THREADS>
__device__ __forceinline__ FillBody fill_body(const FillBodyArgs& A, uint32_t n, uint32_t g, unsigned long long word, uint32_t* s_loc) {
    const uint32_t t = threadIdx.x;
    const PickWord w = pick_word_unpack(word);
    const uint32_t ci = w.contig, rev = w.reverse, a = w.level;
    bool ok = ci < n;
    gf_contig c;
    c.length = 0;
    c.seq_off = 0;
    if (ok) {
        c = A.list.contigs[ci];
        ok = c.gap == g && c.length > 0;
    }
    const char* s = A.list.seq + c.seq_off;
    int64_t b0 = 0, b1 = 0;
    if (ok && A.ctg_pick) {
        const gf_ctg_pick p = A.ctg_pick[ci];
        ok = p.threshold != 0 && p.lp >= 1 && p.rp >= 1;
        b0 = rev ? (int64_t)p.rp - 1 + p.rm : (int64_t)p.lp - 1 + p.lm;
        b1 = rev ? (int64_t)p.lp - 1 : (int64_t)p.rp - 1;
        if (b1 < b0) b1 = b0;
        ok = ok && b1 <= (int64_t)c.length;
    } else if (ok) {
        const uint8_t* tab = a == A.a_l ? A.anc_l : (A.anc_s && a == A.a_s) ? A.anc_s : nullptr;
        const uint8_t* row = tab ? anchor_rows(tab, g) : nullptr;
        ok = row && anchor_rows_set(row) && c.length >= a;
        __syncthreads();                     // (the previous gap's readers of s_loc)
        if (t == 0) { s_loc[0] = EMPTY32; s_loc[1] = 0; }
        __syncthreads();
        if (ok) {
            // forward: leftmost left anchor, rightmost right anchor; reverse word: leftmost rc(right), rightmost rc(left)
            const uint8_t* pa = anchor_row(row, rev ? ANC_RC_RIGHT : ANC_LEFT);
            const uint8_t* pb = anchor_row(row, rev ? ANC_RC_LEFT : ANC_RIGHT);
            for (uint32_t p = t; p + a <= c.length; p += THREADS) {
                uint32_t i = 0;
                while (i < a && (uint8_t)s[p + i] == pa[i]) ++i;
                if (i == a) atomicMin(&s_loc[0], p);
                i = 0;
                while (i < a && (uint8_t)s[p + i] == pb[i]) ++i;
                if (i == a) atomicMax(&s_loc[1], p + 1);
            }
        }
        __syncthreads();
        const uint32_t first = s_loc[0], last1 = s_loc[1];
        ok = ok && first != EMPTY32 && last1 != 0 && last1 - 1 >= first + a;
        if (ok) {
            b0 = (int64_t)first + a;
            b1 = (int64_t)last1 - 1;
            ok = pick_word_span_matches((uint64_t)(b1 - b0) + 1, w.span1);
        }
    }
    return {ok, rev, c, b0, b1};
}

}  // namespace gf
