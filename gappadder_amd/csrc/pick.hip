// pick.hip — flank anchoring on the device: which gaps have a contig that both flanks anchor on the same
// strand, and how long the sequence between the anchors is.  This is the test `ContigsSelection` applies after every assembly
// round (pick_contigs.py:64-358: `bwa mem -T {score} -a` of the two flanks against the gap's contigs; per contig the best
// same-strand pair of a left and a right hit :149-297, over the contigs the longest span :300-321) with bwa replaced by EXACT
// anchors: the last `anchor_len` bases of the left flank and the first `anchor_len` bases of the right flank (anchor_len = the
// reference's bwa_min_score, 30 then 15: assemble_gaps.py:336, 365).  It makes "gaps closed" a quantity of the step instead of a
// host loop over all contigs.  Definition and oracle: oracle/gp_oracle.py::pick_gap (the reference's selection, pinned on its own
// answers, applied to the stand-in's hits); host twin: gappadder_amd/pick_contigs.py.
//
// Per contig: forward hits = leftmost occurrence of the left anchor, rightmost occurrence of the right anchor; reverse hits = the
// same in the reverse-complemented contig, searched as the reverse-complemented anchors in the forward contig.  The reference
// keeps one hit per (side, clip type), the first one on equal match lengths: a flank LONGER than the anchor is clipped in front
// on one strand and behind on the other, so both strands' hits survive; a flank exactly as long as the anchor gives unclipped
// hits on both strands and only the forward one (the first reported) survives.  Of the surviving pairs the forward pair is tried
// first and a later pair must match MORE bases to replace it (:173-291) — so: the forward pair when it exists, else the reverse
// pair; span = bases between the anchors, >= 0 or the contig does not count (:313-321).  Per gap: the longest span, the
// earlier contig on ties; a pick at a longer anchor outranks any pick at a shorter one (the pipeline only picks at 15 what
// 30 left open, assemble_gaps.py:336-366).  gap_best[g] = anchor_len << 56 | (span + 1) << 32 | (0x7FFFFFFF - contig) << 1 |
// reverse; 0 = no contig anchored = gap not closed (a span beyond the 24-bit field saturates; the codec on the device: pick_word.hpp).
#include <cstring>

#include "anchor.hpp"
#include "contig_list.hpp"
#include "gf_internal.hpp"
#include "pick_word.hpp"

namespace gf {

// One wave per contig, ONE pass over it for up to two anchor lengths (a_l > a_s): anchor_scan<true>, anchor.hpp.  (Before: one launch per
// anchor length, four pattern-byte loads per position.)
struct PickParams {
    ContigList list;
    const uint8_t* anc_s;      // table of the short (or only) anchor length
    const uint8_t* anc_l;      // table of the long anchor length, or null
    uint32_t n_gaps, a_s, a_l;
    unsigned long long* gap_best;
    uint32_t* n_closed;
};

// (pick_span, the span of one level from the scan's positions: anchor.hpp, shared with fill_alt.hip)
__global__ __launch_bounds__(256) void pick_anchor_kernel(PickParams P) {
    const uint32_t n = contig_list_end(P.list);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t a = P.a_s, al = P.a_l;
    const bool want[2] = {true, true};
    for (uint32_t ci = contig_list_begin(P.list) + wave; ci < n; ci += n_waves) {
        const gf_contig c = P.list.contigs[ci];
        if (c.gap >= P.n_gaps || c.length < 2 * a) continue;
        const uint8_t* as = anchor_rows(P.anc_s, c.gap);
        if (!anchor_rows_set(as)) continue;                       // (no short anchors: no long ones either)
        const uint8_t* alp = P.anc_l ? anchor_rows(P.anc_l, c.gap) : nullptr;
        const bool has_long = alp && anchor_rows_set(alp) && c.length >= 2 * al;
        // positions where each pattern occurs: min and max per pattern, short [0..3] and long [4..7]
        uint32_t mn[8], mx[8];
        bool any[8];
        anchor_scan<true>(P.list.seq + c.seq_off, c.length, as, has_long ? alp : nullptr, a, al, want, lane, mn, mx, any);
        if (lane != 0) continue;
        uint32_t orient = 0, best = 0, alen = al;                 // best: span + 1
        if (has_long) best = pick_span(any + 4, mn + 4, mx + 4, anchor_flags(alp), al, &orient);
        if (!best) { best = pick_span(any, mn, mx, anchor_flags(as), a, &orient); alen = a; }
        if (!best) continue;
        pick_word_publish(P.gap_best, P.n_closed, c.gap, pick_word_pack(alen, best - 1, ci, orient));
    }
}

// the table of one anchor length (anchor.hpp), built once per length (gf_set_gaps drops the tables)
int anchor_table(gf_ctx* ctx, int anchor_len, const uint8_t** out) {
    const size_t ng = ctx->gaps.size();
    DevBuf& tab = ctx->anchor_tabs[anchor_len];
    if (!tab.p) {
        std::vector<uint8_t> h(ng * ANCHOR_ROW, 0);
        for (size_t g = 0; g < ng; ++g) {
            const std::string &l = ctx->flank_left[g], &r = ctx->flank_right[g];
            if ((int)l.size() < anchor_len || (int)r.size() < anchor_len) continue;
            const char* la = l.data() + l.size() - anchor_len;
            const char* ra = r.data();
            bool ok = true;
            for (int i = 0; i < anchor_len; ++i) ok = ok && base_code4(la[i]) < 4 && base_code4(ra[i]) < 4;
            if (!ok) continue;
            uint8_t* o = anchor_rows(h.data(), g);
            anchor_row(o, ANC_FLAGS)[0] =
                (uint8_t)(((int)l.size() == anchor_len ? ANC_F_LEFT_WHOLE : 0) | ((int)r.size() == anchor_len ? ANC_F_RIGHT_WHOLE : 0));
            for (int i = 0; i < anchor_len; ++i) {
                anchor_row(o, ANC_LEFT)[i] = (uint8_t)la[i];
                anchor_row(o, ANC_RIGHT)[i] = (uint8_t)ra[i];
                anchor_row(o, ANC_RC_LEFT)[i] = (uint8_t)base_comp(la[anchor_len - 1 - i]);
                anchor_row(o, ANC_RC_RIGHT)[i] = (uint8_t)base_comp(ra[anchor_len - 1 - i]);
            }
        }
        int rc = ensure(ctx, tab, h.size() + 64);
        if (rc) return rc;
        GF_HIP(ctx, hipMemcpy(tab.p, h.data(), h.size(), hipMemcpyHostToDevice));
    }
    *out = (const uint8_t*)tab.p;
    return GF_OK;
}

}  // namespace gf

using namespace gf;

extern "C" {

static int pick_anchored2(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                          int anchor_len, int anchor_len_short, const void* d_first, void* d_gap_best, void* d_n_closed) {
    const bool own_ok = d_gap_best && d_n_closed && anchor_len >= 8 && anchor_len <= ANCHOR_MAX &&
                        (!anchor_len_short || (anchor_len_short >= 8 && anchor_len_short < anchor_len));
    PickParams P;
    int rc = contig_list_view(ctx, d_contigs, d_n_contigs, contig_cap, CONTIG_CAP_ANCHORED, d_seq, d_first, own_ok ? GF_OK : GF_E_INVAL, &P.list);
    if (rc) return rc;
    const size_t ng = ctx->gaps.size();
    if (!ng) return GF_OK;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    const int a_s = anchor_len_short ? anchor_len_short : anchor_len;
    P.anc_l = nullptr;
    if (anchor_len_short && (rc = anchor_table(ctx, anchor_len, &P.anc_l))) return rc;
    if ((rc = anchor_table(ctx, a_s, &P.anc_s))) return rc;
    P.a_s = (uint32_t)a_s;
    P.a_l = (uint32_t)anchor_len;
    P.n_gaps = (uint32_t)ng;
    P.gap_best = (unsigned long long*)d_gap_best;
    P.n_closed = (uint32_t*)d_n_closed;
    LaunchTimer tm(ctx, GF_KERNEL_PICK);
    hipLaunchKernelGGL(pick_anchor_kernel, dim3(ctx->n_cu * 8), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_pick_anchored2_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                          int anchor_len, int anchor_len_short, void* d_gap_best, void* d_n_closed) {
    return pick_anchored2(ctx, d_contigs, d_n_contigs, contig_cap, d_seq, anchor_len, anchor_len_short, nullptr, d_gap_best, d_n_closed);
}

int gf_pick_anchored2_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                               int anchor_len, int anchor_len_short, const void* d_first, void* d_gap_best, void* d_n_closed) {
    if (!d_first) return GF_E_INVAL;
    return pick_anchored2(ctx, d_contigs, d_n_contigs, contig_cap, d_seq, anchor_len, anchor_len_short, d_first, d_gap_best, d_n_closed);
}

int gf_pick_anchored_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                         int anchor_len, void* d_gap_best, void* d_n_closed) {
    return gf_pick_anchored2_dev(ctx, d_contigs, d_n_contigs, contig_cap, d_seq, anchor_len, 0, d_gap_best, d_n_closed);
}

}  // extern "C"
