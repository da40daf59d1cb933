// fill_alt.hip — fill alternatives of the closed gaps.  The pick (pick.hip) keeps one contig per gap — level, then span, then
// the earlier contig — and every other contig that carries both anchors loses the atomicMax without a trace.  This round looks at them
// again: per closed gap how many there are, whether their fills are the winner's byte for byte, within max_dist edits of it or further
// away, and which one the pick would have taken had the winner not been there (the rival).  Definition and host twin:
// gappadder_amd/fill_alternatives.py::alts_host (equal byte for byte); the ABI: gf_fill_alts_dev, include/gapfill_hip.h.
//
// Three launches, no host synchronisation:
//   winners  one wave per closed gap: the contig the gap's word names, re-located by its index and scanned again (anchor_scan<true>); when
//            the scan gives the word's level, strand and span, the fill's start, length and strand go to the gap's scratch (AltScratch,
//            zeroed by the call); otherwise the scratch stays zero: the gap is lost
//   peers    one wave per contig, as pick_anchor_kernel loops: the contig's own word and from it its class; for a peer the common prefix
//            and suffix with the winner's fill (64 columns a trip, a ballot each), the banded distance of what lies between (alt_banded),
//            the per-contig record, and lane 0 updates the gap's counters, lengths and rival key with atomics
//   records  one wave per gap: the rival re-located from its key and scanned again, prefix and suffix once more, the record from lane 0
// The rival key is the pick word of a peer without its level (all peers have the winner's) and with the distance in its place:
// span field << 38 | (PICK_CONTIG_MAX - contig) << 7 | strand << 6 | min(dist, 63): the same order, and the records kernel reads the
// distance from it whether the caller passed a per-contig buffer or not.  What a candidate is and how its oriented fill is read:
// fill_alt_dev.hpp (alt_candidate, AltFill), shared with fill_adj.hip.
#include <cstring>

#include "anchor.hpp"
#include "contig_list.hpp"
#include "fill_alt_dev.hpp"
#include "gf_internal.hpp"
#include "pick_word.hpp"

namespace gf {

struct AltScratch {
    unsigned long long rival;        // the largest rival key of the gap, 0: none
    uint32_t start, len;             // the winner's fill on its contig as stored
    uint32_t state;                  // ALT_S_*
    uint32_t n_cand, n_lower, n_ident, n_near, n_far;
    uint32_t len_min_inv, len_max;   // ~(the smallest fill length) over the winner and its peers (so that zero means none), the largest
};
static_assert(sizeof(AltScratch) == 48, "AltScratch");
static_assert(sizeof(gf_fill_alt) == 48, "gf_fill_alt");
static_assert(sizeof(gf_fill_alt_contig) == 8, "gf_fill_alt_contig");

constexpr uint32_t ALT_S_FOUND = 1, ALT_S_REVERSE = 2, ALT_S_OUTRANKED = 4;
constexpr uint32_t ALT_KEY_FAR = 63;

struct AltParams {
    ContigList list;
    const unsigned long long* gap_best;
    const uint8_t *anc_s, *anc_l;      // anchor tables of the short (or only) and the long length (or null)
    uint32_t n_gaps, a_s, a_l, B;
    AltScratch* ws;
    gf_fill_alt* out;
    gf_fill_alt_contig* out_contig;    // or null
    uint32_t* stats;
};

GF_HD unsigned long long alt_key_pack(uint32_t span, uint32_t contig, uint32_t strand, uint32_t dist) {
    const unsigned long long span1 = (uint64_t)span + 1 < PICK_SPAN_SAT ? (uint64_t)span + 1 : PICK_SPAN_SAT;
    return (span1 << 38) | ((unsigned long long)(PICK_CONTIG_MAX - contig) << 7) | ((unsigned long long)strand << 6) | (dist < ALT_KEY_FAR ? dist : ALT_KEY_FAR);
}

// longest common prefix of W and P, at most `limit` <= min(W.len, P.len)
__device__ __forceinline__ uint32_t alt_lcp(const AltFill& W, const AltFill& Pf, uint32_t limit, uint32_t lane) {
    for (uint32_t base = 0; base < limit; base += 64) {
        const uint32_t x = base + lane;
        const unsigned long long b = __ballot(x < limit && W.at(x) != Pf.at(x));
        if (b) return base + (uint32_t)__ffsll((long long)b) - 1;
    }
    return limit;
}

// longest common suffix of W and P, at most `limit` <= min(W.len, P.len) - lcp
__device__ __forceinline__ uint32_t alt_lcs(const AltFill& W, const AltFill& Pf, uint32_t limit, uint32_t lane) {
    for (uint32_t base = 0; base < limit; base += 64) {
        const uint32_t x = base + lane;
        const unsigned long long b = __ballot(x < limit && W.at(W.len - 1 - x) != Pf.at(Pf.len - 1 - x));
        if (b) return base + (uint32_t)__ffsll((long long)b) - 1;
    }
    return limit;
}

// min(Levenshtein(W[off : off + m], P[off : off + n]), B + 1) for |m - n| <= B <= 31, by one wave: an anti-diagonal sweep over the band
// of the diagonals -B .. +B.  Lane l holds diagonal d = l - B (j - i, i into W, j into P); at step t = i + j the lanes with t - d even and
// (i, j) inside the matrix are live.  `cur` is the lane's last cell: (i-1, j-1) two steps ago; the cell above, (i-1, j), is what lane
// l + 1 wrote one step ago, the cell to the left, (i, j-1), what lane l - 1 wrote.  Values saturate at B + 1.  Every cell depends on cells
// of the two fronts before it with costs >= 0, so when no live cell of two consecutive fronts is <= B none ever is again: stop.
__device__ __forceinline__ uint32_t alt_banded(const AltFill& W, const AltFill& Pf, uint32_t off, uint32_t m, uint32_t n, uint32_t B, uint32_t lane) {
    const int d = (int)lane - (int)B;
    const uint32_t INF = B + 1, total = m + n;
    const bool in_band = lane <= 2 * B;
    uint32_t cur = INF;
    bool alive_before = true;
    for (uint32_t t = 0; t <= total; ++t) {
        const uint32_t up = __shfl_down(cur, 1);                       // (lane 2B reads a lane outside the band: INF, 2B + 1 <= 63)
        uint32_t left = __shfl_up(cur, 1);
        if (lane == 0) left = INF;
        const int ti = (int)t - d, i = ti >> 1, j = i + d;
        const bool live = in_band && ti >= 0 && !(ti & 1) && (uint32_t)i <= m && j >= 0 && (uint32_t)j <= n;
        if (live) {
            uint32_t v;
            if (i == 0) v = (uint32_t)j;
            else if (j == 0) v = (uint32_t)i;
            else {
                const uint32_t side = (up < left ? up : left) + 1, diag = cur + (W.at(off + (uint32_t)i - 1) != Pf.at(off + (uint32_t)j - 1));
                v = diag < side ? diag : side;
            }
            cur = v < INF ? v : INF;
        }
        const bool alive = __ballot(live && cur <= B) != 0;
        if (!alive && !alive_before) return INF;
        alive_before = alive;
    }
    return __shfl(cur, (int)(n + B - m));
}

__global__ __launch_bounds__(256) void alt_winners_kernel(AltParams P) {
    const uint32_t n = contig_list_end(P.list);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t g = wave; g < P.n_gaps; g += n_waves) {
        const unsigned long long word = P.gap_best[g];
        if (!word) continue;
        const PickWord w = pick_word_unpack(word);
        if (w.contig >= n) continue;
        const gf_contig c = P.list.contigs[w.contig];
        AltCand k;
        if (c.gap != g || !alt_candidate(P, c, lane, &k)) continue;
        if (k.level != w.level || k.strand != w.reverse || !pick_word_span_matches((uint64_t)k.span + 1, w.span1)) continue;
        if (lane != 0) continue;
        AltScratch* s = P.ws + g;
        s->start = k.start;
        s->len = k.span;
        s->state = ALT_S_FOUND | (k.strand ? ALT_S_REVERSE : 0);
        s->n_cand = 1;
        s->len_min_inv = ~k.span;
        s->len_max = k.span;
    }
}

__global__ __launch_bounds__(256) void alt_peers_kernel(AltParams P) {
    const uint32_t n = contig_list_end(P.list), first = contig_list_begin(P.list);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t n_cand = 0, n_lower = 0, n_ident = 0, n_near = 0, n_far = 0;      // of this wave (uniform over its lanes)
    for (uint32_t ci = wave; ci < n; ci += n_waves) {
        const gf_contig c = P.list.contigs[ci];
        gf_fill_alt_contig rec = {0, 0, GF_FA_C_NONE, 0};
        const unsigned long long word = c.gap < P.n_gaps ? P.gap_best[c.gap] : 0;
        AltScratch* ws = P.ws + c.gap;                                          // (read only behind `word`)
        const uint32_t state = word ? ws->state : 0;
        if (state & ALT_S_FOUND) {
            const PickWord w = pick_word_unpack(word);
            const AltFill W = {P.list.seq + P.list.contigs[w.contig].seq_off, ws->start, ws->len, w.reverse};
            AltCand k;
            if (ci == w.contig) rec = {W.len, GF_FA_DIST_FAR, GF_FA_C_WINNER, (uint8_t)w.reverse};
            else if (ci >= first && alt_candidate(P, c, lane, &k)) {
                ++n_cand;
                if (lane == 0) atomicAdd(&ws->n_cand, 1u);
                if (k.level < w.level) {
                    ++n_lower;
                    rec = {k.span, GF_FA_DIST_FAR, GF_FA_C_LOWER, (uint8_t)k.strand};
                    if (lane == 0) atomicAdd(&ws->n_lower, 1u);
                } else if (k.level > w.level) {
                    if (lane == 0) atomicOr(&ws->state, ALT_S_OUTRANKED);
                } else {
                    const AltFill Pf = {P.list.seq + c.seq_off, k.start, k.span, k.strand};
                    const uint32_t shorter = W.len < Pf.len ? W.len : Pf.len, gap_len = (W.len < Pf.len ? Pf.len : W.len) - shorter;
                    uint32_t cls = GF_FA_C_FAR, dist = GF_FA_DIST_FAR;
                    if (gap_len <= P.B) {                                       // (a length difference beyond B: FAR without a DP)
                        const uint32_t lcp = alt_lcp(W, Pf, shorter, lane);
                        if (lcp == W.len && lcp == Pf.len) cls = GF_FA_C_IDENTICAL;
                        else {
                            const uint32_t lcs = alt_lcs(W, Pf, shorter - lcp, lane);
                            const uint32_t e = alt_banded(W, Pf, lcp, W.len - lcp - lcs, Pf.len - lcp - lcs, P.B, lane);
                            if (e <= P.B) { cls = GF_FA_C_NEAR; dist = e; }
                        }
                    }
                    n_ident += cls == GF_FA_C_IDENTICAL;
                    n_near += cls == GF_FA_C_NEAR;
                    n_far += cls == GF_FA_C_FAR;
                    rec = {k.span, (uint16_t)dist, (uint8_t)cls, (uint8_t)k.strand};
                    if (lane == 0) {
                        if (pick_word_pack(k.level, k.span, ci, k.strand) > word) atomicOr(&ws->state, ALT_S_OUTRANKED);
                        atomicMax(&ws->len_min_inv, ~k.span);
                        atomicMax(&ws->len_max, k.span);
                        atomicAdd(cls == GF_FA_C_IDENTICAL ? &ws->n_ident : cls == GF_FA_C_NEAR ? &ws->n_near : &ws->n_far, 1u);
                        if (cls != GF_FA_C_IDENTICAL) atomicMax(&ws->rival, alt_key_pack(k.span, ci, k.strand, dist));
                    }
                }
            }
        }
        if (P.out_contig && lane == 0) P.out_contig[ci] = rec;
    }
    if (lane != 0) return;
    if (n_cand) atomicAdd(P.stats + GF_FA_CANDIDATES, n_cand);
    if (n_lower) atomicAdd(P.stats + GF_FA_LOWER, n_lower);
    if (n_ident) atomicAdd(P.stats + GF_FA_IDENTICAL, n_ident);
    if (n_near) atomicAdd(P.stats + GF_FA_NEAR, n_near);
    if (n_far) atomicAdd(P.stats + GF_FA_FAR, n_far);
}

__device__ __forceinline__ uint16_t alt_sat16(uint32_t v) { return (uint16_t)(v < 0xFFFFu ? v : 0xFFFFu); }

__global__ __launch_bounds__(256) void alt_records_kernel(AltParams P) {
    const uint32_t n = contig_list_end(P.list);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t n_closed = 0, n_found = 0, n_contested = 0, n_varies = 0, n_outranked = 0, n_lost = 0;
    for (uint32_t g = wave; g < P.n_gaps; g += n_waves) {
        gf_fill_alt r;
        memset(&r, 0, sizeof(r));
        const unsigned long long word = P.gap_best[g];
        if (word) {
            ++n_closed;
            const PickWord w = pick_word_unpack(word);
            const AltScratch s = P.ws[g];
            r.level = (uint8_t)w.level;
            if (!(s.state & ALT_S_FOUND)) {
                r.flags = GF_FA_F_LOST;
                ++n_lost;
            } else {
                ++n_found;
                uint32_t flags = (w.reverse ? GF_FA_F_REVERSE : 0) | (s.state & ALT_S_OUTRANKED ? GF_FA_F_OUTRANKED : 0);
                r.contig = w.contig;
                r.fill_len = s.len;
                r.len_min = ~s.len_min_inv;
                r.len_max = s.len_max;
                r.n_candidates = alt_sat16(s.n_cand);
                r.n_lower = alt_sat16(s.n_lower);
                r.n_identical = alt_sat16(s.n_ident);
                r.n_near = alt_sat16(s.n_near);
                r.n_far = alt_sat16(s.n_far);
                if (r.len_min != r.len_max) { flags |= GF_FA_F_LENGTH_VARIES; ++n_varies; }
                if (flags & GF_FA_F_OUTRANKED) ++n_outranked;
                const uint32_t ci = PICK_CONTIG_MAX - ((uint32_t)(s.rival >> 7) & PICK_CONTIG_MAX);
                AltCand k;
                // (the rival was a candidate of this list: the scan finds it again)
                if (s.rival && ci < n && alt_candidate(P, P.list.contigs[ci], lane, &k)) {
                    const AltFill W = {P.list.seq + P.list.contigs[w.contig].seq_off, s.start, s.len, w.reverse};
                    const AltFill Pf = {P.list.seq + P.list.contigs[ci].seq_off, k.start, k.span, k.strand};
                    const uint32_t shorter = W.len < Pf.len ? W.len : Pf.len, e = (uint32_t)s.rival & ALT_KEY_FAR;
                    r.rival = ci;
                    r.rival_len = k.span;
                    r.lcp = alt_lcp(W, Pf, shorter, lane);
                    r.lcs = alt_lcs(W, Pf, shorter - r.lcp, lane);
                    r.dist = (uint16_t)(e == ALT_KEY_FAR ? GF_FA_DIST_FAR : e);
                    flags |= GF_FA_F_HAS_RIVAL | (k.strand ? GF_FA_F_RIVAL_REVERSE : 0);
                    ++n_contested;
                }
                r.flags = (uint8_t)flags;
            }
        }
        if (lane == 0) P.out[g] = r;
    }
    if (lane != 0) return;
    if (n_closed) atomicAdd(P.stats + GF_FA_CLOSED, n_closed);
    if (n_found) atomicAdd(P.stats + GF_FA_CANDIDATES, n_found);           // (the winners: the peers kernel counted the others)
    if (n_contested) atomicAdd(P.stats + GF_FA_CONTESTED, n_contested);
    if (n_varies) atomicAdd(P.stats + GF_FA_LENGTH_VARIES, n_varies);
    if (n_outranked) atomicAdd(P.stats + GF_FA_OUTRANKED, n_outranked);
    if (n_lost) atomicAdd(P.stats + GF_FA_LOST, n_lost);
}

}  // namespace gf

using namespace gf;

extern "C" {

int gf_fill_alts_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int anchor_len,
                     int anchor_len_short, int max_dist, const void* d_first, const void* d_gap_best, void* d_alt, void* d_alt_contig,
                     void* d_stats) {
    const bool own_ok = d_gap_best && d_alt && d_stats && anchor_len >= 8 && anchor_len <= ANCHOR_MAX &&
                        (!anchor_len_short || (anchor_len_short >= 8 && anchor_len_short < anchor_len)) && max_dist >= 1 &&
                        max_dist <= GF_FA_MAX_DIST;
    AltParams P;
    memset(&P, 0, sizeof(P));
    int rc = contig_list_view(ctx, d_contigs, d_n_contigs, contig_cap, CONTIG_CAP_WORD, d_seq, d_first, own_ok ? GF_OK : GF_E_INVAL, &P.list);
    if (rc) return rc;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(d_stats, 0, 4 * GF_FA_WORDS, ctx->stream));
    const size_t ng = ctx->gaps.size();
    if (!ng) return GF_OK;
    const int a_s = anchor_len_short ? anchor_len_short : anchor_len;
    if (anchor_len_short && (rc = anchor_table(ctx, anchor_len, &P.anc_l))) return rc;
    if ((rc = anchor_table(ctx, a_s, &P.anc_s))) return rc;
    if ((rc = ensure(ctx, ctx->alt_ws, ng * sizeof(AltScratch) + 64))) return rc;
    P.gap_best = (const unsigned long long*)d_gap_best;
    P.n_gaps = (uint32_t)ng;
    P.a_s = (uint32_t)a_s;
    P.a_l = (uint32_t)anchor_len;
    P.B = (uint32_t)max_dist;
    P.ws = (AltScratch*)ctx->alt_ws.p;
    P.out = (gf_fill_alt*)d_alt;
    P.out_contig = (gf_fill_alt_contig*)d_alt_contig;
    P.stats = (uint32_t*)d_stats;
    GF_HIP(ctx, hipMemsetAsync(P.ws, 0, ng * sizeof(AltScratch), ctx->stream));
    LaunchTimer tm(ctx, GF_KERNEL_ALT);
    const unsigned gap_blocks = (unsigned)((ng + 3) / 4 < (size_t)ctx->n_cu * 4 ? (ng + 3) / 4 : (size_t)ctx->n_cu * 4);
    hipLaunchKernelGGL(alt_winners_kernel, dim3(gap_blocks), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(alt_peers_kernel, dim3(ctx->n_cu * 8), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(alt_records_kernel, dim3(gap_blocks), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // extern "C"
