// pick_join.hip — flank-overlap joins: the gaps whose flanks OVERLAP.  A scaffolder puts an N-run between two contig ends
// that share o bases; nothing is missing there, and the assembly builds a contig that runs straight through the junction — but on it the
// right anchor starts before the left anchor ends, pick_span (pick.hip) returns 0 and the gap stays open in every round.  This round looks
// at every gap the last pick leaves open and, per contig and strand, at exactly that case: both anchors present, out of order by
// o = i + a - j >= 1 bases.  Definition and host twin: gappadder_amd/flank_joins.py::joins_host (equal byte for byte); the ABI:
// gf_pick_joins_dev, include/gapfill_hip.h.
//
// Two launches, no host synchronisation:
//   candidates  one wave per contig of an open gap, as pick_anchor_kernel: anchor_scan<true> once, then per strand the candidate from
//               mn / mx (the reverse strand from the rc rows: i = n - a - mx[rc left], j = n - a - mn[rc right]), the rejections in the
//               definition's order, the two comparisons over o + C columns strided over the lanes, and lane 0 publishes the join word
//               (atomicMax) and the gap's counters in the round's scratch (JoinScratch per gap, zeroed by the call)
//   records     one wave per gap: the winner re-located by the same scan, its record and the statistics
// The flank text comes from a table built once per gf_set_gaps and (X + C): per gap the two flank lengths, the LAST W bytes of the left
// flank right-aligned in W bytes and the FIRST W bytes of the right flank, W = X + C rounded up to 4.
#include <cstring>

#include "anchor.hpp"
#include "contig_list.hpp"
#include "gf_internal.hpp"
#include "pick_word.hpp"

namespace gf {

struct JoinScratch {
    unsigned long long word;     // the best join word of the gap, 0: none
    uint32_t n_cand, n_acc;
    uint32_t o_min_inv, o_max;   // 0xFFFF - the smallest accepted o (so that zero means none), the largest
};
static_assert(sizeof(JoinScratch) == 24, "JoinScratch");
static_assert(sizeof(gf_flank_join) == 32, "gf_flank_join");

struct JoinParams {
    ContigList list;
    const unsigned long long* gap_best;
    const uint8_t *anc_s, *anc_l;      // anchor tables of the short (or only) and the long length (or null)
    const uint8_t* flanks;             // the flank table, `stride` bytes per gap
    uint32_t n_gaps, a_s, a_l, W, stride;
    uint32_t X, C, M;
    JoinScratch* ws;
    gf_flank_join* out;
    uint32_t* stats;
};

constexpr int JOIN_TAB_KEY = -(1 << 16);     // ctx->anchor_tabs[JOIN_TAB_KEY - W]: the flank table of width W (dropped by gf_set_gaps)

GF_HD unsigned long long join_word_pack(uint32_t level, uint32_t msum, uint32_t o, uint32_t contig, uint32_t strand) {
    return ((unsigned long long)level << 56) | ((unsigned long long)(255u - (msum < 255u ? msum : 255u)) << 48) |
           ((unsigned long long)(0xFFFFu - o) << 32) | ((unsigned long long)(PICK_CONTIG_MAX - contig) << 1) | strand;
}

struct JoinFlank { uint32_t n_l, n_r; const uint8_t *left_end, *right; };   // left_end: one past the left flank's last byte
__device__ __forceinline__ JoinFlank join_flank(const JoinParams& P, uint32_t gap) {
    const uint8_t* row = P.flanks + (uint64_t)gap * P.stride;
    const uint32_t* n = (const uint32_t*)row;
    return {n[0], n[1], row + 8 + P.W, row + 8 + P.W};
}

// the candidate of one strand: the level (long first: both anchors on the strand at that length, else the short one) and the oriented
// positions; false: the strand carries no pair of anchors at either length
__device__ __forceinline__ bool join_positions(const bool* any, const uint32_t* mn, const uint32_t* mx, bool has_long, uint32_t a_s, uint32_t a_l,
                                               uint32_t n, uint32_t strand, uint32_t* a, uint32_t* i, uint32_t* j, bool* multi) {
    const int L = strand ? ANC_RC_LEFT : ANC_LEFT, R = strand ? ANC_RC_RIGHT : ANC_RIGHT;
    int base;
    if (has_long && any[4 + L] && any[4 + R]) { base = 4; *a = a_l; }
    else if (any[L] && any[R]) { base = 0; *a = a_s; }
    else return false;
    *i = strand ? n - *a - mx[base + L] : mn[base + L];
    *j = strand ? n - *a - mn[base + R] : mx[base + R];
    *multi = mn[base + L] != mx[base + L] || mn[base + R] != mx[base + R];
    return true;
}

// #{x < cnt : S[from + x] != f[x]}, S the oriented strand of the contig s[0 .. n); the columns strided over the lanes, the sum in every lane
__device__ __forceinline__ uint32_t join_mismatches(const char* s, uint32_t n, uint32_t strand, uint32_t from, const uint8_t* f, uint32_t cnt, uint32_t lane) {
    uint32_t m = 0;
    for (uint32_t x = lane; x < cnt; x += 64) {
        const char c = strand ? base_comp(s[n - 1 - (from + x)]) : s[from + x];
        m += (uint8_t)c != f[x];
    }
    for (int d = 32; d >= 1; d >>= 1) m += __shfl_xor(m, d);
    return m;
}

__global__ __launch_bounds__(256) void join_candidates_kernel(JoinParams P) {
    const uint32_t n = contig_list_end(P.list);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t a = P.a_s, al = P.a_l;
    const bool want[2] = {true, true};
    uint32_t n_cand = 0, n_far = 0, n_short = 0, n_ctx = 0, n_mis = 0;       // of this wave (uniform over its lanes)
    for (uint32_t ci = contig_list_begin(P.list) + wave; ci < n; ci += n_waves) {
        const gf_contig c = P.list.contigs[ci];
        if (c.gap >= P.n_gaps || c.length < a || P.gap_best[c.gap]) continue;
        const uint8_t* as = anchor_rows(P.anc_s, c.gap);
        if (!anchor_rows_set(as)) continue;                       // (no short anchors: no long ones either)
        const uint8_t* alp = P.anc_l ? anchor_rows(P.anc_l, c.gap) : nullptr;
        const bool has_long = alp && anchor_rows_set(alp);
        const char* s = P.list.seq + c.seq_off;
        uint32_t mn[8], mx[8];
        bool any[8];
        anchor_scan<true>(s, c.length, as, has_long ? alp : nullptr, a, al, want, lane, mn, mx, any);
        const JoinFlank f = join_flank(P, c.gap);
        for (uint32_t strand = 0; strand < 2; ++strand) {
            uint32_t lvl, i, j;
            bool multi;
            if (!join_positions(any, mn, mx, has_long, a, al, c.length, strand, &lvl, &i, &j, &multi)) continue;
            if (j >= i + lvl) continue;                           // in order: the pick's pair
            const uint32_t o = i + lvl - j;
            ++n_cand;
            if (lane == 0) atomicAdd(&P.ws[c.gap].n_cand, 1u);
            if (o > P.X) { ++n_far; continue; }
            if (o + P.C > f.n_l || o + P.C > f.n_r) { ++n_short; continue; }
            if (j < P.C || i + lvl + P.C > c.length) { ++n_ctx; continue; }
            const uint32_t cols = o + P.C;                        // (<= W, <= both flanks, and [j - C, j + cols) inside the strand)
            const uint32_t m_l = join_mismatches(s, c.length, strand, j - P.C, f.left_end - cols, cols, lane);
            const uint32_t m_r = join_mismatches(s, c.length, strand, j, f.right, cols, lane);
            if (m_l > P.M || m_r > P.M) { ++n_mis; continue; }
            if (lane == 0) {
                JoinScratch* w = P.ws + c.gap;
                atomicMax(&w->word, join_word_pack(lvl, m_l + m_r, o, ci, strand));
                atomicAdd(&w->n_acc, 1u);
                atomicMax(&w->o_min_inv, 0xFFFFu - o);
                atomicMax(&w->o_max, o);
            }
        }
    }
    if (lane != 0) return;
    if (n_cand) atomicAdd(P.stats + GF_FJ_CANDIDATES, n_cand);
    if (n_far) atomicAdd(P.stats + GF_FJ_FAR, n_far);
    if (n_short) atomicAdd(P.stats + GF_FJ_SHORT_FLANK, n_short);
    if (n_ctx) atomicAdd(P.stats + GF_FJ_NO_CONTEXT, n_ctx);
    if (n_mis) atomicAdd(P.stats + GF_FJ_MISMATCH, n_mis);
}

__global__ __launch_bounds__(256) void join_records_kernel(JoinParams P) {
    const uint32_t n = contig_list_end(P.list);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const bool want[2] = {true, true};
    uint32_t n_open = 0, n_joined = 0, n_usable = 0, n_bare = 0;
    for (uint32_t g = wave; g < P.n_gaps; g += n_waves) {
        gf_flank_join r;
        memset(&r, 0, sizeof(r));
        const bool open = P.gap_best[g] == 0;
        const JoinScratch w = P.ws[g];
        if (open) {
            ++n_open;
            if (!anchor_rows_set(anchor_rows(P.anc_s, g))) ++n_bare;
        }
        const uint32_t ci = PICK_CONTIG_MAX - ((uint32_t)(w.word >> 1) & PICK_CONTIG_MAX);
        if (open && w.word && ci < n && P.list.contigs[ci].gap == g && P.list.contigs[ci].length >= P.a_s) {
            const uint32_t strand = (uint32_t)w.word & 1u, o = 0xFFFFu - ((uint32_t)(w.word >> 32) & 0xFFFFu), level = (uint32_t)(w.word >> 56);
            const gf_contig c = P.list.contigs[ci];
            const uint8_t* as = anchor_rows(P.anc_s, g);
            const uint8_t* alp = P.anc_l ? anchor_rows(P.anc_l, g) : nullptr;
            const bool has_long = alp && anchor_rows_set(alp);
            const char* s = P.list.seq + c.seq_off;
            uint32_t mn[8], mx[8], lvl, i, j;
            bool any[8], multi;
            anchor_scan<true>(s, c.length, as, has_long ? alp : nullptr, P.a_s, P.a_l, want, lane, mn, mx, any);
            // (the winner was accepted from these positions: the scan finds them again)
            const JoinFlank f = join_flank(P, g);
            const uint32_t cols = o + P.C;
            if (join_positions(any, mn, mx, has_long, P.a_s, P.a_l, c.length, strand, &lvl, &i, &j, &multi) && lvl == level && i + lvl == j + o &&
                o >= 1 && o <= P.X && cols <= f.n_l && cols <= f.n_r && j >= P.C && i + lvl + P.C <= c.length) {
                const uint32_t m_l = join_mismatches(s, c.length, strand, j - P.C, f.left_end - cols, cols, lane);
                const uint32_t m_r = join_mismatches(s, c.length, strand, j, f.right, cols, lane);
                uint32_t m_f = 0;
                for (uint32_t x = lane; x < o; x += 64) m_f += (f.left_end - o)[x] != f.right[x];
                for (int d = 32; d >= 1; d >>= 1) m_f += __shfl_xor(m_f, d);
                const uint32_t o_min = 0xFFFFu - w.o_min_inv;
                r.contig = ci;
                r.left_pos = i;
                r.right_pos = j;
                r.overlap = (uint16_t)o;
                r.m_left = (uint16_t)m_l;
                r.m_right = (uint16_t)m_r;
                r.m_flanks = (uint16_t)m_f;
                r.n_candidates = (uint16_t)(w.n_cand < 0xFFFFu ? w.n_cand : 0xFFFFu);
                r.n_accepted = (uint16_t)(w.n_acc < 0xFFFFu ? w.n_acc : 0xFFFFu);
                r.o_min = (uint16_t)o_min;
                r.o_max = (uint16_t)w.o_max;
                r.level = (uint8_t)level;
                r.flags = (uint8_t)((strand ? GF_FJ_F_REVERSE : 0) | (o_min != w.o_max ? GF_FJ_F_AMBIGUOUS : 0) | (multi ? GF_FJ_F_MULTI : 0));
                ++n_joined;
                if (!(r.flags & (GF_FJ_F_AMBIGUOUS | GF_FJ_F_MULTI))) ++n_usable;
            }
        }
        if (lane == 0) P.out[g] = r;
    }
    if (lane != 0) return;
    if (n_open) atomicAdd(P.stats + GF_FJ_OPEN, n_open);
    if (n_joined) atomicAdd(P.stats + GF_FJ_JOINED, n_joined);
    if (n_usable) atomicAdd(P.stats + GF_FJ_USABLE, n_usable);
    if (n_bare) atomicAdd(P.stats + GF_FJ_NO_ANCHORS, n_bare);
}

// the flank table of width W (built once per gf_set_gaps and W)
static int join_flank_table(gf_ctx* ctx, uint32_t W, const uint8_t** out) {
    const size_t ng = ctx->gaps.size(), stride = 8 + 2 * (size_t)W;
    DevBuf& tab = ctx->anchor_tabs[JOIN_TAB_KEY - (int)W];
    if (!tab.p) {
        std::vector<uint8_t> h(ng * stride, 0);
        for (size_t g = 0; g < ng; ++g) {
            const std::string &l = ctx->flank_left[g], &r = ctx->flank_right[g];
            if (l.size() >= 65536 || r.size() >= 65536) return GF_E_UNSUPPORTED;
            uint8_t* row = h.data() + g * stride;
            const uint32_t nn[2] = {(uint32_t)l.size(), (uint32_t)r.size()};
            memcpy(row, nn, 8);
            const size_t kl = l.size() < W ? l.size() : W, kr = r.size() < W ? r.size() : W;
            memcpy(row + 8 + W - kl, l.data() + l.size() - kl, kl);
            memcpy(row + 8 + W, r.data(), kr);
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

int gf_pick_joins_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int anchor_len,
                      int anchor_len_short, int max_overlap, int min_context, int max_mismatch, const void* d_first, const void* d_gap_best,
                      void* d_join, void* d_stats) {
    const bool own_ok = d_gap_best && d_join && d_stats && anchor_len >= 8 && anchor_len <= ANCHOR_MAX &&
                        (!anchor_len_short || (anchor_len_short >= 8 && anchor_len_short < anchor_len)) && max_overlap >= 1 &&
                        max_overlap <= GF_FJ_MAX_OVERLAP && min_context >= 0 && min_context <= GF_FJ_MAX_CONTEXT && max_mismatch >= 0 &&
                        max_mismatch <= GF_FJ_MAX_MISMATCH;
    JoinParams P;
    memset(&P, 0, sizeof(P));
    int rc = contig_list_view(ctx, d_contigs, d_n_contigs, contig_cap, CONTIG_CAP_WORD, d_seq, d_first, own_ok ? GF_OK : GF_E_INVAL, &P.list);
    if (rc) return rc;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(d_stats, 0, 4 * GF_FJ_WORDS, ctx->stream));
    const size_t ng = ctx->gaps.size();
    if (!ng) return GF_OK;
    const int a_s = anchor_len_short ? anchor_len_short : anchor_len;
    if (anchor_len_short && (rc = anchor_table(ctx, anchor_len, &P.anc_l))) return rc;
    if ((rc = anchor_table(ctx, a_s, &P.anc_s))) return rc;
    P.W = ((uint32_t)(max_overlap + min_context) + 3u) & ~3u;
    P.stride = 8 + 2 * P.W;
    if ((rc = join_flank_table(ctx, P.W, &P.flanks))) return rc;
    if ((rc = ensure(ctx, ctx->join_ws, ng * sizeof(JoinScratch) + 64))) return rc;
    P.gap_best = (const unsigned long long*)d_gap_best;
    P.n_gaps = (uint32_t)ng;
    P.a_s = (uint32_t)a_s;
    P.a_l = (uint32_t)anchor_len;
    P.X = (uint32_t)max_overlap;
    P.C = (uint32_t)min_context;
    P.M = (uint32_t)max_mismatch;
    P.ws = (JoinScratch*)ctx->join_ws.p;
    P.out = (gf_flank_join*)d_join;
    P.stats = (uint32_t*)d_stats;
    GF_HIP(ctx, hipMemsetAsync(P.ws, 0, ng * sizeof(JoinScratch), ctx->stream));
    LaunchTimer tm(ctx, GF_KERNEL_JOIN);
    hipLaunchKernelGGL(join_candidates_kernel, dim3(ctx->n_cu * 8), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    const unsigned blocks = (unsigned)((ng + 3) / 4 < (size_t)ctx->n_cu * 4 ? (ng + 3) / 4 : (size_t)ctx->n_cu * 4);
    hipLaunchKernelGGL(join_records_kernel, dim3(blocks), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // extern "C"
