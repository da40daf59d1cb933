// pick_ext.hip — partial fills of the gaps that no pick of the step closed: the reference's last stage, run_pick_extended_contig
// (pick_contigs.py:361-539, called at assemble_gaps.py:367-368 with score 15).  For such a gap every clipped hit of a flank on a contig
// is a candidate; per side the FIRST contig with one wins, the same contig on both sides is used on the right only, and the two parts —
// the contig beyond the left anchor, the contig before the right anchor, reverse-strand parts keeping one anchor base — are joined by
// "NN".  "First" needs a contig order the device list does not have: the order is (rank of the contig's (k, kv) pair, merged contigs
// after every pair; length descending; bases ascending; contig index), pick_contigs.extension_order.  Definition and host twin:
// gappadder_amd/pick_contigs.py::pick_extended_sequence on the contigs in that order.  Entry points: gf_pick_extended_dev (exact
// anchors), gf_pick_extended_aligned_dev and gf_pick_extended_gapped_dev (the align- / gapped-mode hits of pick_align.hip),
// include/gapfill_hip.h.
//
// Four launches, no host synchronisation:
//   hits     one wave per contig of an open gap (exact: here, the leftmost / rightmost anchor positions pick_anchor_kernel reduces,
//            without its 2·a length floor — a one-sided hit needs a bases; align: pick_align.hip's seed ranking and walk); a contig
//            with a wanted hit on a side is pushed on the gap's list for that side (atomicExch on the head, the old head is its link)
//   choose   one thread per gap: the minimum of each list under the order above (ties on (rank, length) compare bases), the slices
//            and the fill length
//   scan     one workgroup: fill offsets in gap order, the total, the overflow flag
//   write    one wave per gap: the parts gathered (and reverse-complemented) into the base buffer around "NN"
#include <cstring>

#include "anchor.hpp"
#include "contig_list.hpp"
#include "gf_internal.hpp"

namespace gf {

struct ExtParams {
    ContigList list;
    const unsigned long long* gap_best;
    uint32_t n_gaps;
    ExtHit* hits;                          // per contig index
    uint32_t* heads;                       // [n_gaps][2]
    gf_ext_pick* ext;
    char* bases;
    uint64_t base_cap;
    uint32_t* stats;
    uint32_t n_k;
    uint16_t k[GF_EXT_MAX_PAIRS], kv[GF_EXT_MAX_PAIRS];
};

// exact anchors: per contig forward left = leftmost occurrence of the left anchor, forward right = rightmost occurrence of the right
// anchor, reverse left = rightmost occurrence of rc(left anchor), reverse right = leftmost of rc(right anchor) (anchor_hits: the
// reverse strand searched in the reverse-complemented contig, positions in the contig's own frame).  Wanted: the side's flank is
// longer than the anchor (a flank of exactly `a` bases gives unclipped hits); forward before reverse.
__global__ __launch_bounds__(256) void ext_anchor_kernel(ExtParams P, const uint8_t* anc, uint32_t a) {
    const uint32_t n = contig_list_end(P.list);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t ci = contig_list_begin(P.list) + wave; ci < n; ci += n_waves) {
        const gf_contig c = P.list.contigs[ci];
        if (c.gap >= P.n_gaps || c.length < a || P.gap_best[c.gap]) continue;
        const uint8_t* as = anchor_rows(anc, c.gap);
        const uint32_t fl = anchor_flags(as);
        const bool want[2] = {anchor_row(as, ANC_LEFT)[0] != 0 && !(fl & ANC_F_LEFT_WHOLE),
                              anchor_row(as, ANC_RIGHT)[0] != 0 && !(fl & ANC_F_RIGHT_WHOLE)};   // (no anchors: both rows empty)
        if (!want[0] && !want[1]) continue;
        uint32_t mn[4], mx[4];
        bool any[4];
        anchor_scan<false>(P.list.seq + c.seq_off, c.length, as, nullptr, a, 0, want, lane, mn, mx, any);
        if (lane != 0) continue;
        ExtHit h;
        h.m[0] = h.m[1] = 0;
        h.pad = 0;
        if (any[ANC_LEFT] || any[ANC_RC_LEFT]) {
            h.m[0] = (uint16_t)a;
            h.rev[0] = !any[ANC_LEFT];
            h.pos[0] = (any[ANC_LEFT] ? mn[ANC_LEFT] : mx[ANC_RC_LEFT]) + 1;
        }
        if (any[ANC_RIGHT] || any[ANC_RC_RIGHT]) {
            h.m[1] = (uint16_t)a;
            h.rev[1] = !any[ANC_RIGHT];
            h.pos[1] = (any[ANC_RIGHT] ? mx[ANC_RIGHT] : mn[ANC_RC_RIGHT]) + 1;
        }
        if (!h.m[0] && !h.m[1]) continue;
        ext_hit_publish(P.heads, P.hits, c.gap, ci, h);
    }
}

__device__ __forceinline__ uint32_t ext_rank(const ExtParams& P, const gf_contig& c) {
    for (uint32_t i = 0; i < P.n_k; ++i)
        if (c.k == P.k[i] && c.kv == P.kv[i]) return i;
    if (c.k == GF_RESCUE_MARK && c.kv == GF_RESCUE_MARK) return P.n_k + 1;     // the rescue's bridges: after the merged contigs
    return P.n_k;                          // merged contigs (k = kv = 0) and any pair not in the list: after every pair
}

// contig a before contig b in the extension order
__device__ bool ext_before(const ExtParams& P, uint32_t a, uint32_t b) {
    const gf_contig ca = P.list.contigs[a], cb = P.list.contigs[b];
    const uint32_t ra = ext_rank(P, ca), rb = ext_rank(P, cb);
    if (ra != rb) return ra < rb;
    if (ca.length != cb.length) return ca.length > cb.length;
    const uint8_t *sa = (const uint8_t*)P.list.seq + ca.seq_off, *sb = (const uint8_t*)P.list.seq + cb.seq_off;
    for (uint32_t i = 0; i < ca.length; ++i)
        if (sa[i] != sb[i]) return sa[i] < sb[i];
    return a < b;
}

__global__ __launch_bounds__(256) void ext_choose_kernel(ExtParams P) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.n_gaps) return;
    gf_ext_pick r;
    memset(&r, 0, sizeof(r));
    uint32_t best[2] = {EMPTY32, EMPTY32};
    for (int sd = 0; sd < 2; ++sd)
        for (uint32_t ci = P.heads[2 * g + sd]; ci != EMPTY32; ci = P.hits[ci].next[sd])
            if (best[sd] == EMPTY32 || ext_before(P, ci, best[sd])) best[sd] = ci;
    const uint32_t L = best[0], R = best[1];
    r.left = L;
    r.right = R;
    if (L != EMPTY32 && L != R) {          // the contig beyond the left anchor; reverse: before rc(anchor), its first base kept
        const ExtHit h = P.hits[L];
        const uint32_t n = P.list.contigs[L].length;
        r.l_rev = h.rev[0];
        r.l_beg = h.rev[0] ? 0u : h.pos[0] + h.m[0] - 1;
        r.l_len = h.rev[0] ? h.pos[0] : n - r.l_beg;
    }
    if (R != EMPTY32) {                    // the contig before the right anchor (reverse: after rc(anchor)); the same contig on both
        const ExtHit h = P.hits[R];        // sides: the forward part keeps the anchor's first base (pick_contigs.py:480-486)
        const uint32_t n = P.list.contigs[R].length;
        r.r_rev = h.rev[1];
        r.r_beg = h.rev[1] ? h.pos[1] + h.m[1] - 1 : 0u;
        r.r_len = h.rev[1] ? n - r.r_beg : h.pos[1] - (L == R ? 0u : 1u);
    }
    r.len = r.l_len + r.r_len ? r.l_len + r.r_len + 2 : 0u;     // nothing but "NN": no fill
    P.ext[g] = r;
    if (r.len) {
        atomicAdd(P.stats + GF_EXT_EXTENDED, 1u);
        atomicAdd(P.stats + (L == EMPTY32 ? GF_EXT_RIGHT_ONLY : R == EMPTY32 ? GF_EXT_LEFT_ONLY : GF_EXT_BOTH), 1u);
    }
}

constexpr int EXT_SCAN_THREADS = 1024;

__global__ __launch_bounds__(EXT_SCAN_THREADS) void ext_scan_kernel(ExtParams P) {
    __shared__ unsigned long long part[EXT_SCAN_THREADS];
    const uint32_t t = threadIdx.x, per = (P.n_gaps + EXT_SCAN_THREADS - 1) / EXT_SCAN_THREADS;
    const uint32_t b = t * per < P.n_gaps ? t * per : P.n_gaps, e = b + per < P.n_gaps ? b + per : P.n_gaps;
    unsigned long long sum = 0;
    for (uint32_t i = b; i < e; ++i) sum += P.ext[i].len;
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < EXT_SCAN_THREADS; d <<= 1) {
        const unsigned long long v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long off = part[t] - sum;
    for (uint32_t i = b; i < e; ++i) {
        P.ext[i].off = off;
        off += P.ext[i].len;
    }
    if (t == EXT_SCAN_THREADS - 1) {
        const unsigned long long total = part[t];
        P.stats[GF_EXT_BASES] = (uint32_t)total;
        P.stats[GF_EXT_BASES + 1] = (uint32_t)(total >> 32);
        P.stats[GF_EXT_OVERFLOW] = total > P.base_cap ? 1u : 0u;
    }
}

__device__ __forceinline__ char ext_comp(char c) {        // pick_contigs.revcomp: ACGTacgt -> TGCATGCA, anything else as it is
    switch (c) {
        case 'A': case 'a': return 'T';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        case 'T': case 't': return 'A';
        default: return c;
    }
}

__device__ __forceinline__ void ext_copy(char* o, const char* s, uint32_t n, bool rev, uint32_t lane) {
    if (rev)
        for (uint32_t i = lane; i < n; i += 64) o[i] = ext_comp(s[n - 1 - i]);
    else
        for (uint32_t i = lane; i < n; i += 64) o[i] = s[i];
}

__global__ __launch_bounds__(256) void ext_write_kernel(ExtParams P) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t g = wave; g < P.n_gaps; g += n_waves) {
        const gf_ext_pick r = P.ext[g];
        if (!r.len || r.off + r.len > P.base_cap) continue;     // (beyond the buffer: the overflow flag is set, nothing is cut)
        char* o = P.bases + r.off;
        if (r.l_len) ext_copy(o, P.list.seq + P.list.contigs[r.left].seq_off + r.l_beg, r.l_len, r.l_rev, lane);
        if (lane < 2) o[r.l_len + lane] = 'N';
        if (r.r_len) ext_copy(o + r.l_len + 2, P.list.seq + P.list.contigs[r.right].seq_off + r.r_beg, r.r_len, r.r_rev, lane);
    }
}

}  // namespace gf

using namespace gf;

extern "C" {

static int pick_extended(gf_ctx* ctx, bool align, bool gapped, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int a,
                         const int* k_list, const int* kv_list, int n_k, const void* d_first, const void* d_gap_best, void* d_ext, void* d_bases,
                         size_t base_cap, void* d_stats) {
    const bool own_ok = d_gap_best && d_ext && d_stats && (!base_cap || d_bases) && n_k >= 0 && n_k <= GF_EXT_MAX_PAIRS && (!n_k || (k_list && kv_list)) &&
                        (align ? (a >= 1 && a <= 255) : (a >= 8 && a <= ANCHOR_MAX));
    ExtParams P;
    memset(&P, 0, sizeof(P));
    int rc = contig_list_view(ctx, d_contigs, d_n_contigs, contig_cap, CONTIG_CAP_WORD, d_seq, d_first, own_ok ? GF_OK : GF_E_INVAL, &P.list);
    if (rc) return rc;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(d_stats, 0, 4 * GF_EXT_WORDS, ctx->stream));
    const size_t ng = ctx->gaps.size();
    if (!ng) return GF_OK;
    const uint8_t* anc = nullptr;
    if (!align && (rc = anchor_table(ctx, a, &anc))) return rc;
    const size_t head_bytes = (ng * 8 + 255) & ~(size_t)255;
    if ((rc = ensure(ctx, ctx->ext_ws, head_bytes + contig_cap * sizeof(ExtHit) + 64))) return rc;
    P.gap_best = (const unsigned long long*)d_gap_best;
    P.n_gaps = (uint32_t)ng;
    P.heads = (uint32_t*)ctx->ext_ws.p;
    P.hits = (ExtHit*)((char*)ctx->ext_ws.p + head_bytes);
    P.ext = (gf_ext_pick*)d_ext;
    P.bases = (char*)d_bases;
    P.base_cap = base_cap;
    P.stats = (uint32_t*)d_stats;
    P.n_k = (uint32_t)n_k;
    for (int i = 0; i < n_k; ++i) {
        if (k_list[i] < 0 || k_list[i] > 0xFFFF || kv_list[i] < 0 || kv_list[i] > 0xFFFF) return GF_E_INVAL;
        P.k[i] = (uint16_t)k_list[i];
        P.kv[i] = (uint16_t)kv_list[i];
    }
    GF_HIP(ctx, hipMemsetAsync(P.heads, 0xFF, ng * 8, ctx->stream));
    LaunchTimer tm(ctx, GF_KERNEL_PICK);
    if (align) {
        if ((rc = launch_align_ext(ctx, gapped, P.list, a, d_gap_best, P.hits, P.heads, P.stats + GF_EXT_ALIGN_DROPPED))) return rc;
    } else {
        hipLaunchKernelGGL(ext_anchor_kernel, dim3(ctx->n_cu * 8), dim3(256), 0, ctx->stream, P, anc, (uint32_t)a);
        GF_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(ext_choose_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(ext_scan_kernel, dim3(1), dim3(EXT_SCAN_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(ext_write_kernel, dim3(ctx->n_cu * 4), dim3(256), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_pick_extended_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int anchor_len,
                         const int* k_list, const int* kv_list, int n_k, const void* d_first, const void* d_gap_best, void* d_ext,
                         void* d_bases, size_t base_cap, void* d_stats) {
    return pick_extended(ctx, false, false, d_contigs, d_n_contigs, contig_cap, d_seq, anchor_len, k_list, kv_list, n_k, d_first, d_gap_best, d_ext,
                         d_bases, base_cap, d_stats);
}

int gf_pick_extended_aligned_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t,
                                 const int* k_list, const int* kv_list, int n_k, const void* d_first, const void* d_gap_best, void* d_ext,
                                 void* d_bases, size_t base_cap, void* d_stats) {
    return pick_extended(ctx, true, false, d_contigs, d_n_contigs, contig_cap, d_seq, t, k_list, kv_list, n_k, d_first, d_gap_best, d_ext, d_bases,
                         base_cap, d_stats);
}

int gf_pick_extended_gapped_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t,
                                const int* k_list, const int* kv_list, int n_k, const void* d_first, const void* d_gap_best, void* d_ext,
                                void* d_bases, size_t base_cap, void* d_stats) {
    return pick_extended(ctx, true, true, d_contigs, d_n_contigs, contig_cap, d_seq, t, k_list, kv_list, n_k, d_first, d_gap_best, d_ext, d_bases,
                         base_cap, d_stats);
}

}  // extern "C"
