// merge_export.hip — the contig-merge round with its graph exported (gf_merge_sets_dev / gf_merge_sets): what the CLI's
// MergeContigs.merge_contigs needs per gap for the reference's files (MergeContigs.py:66-99) — the de-duplicated set
// (contigs.fa_no_dup.fa), the graph's edges (merge_edges.txt), the paths (…merge.info), the merged strings and the second dedup over
// [merged strings] + [survivors] (contigs.fa) — from ONE chain of launches over all gaps of a round.
//
//   mx_prepare      the sets' contigs as the round's contig list (gap = set, record order = input order), bases upper-cased in place
//   launch_merge_round (merge.hip)   dedup, prefilter, overlap evaluation, paths, merged strings — its kernels as they are; mg_paths and
//                   mg_strings additionally say which sets they left alone for their graph and how many nodes every path merged
//   mx_count        per set (one workgroup): status, first-dedup flags, edges, paths, truncated paths, path bytes
//   mx_scan         one workgroup: offsets of every set's edges / paths / path nodes / final flags, totals, capacity flags
//   mx_write        per set: edges in the prefilter's (i, j) order, path records + node lists, the second dedup's record list
//   launch_merge_sets (merge.hip)    the second dedup: mg_dedup in record order over that list
//   mx_final        per set: the second dedup's kept flags
// Orders come from scans and from the order of the round's own lists; the only atomics here add up statistics.  Capacities: mx_scan
// compares every total with its capacity and sets stats[GF_MX_FLAGS]; mx_write / mx_final write NOTHING unless the flags are zero, and
// every store is bounded by its capacity besides.
#include <algorithm>
#include <cstring>

#include "gf_internal.hpp"
#include "merge_dev.hpp"

namespace gf {

struct MxParams {
    MgParams R;                              // the round's parameter block (its workspace)
    const unsigned long long* contig_off;    // the caller's sets
    const unsigned long long* set_off;
    uint32_t n_sets, n_contigs;
    gf_mset* sets;
    uint8_t* kept;
    gf_medge* edges;
    gf_mnew* news;
    uint8_t* paths;
    uint8_t* finals;
    uint32_t* stats;
    uint32_t edge_cap, new_cap, path_cap, final_cap;
    uint32_t* st_of_set;                     // [n_sets] the round's set of a caller's set, or EMPTY32
    uint32_t* path_base;                     // [n_sets] path bytes of a set, after mx_scan their first byte
    gf_contig* list2;                        // [contig_cap] the second dedup's records: index = index of the final flag
    uint32_t* n2;
    MgSetsView v2;                           // where the second dedup leaves its sets
};

__device__ __forceinline__ bool mx_is_node(uint32_t len) { return len >= MG_MIN_NODE && len <= MG_MAX_NODE; }

__global__ __launch_bounds__(256) void mx_prepare_kernel(MxParams X, char* seq, unsigned long long n_bytes, gf_contig* contigs, uint32_t* n_contigs,
                                                         unsigned long long* seq_len) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
    for (size_t c = t0; c < X.n_contigs; c += nt) {
        uint32_t lo = 0, hi = X.n_sets;              // the set whose range holds c: the last s with set_off[s] <= c
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (X.set_off[mid + 1] <= c) lo = mid + 1; else hi = mid;
        }
        gf_contig r;
        memset(&r, 0, sizeof r);
        r.gap = lo;                                  // (a contig behind the last set: gap == n_sets, takes no part)
        r.length = (uint32_t)(X.contig_off[c + 1] - X.contig_off[c]);
        r.seq_off = X.contig_off[c];
        contigs[c] = r;
    }
    for (size_t b = t0; b < n_bytes; b += nt) {
        const char ch = seq[b];
        if (ch >= 'a' && ch <= 'z') seq[b] = (char)(ch - 32);
    }
    if (t0 == 0) { *n_contigs = X.n_contigs; *seq_len = n_bytes; }
}

// one workgroup per set
__global__ __launch_bounds__(256) void mx_count_kernel(MxParams X) {
    __shared__ uint32_t s_edges, s_pbytes, s_trunc;
    const MgParams& R = X.R;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_round_sets = R.stats[MG_N_SETS], n_pre = R.stats[MG_N_PRE];
    for (uint32_t g = blockIdx.x; g < X.n_sets; g += gridDim.x) {
        __syncthreads();
        if (tid == 0) { s_edges = 0; s_pbytes = 0; s_trunc = 0; }
        const unsigned long long c0 = X.set_off[g], c1 = X.set_off[g + 1];
        const uint32_t cnt = (uint32_t)(c1 - c0);
        for (uint32_t c = tid; c < cnt; c += blockDim.x) {        // (one contig: it stays; otherwise the dedup's answer below)
            const uint32_t len = (uint32_t)(X.contig_off[c0 + c + 1] - X.contig_off[c0 + c]);
            X.kept[c0 + c] = cnt == 1 ? (uint8_t)(1u | (mx_is_node(len) ? 2u : 0u)) : (uint8_t)0;
        }
        __syncthreads();
        uint32_t status = cnt > MG_MAX_IN ? GF_MSET_SIZE : GF_MSET_NOTHING, n_kept = cnt < 2 ? cnt : 0u, st = EMPTY32, n_new = 0;
        const uint32_t pre = cnt >= 2 && cnt <= MG_MAX_IN ? R.pre_of_gap[g] : EMPTY32;
        if (pre < n_pre) {
            const uint32_t o = R.pre_off[pre], kn = R.kept_n[pre];
            for (uint32_t i = tid; i < kn; i += blockDim.x) {
                const uint32_t id = R.ids[o + i];
                if (id < X.n_contigs) X.kept[id] = (uint8_t)(1u | (mx_is_node(R.contigs[id].length) ? 2u : 0u));
            }
            n_kept = kn;
            if (kn > R.max_set) status = GF_MSET_SIZE;
            else if (kn < 2 || R.node_n[pre] < 2) status = GF_MSET_NOTHING;
            else {
                uint32_t lo = 0, hi = n_round_sets;          // the round's set of this gap: set_pre ascends
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (R.set_pre[mid] < pre) lo = mid + 1; else hi = mid;
                }
                if (lo < n_round_sets && R.set_pre[lo] == pre) st = lo;
                status = st == EMPTY32 || R.x_graph[st] ? GF_MSET_GRAPH : GF_MSET_MERGED;      // (no set: the round's node buffer overflowed, flagged)
            }
        }
        if (status == GF_MSET_MERGED) {
            const uint32_t pb = R.set_range[2 * st], pn = R.set_range[2 * st + 1];
            if ((unsigned long long)pb + pn <= R.pair_cap) {
                uint32_t e = 0;
                for (uint32_t x = tid; x < pn; x += blockDim.x) {
                    const gf_ovl_result r = R.res[pb + x];
                    if (r.res == 2 && !r.containment) ++e;
                }
                if (e) atomicAdd(&s_edges, e);
            }
            const uint32_t jb = R.set_jobs[2 * st];
            n_new = R.set_jobs[2 * st + 1];
            if ((unsigned long long)jb + n_new > R.job_cap) n_new = 0;
            uint32_t pbytes = 0, tr = 0;
            for (uint32_t q = tid; q < n_new; q += blockDim.x) {
                const uint32_t len = R.jobs[jb + q].len, used = min(R.x_used[jb + q], len);
                pbytes += used;
                if (used < len) ++tr;
            }
            if (pbytes) atomicAdd(&s_pbytes, pbytes);
            if (tr) atomicAdd(&s_trunc, tr);
        }
        __syncthreads();
        if (tid == 0) {
            gf_mset m;
            m.status = status; m.n_kept = n_kept; m.n_edges = s_edges; m.edge_off = 0; m.n_new = n_new; m.new_off = 0; m.final_off = 0;
            m.n_truncated = s_trunc;
            X.sets[g] = m;
            X.st_of_set[g] = status == GF_MSET_MERGED ? st : EMPTY32;
            X.path_base[g] = s_pbytes;
        }
    }
}

__device__ __forceinline__ uint32_t mx_n_final(const gf_mset& m) { return m.status == GF_MSET_MERGED || m.status == GF_MSET_NOTHING ? m.n_new + m.n_kept : 0u; }

__global__ __launch_bounds__(1024) void mx_scan_kernel(MxParams X) {
    __shared__ uint32_t s_w[20];
    const MgParams& R = X.R;
    uint32_t ce = 0, cn = 0, cp = 0, cf = 0;
    uint32_t n_st0 = 0, n_st1 = 0, n_st2 = 0, n_st3 = 0, trunc = 0;      // sets by status (GF_MSET_*)
    for (uint32_t g0 = 0; g0 < X.n_sets; g0 += blockDim.x) {
        const uint32_t g = g0 + threadIdx.x;
        gf_mset m;
        memset(&m, 0, sizeof m);
        uint32_t pb = 0;
        if (g < X.n_sets) {
            m = X.sets[g]; pb = X.path_base[g]; trunc += m.n_truncated;
            n_st0 += m.status == GF_MSET_MERGED; n_st1 += m.status == GF_MSET_NOTHING; n_st2 += m.status == GF_MSET_SIZE; n_st3 += m.status == GF_MSET_GRAPH;
        }
        const uint32_t nf = g < X.n_sets ? mx_n_final(m) : 0u;
        uint32_t te, tn, tp, tf;
        const uint32_t ee = mg_block_scan_excl(m.n_edges, s_w, &te);
        const uint32_t en = mg_block_scan_excl(m.n_new, s_w, &tn);
        const uint32_t ep = mg_block_scan_excl(pb, s_w, &tp);
        const uint32_t ef = mg_block_scan_excl(nf, s_w, &tf);
        if (g < X.n_sets) {
            X.sets[g].edge_off = ce + ee;
            X.sets[g].new_off = cn + en;
            X.sets[g].final_off = cf + ef;
            X.path_base[g] = cp + ep;
        }
        ce += te; cn += tn; cp += tp; cf += tf;
        __syncthreads();
    }
    if (n_st0) atomicAdd(&X.stats[GF_MX_TRIED], n_st0);
    if (n_st1) atomicAdd(&X.stats[GF_MX_NOTHING], n_st1);
    if (n_st2) atomicAdd(&X.stats[GF_MX_SKIPPED_SIZE], n_st2);
    if (n_st3) atomicAdd(&X.stats[GF_MX_SKIPPED_GRAPH], n_st3);
    if (trunc) atomicAdd(&X.stats[GF_MX_TRUNCATED], trunc);
    if (threadIdx.x == 0) {
        const uint32_t err = R.stats[MG_ERR];
        const unsigned long long sl = *R.seq_len;
        uint32_t flags = 0;
        if (ce > X.edge_cap) flags |= GF_MX_F_EDGES;
        if (cn > X.new_cap || (err & MG_E_CONTIGS)) flags |= GF_MX_F_NEW;
        if (cp > X.path_cap) flags |= GF_MX_F_PATHS;
        if (sl > R.seq_cap || (err & MG_E_OUTSEQ)) flags |= GF_MX_F_SEQ;
        if (cf > X.final_cap) flags |= GF_MX_F_FINAL;
        if ((err & (MG_E_SEQ | MG_E_PAIRS)) || R.stats[MG_QC_FLAGS]) flags |= GF_MX_F_ROUND;
        X.stats[GF_MX_PAIRS] = R.stats[MG_N_PAIRS];
        X.stats[GF_MX_EDGES] = ce; X.stats[GF_MX_PATHS] = cn; X.stats[GF_MX_PATH_BYTES] = cp; X.stats[GF_MX_FINALS] = cf;
        X.stats[GF_MX_EDGE_RECORDS] = ce; X.stats[GF_MX_NEW_RECORDS] = cn;
        X.stats[GF_MX_ROUND_ERR] = err | (R.stats[MG_QC_FLAGS] << 8);
        X.stats[GF_MX_SEQ_BYTES] = (uint32_t)sl; X.stats[GF_MX_SEQ_BYTES + 1] = (uint32_t)(sl >> 32);
        X.stats[GF_MX_FLAGS] = flags;
        *X.n2 = flags ? 0u : cf;
    }
}

__global__ __launch_bounds__(256) void mx_write_kernel(MxParams X) {
    __shared__ uint32_t s_w[20];
    if (X.stats[GF_MX_FLAGS]) return;
    const MgParams& R = X.R;
    const uint32_t tid = threadIdx.x;
    for (uint32_t g = blockIdx.x; g < X.n_sets; g += gridDim.x) {
        const gf_mset m = X.sets[g];
        const uint32_t st = X.st_of_set[g];
        if (m.status == GF_MSET_MERGED && st != EMPTY32) {
            // edges: the set's pair range is in (i, j) order (quick_check_kernel) = the order of MergeContigs.graph_edges
            const uint32_t pb = R.set_range[2 * st], pn = (unsigned long long)pb + R.set_range[2 * st + 1] <= R.pair_cap ? R.set_range[2 * st + 1] : 0u;
            uint32_t done = 0;
            for (uint32_t x0 = 0; x0 < pn && m.n_edges; x0 += blockDim.x) {
                const uint32_t x = x0 + tid;
                gf_ovl_result r;
                r.res = 0; r.containment = 0; r.first_goes_first = 0; r.overlap = 0;
                if (x < pn) r = R.res[pb + x];
                const bool is_edge = x < pn && r.res == 2 && !r.containment;
                uint32_t tot;
                const uint32_t ex = mg_block_scan_excl(is_edge ? 1u : 0u, s_w, &tot);
                const uint32_t slot = done + ex;
                if (is_edge && slot < m.n_edges && (unsigned long long)m.edge_off + slot < X.edge_cap) {
                    const gf_qcpair q = R.pairs[pb + x];
                    gf_medge e;
                    e.i = q.i; e.j = q.j; e.mode = r.first_goes_first ? 12u : 21u; e.overlap = (uint32_t)r.overlap;
                    X.edges[m.edge_off + slot] = e;
                }
                done += tot;
                __syncthreads();
            }
            // paths: the set's jobs are in sorted path order (mg_paths) = NEW_CONTIG_MERGE_1, _2, ...
            const uint32_t jb = R.set_jobs[2 * st], rec0 = R.set_rec[st];
            uint32_t pdone = 0;
            for (uint32_t q0 = 0; q0 < m.n_new; q0 += blockDim.x) {
                const uint32_t q = q0 + tid;
                uint32_t used = 0;
                MgJob job;
                job.set = 0; job.off = 0; job.len = 0;
                if (q < m.n_new) { job = R.jobs[jb + q]; used = min(R.x_used[jb + q], job.len); }
                uint32_t tot;
                const uint32_t ex = mg_block_scan_excl(used, s_w, &tot);
                const unsigned long long po = (unsigned long long)X.path_base[g] + pdone + ex;
                if (q < m.n_new && (unsigned long long)m.new_off + q < X.new_cap && po + used <= X.path_cap && rec0 + q < R.contig_cap &&
                    (unsigned long long)job.off + used <= R.job_node_cap) {
                    const gf_contig c = R.contigs[rec0 + q];
                    gf_mnew nw;
                    nw.set = g; nw.n_nodes = used; nw.path_off = (uint32_t)po; nw.length = c.length; nw.seq_off = c.seq_off;
                    X.news[m.new_off + q] = nw;
                    for (uint32_t t = 0; t < used; ++t) X.paths[po + t] = R.job_nodes[job.off + t];
                }
                pdone += tot;
                __syncthreads();
            }
        }
        // the second dedup's records, [merged strings in order] + [survivors in order]; a set without merged strings keeps its survivors
        const uint32_t nf = mx_n_final(m);
        if (nf) {
            const uint32_t pre = m.n_new ? R.pre_of_gap[g] : EMPTY32;
            const uint32_t o = pre != EMPTY32 ? R.pre_off[pre] : 0u;
            for (uint32_t r = tid; r < nf; r += blockDim.x) {
                const unsigned long long at = (unsigned long long)m.final_off + r;
                if (at >= X.final_cap || at >= R.contig_cap) continue;
                gf_contig c;
                memset(&c, 0, sizeof c);
                if (m.n_new && st != EMPTY32 && pre != EMPTY32) {
                    const uint32_t src = r < m.n_new ? R.set_rec[st] + r : R.ids[o + (r - m.n_new)];
                    if (src < R.contig_cap) c = R.contigs[src];
                }
                c.gap = g;                       // (length 0 — a set without merged strings: the record takes no part)
                X.list2[at] = c;
                X.finals[at] = m.n_new ? 0 : 1;
            }
        }
    }
}

__global__ __launch_bounds__(256) void mx_final_kernel(MxParams X) {
    if (X.stats[GF_MX_FLAGS]) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t g = blockIdx.x; g < X.n_sets; g += gridDim.x) {
        const gf_mset m = X.sets[g];
        if (m.status != GF_MSET_MERGED || m.n_new == 0) continue;
        const uint32_t pre2 = X.v2.pre_of_gap[g];
        if (pre2 == EMPTY32) {          // more than 1 024 records for the second dedup: the set is left alone after all
            if (tid == 0) {
                X.sets[g].status = GF_MSET_GRAPH; X.sets[g].n_new = 0; X.sets[g].n_edges = 0; X.sets[g].n_truncated = 0;
                atomicSub(&X.stats[GF_MX_TRIED], 1u); atomicAdd(&X.stats[GF_MX_SKIPPED_GRAPH], 1u);
                atomicSub(&X.stats[GF_MX_EDGES], m.n_edges); atomicSub(&X.stats[GF_MX_PATHS], m.n_new); atomicSub(&X.stats[GF_MX_TRUNCATED], m.n_truncated);
            }
            continue;
        }
        const uint32_t o2 = X.v2.pre_off[pre2], k2 = X.v2.kept_n[pre2], nf = m.n_new + m.n_kept;
        for (uint32_t i = tid; i < k2; i += blockDim.x) {
            const uint32_t id = X.v2.ids[o2 + i];
            if (id >= m.final_off && id - m.final_off < nf && id < X.final_cap) X.finals[id] = 1;
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" {

int gf_merge_sets_dev(gf_ctx* ctx, void* d_seq, size_t n_bytes, size_t seq_cap, const void* d_contig_off, const void* d_set_off, size_t n_sets,
                      size_t n_contigs, const gf_ovl_params* params, int kmer_len_quick, int max_set, void* d_sets, void* d_kept, void* d_edges,
                      size_t edge_cap, void* d_new, size_t new_cap, void* d_paths, size_t path_cap, void* d_final, size_t final_cap, void* d_stats) {
    if (!ctx || !params || !d_stats || (n_sets && (!d_contig_off || !d_set_off || !d_sets)) || (n_contigs && !d_kept) || (n_bytes && !d_seq) ||
        (edge_cap && !d_edges) || (new_cap && !d_new) || (path_cap && !d_paths) || (final_cap && !d_final) || n_bytes > seq_cap ||
        n_sets > 0x7FFFFFF0ull || n_contigs + new_cap > 0x7FFFFFFFull || edge_cap > 0xFFFFFFFFull || path_cap > 0xFFFFFFFFull ||
        final_cap > 0xFFFFFFFFull || kmer_len_quick < 4 || kmer_len_quick > 16 || max_set < 2 || max_set > (int)(MG_MAX_NODES / 2))
        return GF_E_INVAL;
    if (params->indel != (double)(int)params->indel || params->max_clip < 0 || params->max_clip > 1e6) {
        ctx->last_error = "gf_merge_sets_dev: the indel score must be integral";
        return GF_E_UNSUPPORTED;
    }
    GF_HIP(ctx, hipSetDevice(ctx->device));
    GF_HIP(ctx, hipMemsetAsync(d_stats, 0, GF_MX_WORDS * 4, ctx->stream));
    if (!n_sets) return GF_OK;
    const size_t contig_cap = n_contigs + new_cap;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_ctg = take(contig_cap * sizeof(gf_contig)), o_list2 = take(contig_cap * sizeof(gf_contig)), o_cnt = take(64),
                 o_best = take(n_sets * 8), o_st1 = take(MG_WORDS * 4), o_st2 = take(MG_WORDS * 4), o_sos = take(n_sets * 4), o_pb = take(n_sets * 4);
    int rc;
    if ((rc = ensure(ctx, ctx->mx_ws, at + 256))) return rc;
    uint8_t* W = (uint8_t*)ctx->mx_ws.p;
    uint32_t* d_n1 = (uint32_t*)(W + o_cnt);
    unsigned long long* d_seq_len = (unsigned long long*)(W + o_cnt + 8);
    uint32_t* d_n2 = (uint32_t*)(W + o_cnt + 16);
    MxParams X;
    memset(&X, 0, sizeof X);
    X.contig_off = (const unsigned long long*)d_contig_off; X.set_off = (const unsigned long long*)d_set_off;
    X.n_sets = (uint32_t)n_sets; X.n_contigs = (uint32_t)n_contigs;
    X.sets = (gf_mset*)d_sets; X.kept = (uint8_t*)d_kept; X.edges = (gf_medge*)d_edges; X.news = (gf_mnew*)d_new; X.paths = (uint8_t*)d_paths;
    X.finals = (uint8_t*)d_final; X.stats = (uint32_t*)d_stats;
    X.edge_cap = (uint32_t)edge_cap; X.new_cap = (uint32_t)new_cap; X.path_cap = (uint32_t)path_cap; X.final_cap = (uint32_t)final_cap;
    X.st_of_set = (uint32_t*)(W + o_sos); X.path_base = (uint32_t*)(W + o_pb);
    X.list2 = (gf_contig*)(W + o_list2); X.n2 = d_n2;
    const unsigned g_sets = (unsigned)std::min<size_t>(n_sets, (size_t)ctx->n_cu * 4);
    const unsigned g_flat = (unsigned)std::min<size_t>(std::max<size_t>(1, (std::max(n_bytes, n_contigs) + 255) / 256), (size_t)ctx->n_cu * 8);
    GF_HIP(ctx, hipMemsetAsync(W + o_cnt, 0, 64, ctx->stream));
    GF_HIP(ctx, hipMemsetAsync(W + o_best, 0, n_sets * 8, ctx->stream));
    {
        LaunchTimer tm(ctx, GF_KERNEL_MERGE);
        hipLaunchKernelGGL(mx_prepare_kernel, dim3(g_flat), dim3(256), 0, ctx->stream, X, (char*)d_seq, (unsigned long long)n_bytes, (gf_contig*)(W + o_ctg), d_n1,
                           d_seq_len);
    }
    if ((rc = launch_merge_round(ctx, W + o_ctg, d_n1, contig_cap, d_seq, d_seq_len, seq_cap, W + o_best, n_sets, params, kmer_len_quick, max_set, nullptr,
                                 nullptr, 0, W + o_st1, nullptr, &X.R)))
        return rc;
    {
        LaunchTimer tm(ctx, GF_KERNEL_MERGE);
        hipLaunchKernelGGL(mx_count_kernel, dim3(g_sets), dim3(256), 0, ctx->stream, X);
        hipLaunchKernelGGL(mx_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, X);
        hipLaunchKernelGGL(mx_write_kernel, dim3(g_sets), dim3(256), 0, ctx->stream, X);
    }
    // the second dedup, in record order over [merged strings] + [survivors] (the round's workspace is the same carve: nothing is reallocated)
    if ((rc = launch_merge_sets(ctx, X.list2, d_n2, contig_cap, d_seq, d_seq_len, seq_cap, W + o_best, n_sets, params, W + o_st2, &X.v2))) return rc;
    {
        LaunchTimer tm(ctx, GF_KERNEL_MERGE);
        hipLaunchKernelGGL(mx_final_kernel, dim3(g_sets), dim3(256), 0, ctx->stream, X);
    }
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_merge_sets(gf_ctx* ctx, const char* seq, const uint64_t* contig_off, const uint64_t* set_off, size_t n_sets, const gf_ovl_params* params,
                  int kmer_len_quick, int max_set, const gf_mcaps* caps, gf_mset* sets, uint8_t* kept, gf_medge* edges, gf_mnew* news, uint8_t* paths,
                  char* new_seq, uint8_t* finals, uint32_t* stats) {
    if (!ctx || !params || !caps || !stats || (n_sets && (!contig_off || !set_off || !sets))) return GF_E_INVAL;
    memset(stats, 0, GF_MX_WORDS * 4);
    if (!n_sets) return GF_OK;
    const size_t n_contigs = (size_t)set_off[n_sets];
    if (set_off[0] != 0 || contig_off[0] != 0 || (n_contigs && !kept)) return GF_E_INVAL;
    for (size_t s = 0; s < n_sets; ++s) if (set_off[s] > set_off[s + 1]) return GF_E_INVAL;
    for (size_t c = 0; c < n_contigs; ++c)
        if (contig_off[c] >= contig_off[c + 1]) {
            ctx->last_error = "gf_merge_sets: contig " + std::to_string(c) + " is empty";
            return GF_E_INVAL;
        }
    const size_t n_bytes = (size_t)contig_off[n_contigs];
    if ((n_bytes && !seq) || (caps->edges && !edges) || (caps->news && !news) || (caps->path_bytes && !paths) || (caps->seq_bytes && !new_seq) ||
        (caps->finals && !finals))
        return GF_E_INVAL;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    // every buffer before the first launch (ensure() may synchronise when it has to grow one)
    const size_t seq_cap = n_bytes + caps->seq_bytes;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_seq = al(seq_cap + 64), b_co = al((n_contigs + 1) * 8), b_so = al((n_sets + 1) * 8);
    const size_t b_sets = al(n_sets * sizeof(gf_mset)), b_kept = al(n_contigs + 1), b_edges = al(caps->edges * sizeof(gf_medge) + 16),
                 b_new = al(caps->news * sizeof(gf_mnew) + 16), b_paths = al(caps->path_bytes + 16), b_fin = al(caps->finals + 16), b_stats = al(GF_MX_WORDS * 4);
    int rc;
    if ((rc = ensure(ctx, ctx->stage_in, b_seq + b_co + b_so + 64))) return rc;
    if ((rc = ensure(ctx, ctx->stage_out, b_sets + b_kept + b_edges + b_new + b_paths + b_fin + b_stats + 64))) return rc;
    uint8_t* d_seq = (uint8_t*)ctx->stage_in.p;
    uint8_t* d_co = d_seq + b_seq;
    uint8_t* d_so = d_co + b_co;
    uint8_t* d_sets = (uint8_t*)ctx->stage_out.p;
    uint8_t* d_kept = d_sets + b_sets;
    uint8_t* d_edges = d_kept + b_kept;
    uint8_t* d_new = d_edges + b_edges;
    uint8_t* d_paths = d_new + b_new;
    uint8_t* d_fin = d_paths + b_paths;
    uint8_t* d_stats = d_fin + b_fin;
    if (n_bytes) GF_HIP(ctx, hipMemcpyAsync(d_seq, seq, n_bytes, hipMemcpyHostToDevice, ctx->stream));
    GF_HIP(ctx, hipMemcpyAsync(d_co, contig_off, (n_contigs + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    GF_HIP(ctx, hipMemcpyAsync(d_so, set_off, (n_sets + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = gf_merge_sets_dev(ctx, d_seq, n_bytes, seq_cap, d_co, d_so, n_sets, n_contigs, params, kmer_len_quick, max_set, d_sets, d_kept, d_edges,
                                caps->edges, d_new, caps->news, d_paths, caps->path_bytes, d_fin, caps->finals, d_stats)))
        return rc;
    GF_HIP(ctx, hipMemcpyAsync(stats, d_stats, GF_MX_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the one synchronisation: the statistics size the download
    // bytes of merged strings behind the sets' own (required capacity whether they fitted or not)
    const unsigned long long sl = (unsigned long long)stats[GF_MX_SEQ_BYTES] | ((unsigned long long)stats[GF_MX_SEQ_BYTES + 1] << 32);
    const unsigned long long new_bytes = sl > n_bytes ? sl - n_bytes : 0;
    stats[GF_MX_SEQ_BYTES] = (uint32_t)new_bytes; stats[GF_MX_SEQ_BYTES + 1] = (uint32_t)(new_bytes >> 32);
    if (stats[GF_MX_FLAGS]) {
        ctx->last_error = "gf_merge_sets: capacity flags " + std::to_string(stats[GF_MX_FLAGS]) + " (needed: edges " + std::to_string(stats[GF_MX_EDGE_RECORDS]) +
                          ", new contigs " + std::to_string(stats[GF_MX_NEW_RECORDS]) + ", path bytes " + std::to_string(stats[GF_MX_PATH_BYTES]) +
                          ", sequence bytes " + std::to_string(new_bytes) + ", final flags " + std::to_string(stats[GF_MX_FINALS]) +
                          "; round flags " + std::to_string(stats[GF_MX_ROUND_ERR]) + ")";
        return GF_E_NOSPACE;
    }
    const size_t ne = stats[GF_MX_EDGE_RECORDS], nn = stats[GF_MX_NEW_RECORDS], np = stats[GF_MX_PATH_BYTES], nf = stats[GF_MX_FINALS];
    GF_HIP(ctx, hipMemcpyAsync(sets, d_sets, n_sets * sizeof(gf_mset), hipMemcpyDeviceToHost, ctx->stream));
    if (n_contigs) GF_HIP(ctx, hipMemcpyAsync(kept, d_kept, n_contigs, hipMemcpyDeviceToHost, ctx->stream));
    if (ne) GF_HIP(ctx, hipMemcpyAsync(edges, d_edges, ne * sizeof(gf_medge), hipMemcpyDeviceToHost, ctx->stream));
    if (nn) GF_HIP(ctx, hipMemcpyAsync(news, d_new, nn * sizeof(gf_mnew), hipMemcpyDeviceToHost, ctx->stream));
    if (np) GF_HIP(ctx, hipMemcpyAsync(paths, d_paths, np, hipMemcpyDeviceToHost, ctx->stream));
    if (nf) GF_HIP(ctx, hipMemcpyAsync(finals, d_fin, nf, hipMemcpyDeviceToHost, ctx->stream));
    if (new_bytes) GF_HIP(ctx, hipMemcpyAsync(new_seq, d_seq + n_bytes, new_bytes, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the download itself)
    for (size_t q = 0; q < nn; ++q) news[q].seq_off -= n_bytes;      // offsets into new_seq
    return GF_OK;
}

}  // extern "C"
