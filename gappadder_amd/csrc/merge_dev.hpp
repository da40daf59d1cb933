// merge_dev.hpp — what the kernels of the contig-merge round (merge.hip) share with the export of its graph (merge_export.hip):
// the round's limits, the words of its statistics, the parameter block of its kernels and the block scan
#pragma once
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t OV_MAXLEN = 8190;   // bases of a node of the overlap kernel (its LDS diagonals)

constexpr uint32_t MG_MAX_IN = 1024;      // contigs of an open gap that the dedup takes (more: the gap is left alone, counted in stats[MG_SKIPPED])
constexpr uint32_t MG_MAX_NODES = 256;    // nodes of a set (2 x max_set)
constexpr uint32_t MG_MAX_EDGES = 4096;   // edges of one set's graph
constexpr uint32_t MG_MAX_PATHS = 2048;   // paths of one set before the twin removal
constexpr uint32_t MG_PATH_BYTES = 1u << 17;   // their nodes (bytes) per workgroup
constexpr uint32_t MG_MIN_NODE = 30, MG_MAX_NODE = OV_MAXLEN;
constexpr uint32_t MG_PER_ROOT = 21;      // MAX_CONTIG_IN_PATH_COUNT + 1 (ContigsCompactor.cpp:34; MergeContigs.find_paths)
enum { MG_N_PRE = 0, MG_N_SETS = 1, MG_SKIPPED = 2, MG_N_PAIRS = 3, MG_QC_FLAGS = 4, MG_N_JOBS = 5, MG_ERR = 6, MG_N0 = 7, MG_N_EDGES = 8,
       MG_SETS_WITH_JOBS = 9, MG_Q_JOBS = 10, MG_Q_SETS = 11, MG_JOB_NODES = 12, MG_Q_DEDUP = 13, MG_Q_COPY = 14, MG_N_NODES = 15, MG_SKIPPED_GRAPH = 16,
       MG_WORDS = 32 };
// error bits: capacities of this call (the caller sizes them: raise).  A set whose GRAPH outgrows the round's own limits — more than
// MG_MAX_EDGES edges, MG_MAX_PATHS paths or MG_PATH_BYTES path nodes (the contig graph of a repeat-bearing gap has thousands of paths) —
// is left alone and counted in stats[MG_SKIPPED_GRAPH], like the sets of more than max_set contigs in stats[MG_SKIPPED]
constexpr uint32_t MG_E_SEQ = 1, MG_E_PAIRS = 2, MG_E_CONTIGS = 32, MG_E_OUTSEQ = 64;
constexpr uint32_t MG_SETS_NO_MAX_SET = 0;   // max_set of MG_MODE_SETS: the dedup alone, no set limit applies

struct MgJob { uint32_t set, off, len; };   // path = job_nodes[off .. off + len)

struct MgParams {
    gf_contig* contigs;
    uint32_t* n_contigs;
    uint32_t contig_cap;
    char* seq;
    unsigned long long* seq_len;
    unsigned long long seq_cap;
    const unsigned long long* gap_best;
    uint32_t n_gaps, max_set;
    uint32_t* stats;
    // workspace
    uint32_t* cnt;          // [n_gaps] contigs of an open gap, later the fill cursor
    uint32_t* pre_of_gap;   // [n_gaps]
    uint32_t* pre_gap;      // [n_gaps]
    uint32_t* pre_off;      // [n_gaps + 1]
    uint32_t* ids;          // [contig_cap]
    uint32_t* kept_n;       // [n_gaps] contigs left by the dedup
    uint32_t* node_n;       // [n_gaps] ... of node length
    unsigned long long* node_bytes;   // [n_gaps]
    uint32_t* set_pre;      // [n_gaps]
    unsigned long long* set_base;     // [n_gaps] first byte of the set in mseq
    unsigned long long* contig_off;   // [node_cap + 1]
    unsigned long long* set_off;      // [n_gaps + 1]
    uint32_t node_cap;
    char* mseq;
    unsigned long long mseq_cap;
    // graph + paths
    const gf_qcpair* pairs;
    const gf_ovl_result* res;
    uint32_t pair_cap;
    const uint32_t* set_range;        // [2 * set]
    uint8_t* path_ws;                 // per workgroup: MG_PATH_BYTES of path nodes
    int32_t* dp_dist;                 // per workgroup: [MG_MAX_NODES roots][MG_MAX_NODES]
    uint8_t* dp_pred;                 // ... pred, and 1 byte of flags (bit 0 reached, bit 1 ends with its node twice)
    uint8_t* dp_flag;
    MgJob* jobs;
    uint32_t job_cap;
    uint8_t* job_nodes;
    uint32_t job_node_cap;
    uint32_t* set_jobs;               // [2 * set]: first job, jobs
    uint32_t* set_rec;                // [set]: contig record of the set's first job
    char* cur_ws;                     // per workgroup: 2 x 16 384 bytes (the running string and its successor)
    gf_ovl_params pr;
    // order of a gap's contigs = the order of its contigs.fa (assemble_gaps.py:124-135): the (k, kv) pairs in list order, inside a pair by
    // (length descending, sequence) — n_k > 0; n_k == 0: record order (contig index)
    uint32_t n_k;
    uint16_t k_list[16], kv_list[16];
    // the rescue round's two uses of these kernels (gf_merge_rescue_dev, gf_rescue_bridges_dev; MG_MODE_*): which records take part,
    // and where the rescue set's marker records (k = kv = GF_RESCUE_MARK, the bridges) stand in a gap's order
    uint32_t mode;
    const uint32_t* gap_bridges;      // [n_gaps] bridges per gap (MG_MODE_RESCUE: a gap without one takes no part)
    const uint32_t* merge_n0;         // the first merge round's first record (its stats[MG_N0]) ...
    const uint32_t* rescue_first;     // ... and the first bridge: [*merge_n0, *rescue_first) = the first merge's records, no part of the rescue set    // the export of the round's graph (gf_merge_sets_dev, merge_export.hip), or null: [set] 1 = left alone for its graph's size;
    // [job] nodes of the path that were merged (fewer than the path has: the running string outgrew the overlap kernel)
    uint32_t* x_graph;
    uint32_t* x_used;
};

__device__ __forceinline__ uint32_t mg_block_scan_excl(uint32_t v, uint32_t* s_w, uint32_t* total) {   // blockDim.x a multiple of 64, <= 1024
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if ((int)lane >= d) x += y;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t q = 0; q < (blockDim.x >> 6); ++q) { const uint32_t t = s_w[q]; if (q < w) base += t; tot += t; }
    *total = tot;
    return base + x - v;
}

// merge.hip: the round's launches on the context's stream.  `exported` (or null): receives the parameter block — the round's workspace,
// valid until the next merge call on the stream — and makes the kernels fill x_graph / x_used
int launch_merge_round(gf_ctx* ctx, void* d_contigs, void* d_n_contigs, size_t contig_cap, void* d_seq, void* d_seq_len, size_t seq_cap,
                       const void* d_gap_best, size_t n_gaps, const gf_ovl_params* params, int kq, int max_set, const int* k_list, const int* kv_list,
                       int n_k, void* d_stats, const MgRescueArgs* rs, MgParams* exported);

}  // namespace gf
