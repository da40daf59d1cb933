// screen_dev.hpp — what the translation units of the read screen share: the kernels' parameter blocks, the device helpers and constants
// more than one of them uses, the LDS sizes the host needs to plan a launch, and the plan itself.
//   screen.hip         plain and pipelined filter, probe geometry, plan_screen, launch_screen
//   screen_pf4.hip     256-bucket partitioned filter (pass A in three forms, pass B, resolve, list) and the probe column's producer
//   screen_verify.hip  verification of the candidates
#pragma once
#include "gf_internal.hpp"

namespace gf {

struct FilterParams {
    const uint8_t* reads;
    uint64_t n_reads;
    uint32_t rb;       // bytes per read
    uint32_t stride2;  // 2 * stride (bits between probed 16-mers)
    uint32_t first2;   // 2 * first: bit offset of the first probed 16-mer in a read (probe j sits at first + j * stride)
    uint32_t np;       // probes per read
    const uint32_t* bitmap;
    const uint32_t* sset;
    uint32_t bm_log2, s_log2;
    uint32_t* cand;
    uint32_t* n_cand;
    // LDS pre-filter variant: a coarser copy of the bitmap (bit i = OR of the 2^(bm_log2-lds_log2) bits it covers)
    const uint32_t* bitmap_lds;
    uint32_t lds_log2;
    const uint32_t* bitmap_mid;   // plain kernel: L2-resident OR-reduction of a level-1 bitmap larger than the L2 (or null)
    uint32_t mid_log2;
    uint32_t stream_policy; // pipelined kernel: cache policy of the read stream (0 default, 1 nt, 2 sc1, 3 sc0 sc1 nt)
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // LDS ops of one wave execute in order: only the compiler must not reorder
    __builtin_amdgcn_wave_barrier();
}

// a probe travels as its scrambled key p = key * S16_MUL (bijective): every bitmap index is a shift of p, and key = p * S16_MUL_INV
constexpr uint32_t mul_inverse_u32(uint32_t a) {
    uint32_t x = a;   // Newton: x <- x (2 - a x) doubles the correct low bits
    for (int i = 0; i < 6; ++i) x *= 2u - a * x;
    return x;
}
constexpr uint32_t S16_MUL_INV = mul_inverse_u32(S16_MUL);
static_assert(S16_MUL * S16_MUL_INV == 1u, "inverse of the level-1 multiplier");

__device__ __forceinline__ bool sset_walk(const FilterParams& P, uint32_t key, uint32_t sl) {
    const uint32_t smask = (1u << P.s_log2) - 1;
    for (;;) {
        const uint32_t v = P.sset[sl & smask];
        if (v == key) return true;
        if (v == EMPTY32) return false;
        ++sl;
    }
}

// Loads of the pipelined kernel and of pass A are issued through inline asm and awaited with explicit s_waitcnt: the compiler's own
// counter bookkeeping falls back to vmcnt(0) for loop-carried loads, which would drain the pipeline every step.  vmcnt
// counts vector-memory operations in issue order, so "wait until at most N are outstanding" is safe whenever at least N
// operations were issued after the awaited one; every step therefore issues the same number of loads (idle slots read a
// dummy address), and anything the compiler issues on its own only makes a wait longer, never shorter.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// global loads with a scalar base and a 32-bit per-lane byte offset
__device__ __forceinline__ void vm_load128(u32x4& d, uint32_t voff, const void* sbase) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(d) : "v"(voff), "s"(sbase));
}
__device__ __forceinline__ void vm_load128_nt(u32x4& d, uint32_t voff, const void* sbase) {
    asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(d) : "v"(voff), "s"(sbase));
}
__device__ __forceinline__ void vm_load128_sc1(u32x4& d, uint32_t voff, const void* sbase) {
    asm volatile("global_load_dwordx4 %0, %1, %2 sc1" : "=v"(d) : "v"(voff), "s"(sbase));
}
__device__ __forceinline__ void vm_load128_sc01nt(u32x4& d, uint32_t voff, const void* sbase) {
    asm volatile("global_load_dwordx4 %0, %1, %2 sc0 sc1 nt" : "=v"(d) : "v"(voff), "s"(sbase));
}
__device__ __forceinline__ void vm_load32(uint32_t& d, uint32_t voff, const void* sbase) {
    asm volatile("global_load_dword %0, %1, %2" : "=v"(d) : "v"(voff), "s"(sbase));
}
template <int N>
__device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// after a wait: uses of x are ordered behind it
__device__ __forceinline__ void vm_ready(uint32_t& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void vm_ready(u32x4& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ const void* uniform_ptr(const void* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));   // the builtin returns int
    uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    // VALU write of an SGPR -> VMEM read of it needs 5 wait states; the hazard recogniser does not look into inline asm
    uint32_t hi2 = hi;
    asm volatile("s_nop 4" : "+s"(hi2), "+s"(lo));
    return (const void*)(((uint64_t)hi2 << 32) | lo);
}
template <int LO, int HI>
__device__ __forceinline__ void vm_wait_range(uint32_t n) {   // s_waitcnt vmcnt(clamp(n, LO, HI)), n wave-uniform: the count is an immediate
    if constexpr (LO == HI) vm_wait<LO>();
    else {
        constexpr int MID = (LO + HI + 1) / 2;
        if (n >= (uint32_t)MID) vm_wait_range<MID, HI>(n); else vm_wait_range<LO, MID - 1>(n);
    }
}

// ---- partitioned filter: 256 buckets, so that a bucket's slice of the LEVEL-1 bitmap itself (2^bm_log2 / 256 bits:
// 128 KiB at 2^28) is what pass B holds in LDS — both bits of a key are tested without leaving the CU, and only the ~1 % that pass
// go on to the exact set.  (An earlier form with 16 buckets, since removed, stopped 52 % of the pairs in LDS and sent the rest to the L2
// at its random-request rate — 1.4e11/s chip-wide, DESIGN.md §4: 1.5 of its pass B's 2.2 ms.)  256 rows per WAVE were tried in round 1 (flush
// bookkeeping: 18 ms); here the unit is the WORKGROUP: sixteen waves scramble one 64-read tile each, every pair takes its rank inside
// its bucket with ONE LDS atomic on a 256-bin histogram, a scan turns the histogram into offsets, the pairs are placed in bucket
// order in LDS and leave as runs (about 16 pairs = 128 B per bucket and iteration) into the workgroup's own part of each bucket.
constexpr uint32_t PF2_NB_LOG2 = 8, PF2_NB = 1u << PF2_NB_LOG2;
constexpr uint32_t PF2_WAVES = 16, PF2_GROUP = 4;                       // waves per workgroup; probes sorted per iteration and read
constexpr uint32_t PF2_TILES = 2;                                      // 64-read tiles per wave and iteration
constexpr uint32_t PF2_BATCH = PF2_WAVES * PF2_TILES * 64 * PF2_GROUP; // 8192 pairs = 64 KiB
static_assert(PF2_WAVES > PF2_NB / 64, "waves 1..4 keep the parts' fill while wave 0 scans");
// (pass B of the 256-bucket filter queues the pairs that pass the bitmap and looks them up in the exact set 64 at a time)
constexpr uint32_t PF2_PEND = 128;   // per wave: < 64 waiting + <= 64 from one step

// ---- 256-bucket filter with 4-BYTE pairs.  8-byte (key, read) pairs (the first 256-bucket form, since removed) triple the stream (38 B of read -> + 32 B written
// + 32 B read back: 3.06 x the algorithmic bytes at C4) and both passes run at the rate the memory system moves those bytes.  What
// pass B needs of a pair: the 24 key bits below the bucket (both bitmap bits and the exact-set key derive from them) — and the read
// only for the ~0.6 % of the pairs that are in the exact set.  So an entry is  key bits << 8 | OCTET of the read inside the
// workgroup's batch (2048 reads = 256 octets of 8 consecutive reads), and the rest of the read id is recovered, exactly:
//   * which BATCH (tile iteration) a pair belongs to follows from its POSITION in the part: pass A records the part's fill before
//     every group (`fills`, staged in LDS and written as 64-byte rows: 3 % of the pair bytes), pass B searches it for the few
//     pairs that need it;
//   * which of the octet's 8 reads: pf4_resolve_kernel fetches the octet (304 contiguous bytes) and keeps the read(s) that have
//     an aligned 16-mer with this scrambled key — those are exactly the reads the pair can have come from, and each of them IS a
//     candidate (it has a seed in the exact set); the `seen` bit per read keeps one entry per read, as before.
struct Part4Params {
    FilterParams F;
    uint32_t n_writers, cap;      // parts: [bucket][writer][cap] entries
    uint32_t* pairs;              // entry = low 24 bits of the scrambled key << 8 | octet in the batch
    uint32_t* count;              // [bucket][writer]
    uint32_t* fills;              // [bucket][writer][gs]: fill of the part before group g, g = 0 .. n_groups
    uint32_t gs, n_groups, n_grp; // row stride; groups in all; groups per tile iteration
    uint32_t tiles_wg;            // tiles per workgroup and tile iteration
    uint32_t* seen;               // one bit per read
    unsigned long long* cand8;    // pairs found in the exact set: {writer << 56 | position in the part << 32 | batch octet << 24 | key bits}; ~0 = unused
    uint8_t* chunk_b;             // bucket of every PF4_CHUNK entries of that list
    uint32_t* n_cand8;
    uint32_t cap8;
    // Chance candidates: a 16-mer seed against 1.1e7 flank 16-mers lets 0.5 % of the probes through by chance.  The probes are
    // therefore spaced for (16 + ext)-base seeds — ext <= 2 bases to the right of the 16-mer, as many as leave the probe count
    // unchanged — and what stands next to the 16-mer in the flanks rides along with the exact set (FlankIndex::d_sgrp): pass B gets
    // it in the request that answers the look-up and forwards it (`cand8x`), the resolve step — the read is in LDS there — drops
    // the pair when the read's own neighbours are none of the flanks' (each base divides the chance rate by 4).
    const uint32_t* sgrp;         // grouped exact set {key x 4, ext x 4}
    uint32_t ext;                 // bases checked next to the seed (0: none)
    uint32_t* cand8x;             // per list entry: the ext word of the pair's 16-mer
    const uint32_t* probes;       // pass A's column form: the library's probe column, `plane` words per probe
    uint64_t plane;
    // pass A alone, for a library's resident parts (launch_parts_build): no gaps, so a pair that finds its part full has nothing to be
    // tested against — it is counted here and skipped, and the caller keeps no parts.  Null: a screen (the pair is tested on the spot).
    uint32_t* spills;
};
constexpr uint32_t PF4_OBUF = 80;     // list entries buffered per wave of pass B (8 + 4 bytes each)
// the pair's key in the grouped exact set, from group g on: found -> its ext word
__device__ __forceinline__ bool pf4_sgrp_walk(const Part4Params& Q, uint32_t key, uint32_t g, uint32_t& ext) {
    const uint32_t gmask = (1u << (Q.F.s_log2 - 2)) - 1;
    for (;;) {
        const uint32_t* G = Q.sgrp + (size_t)(g & gmask) * 8;
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t v = G[j];
            if (v == key) { ext = G[4 + j]; return true; }
            if (v == EMPTY32) return false;
        }
        ++g;
    }
}
constexpr uint32_t PF4_CHUNK = 256;   // entries of the pair list a wave of pass B reserves at a time
constexpr uint32_t PF4_STAGE = 16;   // groups of fill history staged in LDS (one 64-byte row per bucket and flush)
// LDS of pf4_scatter_kernel (unaligned runs): the filter is taken only where this form fits, the whole-line form is chosen on top of it
constexpr size_t pf4_scatter_lds_bytes(size_t slice_words) {
    return (size_t)PF2_WAVES * PF2_TILES * slice_words * 4 + (size_t)PF2_BATCH * 5 + (size_t)PF2_NB * (PF4_STAGE + 1) * 4 + (6 * PF2_NB + 8) * 4;
}
constexpr size_t pf4_slice_words(uint32_t rb) { return ((size_t)64 * rb + 16 + 7) / 8 * 2; }   // a staged 64-read tile + pad, in words
constexpr uint32_t PF4_LINE = 32;
constexpr uint32_t pf4_stage_of(uint32_t G) { return G >= 4 ? 8u : 16u; }   // groups of fill history staged in LDS (what fits beside the lines)
constexpr size_t pf4_lines_lds_bytes(size_t slice_words, uint32_t G) {
    return ((size_t)PF2_WAVES * slice_words + (size_t)G * PF2_WAVES * PF2_TILES * 64 + 2 * PF2_NB * PF4_LINE + PF2_NB * (pf4_stage_of(G) + 1) +
            3 * PF2_NB + 2 * PF2_NB + 4 * PF2_NB + 2 * (PF2_NB + (size_t)G * PF2_WAVES * PF2_TILES * 64 / PF4_LINE) + 8) * 4;
}

struct VerifyParams {
    const uint32_t* reads32;  // packed reads viewed as little-endian words
    uint64_t n_words;         // whole words of the packed array
    uint32_t tail_bytes;      // bytes after the last whole word (0..3)
    const uint32_t* nmask;    // may be null
    uint32_t rb, read_len, k, nmw;
    const uint32_t* cand;
    const uint32_t* n_cand;
    const uint4* table;       // k <= 32: one uint4 per slot {hi.lo32, hi.hi32, gap, 0}; k > 32: two {hi, lo}, {gap,0,0,0}
    uint32_t t_log2;
    uint32_t min_hits;
    uint32_t list_cap;
    gf_hit* out;
    uint32_t cap;
    uint32_t* n_out;
    // window gate: the exact canonical-16-mer set and the filter's probe geometry (sset null = gate off)
    const uint32_t* sset;
    uint32_t s_log2, stride, np, first;   // probed 16-mers: read offsets first + j * stride, j < np
    uint32_t batch;          // candidates per wave and pass (<= 64)
    // seed-and-extend kernel: occurrence lists and packed flanks (index.hip)
    const uint32_t* sval;
    const uint32_t* occ;
    const uint32_t* fpk;
    const uint32_t* foff;
    uint32_t* overflow;      // counter: candidates whose (position, gap) list exceeded list_cap
    uint32_t* overflow_list; // their read ids (re-verified by a second launch with a large list), or null
    uint32_t vlist;          // seed-and-extend kernel: gap entries per candidate (VEXT_LIST / VEXT_LIST_BIG)
    uint32_t n_occ;          // entries of the occurrence lists in all
    gf_hit* stage;           // seed-and-extend kernel: VEXT_STAGE hits per workgroup, collected before they join the hit list
};

// ---- host side: the plan of one screen call --------------------------------------------------------------------------------------------
// plan_screen (screen.hip) alone decides which form the filter takes, its probe geometry and every launch number that follows from them.
// launch_screen launches what the plan says, and fill_probe_geom answers gf_probe_geom::use from the same plan: a column is wanted
// exactly where the screen would stream it.
enum class ScreenForm {
    plain,       // screen_filter_kernel: no LDS level
    pipe,        // screen_filter_pipe_kernel: coarse bitmap in LDS, software-pipelined
    pf4_runs,    // 256-bucket partitioned filter, pass A stores unaligned runs (pf4_scatter_kernel)
    pf4_lines    // ... pass A stores whole lines (pf4_scatter_lines_kernel, or pf4_scatter_col_kernel from a probe column)
};
struct PipeKernel;   // screen.hip: one instantiation of the pipelined kernel and its printed name
struct ScreenPlan {
    ScreenForm form;
    bool col_ok;             // whole lines, all probes of a read in one group, rows not forced (screen_variant 18): pass A may stream a probe column
    uint32_t rb;             // bytes per packed read
    ProbeSpots pg;           // the probed 16-mers, for the filter and the verification
    bool bytes;              // every probe starts at a byte boundary
    // pipelined form
    const PipeKernel* pipe;  // the instantiation for (nch, npt, exact)
    uint32_t nch, npt, nw;   // 16-byte chunks per lane and tile; probes per read, unrolled; waves per workgroup
    bool exact;              // a read has exactly npt probes
    unsigned pipe_grid;
    size_t pipe_slice_words, pipe_lds_bytes;
    // partitioned form (the fields of Part4Params of the same names)
    uint32_t grp, n_grp;     // probes per sorted group; groups per tile iteration
    uint32_t n_writers, tiles_wg, cap, cap8, gs, n_groups;
    uint64_t plane;          // words per plane of a probe column
    size_t slice_words;      // a staged 64-read tile + pad, in words
    size_t lds_a, lds_a_col; // pass A's LDS bytes: from the rows / from a column
    // its workspace: `count` at 0, then the blocks at these byte offsets; zero_bytes from o_n_cand8 are cleared before pass A (the list counter and `seen`).
    // The fill history and the pairs come last: a screen from a library's resident parts needs the workspace up to o_fills only.
    size_t o_n_cand8, o_seen, o_fills, o_cand8, o_cand8x, o_chunk_b, o_pairs, ws_bytes, ws_bytes_resident, zero_bytes;
};
ScreenPlan plan_screen(const gf_ctx* ctx, const FlankIndex& ix, size_t n_reads, int read_len);   // n_reads < 2^32; no HIP call, nothing written

// A library's RESIDENT PARTS (gf_screen_parts_geom): pass A's output in one caller-owned buffer [count | fills | pairs], the pairs followed
// by the 64 words pass A's idle lanes store to.  Nothing in it depends on the gaps.
struct PartsLayout { size_t o_fills, o_pairs, bytes; };
inline PartsLayout parts_layout(uint32_t n_writers, uint32_t cap, uint32_t gs) {
    PartsLayout L;
    L.o_fills = ((size_t)PF2_NB * n_writers * 4 + 255) & ~(size_t)255;
    L.o_pairs = L.o_fills + (size_t)PF2_NB * n_writers * gs * 4;
    L.bytes = L.o_pairs + (size_t)PF2_NB * n_writers * cap * 4 + 64 * 4;
    return L;
}
// the plan whose pass A fills / whose passes B.. read a library's parts, and whether parts are kept at all (g->use); ix: as fill_probe_geom
ScreenPlan fill_parts_geom(gf_ctx* ctx_or_null, const FlankIndex* ix_or_null, size_t n_reads, int read_len, int k, gf_screen_parts_geom* g);

// the filter of a planned screen from the partitioned form (screen_pf4.hip); d_probes: a column valid for this call, or null (the rows);
// d_parts: resident parts valid for this call (pass A is then not launched: passes B, resolve and list read them and write none of it), or null
int launch_filter_pf4(gf_ctx* ctx, const FlankIndex& ix, const ScreenPlan& S, const FilterParams& F, const void* d_probes, const void* d_parts);
// pass A of plan S alone into d_parts (parts_layout); F: the reads and the probe geometry, nothing of an index; spills: device counter
int launch_pass_a_build(gf_ctx* ctx, const ScreenPlan& S, const FilterParams& F, const void* d_probes, void* d_parts, uint32_t* spills);
// candidates (ctx->cand, counted in ctx->counters) -> hits (screen_verify.hip)
int launch_verify_passes(gf_ctx* ctx, const FlankIndex& ix, const ProbeSpots& pg, const void* d_reads, const void* d_nmask, size_t n_reads,
                         int read_len, int min_hits, void* d_out, size_t cap, void* d_n_out);

}  // namespace gf
