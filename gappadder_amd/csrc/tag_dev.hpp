// tag_dev.hpp — what the tagger's units share: the kernels' parameter blocks, the per-wave hit buffer and the wave-queue push, the queue
// records and sizes, the LDS budget, and the launch plan.  tagger.hip: tag_kernel and its launch; tag_map.hip: the key columns and the bin
// maps; tag_low.hip: the second hop's look-up.
#pragma once
#include "gf_internal.hpp"

namespace gf {

struct TagParams {
    const gf_alnrec* recs;
    uint32_t dbg;             // diagnostics (option tag_dbg; results change): 1 no MAPQ-0 by-product, 2 no bin test (nothing passes), 4 candidates dropped unsifted
    const uint2* keys;        // KEYS variants: {pos, ref | (mapq == 0) << 31} per record (gf_alnrec_keys_dev), n + 1 entries
    uint64_t n;
    const gf_gap* gaps;
    const uint32_t* scaf_off;
    uint32_t n_scaffolds;
    int32_t dist1, dist2, clip_dist, anchor_mapq;
    int32_t short_is;
    // coarse bin map: bit (bin_off[s] + (POS >> bin_shift)) is set iff some window of scaffold s touches that bin
    const uint32_t* bin_bits;
    const uint32_t* bin_off;  // n_scaffolds + 1
    const uint32_t* bin_first; // per bin: index of the first gap (of the scaffold) whose right window reaches the bin's first position
    uint32_t bin_shift, bin_words;
    uint32_t off_words;       // > 0: the n_scaffolds + 1 offsets follow the bits in the staged LDS copy as well
    // fine bin map (global, L2-resident, <= 4 MiB): same test on narrower bins for the records the LDS map lets through.
    // Only built when the LDS map's bins are wide (large genomes, many gaps); null otherwise.
    const uint32_t* fine_bits;
    const uint32_t* fine_off;
    uint32_t fine_shift;
    gf_taghit* out;
    uint32_t cap;
    uint32_t* n_out;
    // optional by-product for the second hop: every MAPQ==0 record as {pos, ref, record index}
    gf_lowrec* low;
    uint32_t low_cap;
    uint32_t* n_low;
    gf_lowrec* low_stage;     // LOWSTAGE entries per wave of the launch: where a wave collects its MAPQ==0 records (see flush_low)
    // LIN variants: the linear key column (gf_alnrec_linkeys_dev) — base[ref] + pos per record, 0xFFFFFFFF where the record takes no part —,
    // and its MAPQ-0 bit plane (8 words per 256 records).  The maps are then indexed by key >> shift: n_bins / fine_bins bins, bin_first per
    // bin of the line, and bin_off holds the layout's base[] (n_scaffolds + 1 words; staged behind the bits when off_words > 0).
    const uint32_t* lin_keys;
    const uint32_t* lin_plane;
    uint64_t lin_units;       // 16-byte units of the column that hold a record: (n + 3) / 4
    uint32_t plane_words, n_bins, fine_bins;
};

// (gf_internal.hpp: HOP_NEAR_LOG2, HOP_NEAR_SHIFT, hop_near_bit)
struct LowParams {
    const gf_alnrec* recs;     // full records ...
    uint64_t n;
    const gf_lowrec* low;      // ... or the compacted MAPQ==0 list with its device-side count
    const uint32_t* n_low;
    uint32_t low_cap;
    const uint32_t* upos;      // unique (scaffold-grouped) mate positions, ascending inside a scaffold
    const uint32_t* urow;      // n_unique+1 offsets into the row table
    const uint32_t* scaf_off;  // n_scaffolds+1 offsets into upos
    uint32_t n_scaffolds;
    gf_taghit* out;
    uint32_t cap;
    uint32_t* n_out;
    const uint32_t* near_bits; // optional (hop.hip): bit hop_near_bit(scaffold, pos >> 9) is set for every pos a table row lies near — see low_mapq_compact_kernel
};

// Records are streamed as whole 1-KiB wave loads (16 B per lane, consecutive lanes = consecutive 16-B halves):
// the even lane of a pair holds {pos, mate_pos, tlen, ref}, the odd lane {mate_ref, flag|mapq|clip, read id}.
// Two loads = 64 records; lane L gathers record L's fields from the lanes that hold its halves (tag_kernel).
struct LiveRec { uint32_t pos, ref, mate_ref, meta; int32_t tlen; uint32_t rec; };   // a record that passed the bin map
constexpr uint32_t LIVEQ = 96;   // per wave: < 64 waiting + what one step adds (a step that would overflow it drains first)
// With a second, finer map in global memory (human scale) the records that pass the LDS map (a twentieth) are not looked up in it on
// the spot — nearly every 1-KiB step has such a lane, and the whole wave then waits for two dependent global loads (PMC: waves wait
// 79 % of their cycles in a kernel that only streams) — but queued with 12 bytes each and sifted 64 at a time; the few that pass
// load their record again and join the queue of the window search.
struct CandRec { uint32_t pos, ref, rec; };
struct CandLin { uint32_t lin, rec; };   // the linear key column's: the key is (scaffold, position) in one word
constexpr uint32_t CANDQ = 96;
constexpr uint32_t LOWBUF = 64;       // MAPQ==0 records a wave collects in LDS (tag_kernel: flush_low)
constexpr uint32_t LOWSTAGE = 1024;   // MAPQ==0 records a wave collects before it appends them to the list
constexpr int TAG_UNROLL = 8;  // 8 KiB (256 records) per wave and stage, two stages in flight

__device__ __forceinline__ void tag_wave_sync() {   // LDS hand-off between lanes of ONE wave (in-order LDS: compiler fence only)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The push every per-wave queue of the tagger is filled by: the lanes that `want` append `value` to queue[0 .. n) in lane order (ballot +
// prefix count, no LDS atomic: n is wave-uniform), after make_room() where the step would pass `cap` (make_room leaves n where one step
// fits).  False when no lane wanted.  The caller orders the LDS hand-off (tag_wave_sync) and empties a queue that holds a full wave.
template <typename T, typename MakeRoom>
__device__ __forceinline__ bool wave_push(bool want, const T& value, T* queue, uint32_t& n, uint32_t cap, MakeRoom&& make_room) {
    const unsigned long long bal = __ballot(want);
    if (!bal) return false;
    const uint32_t cnt = (uint32_t)__popcll(bal);
    if (n + cnt > cap) make_room();
    if (want) queue[n + __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1))] = value;
    n += cnt;
    return true;
}

// A single global counter serialises returning atomics at ~11 ns each (MI355X_MICROARCH.md "dequeue"/"fanin" rows), so hits are
// collected in an LDS buffer per WAVE (wave_push: the fill is wave-uniform) that leaves with one global
// atomic per 33-96 hits.  (Rounds 1-3 kept one buffer per workgroup, flushed once when the kernel ended, with direct global appends
// once it was full: at human scale a workgroup finds 10 000-25 000 hits, so nearly every hit took that fall-back — 600 000
// returning atomics per launch of the long-insert library, 6 of its 12 ms.)
constexpr uint32_t WHCAP = 96;   // < 33 waiting + <= 64 from one step
struct WaveHits {
    gf_taghit* h;     // this wave's WHCAP entries (LDS)
    uint32_t n;       // wave-uniform
};
__device__ __forceinline__ void flush_wave_hits(WaveHits& w, gf_taghit* out, uint32_t cap, uint32_t* n_out) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t gb = 0;
    if (lane == 0) gb = atomicAdd(n_out, w.n);
    gb = __shfl(gb, 0);
    for (uint32_t i = lane; i < w.n; i += 64)
        if (gb + i < cap) out[gb + i] = w.h[i];
    w.n = 0;
    tag_wave_sync();
}
__device__ __forceinline__ void emit_hit(bool want, const gf_taghit& h, WaveHits& w, gf_taghit* out, uint32_t cap, uint32_t* n_out) {
    if (!wave_push(want, h, w.h, w.n, WHCAP, [&] { flush_wave_hits(w, out, cap, n_out); })) return;
    tag_wave_sync();
    if (w.n > WHCAP - 64) flush_wave_hits(w, out, cap, n_out);
}
// one GF_KIND_LOWMAPQ hit of record `rec` per table row in [row, row_end): how both second-hop kernels end (lanes without rows idle along)
__device__ __forceinline__ void emit_rows(uint32_t row, uint32_t row_end, uint32_t rec, WaveHits& w, gf_taghit* out, uint32_t cap, uint32_t* n_out) {
    while (true) {
        const bool more = row < row_end;
        if (!__any(more)) break;
        gf_taghit hit;
        hit.rec = rec; hit.gap = row; hit.kind = GF_KIND_LOWMAPQ; hit.to_mate = 0;
        emit_hit(more, hit, w, out, cap, n_out);
        if (more) ++row;
    }
}

// static LDS of tag_kernel<16, ..., FINEQ = true>: hit buffers, MAPQ-0 buffers, the two queues (+ alignment slack)
constexpr size_t TAG16_STATIC_LDS = 16 * (WHCAP * sizeof(gf_taghit) + LOWBUF * sizeof(gf_lowrec) + LIVEQ * sizeof(LiveRec) + CANDQ * sizeof(CandRec)) + 64;
constexpr size_t TAG_LDS_BYTES = 160 * 1024, TAG_MAP_4WAVE_BYTES = 32 * 1024;   // a CU's LDS; the largest map four 4-wave workgroups per CU stage
static_assert(TAG16_STATIC_LDS + 64 * 1024 + 2049 * 4 <= TAG_LDS_BYTES, "tag_kernel<16>: queues + a 64-KiB bin map + 2 049 scaffold offsets must fit a CU's LDS");

// workgroups of 256 threads for a stream of n elements: eight per CU at the most
inline unsigned stream_grid(int n_cu, size_t n) {
    size_t blocks = (n + 255) / 256;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(blocks, (size_t)n_cu * 8));
}

// What launch_tag launches (tagger.hip: plan_tag), from the facts of the call alone — no HIP call.
enum TagForm { TAG_RECORDS = 0, TAG_KEYS8 = 1, TAG_LINEAR = 2 };   // the stream: 32-byte records, 8-byte keys, 4-byte linear keys (gf_tag_last_launch)
struct TagPlan {
    int rc;               // GF_OK, or GF_E_UNSUPPORTED: the map fits no CU's LDS beside the queues
    int form;             // TagForm
    int kernel;           // index into TAG_KERNELS (tagger.hip)
    bool fine;            // the map has a fine map behind it
    uint32_t nw;          // waves per workgroup
    unsigned grid;
    uint32_t off_words;   // TagParams::off_words
    size_t lds_bytes;     // dynamic LDS: the staged map (and offsets)
};
TagPlan plan_tag(size_t n, uint32_t map_words, bool fine, uint32_t n_scaffolds, int n_cu, bool light, bool keys_given, bool lin);

}  // namespace gf
