// tagger.hip — alignment-record tagging.
//
// tag_kernel restates GapReadsCollector.parse_reads_fall_in_gaps_one_scaffold / _short_is
// (collect_reads_for_gaps.py:68-163 / :166-263) on decoded 32-byte records; the reference's per-position dict
// `focal_region` (get_focal_region_of_scaffold_v2, :31-65) becomes a closed-form window test per gap:
//   left  window: 0 <= start-POS < dist2  (keys start-i, i in range(dist2), start-i >= 0; 'c' if i <= clip_dist)
//   right window: 0 <= POS-end   < dist2  (keys end+i)
// This file: tag_kernel, its launch plan and its launch.  The key columns and the bin maps: tag_map.hip; the second hop's look-up
// (low_mapq_kernel): tag_low.hip; what the three share: tag_dev.hpp.
#include <type_traits>

#include "tag_dev.hpp"

namespace gf {

// NW waves per workgroup.  BINS_LDS: the coarse bin map is staged in LDS (the stand-alone form: 33 KiB of LDS per workgroup at
// human scale); BINS_LDS = false reads it through L1/L2 instead and runs one-wave workgroups with ~6 KiB of LDS, so that the
// tagger's workgroups fit on the CUs NEXT TO the k-mer filter's (which own 137-151 KiB of every CU's LDS but leave most of its
// issue slots idle: PMC SQ_WAIT_ANY 53-77 %) — the "light" variant a pipeline launches on its second stream.
// KEYS: the stream is the 8-byte KEY COLUMN of the records — {pos, ref | (mapq == 0) << 31}, built once at ingest — instead of the 32-byte
// records themselves: 99 % of the records are decided by (scaffold, position) alone, and the by-product needs one more bit; the full record is
// fetched only for what passes the bin maps (the path the fine-map queue already had).  A quarter of the bytes per record for the stream.
// LIN (with KEYS): the stream is the 4-byte LINEAR key column — base[ref] + pos, the scaffolds laid end to end on granule boundaries no bin
// crosses — and the MAPQ-0 bit comes from a bit plane: half the bytes per record again, and the bin test is one LDS read of bins[key >> shift]
// without the two per-scaffold offsets.  A candidate waits as {key, record}; (scaffold, position) come back with the 32-byte record for what
// passes, and for the MAPQ-0 by-product (2 % of the records) from a search of base[], made 64 entries at a time when the LDS buffer leaves.
// FORM (TagForm) names the stream; FINEQ: the records form's candidate queue in front of a fine map (the key forms always queue).
template <int NW, bool BINS_LDS, bool FINEQ, int FORM>
__global__ __launch_bounds__(64 * NW) void tag_kernel(TagParams P) {
    constexpr bool KEYS = FORM != TAG_RECORDS, LIN = FORM == TAG_LINEAR;
    static_assert(!KEYS || BINS_LDS, "a key column is tested against the staged map");
    constexpr bool CQ = FINEQ || KEYS;   // records that pass the LDS map wait in the candidate queue (fine map, then the record's fetch)
    using Cand = std::conditional_t<LIN, CandLin, CandRec>;
    extern __shared__ uint32_t bins_lds[];  // the whole bin map (16 or 64 KiB), staged once per workgroup
    __shared__ gf_taghit whits[NW][WHCAP];
    __shared__ LiveRec liveq[NW][LIVEQ];
    __shared__ Cand candq[CQ ? NW : 1][CQ ? CANDQ : 1];
    // MAPQ==0 records (2 % of a library) leave through ONE counter, and returning atomics on one address are served at ~11-15 ns
    // each: flushing a 64-entry LDS buffer per wave straight to the list, the 900 M records of C4 needed 360 000 of them — 4 of the
    // kernel's 5.2 ms; the stream ran at 4.9 instead of 6.0 TB/s.  The LDS buffer (whole 768-byte runs: single 12-byte stores left
    // partial lines in L2) now empties into the wave's private slice of a global staging buffer, without an atomic, and the slice
    // moves to the list 1 000 records at a time: a twentieth of the atomics.
    __shared__ gf_lowrec lowbuf[NW][LOWBUF];
    uint32_t low_n = 0, stage_n = 0;    // wave-uniform: records in the LDS buffer, in the staging slice
    WaveHits hb{whits[threadIdx.x >> 6], 0};
    if (BINS_LDS) for (uint32_t i = threadIdx.x; i < P.bin_words + P.off_words; i += blockDim.x) bins_lds[i] = P.bin_bits[i];   // (bits, then offsets: one array)
    const uint32_t* bins = BINS_LDS ? bins_lds : P.bin_bits;
    const uint32_t* boff = BINS_LDS && P.off_words ? bins_lds + P.bin_words : P.bin_off;   // (LIN: base[], not bit offsets)
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    // (LIN: the wave's number as a value the compiler knows to be wave-uniform, so that what derives from it stays out of the vector registers)
    const uint64_t wave = LIN ? (uint64_t)blockIdx.x * NW + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))
                              : ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    gf_lowrec* const wlow = lowbuf[threadIdx.x >> 6];
    gf_lowrec* const wstage = P.low ? P.low_stage + wave * LOWSTAGE : nullptr;
    auto flush_stage = [&]() {
        uint32_t gb = 0;
        if (lane == 0) gb = atomicAdd(P.n_low, stage_n);
        gb = __shfl(gb, 0);
        const uint32_t fit = gb < P.low_cap ? (stage_n < P.low_cap - gb ? stage_n : P.low_cap - gb) : 0;
        // the wave reads its own stores back from L2 (a store is acknowledged once it is there; the loads bypass the CU's L1,
        // which may still hold the slice as the previous flush read it)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(wstage);
        uint32_t* dst32 = reinterpret_cast<uint32_t*>(P.low + gb);
        for (uint32_t i = lane; i < 3 * fit; i += 64) dst32[i] = __hip_atomic_load(src32 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stage_n = 0;
    };
    auto flush_low = [&]() {   // LDS buffer -> staging slice
        if (stage_n + low_n > LOWSTAGE) flush_stage();
        if constexpr (LIN) {
            // the buffer holds {key, -, record}: the scaffold is the last one whose base is <= key (empty scaffolds share their base with
            // the next one and are stepped over), one search per entry with every lane of the flush at work
            tag_wave_sync();
            if (lane < low_n) {
                const gf_lowrec e = wlow[lane];
                uint32_t lo = 0, hi = P.n_scaffolds;          // invariant: base[lo] <= key, base[hi] > key (the line ends above every key)
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (boff[mid] <= e.pos) lo = mid; else hi = mid;
                }
                wlow[lane] = gf_lowrec{e.pos - boff[lo], lo, e.rec};
            }
            tag_wave_sync();
        }
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(wlow);
        uint32_t* dst32 = reinterpret_cast<uint32_t*>(wstage + stage_n);
        for (uint32_t i = lane; i < 3 * low_n; i += 64) dst32[i] = src32[i];
        stage_n += low_n;
        low_n = 0;
    };
    // ---- per-wave queue of records that passed the bin map
    LiveRec* wlive = liveq[threadIdx.x >> 6];
    uint32_t live_n = 0;   // wave-uniform
    auto drain = [&]() {   // window search + tagging of the last min(64, live_n) queued records, one per lane
        const uint32_t base = live_n > 64 ? live_n - 64 : 0;
        bool live = base + lane < live_n;
        gf_alnrec r = {};
        uint32_t rec = 0, g = 0, g_end = 0;
        if (live) {
            const LiveRec q = wlive[base + lane];
            r.pos = q.pos; r.ref = q.ref; r.tlen = q.tlen; r.mate_ref = q.mate_ref;
            r.flag = (uint16_t)(q.meta & 0xFFFF); r.mapq = (uint8_t)((q.meta >> 16) & 0xFF); r.clipflag = (uint8_t)(q.meta >> 24);
            rec = q.rec;
            g_end = !LIN || r.ref < P.n_scaffolds ? P.scaf_off[r.ref + 1] : 0;
            // the first gap whose right window reaches the record's BIN (one load; the map's third part) — gaps between it and the first
            // one whose window reaches POS itself (end + dist2 > pos; two gaps within one bin) fall through the walk below untagged
            if constexpr (LIN) {
                // (the fetched record says where it lies; a record that does not belong to the column it was listed from finds no bin)
                const uint32_t bi = r.ref < P.n_scaffolds ? (boff[r.ref] + r.pos) >> P.bin_shift : P.n_bins;
                if (bi < P.n_bins) g = P.bin_first[bi]; else g = g_end = 0;
            } else
            g = P.bin_first[boff[r.ref] + (r.pos >> P.bin_shift)];
        }
        const int64_t pos = r.pos;
        // walk the (few) gaps whose windows can contain POS; lanes without work idle through the ballots.  The first two gaps are
        // loaded together (the walk ends at the first gap whose left window starts behind POS: as a rule the second one), so the
        // common walk is two dependent round trips — bin -> first gap, gaps — instead of four
        gf_gap gq[2] = {};
        if (live && g < g_end) gq[0] = P.gaps[g];
        if (live && g + 1 < g_end) gq[1] = P.gaps[g + 1];
        for (uint32_t it = 0;; ++it) {
            gf_gap gp = it == 0 ? gq[0] : gq[1];
            if (it >= 2 && live && g < g_end) gp = P.gaps[g];
            const bool more = live && g < g_end && (int64_t)gp.start - P.dist2 < pos;
            live = more;          // (a lane whose walk has ended stays out: every lane still walking is at its first gap + it)
            if (!__any(more)) break;
            bool clip = false, pair = false, unmap = false;
            if (more) {
                const int64_t il = (int64_t)gp.start - pos, ir = pos - (int64_t)gp.end;
                int tag = -1;  // 0: 0c, 1: 0d, 2: 1c, 3: 1d
                if (il >= 0 && il < P.dist2) tag = il <= P.clip_dist ? 0 : 1;
                else if (ir >= 0 && ir < P.dist2) tag = ir <= P.clip_dist ? 2 : 3;
                if (tag >= 0) {
                    clip = (tag == 0 && r.clipflag >= 2) || (tag == 2 && (r.clipflag == 1 || r.clipflag == 3));
                    const bool mapped = (r.flag & 0x4) == 0, mate_mapped = (r.flag & 0x8) == 0;
                    if (mapped && mate_mapped && (int)r.mapq >= P.anchor_mapq) {
                        if (r.mate_ref != r.ref) pair = true;
                        else {
                            const int64_t t = r.tlen < 0 ? -(int64_t)r.tlen : (int64_t)r.tlen;
                            pair = t >= P.dist2 || (P.short_is && t <= P.dist1);
                        }
                    } else if (mapped && !mate_mapped) {
                        unmap = true;
                    }
                }
            }
            gf_taghit hit;
            hit.rec = rec; hit.gap = g;
            hit.kind = GF_KIND_CLIP; hit.to_mate = 0;
            emit_hit(clip, hit, hb, P.out, P.cap, P.n_out);
            hit.kind = pair ? GF_KIND_DISCORDANT : GF_KIND_UNMAP; hit.to_mate = 1;
            emit_hit(pair || unmap, hit, hb, P.out, P.cap, P.n_out);
            if (more) ++g;
        }
        tag_wave_sync();
        live_n = base;
    };
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t n_half = 2 * P.n;                       // 16-byte halves
    const uint64_t chunk = 64ull * TAG_UNROLL;             // halves per wave iteration
    const uint4* src = reinterpret_cast<const uint4*>(P.recs);
    // ---- per-wave queue of records that passed the LDS map and wait for the fine map (FINEQ)
    Cand* wcand = candq[CQ ? threadIdx.x >> 6 : 0];
    uint32_t cand_n = 0;   // wave-uniform
    auto sift = [&]() {    // fine-map test of the last min(64, cand_n) queued records, one per lane
        const uint32_t base = cand_n > 64 ? cand_n - 64 : 0;
        bool live = base + lane < cand_n;
        Cand c = {};
        if (live) {
            c = wcand[base + lane];
            if constexpr (LIN) {
                if (P.fine_bits) {
                    const uint32_t fb = c.lin >> P.fine_shift;
                    live = fb < P.fine_bins && ((P.fine_bits[fb >> 5] >> (fb & 31)) & 1u);
                }
            } else
            if (FINEQ || P.fine_bits) {   // (KEYS without a fine map: the queue only gathers the records to fetch)
                const uint32_t f0 = P.fine_off[c.ref], fi = c.pos >> P.fine_shift, fb = f0 + fi;
                live = fi < P.fine_off[c.ref + 1] - f0 && ((P.fine_bits[fb >> 5] >> (fb & 31)) & 1u);
            }
        }
        tag_wave_sync();
        cand_n = base;
        // (wave_push written out: the value is the record, fetched only behind the ballot and the drain)
        const unsigned long long lb = __ballot(live);
        if (lb) {
            const uint32_t cnt = (uint32_t)__popcll(lb);
            if (live_n + cnt > LIVEQ) drain();             // (live_n < 64 on entry: one drain makes room)
            if (live) {
                const uint4 a = src[2 * (uint64_t)c.rec], b = src[2 * (uint64_t)c.rec + 1];
                LiveRec q;
                q.pos = a.x; q.ref = a.w; q.tlen = (int32_t)a.z; q.mate_ref = b.x; q.meta = b.y; q.rec = c.rec;
                wlive[live_n + __popcll(lb & ((1ull << lane) - 1))] = q;
            }
            live_n += cnt;
            tag_wave_sync();
            if (live_n >= 64) drain();
        }
    };
    if constexpr (LIN) {
        // the linear key column: 16 bytes = four records per lane and load, TAG_UNROLL loads (2 048 records per wave: the same 8 KiB) in flight
        // behind the chunk at work, and with them the 256 bytes of the MAPQ-0 bit plane that go with a chunk: one load per wave, a word per
        // lane; the four bits of a lane's records come from the word of lane 8 u + lane / 8.  (Plain loops and no closure, as below.)
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4* ksrc4 = reinterpret_cast<const u32x4*>(P.lin_keys);
        // (32-bit unit indices from a wave index the compiler knows to be uniform: a record index fits 32 bits, so a unit's does, and the loop's
        //  bookkeeping stays out of the vector registers — the 16-wave form has 128 of them, 64 hold keys)
        const uint32_t n_k16 = (uint32_t)P.lin_units, kchunk = 64u * TAG_UNROLL;
        const uint32_t wv = (uint32_t)wave, stride = gridDim.x * NW * kchunk;
        u32x4 kn[TAG_UNROLL];
        uint32_t pn = 0;
#pragma unroll
        for (int u = 0; u < TAG_UNROLL; ++u) {
            const uint32_t h = wv * kchunk + 64u * u + lane;
            kn[u] = h < n_k16 ? __builtin_nontemporal_load(ksrc4 + h) : u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        }
        if (P.low) {
            const uint32_t w = ((wv * kchunk) >> 3) + lane;
            if (w < P.plane_words) pn = P.lin_plane[w];
        }
        for (uint32_t h0 = wv * kchunk; h0 < n_k16; h0 += stride) {
            u32x4 v[TAG_UNROLL];
#pragma unroll
            for (int u = 0; u < TAG_UNROLL; ++u) v[u] = kn[u];
            const uint32_t pl = pn;
#pragma unroll
            for (int u = 0; u < TAG_UNROLL; ++u) {
                const uint32_t h = h0 + stride + 64u * u + lane;
                kn[u] = h < n_k16 ? __builtin_nontemporal_load(ksrc4 + h) : u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            }
            pn = 0;
            if (P.low) {
                const uint32_t w = ((h0 + stride) >> 3) + lane;
                if (w < P.plane_words) pn = P.lin_plane[w];
            }
#pragma unroll
            for (int u = 0; u < TAG_UNROLL; ++u) {
                const uint32_t pw = P.low ? __shfl(pl, 8 * u + (int)(lane >> 3)) >> ((lane & 7u) * 4u) : 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t rec = 4u * (h0 + 64u * u + lane) + q;
                    const uint32_t lin = q == 0 ? v[u].x : q == 1 ? v[u].y : q == 2 ? v[u].z : v[u].w;
                    if (P.low) {   // wave-uniform: compact the MAPQ==0 records for the second hop ({key, -, record} until the buffer leaves)
                        const bool z = ((pw >> q) & 1u) && !(P.dbg & 1u);
                        wave_push(z, gf_lowrec{lin, 0u, (uint32_t)rec}, wlow, low_n, LOWBUF, flush_low);
                    }
                    // the pad, unplaced records and unknown scaffolds carry the key 0xFFFFFFFF: a bin behind the last one
                    const uint32_t bi = lin >> P.bin_shift;
                    bool live = bi < P.n_bins && !(P.dbg & 2u);
                    if (live) live = (bins[bi >> 5] >> (bi & 31)) & 1u;
                    if (P.dbg & 4u) live = false;
                    // (wave_push written out: as the helper this push cost the form 3 % — 0.477 against 0.463 ms per 200 M records, IS 300)
                    const unsigned long long cb = __ballot(live);
                    if (!cb) continue;
                    const uint32_t cnt = (uint32_t)__popcll(cb);
                    if (cand_n + cnt > CANDQ) sift();                  // (cand_n < 64 on entry: one sift empties the queue)
                    if (live) wcand[cand_n + __popcll(cb & ((1ull << lane) - 1))] = CandLin{lin, (uint32_t)rec};
                    cand_n += cnt;
                    tag_wave_sync();
                    if (cand_n >= 64) sift();
                }
            }
        }
    } else if constexpr (KEYS) {
        // the key column: 16 bytes = two records per lane and load, TAG_UNROLL loads (1 024 records per wave) in flight behind the chunk at work
        const uint4* ksrc = reinterpret_cast<const uint4*>(P.keys);
        const uint64_t n_k16 = (P.n + 1) / 2;
        const uint64_t kchunk = 64ull * TAG_UNROLL;
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4* ksrc4 = reinterpret_cast<const u32x4*>(ksrc);
        // (plain loops, no lambda and no named pad value: anything whose address a closure takes goes to scratch memory — the first form of
        //  this loop kept its sixteen prefetched keys there, 144 bytes per lane, and ran no faster than the 32-byte stream)
        u32x4 kn[TAG_UNROLL];
#pragma unroll
        for (int u = 0; u < TAG_UNROLL; ++u) {
            const uint64_t h = wave * kchunk + 64ull * u + lane;
            kn[u] = h < n_k16 ? __builtin_nontemporal_load(ksrc4 + h) : u32x4{0u, 0x7FFFFFFFu, 0u, 0x7FFFFFFFu};
        }
        for (uint64_t h0 = wave * kchunk; h0 < n_k16; h0 += n_waves * kchunk) {
            u32x4 v[TAG_UNROLL];
#pragma unroll
            for (int u = 0; u < TAG_UNROLL; ++u) v[u] = kn[u];
#pragma unroll
            for (int u = 0; u < TAG_UNROLL; ++u) {
                const uint64_t h = h0 + n_waves * kchunk + 64ull * u + lane;
                kn[u] = h < n_k16 ? __builtin_nontemporal_load(ksrc4 + h) : u32x4{0u, 0x7FFFFFFFu, 0u, 0x7FFFFFFFu};
            }
#pragma unroll
            for (int u = 0; u < TAG_UNROLL; ++u) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const uint64_t rec = 2 * (h0 + 64ull * u + lane) + half;
                    const uint32_t pos = half ? v[u].z : v[u].x, w = half ? v[u].w : v[u].y;
                    const uint32_t ref = w & 0x7FFFFFFFu;
                    bool live = rec < P.n && ref < P.n_scaffolds;
                    if (P.low) {   // wave-uniform: compact the MAPQ==0 records for the second hop
                        const bool z = live && (w >> 31) && !(P.dbg & 1u);
                        wave_push(z, gf_lowrec{pos, ref, (uint32_t)rec}, wlow, low_n, LOWBUF, flush_low);
                    }
                    if (P.dbg & 2u) live = false;
                    if (live) {
                        const uint32_t b0 = boff[ref], nbin = boff[ref + 1] - b0, bi = pos >> P.bin_shift;
                        live = bi < nbin && ((bins[(b0 + bi) >> 5] >> ((b0 + bi) & 31)) & 1u);
                    }
                    if (P.dbg & 4u) live = false;
                    if (!wave_push(live, CandRec{pos, ref, (uint32_t)rec}, wcand, cand_n, CANDQ, sift)) continue;   // (cand_n < 64 on entry: one sift empties the queue)
                    tag_wave_sync();
                    if (cand_n >= 64) sift();
                }
            }
        }
    } else {
    // software pipeline: the next chunk's loads are issued before the current chunk is processed
    uint4 vn[TAG_UNROLL];
    auto fetch = [&](uint64_t h0) {
#pragma unroll
        for (int u = 0; u < TAG_UNROLL; ++u) {
            const uint64_t h = h0 + 64ull * u + lane;
            // the forms that stage the map in LDS load the stream non-temporally: it no longer evicts the fine map from the L2s.  Measured on
            // the C4 layout (200 M records, rocprof): 2^25-bit global map 2.24 ms; + nt loads 1.90 ms; 2^23 bits + nt 1.82 ms
            if (BINS_LDS) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 t = h < n_half ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + h) : u32x4{0, 0, 0, 0xFFFFFFFFu};
                vn[u] = make_uint4(t.x, t.y, t.z, t.w);
            } else
            vn[u] = h < n_half ? src[h] : make_uint4(0, 0, 0, 0xFFFFFFFFu);
        }
    };
    fetch(wave * chunk);
    for (uint64_t h0 = wave * chunk; h0 < n_half; h0 += n_waves * chunk) {
        uint4 v[TAG_UNROLL];
#pragma unroll
        for (int u = 0; u < TAG_UNROLL; ++u) v[u] = vn[u];
        fetch(h0 + n_waves * chunk);
        // Two 1-KiB loads hold 64 records as 128 halves, even lanes {pos, mate_pos, tlen, ref}, odd lanes {mate_ref, flag|mapq|clip, ..}:
        // lane L takes record L of the 64 — its halves sit in lanes 2L and 2L + 1 of the first load (L < 32) or of the second — so
        // that every step below works on 64 records, not on the 32 even lanes of one load (the kernel issues ~60 instructions per step
        // whatever the number of busy lanes: at 13 % of the records passing the map, the long-insert library, it was issue-bound).
        const uint32_t s0 = (lane << 1) & 63u, s1 = s0 + 1;
        const bool upper = lane >= 32;
#pragma unroll
        for (int u = 0; u < TAG_UNROLL; u += 2) {
            auto gather = [&](uint32_t a, uint32_t b, uint32_t sl) -> uint32_t {
                const uint32_t x = __shfl(a, sl), y = __shfl(b, sl);
                return upper ? y : x;
            };
            const uint64_t h = h0 + 64ull * u + 2ull * lane;      // first half of this lane's record
            gf_alnrec r = {};
            r.pos = gather(v[u].x, v[u + 1].x, s0);
            r.ref = gather(v[u].w, v[u + 1].w, s0);               // (halves beyond the input carry ref = 0xFFFFFFFF)
            const uint32_t meta = gather(v[u].y, v[u + 1].y, s1);
            bool live = h < n_half && r.ref < P.n_scaffolds;
            if (P.low) {   // wave-uniform: compact the MAPQ==0 records for the second hop
                const bool z = live && ((meta >> 16) & 0xFF) == 0;
                wave_push(z, gf_lowrec{r.pos, r.ref, (uint32_t)(h >> 1)}, wlow, low_n, LOWBUF, flush_low);
            }
            if (live) {  // coarse test first: almost every record lies far from every gap
                const uint32_t b0 = boff[r.ref], nbin = boff[r.ref + 1] - b0, bi = r.pos >> P.bin_shift;
                live = bi < nbin && ((bins[(b0 + bi) >> 5] >> ((b0 + bi) & 31)) & 1u);
            }
            if (FINEQ) {   // (launched with FINEQ only when the fine map exists)
                if (!wave_push(live, CandRec{r.pos, r.ref, (uint32_t)(h >> 1)}, wcand, cand_n, CANDQ, sift)) continue;   // (cand_n < 64 on entry: one sift empties the queue)
                tag_wave_sync();
                if (cand_n >= 64) sift();
                continue;
            }
            if (live && P.fine_bits) {
                const uint32_t f0 = P.fine_off[r.ref], fi = r.pos >> P.fine_shift, fb = f0 + fi;
                live = fi < P.fine_off[r.ref + 1] - f0 && ((P.fine_bits[fb >> 5] >> (fb & 31)) & 1u);
            }
            // survivors (a few per mille to a tenth) are queued; the window search runs on 64 of them at a time instead of once per
            // load with a few busy lanes.  (wave_push written out: the value's last two fields are gathered only behind the ballot — four
            // shuffles that every step of every wave would otherwise make)
            const unsigned long long lb = __ballot(live);
            if (!lb) continue;
            const uint32_t tlen = gather(v[u].z, v[u + 1].z, s0), mate_ref = gather(v[u].x, v[u + 1].x, s1);
            const uint32_t cnt = (uint32_t)__popcll(lb);
            if (live_n + cnt > LIVEQ) drain();                     // (live_n < 64 on entry: one drain empties the queue)
            if (live) {
                LiveRec q;
                q.pos = r.pos; q.ref = r.ref; q.tlen = (int32_t)tlen; q.mate_ref = mate_ref; q.meta = meta; q.rec = (uint32_t)(h >> 1);
                wlive[live_n + __popcll(lb & ((1ull << lane) - 1))] = q;
            }
            live_n += cnt;
            tag_wave_sync();
            if (live_n >= 64) drain();
        }
    }
    }
    if (CQ) while (cand_n) sift();
    while (live_n) drain();
    if (P.low && low_n) flush_low();
    if (P.low && stage_n) flush_stage();
    if (hb.n) flush_wave_hits(hb, P.out, P.cap, P.n_out);
}

// tag_kernel's instantiations: the kernel, what selects it, and the name a profiler prints for it, in one entry (gf_tag_kernel reports the
// entry launched).  light: one-wave workgroups without the LDS bin map, co-resident with the k-mer filter's workgroups; 16 waves: the
// 64-KiB map, one workgroup per CU; the records form queues its candidates (FINEQ) where a fine map exists.
struct TagKernel {
    void (*fn)(TagParams);
    uint32_t nw;
    int form;
    bool fineq;
    const char* name;
};
#define TAG_K(NW, LDS, FQ, FORM) {tag_kernel<NW, LDS, FQ, FORM>, NW, FORM, FQ, "tag_kernel<" #NW ", " #LDS ", " #FQ ", " #FORM ">"}
static const TagKernel TAG_KERNELS[] = {   // (FORM as the number the name is printed with: 0 TAG_RECORDS, 1 TAG_KEYS8, 2 TAG_LINEAR)
    TAG_K(1, false, false, 0), TAG_K(4, true, false, 0), TAG_K(4, true, true, 0), TAG_K(16, true, false, 0), TAG_K(16, true, true, 0),
    TAG_K(4, true, false, 1),  TAG_K(16, true, false, 1),
    TAG_K(4, true, false, 2),  TAG_K(16, true, false, 2)};
#undef TAG_K

// n records against a map of map_words bit words (`fine`: with a fine map behind it) on n_cu CUs.  light: option tag_light;
// keys_given: the caller handed an 8-byte key column; lin: its linear key column was accepted (launch_tag).
TagPlan plan_tag(size_t n, uint32_t map_words, bool fine, uint32_t n_scaffolds, int n_cu, bool light, bool keys_given, bool lin) {
    TagPlan T = {};
    T.rc = GF_OK;
    T.fine = fine;
    T.form = lin ? TAG_LINEAR : keys_given && !light ? TAG_KEYS8 : TAG_RECORDS;
    const size_t map_bytes = (size_t)map_words * 4;
    const bool big_map = map_bytes > TAG_MAP_4WAVE_BYTES;
    T.nw = light ? 1u : big_map ? 16u : 4u;
    T.grid = light ? 4 * stream_grid(n_cu, n) : big_map ? (unsigned)std::max<size_t>(1, std::min<size_t>((n + 1023) / 1024, (size_t)n_cu)) : stream_grid(n_cu, n);
    T.off_words = n_scaffolds + 1 <= 2048 ? n_scaffolds + 1 : 0;   // the per-scaffold offsets ride along in LDS when they are few
    T.lds_bytes = map_bytes + (size_t)T.off_words * 4;
    // the 16-wave form keeps TAG16_STATIC_LDS bytes of queues and buffers beside the staged map: when the two do not fit a CU's LDS
    // the per-scaffold offsets stay in global memory
    if (big_map && TAG16_STATIC_LDS + T.lds_bytes > TAG_LDS_BYTES) {
        T.off_words = 0;
        T.lds_bytes = map_bytes;
        if (TAG16_STATIC_LDS + T.lds_bytes > TAG_LDS_BYTES) T.rc = GF_E_UNSUPPORTED;   // (a 64-KiB map is the largest ensure_bin_map builds)
    }
    if (light) T.lds_bytes = 0;   // (the map is read through L1/L2)
    T.kernel = -1;
    for (size_t i = 0; i < sizeof(TAG_KERNELS) / sizeof(TAG_KERNELS[0]); ++i) {
        const TagKernel& k = TAG_KERNELS[i];
        if (k.nw == T.nw && k.form == T.form && k.fineq == (T.form == TAG_RECORDS && !light && fine)) T.kernel = (int)i;
    }
    return T;
}

int launch_tag(gf_ctx* ctx, const void* d_recs, size_t n, int insert_size, int sd, int clip_dist, int anchor_mapq,
               void* d_out, size_t cap, void* d_n_out, void* d_low, size_t low_cap, void* d_n_low, const void* d_keys, const void* d_lin,
               const gf_tag_layout* lin_for) {
    if (!ctx->d_gaps) return GF_E_STATE;
    if (n >= 0xFFFFFFFFull || cap > 0xFFFFFFFFull) return GF_E_INVAL;
    zero_regions(ctx, ZeroList{{(uint32_t*)d_n_out, (uint32_t*)d_n_low, nullptr, nullptr}, {1, d_n_low ? 1u : 0u, 0, 0}});
    if (n == 0) return GF_OK;
    const int dist2 = insert_size + 3 * sd;
    // The linear key column is streamed only when it was built for exactly this call (record count, scaffolds; ensure_bin_map checks base[]
    // against the layout's checksum) and the map's bins fit its granule; a stale column or a map it cannot serve is refused, and the call
    // answers from the 8-byte column or the records.
    gf_ctx::TagMap* M = nullptr;
    int rc = GF_OK;
    bool lin = d_lin && lin_for && lin_for->use && !ctx->tag_light && lin_for->n_recs == n && lin_for->n_scaffolds == ctx->n_scaffolds;
    const LinCol lc = lin_col(n, ctx->n_scaffolds);
    if (lin) {
        rc = ensure_bin_map(ctx, dist2, &M, lin_for, (const uint32_t*)((const uint8_t*)d_lin + lc.base_off));
        if (rc == GF_E_UNSUPPORTED || rc == GF_E_INVAL) { lin = false; M = nullptr; }
        else if (rc) return rc;
    }
    if (!lin) rc = ensure_bin_map(ctx, dist2, &M);
    if (rc) return rc;
    const TagPlan T = plan_tag(n, M->words, M->fine_words != 0, ctx->n_scaffolds, ctx->n_cu, ctx->tag_light != 0, d_keys != nullptr, lin);
    if (T.rc) return T.rc;
    if (T.kernel < 0) return GF_E_UNSUPPORTED;   // (the table holds every form the plan can ask for)
    const TagKernel& K = TAG_KERNELS[T.kernel];

    TagParams P;
    P.recs = (const gf_alnrec*)d_recs;
    P.keys = (const uint2*)d_keys;
    P.dbg = (uint32_t)ctx->tag_dbg;
    P.n = n;
    P.gaps = ctx->d_gaps;
    P.scaf_off = ctx->d_scaf_off;
    P.n_scaffolds = ctx->n_scaffolds;
    P.dist1 = insert_size - 3 * sd;
    P.dist2 = dist2;
    P.clip_dist = clip_dist;
    P.anchor_mapq = anchor_mapq;
    P.short_is = insert_size < 750;  // collect_reads_for_gaps.py:275
    P.out = (gf_taghit*)d_out;
    P.cap = (uint32_t)cap;
    P.n_out = (uint32_t*)d_n_out;
    P.lin_keys = lin ? (const uint32_t*)d_lin : nullptr;
    P.lin_plane = lin ? (const uint32_t*)((const uint8_t*)d_lin + lc.plane_off) : nullptr;
    P.lin_units = (n + 3) / 4;
    P.plane_words = (uint32_t)lc.plane_words;
    P.n_bins = M->n_bins;
    P.fine_bins = M->fine_bins;
    P.bin_bits = (const uint32_t*)M->map.p;
    P.bin_off = P.bin_bits + M->words;
    P.bin_first = P.bin_off + ctx->n_scaffolds + 1;
    P.bin_shift = M->shift;
    P.bin_words = M->words;
    P.off_words = T.off_words;
    P.fine_bits = T.fine ? (const uint32_t*)M->fine.p : nullptr;
    P.fine_off = P.fine_bits ? P.fine_bits + M->fine_words : nullptr;
    P.fine_shift = M->fine_shift;
    const bool by_product = d_low && d_n_low;
    P.low = by_product ? (gf_lowrec*)d_low : nullptr;
    P.low_cap = (uint32_t)std::min<size_t>(low_cap, 0xFFFFFFFFu);
    P.n_low = by_product ? (uint32_t*)d_n_low : nullptr;
    P.low_stage = nullptr;
    if (P.low) {   // the staging buffer of the MAPQ-0 by-product has a slice per wave of the launch
        if ((rc = ensure(ctx, ctx->tag_stage, (size_t)T.grid * T.nw * LOWSTAGE * sizeof(gf_lowrec)))) return rc;
        P.low_stage = (gf_lowrec*)ctx->tag_stage.p;
    }
    {
        LaunchTimer tm(ctx, GF_KERNEL_TAG);
        ctx->tag_last_nw = (int)T.nw;
        ctx->tag_last_form = T.form;
        ctx->tag_kernel = std::string(K.name) + (T.fine ? "+fine" : "");
        hipLaunchKernelGGL(K.fn, dim3(T.grid), dim3(64 * T.nw), T.lds_bytes, ctx->stream, P);
    }
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // namespace gf
