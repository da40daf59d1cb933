// rescue.hip — the reference's rescue round inside the device step (assemble_gaps.py:357-366, body :166-217): a gap's high-quality reads that
// align CLIPPED to two or more of its merged contigs are bridges; they join the gap's own contigs as records of their own, the set is merged
// again (merge.hip, MG_MODE_RESCUE) and picked at the short anchor.  Definition: gappadder_amd/assemble_gaps.py::bridging_reads and its host
// C++ form gf_bridging_reads (textio.hip) with seed_len 30, budget 2; DESIGN.md §12.
//   keys      one thread per tagger hit of a library: MAPQ-60 records with a read -> gap << 40 | lib << 36 | mate side << 35 | pair
//   pools     radix sort, unique flags, scan: the HQ reads of every tried gap in (gap, library, mate side, pair) order
//   sets      merge.hip's count / fill / dedup (MG_MODE_SETS): per tried gap the alignment set = exact-containment dedup of its records
//   windows   one thread per (HQ read, window): the 30-base windows without an N-masked base into an open-addressing set of (window, gap)
//   seeds     one workgroup per set: every 30-base ACGT window of the set's contigs, both strands, that some HQ read of the gap shares ->
//             (window, gap << 35 | contig << 25 | strand << 24 | offset), radix-sorted by offset key then (stably) by window: per (window, gap)
//             a run ordered by (contig, strand, offset), so the first 8 occurrences per contig strand are the run's first 8 per (contig, strand)
//   bridges   one wave per HQ read: its windows looked up in the seeds, placements (contig, strand, diagonal, read offset) in LDS, the first
//             seed per (contig, strand, diagonal) verified ungapped against the contig, clipped-at-contig counted: one flag per read
//   append    scan of the flags: bridges decoded to bases (N where masked) and appended as records with k = kv = GF_RESCUE_MARK
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gf_internal.hpp"

namespace gf {

namespace {

constexpr uint32_t RS_SEED = 30, RS_BUDGET = 2, RS_MAX_OCC = 8;
constexpr uint32_t RS_PLACE_SLOTS = 512;        // (contig, strand, diagonal) placements of one read in LDS (more: the read is dropped,
                                                // stats[GF_RS_PLACE_OVF])
constexpr uint32_t RS_MAX_READ = 1000;          // (the assembly's bound)
constexpr unsigned long long RS_EMPTY = ~0ull;
constexpr uint64_t RS_WIN_MASK = (1ull << 60) - 1;
// linear probing stops after this many slots: an entry that finds no room within them is counted (stats[GF_RS_TAB_FULL], the caller grows
// the table), so a look-up that walks as far finds every entry there is — and a table far too small for its windows (the first sizing
// pass) costs a bounded walk per window instead of one over the whole table
constexpr uint32_t RS_MAX_PROBES = 128;

struct RsSlot {
    unsigned long long win;
    uint32_t gap, state;
};
static_assert(sizeof(RsSlot) == 16, "slot layout");

struct RsLibs {
    const uint8_t* reads[GF_R2_MAX_LIBS];
    const uint32_t* nmask[GF_R2_MAX_LIBS];
};

// the caller's work buffer, carved (gf_rescue_work_bytes)
struct RsWork {
    unsigned long long *keys, *sorted, *hq;        // [hq_cap]
    uint32_t *flag, *uidx;                          // [hq_cap]: unique flags and their scan; later the bridge flags and their scan
    uint32_t *gap_hq, *gap_bridges;                 // [n_gaps]
    RsSlot* tab;                                    // [2^log2]
    unsigned long long *sd_loc, *sd_win, *sd_loc2, *sd_win2;   // [seed_cap]
    size_t bytes;
};

inline size_t rs_align(size_t x) { return (x + 255) & ~(size_t)255; }

RsWork rs_carve(void* base, size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2) {
    RsWork w{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += rs_align(b); return (uint8_t*)base + o; };
    w.keys = (unsigned long long*)take(hq_cap * 8);
    w.sorted = (unsigned long long*)take(hq_cap * 8);
    w.hq = (unsigned long long*)take(hq_cap * 8);
    w.flag = (uint32_t*)take(hq_cap * 4);
    w.uidx = (uint32_t*)take(hq_cap * 4);
    w.gap_hq = (uint32_t*)take(n_gaps * 4);
    w.gap_bridges = (uint32_t*)take(n_gaps * 4);
    w.tab = (RsSlot*)take(sizeof(RsSlot) << log2);
    w.sd_loc = (unsigned long long*)take(seed_cap * 8);
    w.sd_win = (unsigned long long*)take(seed_cap * 8);
    w.sd_loc2 = (unsigned long long*)take(seed_cap * 8);
    w.sd_win2 = (unsigned long long*)take(seed_cap * 8);
    w.bytes = at;
    return w;
}

unsigned rs_grid(gf_ctx* ctx, uint64_t work, unsigned per = 256) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->n_cu * 16, (work + per - 1) / per));
}

__device__ __forceinline__ uint32_t rs_slot_of(unsigned long long win, uint32_t gap, uint32_t log2) {
    const unsigned long long h = (win ^ ((unsigned long long)gap * 0x9E3779B97F4A7C15ull)) * 0xC2B2AE3D27D4EB4Full;
    return (uint32_t)(h >> (64 - log2));
}

// ---- keys: the HQ reads of one library's tagger hits (device_collect.py's gap_reads_high_quality: MAPQ == 60, a read, read ^ to_mate)
__global__ __launch_bounds__(256) void rs_keys_kernel(const gf_taghit* hits, const uint32_t* d_n, uint64_t hit_cap, const gf_alnrec* recs,
                                                      uint64_t n_reads, uint32_t lib, uint64_t n_gaps, unsigned long long* keys, uint64_t key_cap,
                                                      uint32_t* stats) {
    const uint64_t n = min((uint64_t)*d_n, hit_cap);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const gf_taghit h = hits[i];
        if (h.gap >= n_gaps) continue;
        const gf_alnrec r = recs[h.rec];
        const uint32_t rd = (uint32_t)r.read;
        if (r.mapq != 60 || rd == 0xFFFFFFFFu) continue;
        const uint64_t t = (uint64_t)(rd ^ (uint32_t)(h.to_mate & 1));
        if (t >= n_reads) continue;
        const uint32_t j = atomicAdd(stats + GF_RS_HQ_KEYS, 1u);
        if (j < key_cap) keys[j] = ((unsigned long long)h.gap << 40) | ((unsigned long long)lib << 36) | ((t & 1ull) << 35) | (t >> 1);
    }
}

// ---- pools: unique keys of the tried gaps, compacted in sorted order
__global__ __launch_bounds__(256) void rs_mark_kernel(const unsigned long long* s, uint64_t n, const uint64_t* best, uint64_t n_gaps, uint32_t* flag,
                                                      uint32_t* gap_hq, uint32_t* stats) {
    uint32_t mine = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long x = s[i];
        const uint32_t g = (uint32_t)(x >> 40);
        const bool u = x != RS_EMPTY && g < n_gaps && best[g] == 0 && (i == 0 || s[i - 1] != x);
        flag[i] = u;
        if (u) { atomicAdd(gap_hq + g, 1u); ++mine; }
    }
    if (mine) atomicAdd(stats + GF_RS_HQ, mine);
}

__global__ __launch_bounds__(256) void rs_compact_kernel(const unsigned long long* s, uint64_t n, const uint32_t* flag, const uint32_t* uidx,
                                                         unsigned long long* hq) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (flag[i]) hq[uidx[i]] = s[i];
}

__device__ __forceinline__ void rs_read_of(const RsLibs& L, unsigned long long key, uint32_t rb, uint32_t nmw, const uint8_t** row, const uint32_t** mrow) {
    const uint32_t lib = (uint32_t)(key >> 36) & (GF_R2_MAX_LIBS - 1);
    const uint64_t read = 2 * (key & ((1ull << 35) - 1)) + ((key >> 35) & 1);
    *row = L.reads[lib] + read * rb;
    *mrow = L.nmask[lib] ? L.nmask[lib] + read * nmw : nullptr;
}

__device__ __forceinline__ uint32_t rs_code(const uint8_t* row, const uint32_t* mrow, uint32_t i) {   // 0-3, 4 = N-masked
    if (mrow && ((mrow[i >> 5] >> (i & 31)) & 1u)) return 4u;
    return (row[i >> 2] >> (6 - 2 * (i & 3))) & 3u;
}

// ---- windows: (window, gap) of every HQ read window without an N-masked base
__global__ __launch_bounds__(256) void rs_windows_kernel(const unsigned long long* hq, const uint32_t* stats_ro, RsLibs L, uint32_t len, uint32_t rb,
                                                         uint32_t nmw, RsSlot* tab, uint32_t log2, uint32_t* stats) {
    const uint32_t nw = len - RS_SEED + 1;                // one thread per (read, window): independent probes, no serial walk per read
    const uint64_t n = (uint64_t)stats_ro[GF_RS_HQ] * nw;
    const uint32_t mask = (uint32_t)((1ull << log2) - 1);
    uint32_t mine = 0;
    for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < n; w += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = w / nw;
        const uint32_t i0 = (uint32_t)(w - q * nw);
        const unsigned long long key = hq[q];
        const uint32_t gap = (uint32_t)(key >> 40);
        const uint8_t* row;
        const uint32_t* mrow;
        rs_read_of(L, key, rb, nmw, &row, &mrow);
        unsigned long long v = 0;
        bool ok = true;
        for (uint32_t i = i0; i < i0 + RS_SEED; ++i) {
            const uint32_t b = rs_code(row, mrow, i);
            ok = ok && b != 4u;
            v = (v << 2) | (b & 3u);
        }
        if (!ok) continue;
        ++mine;
        uint32_t pos = rs_slot_of(v, gap, log2);
        uint32_t probes = 0;
        const uint32_t max_probes = mask < RS_MAX_PROBES ? mask + 1 : RS_MAX_PROBES;
        while (probes < max_probes) {
            RsSlot* s = tab + pos;
            const uint32_t st = __hip_atomic_load(&s->state, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (st == 0u) {
                if (atomicCAS(&s->state, 0u, 1u) == 0u) {
                    __hip_atomic_store(&s->win, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&s->gap, gap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&s->state, 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                continue;            // lost the claim: read the same slot again
            }
            if (st == 1u) continue;  // being written: read it again in the next turn
            if (__hip_atomic_load(&s->win, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == v &&
                __hip_atomic_load(&s->gap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gap)
                break;
            pos = (pos + 1) & mask;
            ++probes;
        }
        if (probes >= max_probes) atomicAdd(stats + GF_RS_TAB_FULL, 1u);
    }
    if (mine) atomicAdd(stats + GF_RS_WINDOWS, mine);
}

__device__ __forceinline__ bool rs_lookup(const RsSlot* tab, uint32_t log2, unsigned long long v, uint32_t gap) {
    const uint32_t mask = (uint32_t)((1ull << log2) - 1);
    uint32_t pos = rs_slot_of(v, gap, log2);
    const uint32_t max_probes = mask < RS_MAX_PROBES ? mask + 1 : RS_MAX_PROBES;
    for (uint32_t probes = 0; probes < max_probes; ++probes) {
        const RsSlot& s = tab[pos];
        if (s.state == 0u) return false;
        if (s.win == v && s.gap == gap) return true;
        pos = (pos + 1) & mask;
    }
    return false;
}

// ---- seeds: one workgroup per alignment set (gap with HQ reads); windows rolled over a stretch of 64 positions per thread
__global__ __launch_bounds__(256) void rs_seeds_kernel(const gf_contig* ctg, const char* seq, MgSetsView V, const uint32_t* sets_stats,
                                                       const uint32_t* gap_hq, uint64_t n_gaps, const RsSlot* tab, uint32_t log2,
                                                       unsigned long long* loc, unsigned long long* win, uint64_t seed_cap, uint32_t* stats) {
    const uint32_t n_sets = sets_stats[0];      // (MG_N_PRE)
    constexpr uint32_t STRETCH = 64;
    for (uint32_t pre = blockIdx.x; pre < n_sets; pre += gridDim.x) {
        const uint32_t o = V.pre_off[pre], kn = V.kept_n[pre];
        const gf_contig c0 = ctg[V.ids[o]];
        const uint32_t gap = c0.gap;
        if (gap >= n_gaps || !gap_hq[gap] || kn < 2) continue;        // (uniform in the block)
        for (uint32_t ci = 0; ci < kn; ++ci) {
            const gf_contig c = ctg[V.ids[o + ci]];
            if (c.length < RS_SEED) continue;
            if (c.length >= (1u << 24)) { if (threadIdx.x == 0) atomicAdd(stats + GF_RS_LONG, 1u); continue; }
            const char* s = seq + c.seq_off;
            const uint32_t n_win = c.length - RS_SEED + 1;
            for (uint32_t p0 = threadIdx.x * STRETCH; p0 < n_win; p0 += blockDim.x * STRETCH) {
                unsigned long long f = 0, r = 0;
                uint32_t run = 0;
                const uint32_t p1 = min(p0 + STRETCH, n_win);
                for (uint32_t x = p0; x < p1 + RS_SEED - 1; ++x) {      // bases p0 .. p1 + 28: windows starting at p0 .. p1 - 1
                    const uint32_t b = base_code4(s[x]);
                    run = b == 4u ? 0 : run + 1;
                    f = ((f << 2) | (b & 3u)) & RS_WIN_MASK;
                    r = (r >> 2) | ((unsigned long long)(3u - (b & 3u)) << (2 * (RS_SEED - 1)));
                    if (run < RS_SEED) continue;
                    const uint32_t p = x + 1 - RS_SEED;
                    for (uint32_t st = 0; st < 2; ++st) {
                        const unsigned long long v = st ? r : f;
                        if (!rs_lookup(tab, log2, v, gap)) continue;
                        const uint32_t j = st ? c.length - RS_SEED - p : p;
                        const uint32_t at = atomicAdd(stats + GF_RS_SEEDS, 1u);
                        if (at < seed_cap) {
                            loc[at] = ((unsigned long long)gap << 35) | ((unsigned long long)ci << 25) | ((unsigned long long)st << 24) | j;
                            win[at] = v;
                        }
                    }
                }
            }
        }
    }
}

// ---- bridges: one wave (= one workgroup of 64) per HQ read
__device__ __forceinline__ uint32_t rs_lower(const unsigned long long* win, const unsigned long long* loc, uint32_t n, unsigned long long v,
                                             unsigned long long l) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        const bool less = win[m] < v || (win[m] == v && loc[m] < l);
        if (less) lo = m + 1; else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(64) void rs_bridge_kernel(const gf_contig* ctg, const char* seq, MgSetsView V, const unsigned long long* hq,
                                                       const uint32_t* stats_ro, RsLibs L, uint32_t len, uint32_t rb, uint32_t nmw,
                                                       const unsigned long long* win, const unsigned long long* loc, uint64_t seed_cap,
                                                       uint32_t* bflag, uint32_t* gap_bridges, uint32_t* stats) {
    __shared__ char s_rd[RS_MAX_READ];
    __shared__ unsigned long long s_key[RS_PLACE_SLOTS];    // (contig, strand, diagonal) of a placement, RS_EMPTY: free
    __shared__ uint32_t s_mi[RS_PLACE_SLOTS];               // ... its first seed (lowest read offset)
    __shared__ uint16_t s_list[RS_PLACE_SLOTS];
    __shared__ uint8_t s_clip[RS_PLACE_SLOTS];
    __shared__ uint32_t s_n, s_ovf;
    const uint32_t lane = threadIdx.x;
    const uint64_t n_hq = stats_ro[GF_RS_HQ];
    const uint32_t n_seeds = (uint32_t)min((uint64_t)stats_ro[GF_RS_SEEDS], seed_cap);
    for (uint64_t q = blockIdx.x; q < n_hq; q += gridDim.x) {
        const unsigned long long key = hq[q];
        const uint32_t gap = (uint32_t)(key >> 40);
        const uint32_t pre = V.pre_of_gap[gap];
        if (pre == EMPTY32) { if (lane == 0) bflag[q] = 0; continue; }      // (fewer than two contigs: no bridge)
        const uint32_t o = V.pre_off[pre];
        const uint8_t* row;
        const uint32_t* mrow;
        rs_read_of(L, key, rb, nmw, &row, &mrow);
        __syncthreads();
        for (uint32_t i = lane; i < len; i += 64) s_rd[i] = "ACGTN"[rs_code(row, mrow, i)];
        for (uint32_t x = lane; x < RS_PLACE_SLOTS; x += 64) { s_key[x] = RS_EMPTY; s_mi[x] = EMPTY32; }
        if (lane == 0) { s_n = 0; s_ovf = 0; }
        __syncthreads();
        // placements: every window of the read against the gap's seeds (kept: the first RS_MAX_OCC per contig strand); per (contig,
        // strand, diagonal) one LDS slot that keeps the lowest read offset = the first seed
        for (uint32_t i = lane; i + RS_SEED <= len; i += 64) {
            unsigned long long v = 0;
            bool ok = true;
            for (uint32_t t = 0; t < RS_SEED; ++t) {
                const uint32_t b = base_code4(s_rd[i + t]);
                ok = ok && b != 4u;
                v = (v << 2) | (b & 3u);
            }
            if (!ok) continue;
            const uint32_t lo = rs_lower(win, loc, n_seeds, v, (unsigned long long)gap << 35);
            for (uint32_t e = lo; e < n_seeds && win[e] == v && (uint32_t)(loc[e] >> 35) == gap; ++e) {
                const unsigned long long l = loc[e];
                const bool kept = e - lo < RS_MAX_OCC || win[e - RS_MAX_OCC] != v || (loc[e - RS_MAX_OCC] >> 24) != (l >> 24);
                if (!kept) continue;
                // (diagonal + read length >= 0, < 2^25: contig offsets are below 2^24)
                const unsigned long long pk = (((l >> 24) & 2047ull) << 25) | (unsigned long long)((int64_t)(l & 0xFFFFFFu) - (int64_t)i + RS_MAX_READ);
                uint32_t h = (uint32_t)((pk * 0x9E3779B97F4A7C15ull) >> 55) & (RS_PLACE_SLOTS - 1);
                bool placed = false;
                for (uint32_t t = 0; t < RS_PLACE_SLOTS && !placed; ++t, h = (h + 1) & (RS_PLACE_SLOTS - 1)) {
                    const unsigned long long old = atomicCAS(&s_key[h], RS_EMPTY, pk);
                    if (old == RS_EMPTY || old == pk) { atomicMin(&s_mi[h], i); placed = true; }
                }
                if (!placed) s_ovf = 1;
            }
        }
        __syncthreads();
        if (s_ovf) {
            if (lane == 0) { bflag[q] = 0; atomicAdd(stats + GF_RS_PLACE_OVF, 1u); }
            continue;
        }
        for (uint32_t x = lane; x < RS_PLACE_SLOTS; x += 64)
            if (s_key[x] != RS_EMPTY) s_list[atomicAdd(&s_n, 1u)] = (uint16_t)x;
        __syncthreads();
        const uint32_t np = s_n;
        // every placement verified from its first seed
        for (uint32_t p = lane; p < np; p += 64) {
            const uint32_t x = s_list[p];
            const unsigned long long pk = s_key[x];
            const uint32_t ci = (uint32_t)(pk >> 26), st = (uint32_t)(pk >> 25) & 1u, si = s_mi[x];
            const int64_t start = (int64_t)(pk & ((1ull << 25) - 1)) - RS_MAX_READ;
            const gf_contig c = ctg[V.ids[o + ci]];
            bool clipped = start < 0 || (uint64_t)start + len > c.length;
            if (!clipped) {
                const char* cs = seq + c.seq_off;
                uint32_t left = 0, right = 0;
                for (uint32_t t = 0; t < len && left <= RS_BUDGET && right <= RS_BUDGET; ++t) {
                    if (t >= si && t < si + RS_SEED) continue;
                    const uint64_t cp = (uint64_t)start + t;
                    const char cb = st ? base_comp(cs[c.length - 1 - cp]) : cs[cp];
                    if (s_rd[t] != cb) { if (t < si) ++left; else ++right; }
                }
                clipped = left > RS_BUDGET || right > RS_BUDGET;
            }
            s_clip[p] = clipped;
        }
        __syncthreads();
        // clipped AT a contig: every placement there clipped; a bridge is clipped at two contigs at least
        uint32_t mine = 0;
        for (uint32_t p = lane; p < np; p += 64) {
            const uint32_t ci = (uint32_t)(s_key[s_list[p]] >> 26);
            bool rep = true, all = true;
            for (uint32_t x = 0; x < np; ++x) {
                if ((uint32_t)(s_key[s_list[x]] >> 26) != ci) continue;
                if (x < p) rep = false;
                if (!s_clip[x]) all = false;
            }
            mine += rep && all;
        }
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
        if (lane == 0) {
            const bool br = mine >= 2;
            bflag[q] = br;
            if (br) atomicAdd(gap_bridges + gap, 1u);
        }
    }
}

// ---- append: bridge b of the scan at record first + b, its bases at seq_len + b * len (no record at or beyond contig_cap, a
// record whose bases do not fit is a tombstone, the counters count every bridge, a list that arrives overflowed is left unchanged)
__global__ __launch_bounds__(256) void rs_append_kernel(gf_contig* ctg, const uint32_t* d_n, uint64_t contig_cap, char* seq, const uint64_t* d_s,
                                                        uint64_t seq_cap, const unsigned long long* hq, const uint32_t* stats_ro, const uint32_t* bflag,
                                                        const uint32_t* bidx, RsLibs L, uint32_t len, uint32_t rb, uint32_t nmw) {
    const uint64_t n1 = *d_n, s1 = *d_s, n_hq = stats_ro[GF_RS_HQ];
    if (n1 > contig_cap || s1 > seq_cap) return;
    for (uint64_t q = blockIdx.x; q < n_hq; q += gridDim.x) {
        if (!bflag[q]) continue;                                  // (uniform in the block)
        const uint64_t b = bidx[q], rec = n1 + b, so = s1 + b * len;
        if (rec >= contig_cap) continue;
        const bool fits = so + len <= seq_cap;
        const unsigned long long key = hq[q];
        if (fits) {
            const uint8_t* row;
            const uint32_t* mrow;
            rs_read_of(L, key, rb, nmw, &row, &mrow);
            for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) seq[so + i] = "ACGTN"[rs_code(row, mrow, i)];
        }
        if (threadIdx.x == 0) {
            gf_contig c;
            memset(&c, 0, sizeof c);
            c.gap = (uint32_t)(key >> 40);
            c.k = GF_RESCUE_MARK;
            c.kv = GF_RESCUE_MARK;
            c.length = fits ? len : 0u;
            c.seq_off = fits ? so : 0ull;
            ctg[rec] = c;
        }
    }
}

__global__ void rs_append_counts_kernel(uint32_t* d_n, uint64_t contig_cap, uint64_t* d_s, uint64_t seq_cap, const uint32_t* bflag, const uint32_t* bidx,
                                        uint32_t len, uint32_t* stats) {
    const uint64_t n1 = *d_n, s1 = *d_s, n_hq = stats[GF_RS_HQ];
    const uint64_t nb = n_hq ? (uint64_t)bidx[n_hq - 1] + bflag[n_hq - 1] : 0;
    stats[GF_RS_FIRST] = (uint32_t)n1;
    stats[GF_RS_BRIDGES] = (uint32_t)nb;
    if (n1 > contig_cap || s1 > seq_cap) { stats[GF_RS_APPEND_ERR] = 1; return; }
    *d_n = (uint32_t)(n1 + nb);
    *d_s = s1 + nb * len;
    if (n1 + nb > contig_cap || s1 + nb * len > seq_cap) stats[GF_RS_APPEND_ERR] = 2;
}

__global__ __launch_bounds__(256) void rs_gap_stats_kernel(const uint64_t* best, uint64_t n_gaps, const uint32_t* gap_bridges, uint32_t* stats) {
    uint32_t tried = 0, with = 0;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < n_gaps; g += (uint64_t)gridDim.x * blockDim.x) {
        tried += best[g] == 0;
        with += gap_bridges[g] != 0;
    }
    if (tried) atomicAdd(stats + GF_RS_TRIED, tried);
    if (with) atomicAdd(stats + GF_RS_GAPS_BRIDGED, with);
}

bool rs_caps_ok(size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2) {
    return n_gaps > 0 && n_gaps < (1ull << 24) && hq_cap > 0 && hq_cap <= 0xFFFFFFFFull && seed_cap > 0 && seed_cap <= 0xFFFFFFFFull && log2 >= 4 &&
           log2 <= 32;
}

}  // namespace
}  // namespace gf

using namespace gf;

extern "C" {

size_t gf_rescue_work_bytes(size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2_slots) {
    if (!rs_caps_ok(n_gaps, hq_cap, seed_cap, log2_slots)) return 0;
    return rs_carve(nullptr, n_gaps, hq_cap, seed_cap, log2_slots).bytes + 256;
}

int gf_rescue_reset_dev(gf_ctx* ctx, void* d_work, size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2_slots, void* d_stats) {
    if (!ctx || !d_work || !d_stats) return GF_E_INVAL;
    if (!rs_caps_ok(n_gaps, hq_cap, seed_cap, log2_slots)) return GF_E_UNSUPPORTED;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    const RsWork w = rs_carve(d_work, n_gaps, hq_cap, seed_cap, log2_slots);
    GF_HIP(ctx, hipMemsetAsync(d_stats, 0, GF_RS_WORDS * 4, ctx->stream));
    GF_HIP(ctx, hipMemsetAsync(w.keys, 0xFF, hq_cap * 8, ctx->stream));
    return GF_OK;
}

int gf_rescue_hq_keys_dev(gf_ctx* ctx, const void* d_thits, const void* d_n_thits, size_t thit_cap, const void* d_recs, size_t n_reads, int lib,
                          size_t n_gaps, void* d_work, size_t hq_cap, size_t seed_cap, int log2_slots, void* d_stats) {
    if (!ctx || !d_n_thits || !d_work || !d_stats || (thit_cap && (!d_thits || !d_recs))) return GF_E_INVAL;
    if (!rs_caps_ok(n_gaps, hq_cap, seed_cap, log2_slots) || lib < 0 || lib >= GF_R2_MAX_LIBS || n_reads > (1ull << 36)) return GF_E_UNSUPPORTED;
    if (!thit_cap) return GF_OK;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    const RsWork w = rs_carve(d_work, n_gaps, hq_cap, seed_cap, log2_slots);
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    hipLaunchKernelGGL(rs_keys_kernel, dim3(rs_grid(ctx, thit_cap)), dim3(256), 0, ctx->stream, (const gf_taghit*)d_thits, (const uint32_t*)d_n_thits,
                       (uint64_t)thit_cap, (const gf_alnrec*)d_recs, (uint64_t)n_reads, (uint32_t)lib, (uint64_t)n_gaps, w.keys, (uint64_t)hq_cap,
                       (uint32_t*)d_stats);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_rescue_bridges_dev(gf_ctx* ctx, void* d_contigs, void* d_n_contigs, size_t contig_cap, void* d_seq, void* d_seq_len, size_t seq_cap,
                          const void* d_gap_best, size_t n_gaps, const void* const* d_lib_reads, const void* const* d_lib_nmask, int n_lib, int read_len,
                          void* d_work, size_t hq_cap, size_t seed_cap, int log2_slots, void* d_sets_stats, void* d_stats) {
    if (!ctx || !d_contigs || !d_n_contigs || !d_seq || !d_seq_len || !d_gap_best || !d_lib_reads || !d_work || !d_sets_stats || !d_stats)
        return GF_E_INVAL;
    if (!rs_caps_ok(n_gaps, hq_cap, seed_cap, log2_slots) || n_lib < 1 || n_lib > GF_R2_MAX_LIBS || read_len < (int)RS_SEED ||
        read_len > (int)RS_MAX_READ || contig_cap > 0x7FFFFFFFull)
        return GF_E_UNSUPPORTED;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    RsLibs libs{};
    for (int l = 0; l < n_lib; ++l) {
        if (!d_lib_reads[l]) return GF_E_INVAL;
        libs.reads[l] = (const uint8_t*)d_lib_reads[l];
        libs.nmask[l] = d_lib_nmask ? (const uint32_t*)d_lib_nmask[l] : nullptr;
    }
    const RsWork w = rs_carve(d_work, n_gaps, hq_cap, seed_cap, log2_slots);
    const uint32_t len = (uint32_t)read_len, rb = (uint32_t)gf_packed_read_bytes(read_len), nmw = (uint32_t)((read_len + 31) / 32);
    uint32_t* st = (uint32_t*)d_stats;
    const uint64_t* best = (const uint64_t*)d_gap_best;
    // the alignment sets first (they need the merge workspace; every later launch of this call reads them from there)
    gf_ovl_params pr{};
    MgSetsView V{};
    int rc;
    if ((rc = launch_merge_sets(ctx, d_contigs, d_n_contigs, contig_cap, d_seq, d_seq_len, seq_cap, d_gap_best, n_gaps, &pr, d_sets_stats, &V))) return rc;
    size_t t_sort = 0, t_pairs = 0, t_scan = 0;
    GF_HIP(ctx, rocprim::radix_sort_keys(nullptr, t_sort, w.keys, w.sorted, hq_cap, 0, 64, ctx->stream));
    GF_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t_pairs, w.sd_loc, w.sd_loc2, w.sd_win, w.sd_win2, seed_cap, 0, 64, ctx->stream));
    GF_HIP(ctx, rocprim::exclusive_scan(nullptr, t_scan, w.flag, w.uidx, 0u, hq_cap, rocprim::plus<uint32_t>(), ctx->stream));
    if ((rc = ensure(ctx, ctx->rs_tmp, std::max(t_sort, std::max(t_pairs, t_scan)) + 64))) return rc;
    LaunchTimer tm(ctx, GF_KERNEL_POOL);
    // HQ reads of the tried gaps
    GF_HIP(ctx, hipMemsetAsync(w.gap_hq, 0, n_gaps * 4, ctx->stream));
    GF_HIP(ctx, hipMemsetAsync(w.gap_bridges, 0, n_gaps * 4, ctx->stream));
    GF_HIP(ctx, hipMemsetAsync(w.tab, 0, sizeof(RsSlot) << log2_slots, ctx->stream));
    GF_HIP(ctx, rocprim::radix_sort_keys(ctx->rs_tmp.p, t_sort, w.keys, w.sorted, hq_cap, 0, 64, ctx->stream));
    const unsigned gk = rs_grid(ctx, hq_cap);
    hipLaunchKernelGGL(rs_mark_kernel, dim3(gk), dim3(256), 0, ctx->stream, w.sorted, (uint64_t)hq_cap, best, (uint64_t)n_gaps, w.flag, w.gap_hq, st);
    GF_HIP(ctx, rocprim::exclusive_scan(ctx->rs_tmp.p, t_scan, w.flag, w.uidx, 0u, hq_cap, rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(rs_compact_kernel, dim3(gk), dim3(256), 0, ctx->stream, w.sorted, (uint64_t)hq_cap, w.flag, w.uidx, w.hq);
    // their windows, then the seeds of the sets that share one
    hipLaunchKernelGGL(rs_windows_kernel, dim3(rs_grid(ctx, (uint64_t)hq_cap * (len - RS_SEED + 1))), dim3(256), 0, ctx->stream, w.hq, st, libs, len, rb, nmw, w.tab, (uint32_t)log2_slots, st);
    GF_HIP(ctx, hipMemsetAsync(w.sd_loc, 0xFF, seed_cap * 8, ctx->stream));
    GF_HIP(ctx, hipMemsetAsync(w.sd_win, 0xFF, seed_cap * 8, ctx->stream));
    hipLaunchKernelGGL(rs_seeds_kernel, dim3((unsigned)std::min<size_t>(n_gaps, (size_t)ctx->n_cu * 8)), dim3(256), 0, ctx->stream, (const gf_contig*)d_contigs,
                       (const char*)d_seq, V, (const uint32_t*)d_sets_stats, w.gap_hq, (uint64_t)n_gaps, w.tab, (uint32_t)log2_slots, w.sd_loc, w.sd_win,
                       (uint64_t)seed_cap, st);
    // (offset key, then window: a stable second pass leaves every window's run in (gap, contig, strand, offset) order)
    GF_HIP(ctx, rocprim::radix_sort_pairs(ctx->rs_tmp.p, t_pairs, w.sd_loc, w.sd_loc2, w.sd_win, w.sd_win2, seed_cap, 0, 64, ctx->stream));
    GF_HIP(ctx, rocprim::radix_sort_pairs(ctx->rs_tmp.p, t_pairs, w.sd_win2, w.sd_win, w.sd_loc2, w.sd_loc, seed_cap, 0, 64, ctx->stream));
    // bridges: flags in w.flag, their scan in w.uidx (the unique flags are done with)
    GF_HIP(ctx, hipMemsetAsync(w.flag, 0, hq_cap * 4, ctx->stream));
    const unsigned gb = (unsigned)std::min<size_t>(hq_cap, (size_t)ctx->n_cu * 32);
    hipLaunchKernelGGL(rs_bridge_kernel, dim3(gb), dim3(64), 0, ctx->stream, (const gf_contig*)d_contigs, (const char*)d_seq, V, w.hq, st, libs, len, rb,
                       nmw, w.sd_win, w.sd_loc, (uint64_t)seed_cap, w.flag, w.gap_bridges, st);
    GF_HIP(ctx, rocprim::exclusive_scan(ctx->rs_tmp.p, t_scan, w.flag, w.uidx, 0u, hq_cap, rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(rs_append_kernel, dim3(gb), dim3(64), 0, ctx->stream, (gf_contig*)d_contigs, (const uint32_t*)d_n_contigs, (uint64_t)contig_cap,
                       (char*)d_seq, (const uint64_t*)d_seq_len, (uint64_t)seq_cap, w.hq, st, w.flag, w.uidx, libs, len, rb, nmw);
    hipLaunchKernelGGL(rs_append_counts_kernel, dim3(1), dim3(1), 0, ctx->stream, (uint32_t*)d_n_contigs, (uint64_t)contig_cap, (uint64_t*)d_seq_len,
                       (uint64_t)seq_cap, w.flag, w.uidx, len, st);
    hipLaunchKernelGGL(rs_gap_stats_kernel, dim3(rs_grid(ctx, n_gaps)), dim3(256), 0, ctx->stream, best, (uint64_t)n_gaps, w.gap_bridges, st);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

const void* gf_rescue_gap_bridges(void* d_work, size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2_slots) {
    if (!d_work || !rs_caps_ok(n_gaps, hq_cap, seed_cap, log2_slots)) return nullptr;
    return rs_carve(d_work, n_gaps, hq_cap, seed_cap, log2_slots).gap_bridges;
}

}  // extern "C"
