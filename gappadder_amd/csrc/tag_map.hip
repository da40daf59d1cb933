// tag_map.hip — what the tagger reads beside the records: the key columns of a record array (8-byte keys; 4-byte linear keys with their
// layout) and the bin maps of the gap windows.
#include <cstring>

#include "gf_internal.hpp"

namespace gf {

// the key column of a record array: {pos, ref | (mapq == 0) << 31}; an unplaced record ('*': ref 0xFFFFFFFF) keeps an invalid scaffold; entry
// n (the pad of an odd count: the tagger loads two keys at a time) is invalid too
__global__ __launch_bounds__(256) void alnrec_keys_kernel(const gf_alnrec* recs, uint64_t n, uint2* keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    uint2 k = make_uint2(0u, 0x7FFFFFFFu);
    if (i < n) {
        const uint4 a = reinterpret_cast<const uint4*>(recs)[2 * i], b = reinterpret_cast<const uint4*>(recs)[2 * i + 1];
        const uint32_t ref = a.w < 0x7FFFFFFFu ? a.w : 0x7FFFFFFFu, mapq = (b.y >> 16) & 0xFFu;
        k = make_uint2(a.x, ref | (mapq == 0 ? 0x80000000u : 0u));
    }
    keys[i] = k;
}

int launch_alnrec_keys(gf_ctx* ctx, const void* d_recs, size_t n, void* d_keys) {
    LaunchTimer tm(ctx, GF_KERNEL_INGEST);
    hipLaunchKernelGGL(alnrec_keys_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, ctx->stream, (const gf_alnrec*)d_recs, (uint64_t)n, (uint2*)d_keys);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

// ---- the linear key column (gf_tag_layout)
// exclusive end of every scaffold: max(pos) + 1 over the placed records.  A wave walks ENDS_RUN consecutive records, 64 at a time, every lane
// keeping the maximum of the scaffold it is on (it hands the maximum over when its scaffold changes).  A BAM is sorted, so at the end the lanes
// of a wave are on one scaffold as a rule: one atomic per wave and run then — a wave per 64 records and its atomic, 14 M of them on 620
// addresses at C4, took 370 ms —, one per lane where the run straddles a boundary.
constexpr uint32_t ENDS_RUN = 4096;
__global__ __launch_bounds__(256) void alnrec_ends_kernel(const gf_alnrec* recs, uint64_t n, uint32_t n_scaffolds, uint32_t* ends) {
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint32_t ref = 0xFFFFFFFFu, end = 0;
    for (uint32_t it = 0; it < ENDS_RUN / 64; ++it) {
        const uint64_t i = wave * ENDS_RUN + 64ull * it + (threadIdx.x & 63);
        if (i >= n) break;
        const uint4 a = reinterpret_cast<const uint4*>(recs)[2 * i];
        if (a.w >= n_scaffolds) continue;
        const uint32_t e = a.x == 0xFFFFFFFFu ? a.x : a.x + 1;
        if (a.w != ref) {
            if (ref != 0xFFFFFFFFu) atomicMax(ends + ref, end);
            ref = a.w;
            end = e;
        } else if (e > end) end = e;
    }
    const unsigned long long placed = __ballot(ref != 0xFFFFFFFFu);
    if (!placed) return;
    const uint32_t ref0 = __shfl(ref, __ffsll((long long)placed) - 1);
    if (__all(ref == ref0 || ref == 0xFFFFFFFFu)) {
        for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(end, d); end = o > end ? o : end; }
        if ((threadIdx.x & 63) == 0) atomicMax(ends + ref0, end);
    } else if (ref != 0xFFFFFFFFu) atomicMax(ends + ref, end);
}

// keys and bit plane: thread i writes key i (the pad included) and, as lanes 0 and 32 of its wave, the plane words of the wave's 64 records
__global__ __launch_bounds__(256) void alnrec_linkeys_kernel(const gf_alnrec* recs, uint64_t n, uint32_t n_scaffolds, const uint32_t* base,
                                                             uint32_t* keys, uint64_t key_words, uint32_t* plane, uint64_t plane_words) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t key = 0xFFFFFFFFu;
    bool z = false;
    if (i < n) {
        const uint4 a = reinterpret_cast<const uint4*>(recs)[2 * i], b = reinterpret_cast<const uint4*>(recs)[2 * i + 1];
        if (a.w < n_scaffolds) {
            key = base[a.w] + a.x;
            z = ((b.y >> 16) & 0xFFu) == 0;
        }
    }
    if (i < key_words) keys[i] = key;
    const unsigned long long zb = __ballot(z);
    const uint32_t lane = threadIdx.x & 63;
    if ((lane & 31) == 0 && (i >> 5) < plane_words) plane[i >> 5] = (uint32_t)(zb >> lane);
}

LinCol lin_col(size_t n, uint32_t n_scaffolds) {
    LinCol c;
    c.key_words = ((n + 3) & ~(size_t)3) + 4;                   // the next multiple of 4 keys plus one 16-byte load
    c.plane_off = (c.key_words * 4 + 31) & ~(size_t)31;
    c.plane_words = (n + 255) / 256 * 8;                        // a whole 32-byte piece per 256 records
    c.base_off = c.plane_off + c.plane_words * 4;
    c.bytes = c.base_off + ((size_t)n_scaffolds + 1) * 4;
    return c;
}

constexpr int LIN_GRANULE_MAX = 20, LIN_GRANULE_MIN = 6, LIN_LDS_BITS_LOG2 = 17;   // (6: the narrowest bins ensure_bin_map makes; 17: its default)
static uint64_t lin_checksum(const uint32_t* base, size_t n_words) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n_words; ++i)
        for (int b = 0; b < 4; ++b) { h ^= (base[i] >> (8 * b)) & 0xFFu; h *= 0x100000001b3ull; }
    return h;
}

int tag_layout_from_ends(const uint32_t* ends, uint32_t n_scaffolds, uint64_t n_recs, gf_tag_layout* out, uint32_t* base_out) {
    gf_tag_layout L = {};
    L.n_recs = n_recs;
    L.n_scaffolds = n_scaffolds;
    std::vector<uint32_t> base((size_t)n_scaffolds + 1, 0);
    // the largest granule whose line fits 32 bits with the sentinel's bin to spare and is no narrower than the bins of the default LDS map
    // over that line (a wider granule wastes more of the line per scaffold: many small scaffolds end up with a small one)
    for (int a = LIN_GRANULE_MAX; a >= LIN_GRANULE_MIN && !L.use; --a) {
        const uint64_t gr = 1ull << a;
        uint64_t total = 0;
        for (uint32_t s = 0; s < n_scaffolds; ++s) total += ((uint64_t)ends[s] + gr - 1) & ~(gr - 1);
        if (total >= (1ull << 32) - gr) continue;
        int need = LIN_GRANULE_MIN;
        while ((total >> need) + 1 > (1ull << LIN_LDS_BITS_LOG2)) ++need;
        if (need > a) continue;
        L.use = 1;
        L.granule_log2 = (uint32_t)a;
        L.span = total;
        uint64_t at = 0;
        for (uint32_t s = 0; s < n_scaffolds; ++s) { base[s] = (uint32_t)at; at += ((uint64_t)ends[s] + gr - 1) & ~(gr - 1); }
        base[n_scaffolds] = (uint32_t)at;
    }
    L.checksum = L.use ? lin_checksum(base.data(), base.size()) : 0;
    *out = L;
    if (base_out && L.use) memcpy(base_out, base.data(), base.size() * 4);
    return GF_OK;
}

int launch_alnrec_linkeys(gf_ctx* ctx, const void* d_recs, size_t n, void* d_col, gf_tag_layout* built_for) {
    if (n >= 0xFFFFFFFFull) return GF_E_INVAL;
    const uint32_t ns = ctx->n_scaffolds;
    const LinCol c = lin_col(n, ns);
    uint32_t* d_base = (uint32_t*)((uint8_t*)d_col + c.base_off);
    std::vector<uint32_t> ends((size_t)ns + 1, 0), base((size_t)ns + 1, 0);
    LaunchTimer tm(ctx, GF_KERNEL_INGEST);
    GF_HIP(ctx, hipMemsetAsync(d_base, 0, ((size_t)ns + 1) * 4, ctx->stream));   // (the ends are measured in the place of base[])
    if (n) hipLaunchKernelGGL(alnrec_ends_kernel, dim3((unsigned)((n + 4 * ENDS_RUN - 1) / (4 * ENDS_RUN))), dim3(256), 0, ctx->stream, (const gf_alnrec*)d_recs, (uint64_t)n, ns, d_base);
    GF_HIP(ctx, hipGetLastError());
    GF_HIP(ctx, hipMemcpyAsync(ends.data(), d_base, ((size_t)ns + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = tag_layout_from_ends(ends.data(), ns, n, built_for, base.data());
    if (rc || !built_for->use) return rc;
    GF_HIP(ctx, hipMemcpyAsync(d_base, base.data(), base.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const size_t threads = std::max(c.key_words, c.plane_words * 32);
    hipLaunchKernelGGL(alnrec_linkeys_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, (const gf_alnrec*)d_recs, (uint64_t)n,
                       ns, d_base, (uint32_t*)d_col, (uint64_t)c.key_words, (uint32_t*)((uint8_t*)d_col + c.plane_off), (uint64_t)c.plane_words);
    GF_HIP(ctx, hipGetLastError());
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (base goes out of scope)
    return GF_OK;
}

// ---- the bin maps (gf_ctx::TagMap)
static void free_tag_map(gf_ctx::TagMap& m) {
    if (m.map.p) (void)hipFree(m.map.p);
    if (m.fine.p) (void)hipFree(m.fine.p);
    m.map = m.fine = DevBuf{};
}

void drop_tag_maps(gf_ctx* ctx) {
    if (ctx->tag_maps.empty()) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (gf_ctx::TagMap& m : ctx->tag_maps) free_tag_map(m);
    ctx->tag_maps.clear();
}

// The axis a map's bins lie on, and the one place that knows which of the two it is.  Without a layout every scaffold has bits of its own,
// for positions 0 .. its last window end, and the map's middle part holds their offsets.  With the layout of a linear key column (lin) the
// map is indexed by `key >> shift` over the line of scaffolds: a gap's windows are clamped to its own scaffold's stretch
// [base[s], base[s + 1]) — a left window that starts below position 0 must not reach the scaffold before, a right window that passes the
// scaffold's last record not the one behind —, the bits end with the last window of the line, and the middle part is the layout's base[].
struct BinAxis {
    bool lin = false;
    uint32_t granule = 0;          // lin: log2 of what every base[] is a multiple of
    int64_t d2 = 0;
    std::vector<uint32_t> base;    // lin: the layout's base[], n_scaffolds + 1
    std::vector<uint64_t> span;    // per scaffold: exclusive end of the positions its windows cover ...
    uint64_t lin_end = 0;          // ... lin: and of the keys they cover

    BinAxis(const std::vector<gf_gap>& gaps, uint32_t n_scaffolds, int dist2, std::vector<uint32_t> layout_base, uint32_t granule_log2)
        : lin(!layout_base.empty()), granule(granule_log2), d2(dist2 > 0 ? dist2 : 0), base(std::move(layout_base)), span(n_scaffolds, 0) {
        for (const gf_gap& g : gaps) {
            span[g.scaffold] = std::max<uint64_t>(span[g.scaffold], (uint64_t)g.end + d2);
            int64_t lo, hi;
            if (lin && window(g, lo, hi)) lin_end = std::max<uint64_t>(lin_end, (uint64_t)base[g.scaffold] + hi + 1);
        }
    }
    // positions lo .. hi (inclusive) of its scaffold that the windows of a gap cover: false when there are none
    bool window(const gf_gap& g, int64_t& lo, int64_t& hi) const {
        lo = std::max<int64_t>(0, (int64_t)g.start - d2 + 1);
        hi = (int64_t)g.end + d2 - 1;
        if (d2 == 0) return false;
        if (!lin) return true;
        hi = std::min(hi, (int64_t)base[g.scaffold + 1] - (int64_t)base[g.scaffold] - 1);
        return lo <= hi;
    }
    uint64_t nbits(int sh) const {
        if (lin) return (lin_end >> sh) + (lin_end ? 1 : 0);
        uint64_t t = 0; for (uint64_t v : span) t += (v >> sh) + (v ? 1 : 0); return t;
    }
    // bins [first[s], first[s + 1]) are scaffold s's, the bin of its position p is first[s] + (p >> sh).  (lin: the scaffold's bins of the
    // line as far as the line's bits go — granule >= bin: they are its own, and its base is the start of its first bin)
    std::vector<uint32_t> first_bins(int sh) const {
        std::vector<uint32_t> first(span.size() + 1, 0);
        const uint64_t n = nbits(sh);
        for (size_t s = 0; s < span.size(); ++s) first[s + 1] = lin ? 0 : first[s] + (uint32_t)((span[s] >> sh) + (span[s] ? 1 : 0));
        if (lin) for (size_t s = 0; s < first.size(); ++s) first[s] = (uint32_t)std::min<uint64_t>(base[s] >> sh, n);
        return first;
    }
    bool fits(int sh) const { return !lin || sh <= (int)granule; }          // no bin covers two scaffolds
    uint32_t key_bins(int sh) const { return lin ? (uint32_t)nbits(sh) : 0; }   // bins a key of the line is tested against (TagParams::n_bins)
    const std::vector<uint32_t>& middle(const std::vector<uint32_t>& first) const { return lin ? base : first; }
};

// step 2: the layout's base[], as the column carries it; GF_E_INVAL where it is not what the layout was built from
static int fetch_layout_base(gf_ctx* ctx, const gf_tag_layout* lay, const uint32_t* d_base, std::vector<uint32_t>& base) {
    base.resize((size_t)ctx->n_scaffolds + 1);
    GF_HIP(ctx, hipMemcpyAsync(base.data(), d_base, base.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    bool ok = lin_checksum(base.data(), base.size()) == lay->checksum && base[0] == 0 && base[ctx->n_scaffolds] == lay->span;
    for (uint32_t s = 0; ok && s < ctx->n_scaffolds; ++s) ok = base[s] <= base[s + 1] && (base[s] & ((1u << lay->granule_log2) - 1)) == 0;
    return ok ? GF_OK : GF_E_INVAL;
}

// step 3: room for one more map — drop the one that was not used for the longest time
static int evict_tag_map(gf_ctx* ctx) {
    if (ctx->tag_maps.size() < 4) return GF_OK;
    size_t old = 0;
    for (size_t i = 1; i < ctx->tag_maps.size(); ++i) if (ctx->tag_maps[i].used < ctx->tag_maps[old].used) old = i;
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_tag_map(ctx->tag_maps[old]);
    ctx->tag_maps.erase(ctx->tag_maps.begin() + (long)old);
    return GF_OK;
}

// step 6: one map = bit words (one zero word behind the last bin) followed by the n_scaffolds + 1 words of the axis' middle part
static void build_bits(const gf_ctx* ctx, const BinAxis& A, int shift, std::vector<uint32_t>& h, uint32_t& words) {
    const std::vector<uint32_t> first = A.first_bins(shift);
    words = (uint32_t)((A.nbits(shift) + 31) / 32 + 1);
    h.assign(words, 0);
    for (const gf_gap& g : ctx->gaps) {
        int64_t lo, hi;
        if (!A.window(g, lo, hi)) continue;
        for (int64_t b = lo >> shift; b <= (hi >> shift); ++b) {
            const uint32_t bit = first[g.scaffold] + (uint32_t)b;
            h[bit >> 5] |= 1u << (bit & 31);
        }
    }
    const std::vector<uint32_t>& mid = A.middle(first);
    h.insert(h.end(), mid.begin(), mid.end());
}
static uint64_t count_bits(const std::vector<uint32_t>& h, uint32_t words) {
    uint64_t set = 0;
    for (uint32_t i = 0; i < words; ++i) set += (uint64_t)__builtin_popcount(h[i]);
    return set;
}

// step 7: per bin, the first gap of the scaffold whose RIGHT window still reaches the bin's first position (end + dist2 > bin << shift;
// ends ascend) — where the window search of a record in that bin starts.  It replaces a binary search over the scaffold's gaps (five
// dependent loads at 32 gaps per scaffold) by one load.
static std::vector<uint32_t> bin_first_gaps(const gf_ctx* ctx, const BinAxis& A, int shift) {
    const std::vector<uint32_t> first = A.first_bins(shift);
    std::vector<uint32_t> out(A.nbits(shift), 0);
    size_t g = 0;
    for (uint32_t s = 0; s < ctx->n_scaffolds; ++s) {
        while (g < ctx->gaps.size() && ctx->gaps[g].scaffold < s) ++g;
        for (uint32_t b = first[s]; b < first[s + 1]; ++b) {
            while (g < ctx->gaps.size() && ctx->gaps[g].scaffold == s && (int64_t)ctx->gaps[g].end + A.d2 <= ((int64_t)(b - first[s]) << shift)) ++g;
            out[b] = (uint32_t)g;   // (== the scaffold's last gap + 1 when no window reaches the bin)
        }
    }
    return out;
}

// step 9: a host image to a device buffer of the map
static int upload_words(gf_ctx* ctx, DevBuf& b, const std::vector<uint32_t>& h) {
    const int rc = ensure(ctx, b, h.size() * 4);
    if (rc) return rc;
    GF_HIP(ctx, hipMemcpyAsync(b.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    GF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GF_OK;
}

// Coarse bin map of the gap windows for one dist2 (host build: n_gaps work; kept until the gaps change, the four last used dist2), in the
// steps the numbers name.  With a layout (lay, d_base: a linear key column's) it is the map of that layout's line (BinAxis).
int ensure_bin_map(gf_ctx* ctx, int dist2, gf_ctx::TagMap** out, const gf_tag_layout* lay, const uint32_t* d_base) {
    const uint32_t lin_granule = lay ? lay->granule_log2 : 0;
    const uint64_t lin_checksum_want = lay ? lay->checksum : 0;
    if (lay && (!lay->use || !d_base || lay->n_scaffolds != ctx->n_scaffolds || lin_granule < (uint32_t)LIN_GRANULE_MIN || lin_granule > (uint32_t)LIN_GRANULE_MAX))
        return GF_E_INVAL;
    // 1: the cache
    for (gf_ctx::TagMap& m : ctx->tag_maps)
        if (m.dist2 == dist2 && m.map.p && m.lin_granule == lin_granule && m.lin_checksum == lin_checksum_want) { m.used = ++ctx->tag_map_clock; *out = &m; return GF_OK; }
    // 2, 3, 4
    std::vector<uint32_t> base;
    int rc = lay ? fetch_layout_base(ctx, lay, d_base, base) : GF_OK;
    if (rc || (rc = evict_tag_map(ctx))) return rc;
    const BinAxis A(ctx->gaps, ctx->n_scaffolds, dist2, std::move(base), lin_granule);
    // 5: the shift
    int shift = 6;
    while (A.nbits(shift) > (1u << ctx->tag_bins_log2)) ++shift;  // <= 16 KiB of LDS by default (measured: an 8 KiB map sends more records down the slow path and loses)
    if (!A.fits(shift)) return GF_E_UNSUPPORTED;   // a bin would cover two scaffolds
    uint32_t words = 0;
    std::vector<uint32_t> h;
    build_bits(ctx, A, shift, h, words);
    // Many gaps on a large genome (human scale: 19 840 windows over 3.1 Gb) leave a 16-KiB map with 24-kb bins, a fifth of them
    // set: then a 64-KiB map (6-kb bins, a twentieth set) shared by ONE 16-wave workgroup per CU takes its place — the same 16 waves
    // and 132 KiB of LDS per CU as four 4-wave workgroups with 16 KiB each (which is why a 64-KiB map per 4-wave workgroup lost:
    // half the waves).  Only when the option was left at its default.
    if (ctx->tag_bins_log2 == 17 && shift > 8 && count_bits(h, words) * 10 > A.nbits(shift)) {
        while (shift > 6 && A.nbits(shift - 1) <= (1u << 19)) --shift;
        build_bits(ctx, A, shift, h, words);   // 6
    }
    const uint64_t set_bits = count_bits(h, words);
    // 7: behind the middle part
    const std::vector<uint32_t> bin_first = bin_first_gaps(ctx, A, shift);
    h.insert(h.end(), bin_first.begin(), bin_first.end());
    gf_ctx::TagMap M;
    // 8: Human-scale genomes leave the LDS map with ~24 kb bins, a third of them set by 20 000 gaps: a second, finer map in
    // global memory (<= 2^25 bits, stays in L2) restores the per-mille pass rate before the window search.
    std::vector<uint32_t> hf;
    if (shift > 9 && set_bits * 20 > A.nbits(shift)) {   // worth a second look-up only when the LDS map passes > 5 %
        int fs = 7;
        while (A.nbits(fs) > (1u << ctx->tag_fine_log2)) ++fs;
        if (fs + 2 <= shift) {
            uint32_t fw = 0;
            build_bits(ctx, A, fs, hf, fw);
            // ... and only when the finer bins stop a good part of what the LDS map lets through.  Long-insert libraries do not:
            // their windows (2 x dist2 + the gap, 15 kb at IS 5 000) are wider than the LDS map's bins, 13 % of the records pass the
            // LDS map and 10 % lie in a window — the second look-up and the re-load of the record it implies (13 % of the records a
            // second time, at random) cost more than the window search of the 3 % it would stop.
            const double cover_lds = (double)set_bits * (double)(1ull << shift), cover_fine = (double)count_bits(hf, fw) * (double)(1ull << fs);
            if (cover_fine <= 0.6 * cover_lds) {
                M.fine_words = fw;
                M.fine_shift = fs;
                M.fine_bins = A.key_bins(fs);
            } else hf.clear();
        }
    }
    // 9
    rc = upload_words(ctx, M.map, h);
    if (!rc && !hf.empty()) rc = upload_words(ctx, M.fine, hf);
    if (rc) { free_tag_map(M); return rc; }
    M.dist2 = dist2;
    M.shift = shift;
    M.words = words;
    M.lin_granule = lin_granule;
    M.lin_checksum = lin_checksum_want;
    M.n_bins = A.key_bins(shift);
    M.used = ++ctx->tag_map_clock;
    ctx->tag_maps.push_back(M);
    *out = &ctx->tag_maps.back();
    return GF_OK;
}

}  // namespace gf
