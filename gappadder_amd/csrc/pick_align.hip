// pick_align.hip — flank anchoring by ungapped seed-and-extend of the WHOLE flanks (the "align" mode of the picker): the stand-in
// for `bwa mem -T {score} -a` that aligns through a draft base that differs from the reads near a flank's gap-side end, where the
// exact anchors of pick.hip lose the gap.  Definition (bwa mem's defaults as constants, written out): the docstring of
// gappadder_amd/pick_contigs.py, host twin align_hits; the selection after the hits is select_full (pick_contigs.py:97-321), as in
// pick.hip.  Entry points: gf_pick_aligned_dev / gf_pick_aligned_from_dev, gf_pick_gapped_dev / gf_pick_gapped_from_dev
// (include/gapfill_hip.h).
//
// One one-wave workgroup per contig.  The four queries of the contig's gap (left, revcomp(left), right, revcomp(right); codes 0-3,
// 4 = non-ACGT) and a sorted table of their 19-mers are built once per gf_set_gaps.  Seeds: every lane rolls the 19-mers of a
// stretch of the contig and looks each one up in the table (binary search); a (query, position) hit is a seed when it STARTS a run
// of identical ACGT bases (the bases before it differ), so every maximal run of >= 19 identical bases on a diagonal is found
// exactly once.  The seeds (<= SEED_MAX per contig) are ranked in LDS by (query, diagonal, query start) — the production order of
// the definition —, extended one per lane, and lane 0 walks them in that order: the skip rule (a seed inside an alignment already
// produced on its diagonal), the cap per (query), the per-(side, clip type) best hit of select_full and its seven pairs.
//
// The "gapped" mode (gf_pick_gapped_dev, host twin gapped_hits) is the same body with another extension: a banded affine-gap DP
// (gap of g bases = 6 + g, 31 diagonals either side of the seed's) that aligns THROUGH an indel between flank and contig.  There the
// wave takes the seeds one after the other in rank order and spreads the BAND over its lanes: lane b holds diagonal i - j = b - 31 and
// sweeps anti-diagonals t = i + j, so a cell needs (i-1, j) from lane b - 1 and (i, j-1) from lane b + 1 of step t - 1 — two wave
// shuffles of a packed (H, gap state) word — and (i-1, j-1) from its own step t - 2.  H, E and F stay in registers; the codes of the
// query and the contig beyond the seed are staged in LDS in the direction of extension.  The maximum and the last-column maximum are
// kept per lane (a lane meets its cells in ascending i) and reduced over the wave on (score, i, j) keys, so the twin's first-maximum
// rule holds whatever the sweep order.  The skip rule (a seed inside an alignment kept for its query) and the cap decide whether a seed
// is extended at all, so they run there, against the query's kept alignments in LDS; the walk reads each seed's outcome.
#include <algorithm>
#include <cstring>

#include "contig_list.hpp"
#include "gf_internal.hpp"
#include "pick_word.hpp"

namespace gf {

constexpr int AL_SEED = 19, AL_MATCH = 1, AL_MISMATCH = -4, AL_NSCORE = -1, AL_ZDROP = 100, AL_CLIP = 5;
constexpr int AL_FLANK_MAX = 1024, AL_SEED_MAX = 1024, AL_CAP = 64;
constexpr int AL_TAB_META = -1, AL_TAB_KMERS = -2;      // keys of ctx->anchor_tabs (dropped with the exact anchors by gf_set_gaps)
constexpr int CT_LEFT = 0, CT_RIGHT = 1, CT_NONE = 2;    // clip types the selection keeps (BOTH is never used, pick_contigs.py:104)
constexpr int GP_OPEN = 6, GP_EXT = 1, GP_BAND = 31;     // gapped mode: bwa mem -O, -E; 2 * 31 + 1 diagonals = one wave (lane 63 idles)
constexpr int GP_CTG = AL_FLANK_MAX + GP_BAND + 1;       // contig bases a side can take: the query's and the band's
constexpr unsigned long long GP_SKIPPED = 1ull << 45, GP_DROPPED = 2ull << 45;   // a seed's outcome word: status above score, M, qb, qe

struct AlignMeta {
    uint32_t kbeg, kn;     // the gap's 19-mer entries: kmer << 12 | query << 10 | query position, ascending
    uint32_t qoff;         // the gap's query bytes: left, revcomp(left), right, revcomp(right) back to back
    uint16_t nl, nr;
};
static_assert(sizeof(AlignMeta) == 16, "AlignMeta");

struct AlignParams {
    ContigList list;
    const AlignMeta* meta;
    const uint8_t* qbytes;
    const unsigned long long* kmers;
    uint32_t n_gaps, t_long, t_short;
    unsigned long long* gap_best;
    uint32_t* n_closed;
    gf_ctg_pick* ctg_pick;
    uint32_t* stats;           // [0] alignments beyond the cap, [1] contigs with more than AL_SEED_MAX seeds
    ExtHit* ext_hits;          // the extended fill (pick_ext.hip): per contig its wanted hit per side, pushed on ...
    uint32_t* ext_heads;       // ... the lists of its gap (t_long = the threshold; gap_best is read, not written)
};

struct AlHit {
    uint32_t m, score, rev, pos;   // m == 0: none
};

__device__ __forceinline__ int al_score(uint32_t a, uint32_t b) {
    return (a > 3 || b > 3) ? AL_NSCORE : a == b ? AL_MATCH : AL_MISMATCH;
}

// one seed -> score << 33 | seed end << 22 | query begin << 11 | query end (pick_contigs.py::_extend)
__device__ uint64_t al_extend(const uint8_t* Q, int n, const char* s, int m, int d, int qs) {
    int se = qs;
    while (se < n && se + d < m && Q[se] < 4 && Q[se] == base_code4(s[se + d])) ++se;
    int run = se - qs, best = run, qb = qs, i = qs - 1;
    bool stopped = false;
    for (; i >= 0 && i + d >= 0; --i) {
        run += al_score(Q[i], base_code4(s[i + d]));
        if (run > best) { best = run; qb = i; }
        else if (best - run > AL_ZDROP) { stopped = true; break; }
    }
    int score = best;
    if (!stopped && i < 0 && run > 0 && run > best - AL_CLIP) { qb = 0; score = run; }
    run = best = score;
    int qe = se, j = se;
    stopped = false;
    for (; j < n && j + d < m; ++j) {
        run += al_score(Q[j], base_code4(s[j + d]));
        if (run > best) { best = run; qe = j + 1; }
        else if (best - run > AL_ZDROP) { stopped = true; break; }
    }
    score = best;
    if (!stopped && j == n && run > 0 && run > best - AL_CLIP) { qe = n; score = run; }
    return ((uint64_t)(uint32_t)score << 33) | ((uint64_t)se << 22) | ((uint64_t)qb << 11) | (uint64_t)qe;
}

// One side of the gapped extension (pick_contigs.py::_gapped_side), by the whole wave: qst[j - 1] / cst[i - 1] = the code of the j-th
// query / i-th contig base beyond the seed in the direction of extension (LDS), J / I = how many there are (I <= J + GP_BAND), h0 = the
// score so far.  Returns score << 22 | contig bases taken << 11 | query bases taken (64 bits: a score can be 1 024), the same in every lane.  A value <= 0 is dead and
// is held as 0; H <= 1 024, so H << 16 | gap state packs in one word.
__device__ __forceinline__ unsigned long long gp_side(const uint8_t* qst, const uint8_t* cst, int I, int J, int h0, int lane) {
    uint32_t hf = lane == GP_BAND ? (uint32_t)h0 << 16 : 0u, he = hf;     // H << 16 | F and H << 16 | E of the lane's last cell
    int best = lane == GP_BAND ? h0 : 0, best_i = 0;
    int g = (lane == GP_BAND && J == 0) ? h0 : 0, g_i = 0;
    const int t_end = min(I + J, 2 * min(I, J) + GP_BAND);
    bool prev_dead = false;
    for (int t = 1; t <= t_end; ++t) {
        uint32_t up = __shfl_up(hf, 1), left = __shfl_down(he, 1);       // (i-1, j) from lane b - 1, (i, j-1) from lane b + 1
        if (lane == 0) up = 0;
        const int i2 = t + lane - GP_BAND;                                // 2 i: i - j = lane - GP_BAND, i + j = t
        const bool mine = !(i2 & 1);                                      // (every other step is this lane's)
        const int i = i2 >> 1, j = t - i;
        int H = 0, E = 0, F = 0;
        if (mine && lane < 2 * GP_BAND + 1 && i >= 0 && j >= 0 && i <= I && j <= J) {
            F = max(max((int)(up >> 16) - (GP_OPEN + GP_EXT), (int)(up & 0xFFFFu) - GP_EXT), 0);
            E = max(max((int)(left >> 16) - (GP_OPEN + GP_EXT), (int)(left & 0xFFFFu) - GP_EXT), 0);
            const int diag = (int)(hf >> 16);                             // (i-1, j-1): this lane, two steps ago
            int M = 0;
            if (diag > 0 && i >= 1 && j >= 1) M = max(diag + al_score(qst[j - 1], cst[i - 1]), 0);
            H = max(M, max(E, F));
            if (H > best) { best = H; best_i = i; }                       // the lane's first maximum: its cells come in ascending i
            if (j == J && H > 0) { g = H; g_i = i; }                      // (one cell per lane in the last column)
        }
        if (mine) {
            hf = (uint32_t)H << 16 | (uint32_t)F;
            he = (uint32_t)H << 16 | (uint32_t)E;
        }
        const bool dead = !__any(mine && H > 0);
        if (dead && prev_dead) break;                                     // two dead anti-diagonals: nothing lives on
        prev_dead = dead;
    }
    // the first maximum in (i ascending, j ascending) order = the largest (score, -i, -j) key
    unsigned long long kb = (unsigned long long)best << 22 | (unsigned long long)(2047 - best_i) << 11 |
                            (unsigned long long)(2047 - (best_i - (lane - GP_BAND)));
    uint32_t kg = (uint32_t)g << 11 | (uint32_t)(2047 - g_i);
    for (int o = 32; o; o >>= 1) {
        const unsigned long long ob = __shfl_xor(kb, o);
        const uint32_t og = __shfl_xor(kg, o);
        kb = ob > kb ? ob : kb;
        kg = og > kg ? og : kg;
    }
    const int bs = (int)(kb >> 22), gs = (int)(kg >> 11);
    if (gs > 0 && gs > bs - AL_CLIP) return (unsigned long long)gs << 22 | (unsigned long long)(2047u - (kg & 2047u)) << 11 | (unsigned long long)J;
    return (unsigned long long)bs << 22 | (2047ull - ((kb >> 11) & 2047u)) << 11 | (2047ull - (kb & 2047u));
}

// the selection of one threshold (pick_contigs.py::select_per_contig): false when no same-strand pair with a span >= 0
__device__ bool al_select(const AlHit* left, const AlHit* right, uint32_t* lp, uint32_t* rp, uint32_t* lm, uint32_t* rm, uint32_t* rc,
                          int* span) {
    const int pairs[7][2] = {{CT_NONE, CT_NONE}, {CT_NONE, CT_LEFT}, {CT_NONE, CT_RIGHT}, {CT_LEFT, CT_NONE},
                             {CT_LEFT, CT_RIGHT}, {CT_RIGHT, CT_NONE}, {CT_RIGHT, CT_LEFT}};
    int top = -1;
    bool any = false;
    *rc = 0;
#pragma unroll
    for (int p = 0; p < 7; ++p) {
        const AlHit l = left[pairs[p][0]], r = right[pairs[p][1]];
        if (!l.m || !r.m || l.rev != r.rev || !(top < (int)(l.m + r.m))) continue;
        top = (int)(l.m + r.m);
        *lp = l.pos; *rp = r.pos; *lm = l.m; *rm = r.m;
        *rc |= l.rev;                       // (:176-177: set by any winning reverse pair, never cleared)
        any = true;
    }
    if (!any) return false;
    *span = *rc ? (int)*lp - (int)(*rp + *rm) : (int)*rp - (int)(*lp + *lm);
    return *span >= 0;
}

// EXT: the hits of the extended fill instead of the pick: per contig of an open gap and side the FIRST hit in align_hits' order (score
// descending, forward before reverse, pos ascending; production order on full ties) whose clip type is the wanted one — the flank clipped
// on its far side: LEFT for the left flank forward and rc(right flank), RIGHT for rc(left flank) and the right flank forward
// GAPPED: the gapped mode's extension (gp_side) and its skip rule and cap in place of the ungapped ones; everything else is shared
template <bool EXT, bool GAPPED>
__device__ __forceinline__ void pick_align_body(const AlignParams& P) {
    __shared__ unsigned long long keys[AL_SEED_MAX];   // seeds as found, then the extension results in rank order
    __shared__ unsigned long long srt[AL_SEED_MAX];    // seeds in (query, diagonal, query start) order
    __shared__ uint32_t cnt;
    // gapped mode: per seed the first contig base of its alignment; the alignments kept for the current query (query begin | end << 16,
    // contig begin, contig end) for the skip rule; the staged codes of one side
    __shared__ uint32_t cbeg[GAPPED ? AL_SEED_MAX : 1];
    __shared__ uint32_t kept_q[GAPPED ? AL_CAP : 1], kept_cb[GAPPED ? AL_CAP : 1], kept_ce[GAPPED ? AL_CAP : 1];
    __shared__ uint8_t qst[GAPPED ? AL_FLANK_MAX : 4], cst[GAPPED ? GP_CTG : 4];
    __shared__ AlHit tab[2][2][3];                     // [threshold][side][clip type] (lane 0)
    const uint32_t n_ctg = contig_list_end(P.list);
    const int lane = threadIdx.x;
    for (uint32_t ci = contig_list_begin(P.list) + blockIdx.x; ci < n_ctg; ci += gridDim.x) {
        const gf_contig c = P.list.contigs[ci];
        if (c.gap >= P.n_gaps || c.length < (uint32_t)AL_SEED) continue;        // (uniform over the workgroup)
        if (EXT && P.gap_best[c.gap]) continue;
        const AlignMeta M = P.meta[c.gap];
        if (!M.kn) continue;
        const char* s = P.list.seq + c.seq_off;
        const int m = (int)c.length, nl = M.nl, nr = M.nr;
        const uint8_t* qb0 = P.qbytes + M.qoff;
        const unsigned long long* km = P.kmers + M.kbeg;
        if (lane == 0) cnt = 0;
        __syncthreads();
        // ---- seeds: run starts among the 19-mer hits
        const int npos = m - AL_SEED + 1, chunk = (npos + 63) / 64;
        const int p0 = lane * chunk, p1 = min(npos, p0 + chunk);
        if (p0 < p1) {
            uint64_t kmer = 0;
            int run = 0;
            for (int j = p0; j < p1 + AL_SEED - 1; ++j) {
                const uint32_t b = base_code4(s[j]);
                if (b < 4) { kmer = ((kmer << 2) | b) & ((1ull << (2 * AL_SEED)) - 1); ++run; } else run = 0;
                if (j < p0 + AL_SEED - 1 || run < AL_SEED) continue;
                const int p = j - AL_SEED + 1;
                const unsigned long long lo = (unsigned long long)kmer << 12;
                uint32_t a = 0, z = M.kn;                  // first entry >= lo
                while (a < z) {
                    const uint32_t h = (a + z) >> 1;
                    if (km[h] < lo) a = h + 1; else z = h;
                }
                const uint32_t prev = p > 0 ? base_code4(s[p - 1]) : 4u;
                for (; a < M.kn && (km[a] >> 12) == kmer; ++a) {
                    const uint32_t qi = (uint32_t)(km[a] >> 10) & 3u, q = (uint32_t)km[a] & 1023u;
                    const uint8_t* Q = qb0 + (qi == 0 ? 0 : qi == 1 ? nl : qi == 2 ? 2 * nl : 2 * nl + nr);
                    if (p > 0 && q > 0 && Q[q - 1] < 4 && Q[q - 1] == prev) continue;     // not the start of its run
                    const uint32_t at = atomicAdd(&cnt, 1u);
                    if (at < (uint32_t)AL_SEED_MAX)
                        keys[at] = ((unsigned long long)qi << 62) | ((unsigned long long)(p - (int)q + AL_FLANK_MAX) << 11) | q;
                }
            }
        }
        __syncthreads();
        const uint32_t n = cnt;
        if (n > (uint32_t)AL_SEED_MAX) {
            if (lane == 0) atomicAdd(P.stats + 1, 1u);
            __syncthreads();
            continue;
        }
        // ---- rank sort (keys are distinct)
        for (uint32_t i = lane; i < n; i += 64) {
            const unsigned long long k = keys[i];
            uint32_t r = 0;
            for (uint32_t j = 0; j < n; ++j) r += keys[j] < k;
            srt[r] = k;
        }
        __syncthreads();
        if constexpr (GAPPED) {
            // ---- extension, the wave on one seed after the other (everything here is uniform over the wave)
            uint32_t cur_q = 4, produced = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const unsigned long long k = srt[i];
                const uint32_t qi = (uint32_t)(k >> 62);
                const int q = (int)((uint32_t)k & 2047u), d = (int)((k >> 11) & ((1ull << 51) - 1)) - AL_FLANK_MAX;
                const uint8_t* Q = qb0 + (qi == 0 ? 0 : qi == 1 ? nl : qi == 2 ? 2 * nl : 2 * nl + nr);
                const int nq = qi < 2 ? nl : nr;
                if (qi != cur_q) { cur_q = qi; produced = 0; }
                int se = q + AL_SEED;                             // the end of the seed's run of identical ACGT bases
                for (;;) {
                    const int x = se + lane;
                    const bool on = x < nq && x + d < m && Q[x] < 4 && Q[x] == base_code4(s[x + d]);
                    const unsigned long long off = __ballot(!on);
                    if (off) { se += __ffsll((long long)off) - 1; break; }
                    se += 64;
                }
                const uint32_t n_kept = produced < (uint32_t)AL_CAP ? produced : (uint32_t)AL_CAP;
                bool inside = false;
                if ((uint32_t)lane < n_kept) {
                    const uint32_t kq = kept_q[lane];
                    inside = (int)(kq & 0xFFFFu) <= q && se <= (int)(kq >> 16) && (int)kept_cb[lane] <= q + d && q + d < (int)kept_ce[lane];
                }
                if (__any(inside)) {                              // inside an alignment kept for this query
                    if (lane == 0) keys[i] = GP_SKIPPED;
                    continue;
                }
                if (++produced > (uint32_t)AL_CAP) {
                    if (lane == 0) keys[i] = GP_DROPPED;
                    continue;
                }
                // left of the seed: query bases q-1 .. 0 against contig bases q+d-1 .. 0
                int J = q, I = min(q + d, J + GP_BAND);
                for (int x = lane; x < J; x += 64) qst[x] = Q[q - 1 - x];
                for (int x = lane; x < I; x += 64) cst[x] = (uint8_t)base_code4(s[q + d - 1 - x]);
                __syncthreads();
                const unsigned long long lres = gp_side(qst, cst, I, J, se - q, lane);
                __syncthreads();
                const int qb = q - (int)(lres & 2047u), cb = q + d - (int)((lres >> 11) & 2047u);
                // right of it: query bases se .. against contig bases se+d ..
                J = nq - se;
                I = min(m - se - d, J + GP_BAND);
                for (int x = lane; x < J; x += 64) qst[x] = Q[se + x];
                for (int x = lane; x < I; x += 64) cst[x] = (uint8_t)base_code4(s[se + d + x]);
                __syncthreads();
                const unsigned long long rres = gp_side(qst, cst, I, J, (int)(lres >> 22), lane);
                const int qe = se + (int)(rres & 2047u), ce = se + d + (int)((rres >> 11) & 2047u);
                if (lane == 0) {
                    keys[i] = (unsigned long long)(rres >> 22) << 34 | (unsigned long long)(ce - cb) << 22 | (unsigned long long)qb << 11 |
                              (unsigned long long)qe;
                    cbeg[i] = (uint32_t)cb;
                    kept_q[produced - 1] = (uint32_t)qb | (uint32_t)qe << 16;
                    kept_cb[produced - 1] = (uint32_t)cb;
                    kept_ce[produced - 1] = (uint32_t)ce;
                }
                __syncthreads();
            }
        } else {
            // ---- extension, one seed per lane
            for (uint32_t i = lane; i < n; i += 64) {
                const unsigned long long k = srt[i];
                const uint32_t qi = (uint32_t)(k >> 62), q = (uint32_t)k & 2047u;
                const int d = (int)((k >> 11) & ((1ull << 51) - 1)) - AL_FLANK_MAX;
                const uint8_t* Q = qb0 + (qi == 0 ? 0 : qi == 1 ? nl : qi == 2 ? 2 * nl : 2 * nl + nr);
                keys[i] = al_extend(Q, qi < 2 ? nl : nr, s, m, d, (int)q);
            }
        }
        __syncthreads();
        if (lane == 0) {
            AlHit fh_l{0, 0, 0, 0}, fh_r{0, 0, 0, 0};                        // (EXT: two register sets, not an indexed array: no scratch)
            if (!EXT)
                for (int t = 0; t < 2; ++t)
                    for (int sd = 0; sd < 2; ++sd)
                        for (int ct = 0; ct < 3; ++ct) tab[t][sd][ct] = AlHit{0, 0, 0, 0};
            uint32_t produced[4] = {0, 0, 0, 0}, drops = 0;
            unsigned long long last = ~0ull;
            int max_qe = -1;
            for (uint32_t i = 0; i < n; ++i) {
                const unsigned long long k = srt[i], r = keys[i];
                const uint32_t qi = (uint32_t)(k >> 62);
                const int qb = (int)((r >> 11) & 2047u), qe = (int)(r & 2047u);
                uint32_t score, hm, hpos;                           // the hit: score, contig bases covered, 1-based first contig base
                if constexpr (GAPPED) {                             // (the skip rule and the cap ran with the extension)
                    if (r & GP_SKIPPED) continue;
                    if (r & GP_DROPPED) { ++drops; continue; }
                    score = (uint32_t)(r >> 34) & 2047u;
                    hm = (uint32_t)(r >> 22) & 4095u;
                    hpos = cbeg[i] + 1;
                } else {
                    if ((k >> 11) != last) { last = k >> 11; max_qe = -1; }
                    const int se = (int)((r >> 22) & 2047u);
                    score = (uint32_t)(r >> 33);
                    if (se <= max_qe) continue;                     // inside an alignment already produced on this diagonal
                    max_qe = qe > max_qe ? qe : max_qe;
                    const uint32_t np = qi == 0 ? ++produced[0] : qi == 1 ? ++produced[1] : qi == 2 ? ++produced[2] : ++produced[3];
                    if (np > (uint32_t)AL_CAP) { ++drops; continue; }
                    const int d = (int)((k >> 11) & ((1ull << 51) - 1)) - AL_FLANK_MAX;
                    hm = (uint32_t)(qe - qb);
                    hpos = (uint32_t)(d + qb + 1);
                }
                const int nq = qi < 2 ? nl : nr;
                const bool cl = qb > 0, cr = qe < nq;
                if (cl && cr) continue;                             // BOTH: never selected
                const int ct = cl ? CT_LEFT : cr ? CT_RIGHT : CT_NONE;
                const AlHit h{hm, score, qi & 1u, hpos};
                if (EXT) {
                    if (score < P.t_long || ct != ((qi == 0 || qi == 3) ? CT_LEFT : CT_RIGHT)) continue;
                    auto first = [&h](const AlHit& o) {
                        return !o.m || h.score > o.score || (h.score == o.score && (h.rev < o.rev || (h.rev == o.rev && h.pos < o.pos)));
                    };
                    if (qi >> 1) { if (first(fh_r)) fh_r = h; }
                    else if (first(fh_l)) fh_l = h;
                    continue;
                }
                for (int t = 0; t < 2; ++t) {
                    const uint32_t T = t == 0 ? P.t_long : P.t_short;
                    if (!T || score < T) continue;
                    AlHit& o = tab[t][qi >> 1][ct];
                    // the hit with the longest match; equal matches: the first in align_hits' order (score desc, forward, pos asc)
                    if (!o.m || h.m > o.m ||
                        (h.m == o.m && (h.score > o.score || (h.score == o.score && (h.rev < o.rev || (h.rev == o.rev && h.pos < o.pos))))))
                        o = h;
                }
            }
            if (drops) atomicAdd(P.stats, drops);
            if (EXT && (fh_l.m || fh_r.m)) {
                ExtHit eh;
                eh.pad = 0;
#pragma unroll
                for (int sd = 0; sd < 2; ++sd) {
                    const AlHit o = sd ? fh_r : fh_l;
                    eh.m[sd] = (uint16_t)o.m;
                    eh.rev[sd] = (uint8_t)o.rev;
                    eh.pos[sd] = o.pos;
                }
                ext_hit_publish(P.ext_heads, P.ext_hits, c.gap, ci, eh);
            }
            uint32_t lp = 0, rp = 0, lm = 0, rm = 0, rc = 0, T = 0;
            int span = -1;
            if (EXT) T = 0;
            else if (al_select(tab[0][0], tab[0][1], &lp, &rp, &lm, &rm, &rc, &span)) T = P.t_long;
            else if (P.t_short && al_select(tab[1][0], tab[1][1], &lp, &rp, &lm, &rm, &rc, &span)) T = P.t_short;
            if (T) {
                gf_ctg_pick* cp = P.ctg_pick + ci;
                if (T > cp->threshold) {      // calls accumulate: the highest threshold a contig selects at stays
                    gf_ctg_pick v;
                    v.lp = lp; v.rp = rp; v.lm = (uint16_t)lm; v.rm = (uint16_t)rm; v.reverse = (uint8_t)rc; v.threshold = (uint8_t)T;
                    v.reserved = 0;
                    *cp = v;
                }
                pick_word_publish(P.gap_best, P.n_closed, c.gap, pick_word_pack(T, (uint64_t)span, ci, rc));   // (pick_word.hpp; T: the word's level)
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void pick_align_kernel(AlignParams P) { pick_align_body<false, false>(P); }

__global__ __launch_bounds__(64) void pick_align_ext_kernel(AlignParams P) { pick_align_body<true, false>(P); }

__global__ __launch_bounds__(64) void pick_gapped_kernel(AlignParams P) { pick_align_body<false, true>(P); }

__global__ __launch_bounds__(64) void pick_gapped_ext_kernel(AlignParams P) { pick_align_body<true, true>(P); }

}  // namespace gf

using namespace gf;

extern "C" {

static int align_tables(gf_ctx* ctx, const AlignMeta** meta, const uint8_t** qbytes, const unsigned long long** kmers) {
    const size_t ng = ctx->gaps.size();
    DevBuf &tm = ctx->anchor_tabs[AL_TAB_META], &tk = ctx->anchor_tabs[AL_TAB_KMERS];
    if (!tm.p || !tk.p) {   // built once per gf_set_gaps, which drops them
        std::vector<AlignMeta> mt(ng);
        std::vector<uint8_t> qb;
        std::vector<unsigned long long> km;
        for (size_t g = 0; g < ng; ++g) {
            const std::string &l = ctx->flank_left[g], &r = ctx->flank_right[g];
            if ((int)l.size() > AL_FLANK_MAX || (int)r.size() > AL_FLANK_MAX) {
                ctx->last_error = "gf_pick_aligned: gap " + std::to_string(g) + " has a flank longer than 1024 bases";
                return GF_E_UNSUPPORTED;
            }
            AlignMeta& M = mt[g];
            M.qoff = (uint32_t)qb.size();
            M.nl = (uint16_t)l.size();
            M.nr = (uint16_t)r.size();
            M.kbeg = (uint32_t)km.size();
            const std::string* fl[2] = {&l, &r};
            for (int qi = 0; qi < 4; ++qi) {
                const std::string& f = *fl[qi >> 1];
                const size_t n = f.size(), q0 = qb.size();
                for (size_t i = 0; i < n; ++i) {
                    const uint8_t b = (uint8_t)base_code4((qi & 1) ? f[n - 1 - i] : f[i]);
                    qb.push_back((qi & 1) && b < 4 ? (uint8_t)(3 - b) : b);
                }
                uint64_t kmer = 0;
                int run = 0;
                for (size_t i = 0; i < n; ++i) {
                    const uint8_t b = qb[q0 + i];
                    if (b < 4) { kmer = ((kmer << 2) | b) & ((1ull << (2 * AL_SEED)) - 1); ++run; } else run = 0;
                    if (run >= AL_SEED) km.push_back(((unsigned long long)kmer << 12) | ((unsigned long long)qi << 10) | (i + 1 - AL_SEED));
                }
            }
            M.kn = (uint32_t)(km.size() - M.kbeg);
            std::sort(km.begin() + M.kbeg, km.end());
        }
        if (qb.size() > 0xFFFFFFFFull || km.size() > 0xFFFFFFFFull) return GF_E_UNSUPPORTED;
        const size_t mbytes = ng * sizeof(AlignMeta), all = mbytes + qb.size();
        int rc = ensure(ctx, tm, all + 64);
        if (!rc) rc = ensure(ctx, tk, km.size() * 8 + 64);
        if (rc) return rc;
        GF_HIP(ctx, hipMemcpy(tm.p, mt.data(), mbytes, hipMemcpyHostToDevice));
        if (!qb.empty()) GF_HIP(ctx, hipMemcpy((char*)tm.p + mbytes, qb.data(), qb.size(), hipMemcpyHostToDevice));
        if (!km.empty()) GF_HIP(ctx, hipMemcpy(tk.p, km.data(), km.size() * 8, hipMemcpyHostToDevice));
    }
    *meta = (const AlignMeta*)tm.p;
    *qbytes = (const uint8_t*)tm.p + ng * sizeof(AlignMeta);
    *kmers = (const unsigned long long*)tk.p;
    return GF_OK;
}

// what both launches of pick_align_body read the same way: the tables, the list, the gaps, the thresholds, the picks and the statistics
static int align_params(gf_ctx* ctx, const ContigList& list, int t_long, int t_short, const void* d_gap_best, void* d_stats, AlignParams* P) {
    memset(P, 0, sizeof(*P));
    const int rc = align_tables(ctx, &P->meta, &P->qbytes, &P->kmers);
    if (rc) return rc;
    P->list = list;
    P->n_gaps = (uint32_t)ctx->gaps.size();
    P->t_long = (uint32_t)t_long;
    P->t_short = (uint32_t)t_short;
    P->gap_best = (unsigned long long*)d_gap_best;
    P->stats = (uint32_t*)d_stats;
    return GF_OK;
}

static int pick_aligned(gf_ctx* ctx, bool gapped, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                        int t_short, const void* d_first, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats) {
    const bool own_ok = d_gap_best && d_n_closed && d_ctg_pick && d_stats && t_long >= 1 && t_long <= 255 && t_short >= 0 && (!t_short || t_short < t_long);
    ContigList list;
    int rc = contig_list_view(ctx, d_contigs, d_n_contigs, contig_cap, CONTIG_CAP_WORD, d_seq, d_first, own_ok ? GF_OK : GF_E_INVAL, &list);
    if (rc) return rc;
    if (!ctx->gaps.size()) return GF_OK;
    GF_HIP(ctx, hipSetDevice(ctx->device));
    AlignParams P;
    if ((rc = align_params(ctx, list, t_long, t_short, d_gap_best, d_stats, &P))) return rc;
    P.n_closed = (uint32_t*)d_n_closed;
    P.ctg_pick = (gf_ctg_pick*)d_ctg_pick;
    LaunchTimer tm(ctx, GF_KERNEL_PICK);
    hipLaunchKernelGGL(gapped ? pick_gapped_kernel : pick_align_kernel, dim3(ctx->n_cu * 16), dim3(64), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

int gf_pick_aligned_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                        int t_short, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats) {
    return pick_aligned(ctx, false, d_contigs, d_n_contigs, contig_cap, d_seq, t_long, t_short, nullptr, d_gap_best, d_n_closed, d_ctg_pick, d_stats);
}

int gf_pick_aligned_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                             int t_short, const void* d_first, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats) {
    if (!d_first) return GF_E_INVAL;
    return pick_aligned(ctx, false, d_contigs, d_n_contigs, contig_cap, d_seq, t_long, t_short, d_first, d_gap_best, d_n_closed, d_ctg_pick, d_stats);
}

int gf_pick_gapped_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                       int t_short, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats) {
    return pick_aligned(ctx, true, d_contigs, d_n_contigs, contig_cap, d_seq, t_long, t_short, nullptr, d_gap_best, d_n_closed, d_ctg_pick, d_stats);
}

int gf_pick_gapped_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                            int t_short, const void* d_first, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats) {
    if (!d_first) return GF_E_INVAL;
    return pick_aligned(ctx, true, d_contigs, d_n_contigs, contig_cap, d_seq, t_long, t_short, d_first, d_gap_best, d_n_closed, d_ctg_pick, d_stats);
}

}  // extern "C"

namespace gf {

int launch_align_ext(gf_ctx* ctx, bool gapped, const ContigList& list, int t, const void* d_gap_best, ExtHit* hits, uint32_t* heads,
                     uint32_t* stats) {   // (pick_ext.hip, which checked the arguments; gap_best is read, not written)
    AlignParams P;
    const int rc = align_params(ctx, list, t, 0, d_gap_best, stats, &P);
    if (rc) return rc;
    P.ext_hits = hits;
    P.ext_heads = heads;
    hipLaunchKernelGGL(gapped ? pick_gapped_ext_kernel : pick_align_ext_kernel, dim3(ctx->n_cu * 16), dim3(64), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}

}  // namespace gf
