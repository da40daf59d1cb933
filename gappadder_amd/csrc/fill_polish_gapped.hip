// fill_polish_gapped.hip — the indel-aware consensus polish of the closed gaps: fill_polish.hip's round with rows that may be placed with
// one indel (fill_place_split.hpp), votes on indel events as well as on columns, and a polished contig that may change length
// (gf_fill_polish_gapped_dev, include/gapfill_hip.h; definition and host twin: gappadder_amd/polish_gapped.py).
//
// One workgroup of 256 threads per closed gap, grid-stride over the gaps, one row per thread; gap prologue, staging and index as in
// fill_polish.hip.  Per gap:
//   vote     passes of PLG_VCHUNK body columns over the pool, as there.  In the first pass a row placed split also enters its event —
//            when it lies in the body — into an LDS table of GF_PLG_MAX_EVENTS 64-bit keys (plg_event), claimed by a 64-bit CAS, with a
//            counter per entry; a key that finds the table full sets the EVENTS flag, which depends on the number of distinct keys only
//   decide   the columns as in fill_polish.hip, but into LDS (2 bits a column): where they go in the output is not known yet
//   against  only with events: one more walk over the pool.  The placement is COMPUTED AGAIN, as the vote passes do it, not kept per row:
//            the entry takes no buffer of pool_rows words, gaps without any split row (most) never get here, and a row's placement
//            is cheap next to what staging it costs.  A placed row counts against every entry it does not vote whose site one of its
//            parts covers
//   events   one thread: the passing entries by (votes descending, key ascending), accepted unless they touch an accepted one or break
//            the insertion cap.  The output length is then known and the offset is taken from the u64 counter in d_stats
//   write    all threads: every column finds its output index from the accepted events (at most 64, mostly none or one); the
//            inserted bases come from the keys
// LDS: 63.0 KB static (the vote chunk is 768 columns, not fill_polish.hip's 1 024, to make room for the decided columns and the table): two
// workgroups per CU.  Resources: DESIGN.md §22; no scratch.
#include <cstring>

#include "fill_body.hpp"
#include "fill_place.hpp"
#include "fill_place_split.hpp"
#include "fill_round.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t PLG_VCHUNK = 768, PLG_EV = GF_PLG_MAX_EVENTS;
static_assert((PLG_EV & (PLG_EV - 1)) == 0 && PL_MAX < (1u << 14) && GF_PLG_MAX_INDEL <= 16, "event key geometry");

struct PlgParams {
    PlPlaceArgs place;
    FillRoundArgs round;
    uint32_t min_votes, max_indel;
    gf_fill_polish_gapped* out;
    uint8_t* bases;
    uint64_t base_cap;
};

__device__ __forceinline__ uint32_t plg_key_p(unsigned long long k) { return (uint32_t)(k >> 38); }
__device__ __forceinline__ uint32_t plg_key_ins(unsigned long long k) { return (uint32_t)(k >> 37) & 1u; }
__device__ __forceinline__ uint32_t plg_key_len(unsigned long long k) { return (uint32_t)(k >> 32) & 31u; }

// one aligned part of a placed row — read positions [a, b) on diagonal D of its strand's array — as columns of the stored contig
__device__ __forceinline__ void plg_part_cols(uint32_t strand, int32_t D, uint32_t a, uint32_t b, uint32_t n, int32_t* lo, int32_t* hi) {
    *lo = strand ? (int32_t)n - (D + (int32_t)b) : D + (int32_t)a;
    *hi = strand ? (int32_t)n - (D + (int32_t)a) : D + (int32_t)b;
}

__global__ __launch_bounds__(PL_THREADS) void fill_polish_gapped_kernel(PlgParams P) {
    __shared__ uint32_t s_idx[PL_SLOTS / 2];
    __shared__ uint32_t s_votes[PLG_VCHUNK * 4];
    __shared__ uint32_t s_fwd[PL_CTG_WORDS];
    __shared__ uint32_t s_rc[PL_CTG_WORDS];
    __shared__ uint32_t s_rows[PL_ROW_WORDS];
    __shared__ uint32_t s_dec[PL_MAX / 16];     // the decided body columns, 2 bits each
    __shared__ unsigned long long s_ekey[PLG_EV];
    __shared__ uint32_t s_evotes[PLG_EV], s_eagainst[PLG_EV];
    __shared__ uint32_t s_eacc[PLG_EV];         // the accepted entries
    __shared__ uint32_t s_loc[2];
    __shared__ uint32_t s_acc[12];              // 0 a byte that is no base, 1 changed, 2 uncovered, 3 placed, 4 ambiguous, 5 split, 6 events outside,
                                                // 7 entries claimed, 8 table full, 9 accepted, 10 inserted, 11 deleted
    __shared__ uint32_t s_flags;
    __shared__ unsigned long long s_off;
    const uint32_t t = threadIdx.x, L = P.place.L;
    const uint32_t n_list = contig_list_end(P.round.body.list);
    for (uint32_t g = blockIdx.x; g < P.round.n_gaps; g += gridDim.x) {
        gf_fill_polish_gapped rec;
        memset(&rec, 0, sizeof(rec));
        const FillGap fg = fill_gap_open<PL_THREADS>(P.round, n_list, g, s_loc);        // (fill_round.hpp; the same in all threads)
        if (fg.state == FILL_GAP_OPEN) {
            if (t == 0) P.out[g] = rec;
            continue;
        }
        if (fg.state == FILL_GAP_MISMATCH) {
            if (t == 0) {
                P.out[g] = rec;
                atomicAdd(P.round.stats + GF_PL_MISMATCH, 1u);
            }
            continue;
        }
        const uint32_t n = fg.fb.c.length;
        const char* ctg = P.round.body.list.seq + fg.fb.c.seq_off;
        const uint32_t b0 = (uint32_t)fg.fb.b0, b1 = (uint32_t)fg.fb.b1, n_cols = b1 - b0;
        if (t < 12) s_acc[t] = 0;
        for (uint32_t i = t; i < PLG_EV; i += PL_THREADS) {
            s_ekey[i] = 0;
            s_evotes[i] = s_eagainst[i] = 0;
        }
        for (uint32_t i = t; i < PL_MAX / 16; i += PL_THREADS) s_dec[i] = 0;
        __syncthreads();
        // ---- stage, or skip (fill_place.hpp)
        const uint32_t skip = pl_stage_or_skip(ctg, n, s_fwd, s_rc, s_idx, &s_acc[0], GF_PL_F_LONG, GF_PL_F_NON_ACGT);
        if (skip) {                              // copied out unpolished
            if (t == 0) s_off = atomicAdd((unsigned long long*)(P.round.stats + GF_PL_BASES), (unsigned long long)n);
            __syncthreads();
            const uint64_t off = s_off;
            const bool fits = off + n <= P.base_cap;
            if (fits)
                for (uint32_t i = t; i < n; i += PL_THREADS) P.bases[off + i] = (uint8_t)ctg[i];
            if (t == 0) {
                rec.off = fits ? off : 0;
                rec.len = fits ? n : 0;
                rec.flags = skip | (fits ? 0u : (uint32_t)GF_PL_F_OVERFLOW);
                rec.n_cols = n_cols;
                P.out[g] = rec;
                atomicAdd(P.round.stats + (skip == GF_PL_F_LONG ? GF_PL_SKIPPED_LONG : GF_PL_SKIPPED_NON_ACGT), 1u);
                if (!fits) atomicAdd(P.round.stats + GF_PL_OVERFLOW, 1u);
            }
            continue;
        }
        // ---- index
        pl_build_index(s_fwd, s_idx, n, P.place.s);
        const FillRows rows = fill_gap_rows(P.round, g);
        const uint64_t r0 = rows.r0, r1 = rows.r1;
        // ---- place, vote and decide: PLG_VCHUNK body columns per pass (one pass for an empty body: the rows are still counted)
        for (uint32_t c_lo = b0, pass = 0; pass == 0 || c_lo < b1; c_lo += PLG_VCHUNK, ++pass) {
            const uint32_t c_hi = b1 - c_lo < PLG_VCHUNK ? b1 : c_lo + PLG_VCHUNK;
            for (uint32_t i = t; i < PLG_VCHUNK * 4; i += PL_THREADS) s_votes[i] = 0;
            __syncthreads();                     // (also: the index is built)
            for (uint64_t row0 = r0; row0 < r1; row0 += P.place.batch_rows) {
                const uint32_t nb = r1 - row0 < P.place.batch_rows ? (uint32_t)(r1 - row0) : P.place.batch_rows;
                const uint32_t mis = pl_stage_rows(P.place, row0, nb, s_rows);
                if (t < nb) {
                    const uint32_t* nm = P.place.nmask ? P.place.nmask + (row0 + t) * P.place.nmw : nullptr;
                    const uint32_t rbit = (mis + t * P.place.rb) * 8;
                    const PlgPlacement pm = plg_place_row(P.place, P.max_indel, s_rows, rbit, nm, s_fwd, s_rc, s_idx, n);
                    const bool split = pm.D2 != pm.D;
                    if (pass == 0 && pm.cnt) atomicAdd(&s_acc[pm.cnt == 1 ? 3 : 4], 1u);
                    if (pass == 0 && pm.cnt == 1 && split) {
                        atomicAdd(&s_acc[5], 1u);
                        uint32_t p, gd;
                        const unsigned long long key = plg_event(pm, s_rows, rbit, n, &p, &gd);
                        if (gd ? (b0 <= p && p + gd <= b1) : (b0 <= p && p <= b1)) {
                            uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 58), tries = 0;
                            for (; tries < PLG_EV; ++tries, h = (h + 1) & (PLG_EV - 1)) {
                                unsigned long long cur = s_ekey[h];
                                if (cur == 0) {
                                    cur = atomicCAS(&s_ekey[h], 0ull, key);
                                    if (cur == 0) {
                                        atomicAdd(&s_acc[7], 1u);
                                        cur = key;
                                    }
                                }
                                if (cur == key) {
                                    atomicAdd(&s_evotes[h], 1u);
                                    break;
                                }
                            }
                            if (tries == PLG_EV) s_acc[8] = 1u;
                        } else {
                            atomicAdd(&s_acc[6], 1u);
                        }
                    }
                    if (pm.cnt == 1 && c_hi > c_lo) {
                        // strand 0: read base i on column D + i; strand 1: its complement on column n - 1 - D - i; a split row: two parts
                        const uint32_t gi = pm.D2 < pm.D ? (uint32_t)(pm.D - pm.D2) : 0u;
                        const uint8_t* rowb = (const uint8_t*)s_rows + mis + t * P.place.rb;
                        for (uint32_t part = 0; part < (split ? 2u : 1u); ++part) {
                            const int32_t D = part ? pm.D2 : pm.D;
                            int32_t i0 = D < 0 ? -D : 0, i1 = (int32_t)L < (int32_t)n - D ? (int32_t)L : (int32_t)n - D;
                            if (split && part == 0) i1 = (int32_t)pm.x;
                            if (split && part == 1) i0 = (int32_t)(pm.x + gi);
                            int32_t lo = pm.strand ? (int32_t)n - D - (int32_t)c_hi : (int32_t)c_lo - D;
                            int32_t hi = pm.strand ? (int32_t)n - D - (int32_t)c_lo : (int32_t)c_hi - D;
                            lo = lo > i0 ? lo : i0;
                            hi = hi < i1 ? hi : i1;
                            for (int32_t i = lo; i < hi; ++i) {
                                if (nm && ((nm[i >> 5] >> (i & 31)) & 1u)) continue;
                                const uint32_t code = (rowb[i >> 2] >> (6 - 2 * (i & 3))) & 3u;
                                const uint32_t col = pm.strand ? n - 1 - (uint32_t)(D + i) : (uint32_t)(D + i);
                                atomicAdd(&s_votes[(col - c_lo) * 4 + (pm.strand ? 3u - code : code)], 1u);
                            }
                        }
                    }
                }
                __syncthreads();
            }
            uint32_t changed = 0, uncovered = 0;
            for (uint32_t j = c_lo + t; j < c_hi; j += PL_THREADS) {
                const uint32_t* v = s_votes + (j - c_lo) * 4;
                const uint32_t v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
                const uint32_t cur = stream32(s_fwd, 2 * (PL_LEAD + j)) >> 30;
                uint32_t bb = 0, bv = v0;
                if (v1 > bv) { bb = 1; bv = v1; }
                if (v2 > bv) { bb = 2; bv = v2; }
                if (v3 > bv) { bb = 3; bv = v3; }
                const uint32_t vc = cur == 0 ? v0 : cur == 1 ? v1 : cur == 2 ? v2 : v3;
                const bool change = bv >= P.min_votes && bv > vc;
                changed += change;
                uncovered += (v0 | v1 | v2 | v3) == 0;
                atomicOr(&s_dec[j >> 4], (change ? bb : cur) << (2 * (j & 15)));
            }
            if (changed) atomicAdd(&s_acc[1], changed);
            if (uncovered) atomicAdd(&s_acc[2], uncovered);
            __syncthreads();                     // (the votes are read: the next pass clears them; the table is complete)
        }
        // ---- against: the placed rows that cross an entry's site in one piece without voting it
        const bool table_full = s_acc[8] != 0;
        if (s_acc[7] && !table_full) {
            for (uint64_t row0 = r0; row0 < r1; row0 += P.place.batch_rows) {
                const uint32_t nb = r1 - row0 < P.place.batch_rows ? (uint32_t)(r1 - row0) : P.place.batch_rows;
                const uint32_t mis = pl_stage_rows(P.place, row0, nb, s_rows);
                if (t < nb) {
                    const uint32_t* nm = P.place.nmask ? P.place.nmask + (row0 + t) * P.place.nmw : nullptr;
                    const uint32_t rbit = (mis + t * P.place.rb) * 8;
                    const PlgPlacement pm = plg_place_row(P.place, P.max_indel, s_rows, rbit, nm, s_fwd, s_rc, s_idx, n);
                    if (pm.cnt == 1) {
                        const bool split = pm.D2 != pm.D;
                        const uint32_t gi = pm.D2 < pm.D ? (uint32_t)(pm.D - pm.D2) : 0u;
                        unsigned long long own = 0;
                        uint32_t p, gd;
                        if (split) own = plg_event(pm, s_rows, rbit, n, &p, &gd);
                        const uint32_t a0 = pm.D < 0 ? (uint32_t)(-pm.D) : 0u;
                        const uint32_t e1 = (int32_t)L < (int32_t)n - pm.D2 ? L : (uint32_t)((int32_t)n - pm.D2);
                        int32_t lo0, hi0, lo1 = 0, hi1 = 0;
                        plg_part_cols(pm.strand, pm.D, a0, split ? pm.x : e1, n, &lo0, &hi0);
                        if (split) plg_part_cols(pm.strand, pm.D2, pm.x + gi, e1, n, &lo1, &hi1);
                        for (uint32_t e = 0; e < PLG_EV; ++e) {
                            const unsigned long long key = s_ekey[e];
                            if (key == 0 || key == own) continue;
                            const int32_t ep = (int32_t)plg_key_p(key), egd = plg_key_ins(key) ? 0 : (int32_t)plg_key_len(key);
                            const int32_t slo = ep - (int32_t)P.place.s > 0 ? ep - (int32_t)P.place.s : 0;
                            const int32_t shi = ep + egd + (int32_t)P.place.s < (int32_t)n ? ep + egd + (int32_t)P.place.s : (int32_t)n;
                            if ((lo0 <= slo && shi <= hi0) || (split && lo1 <= slo && shi <= hi1)) atomicAdd(&s_eagainst[e], 1u);
                        }
                    }
                }
                __syncthreads();
            }
        }
        // ---- events: one thread sorts and accepts
        if (t == 0) {
            uint32_t n_acc = 0, inserted = 0, deleted = 0, flags = table_full ? (uint32_t)GF_PL_F_EVENTS : 0u;
            if (s_acc[7] && !table_full) {
                for (uint32_t e = 0; e < PLG_EV; ++e)        // s_evotes becomes 0 for an entry that does not pass or is dealt with
                    if (s_ekey[e] == 0 || s_evotes[e] < P.min_votes || s_evotes[e] <= s_eagainst[e]) s_evotes[e] = 0;
                for (;;) {
                    uint32_t be = PLG_EV, bv = 0;
                    unsigned long long bk = 0;
                    for (uint32_t e = 0; e < PLG_EV; ++e) {
                        const uint32_t v = s_evotes[e];
                        if (v && (v > bv || (v == bv && s_ekey[e] < bk))) {
                            be = e;
                            bv = v;
                            bk = s_ekey[e];
                        }
                    }
                    if (be == PLG_EV) break;
                    s_evotes[be] = 0;
                    const uint32_t lo = plg_key_p(bk), len = plg_key_len(bk), ins = plg_key_ins(bk), hi = lo + (ins ? 0u : len);
                    bool meets = false;
                    for (uint32_t a = 0; a < n_acc && !meets; ++a) {
                        const unsigned long long ak = s_ekey[s_eacc[a]];
                        const uint32_t alo = plg_key_p(ak), ahi = alo + (plg_key_ins(ak) ? 0u : plg_key_len(ak));
                        meets = !(hi < alo || ahi < lo);
                    }
                    if (meets) continue;
                    if (ins && inserted + len > GF_PLG_MAX_INSERTED) {
                        flags |= GF_PL_F_INS_CAP;
                        continue;
                    }
                    inserted += ins ? len : 0u;
                    deleted += ins ? 0u : len;
                    s_eacc[n_acc++] = be;
                }
            }
            s_acc[9] = n_acc;
            s_acc[10] = inserted;
            s_acc[11] = deleted;
            s_flags = flags;
            s_off = atomicAdd((unsigned long long*)(P.round.stats + GF_PL_BASES), (unsigned long long)(n + inserted - deleted));
        }
        __syncthreads();
        // ---- write
        const uint32_t n_acc = s_acc[9], n_out = n + s_acc[10] - s_acc[11];
        const uint64_t off = s_off;
        const bool fits = off + n_out <= P.base_cap;
        uint8_t* outp = P.bases + off;
        if (fits) {
            for (uint32_t j = t; j < n; j += PL_THREADS) {
                int32_t shift = 0;
                bool gone = false;
                for (uint32_t a = 0; a < n_acc; ++a) {
                    const unsigned long long ak = s_ekey[s_eacc[a]];
                    const uint32_t ap = plg_key_p(ak), al = plg_key_len(ak);
                    if (plg_key_ins(ak)) {
                        if (ap <= j) shift += (int32_t)al;
                    } else if (ap <= j) {
                        gone = gone || j < ap + al;
                        shift -= (int32_t)(j - ap < al ? j - ap : al);
                    }
                }
                if (gone) continue;
                const uint32_t code = (s_dec[j >> 4] >> (2 * (j & 15))) & 3u;
                const uint8_t base = (j >= b0 && j < b1) ? (uint8_t)(code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T') : (uint8_t)ctg[j];
                outp[(uint32_t)((int32_t)j + shift)] = base;
            }
            if (t < n_acc) {                     // the inserted bases of accepted entry t: before the output index of its column
                const unsigned long long ek = s_ekey[s_eacc[t]];
                if (plg_key_ins(ek)) {
                    const uint32_t ep = plg_key_p(ek), el = plg_key_len(ek);
                    int32_t shift = 0;
                    for (uint32_t a = 0; a < n_acc; ++a) {
                        const unsigned long long ak = s_ekey[s_eacc[a]];
                        const uint32_t ap = plg_key_p(ak), al = plg_key_len(ak);
                        if (plg_key_ins(ak)) {
                            if (ap < ep) shift += (int32_t)al;
                        } else if (ap <= ep) {
                            shift -= (int32_t)al;        // (accepted events do not touch: a deletion left of ep ends before it)
                        }
                    }
                    for (uint32_t k = 0; k < el; ++k) {
                        const uint32_t code = (uint32_t)(ek >> (2 * (el - 1 - k))) & 3u;
                        outp[(uint32_t)((int32_t)ep + shift) + k] = (uint8_t)(code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T');
                    }
                }
            }
        }
        if (t == 0) {
            const uint32_t flags = s_flags;
            rec.off = fits ? off : 0;
            rec.len = fits ? n_out : 0;
            rec.flags = flags | (fits ? 0u : (uint32_t)GF_PL_F_OVERFLOW);
            rec.n_cols = n_cols;
            rec.n_changed = s_acc[1];
            rec.n_uncovered = s_acc[2];
            rec.reads_placed = s_acc[3];
            rec.reads_ambiguous = s_acc[4];
            rec.n_events = n_acc;
            rec.n_inserted = s_acc[10];
            rec.n_deleted = s_acc[11];
            rec.reads_split = s_acc[5];
            rec.events_seen = table_full ? PLG_EV + 1 : s_acc[7];
            rec.events_outside = s_acc[6];
            P.out[g] = rec;
            atomicAdd(P.round.stats + GF_PL_GAPS, 1u);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PL_CHANGED), (unsigned long long)s_acc[1]);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PL_PLACED), (unsigned long long)s_acc[3]);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PL_AMBIGUOUS), (unsigned long long)s_acc[4]);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PLG_EVENTS), (unsigned long long)n_acc);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PLG_INSERTED), (unsigned long long)s_acc[10]);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PLG_DELETED), (unsigned long long)s_acc[11]);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PLG_SPLIT), (unsigned long long)s_acc[5]);
            if (flags & GF_PL_F_EVENTS) atomicAdd(P.round.stats + GF_PLG_F_EVENTS, 1u);
            if (flags & GF_PL_F_INS_CAP) atomicAdd(P.round.stats + GF_PLG_F_INS_CAP, 1u);
            if (!fits) atomicAdd(P.round.stats + GF_PL_OVERFLOW, 1u);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_polish_gapped_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off,
                                         size_t pool_rows, int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap,
                                         const void* d_seq, const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short,
                                         int seed, int max_mismatch, int min_overlap, int min_votes, int max_indel, void* d_polish, void* d_bases,
                                         size_t base_cap, void* d_stats) {
    if (base_cap && !d_bases) return GF_E_INVAL;
    PlgParams P;
    memset(&P, 0, sizeof(P));
    int own = pl_place_setup(d_pool_packed, d_nmask_or_null, read_len, seed, max_mismatch, min_overlap, &P.place);
    if (min_votes < 1 || max_indel < 1 || max_indel > GF_PLG_MAX_INDEL) own = GF_E_UNSUPPORTED;
    const FillRoundIn in = {d_pool_packed, d_pool_off, pool_rows, read_len, d_contigs, d_n_contigs, contig_cap, d_seq, d_gap_best, d_ctg_pick_or_null,
                            anchor_long, anchor_short, d_polish, d_stats};
    size_t blocks;
    const int rc = fill_round_setup(ctx, in, own, GF_PLG_WORDS, 2, &P.round, &blocks);  // 2: workgroups the static LDS lets a CU hold
    if (rc || !blocks) return rc;
    P.min_votes = (uint32_t)min_votes;
    P.max_indel = (uint32_t)max_indel;
    P.out = (gf_fill_polish_gapped*)d_polish;
    P.bases = (uint8_t*)d_bases;
    P.base_cap = base_cap;
    LaunchTimer tm(ctx, GF_KERNEL_POLISH_GAPPED);
    hipLaunchKernelGGL(fill_polish_gapped_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
