// fill_polish.hip — consensus polish of the closed gaps: the reads of a gap's own pool are placed without gaps on the gap's winning
// contig, every column of the fill takes a vote, and the polished contig is written out with one record per gap (gf_fill_polish_dev,
// include/gapfill_hip.h; definition and host twin: gappadder_amd/polish.py).  The reference has no such stage.
//
// One workgroup of 256 threads per closed gap, grid-stride over the gaps.  A gap is opened by fill_round.hpp (open / mismatch / ok, the
// body [b0, b1) of fill_body.hpp, the gap's pool rows); the launch is set up by fill_round_setup and pl_place_setup.  Per gap:
//   stage, index, place   fill_place.hpp (pl_stage_or_skip: a long or non-ACGT contig is copied out unpolished): the contig 2-bit packed on
//            both strands and the multimap of its s-mers in LDS, the pool's packed rows staged a batch at a time, one row per thread,
//            each row's best (strand, diagonal) with its multiplicity
//   vote     a row with one best placement adds its unmasked bases to the columns' four counters (LDS atomics) — PL_VCHUNK body
//            columns per pass; a longer body costs another pass over the pool (the placement is computed again), never a result
//   decide   per column, integer comparisons of the four counters: independent of the order of the atomics.  The polished contig goes
//            to d_bases with byte stores, at an offset from the u64 counter in d_stats
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md §16; no scratch, static LDS below 64 KB.
#include <cstring>

#include "fill_body.hpp"
#include "fill_place.hpp"
#include "fill_round.hpp"
#include "gf_internal.hpp"

namespace gf {

constexpr uint32_t PL_VCHUNK = 1024;

struct PlParams {
    PlPlaceArgs place;
    FillRoundArgs round;
    uint32_t min_votes;
    gf_fill_polish* out;
    uint8_t* bases;
    uint64_t base_cap;
};

__global__ __launch_bounds__(PL_THREADS) void fill_polish_kernel(PlParams P) {
    __shared__ uint32_t s_idx[PL_SLOTS / 2];
    __shared__ uint32_t s_votes[PL_VCHUNK * 4];
    __shared__ uint32_t s_fwd[PL_CTG_WORDS];
    __shared__ uint32_t s_rc[PL_CTG_WORDS];
    __shared__ uint32_t s_rows[PL_ROW_WORDS];
    __shared__ uint32_t s_loc[2];
    __shared__ uint32_t s_acc[5];               // a byte that is no base, columns changed, columns uncovered, rows placed, rows ambiguous
    __shared__ unsigned long long s_off;
    const uint32_t t = threadIdx.x, L = P.place.L;
    const uint32_t n_list = contig_list_end(P.round.body.list);
    for (uint32_t g = blockIdx.x; g < P.round.n_gaps; g += gridDim.x) {
        gf_fill_polish rec;
        rec.off = 0;
        rec.len = rec.flags = rec.n_cols = rec.n_changed = rec.n_uncovered = rec.reads_placed = rec.reads_ambiguous = rec.reserved = 0;
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
        if (t == 0) {
            s_acc[0] = s_acc[1] = s_acc[2] = s_acc[3] = s_acc[4] = 0;
            s_off = atomicAdd((unsigned long long*)(P.round.stats + GF_PL_BASES), (unsigned long long)n);
        }
        __syncthreads();
        // ---- stage, or skip (fill_place.hpp)
        const uint32_t skip = pl_stage_or_skip(ctg, n, s_fwd, s_rc, s_idx, &s_acc[0], GF_PL_F_LONG, GF_PL_F_NON_ACGT);
        const uint64_t off = s_off;
        const bool fits = off + n <= P.base_cap;
        uint8_t* outp = P.bases + off;
        if (skip) {                              // copied out unpolished
            if (fits)
                for (uint32_t i = t; i < n; i += PL_THREADS) outp[i] = (uint8_t)ctg[i];
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
        // ---- place, vote and decide: PL_VCHUNK body columns per pass (one pass for an empty body: the rows are still counted)
        for (uint32_t c_lo = b0, pass = 0; pass == 0 || c_lo < b1; c_lo += PL_VCHUNK, ++pass) {
            const uint32_t c_hi = b1 - c_lo < PL_VCHUNK ? b1 : c_lo + PL_VCHUNK;
            for (uint32_t i = t; i < PL_VCHUNK * 4; i += PL_THREADS) s_votes[i] = 0;
            __syncthreads();                     // (also: the index is built)
            for (uint64_t row0 = r0; row0 < r1; row0 += P.place.batch_rows) {
                const uint32_t nb = r1 - row0 < P.place.batch_rows ? (uint32_t)(r1 - row0) : P.place.batch_rows;
                const uint32_t mis = pl_stage_rows(P.place, row0, nb, s_rows);
                if (t < nb) {
                    const uint32_t* nm = P.place.nmask ? P.place.nmask + (row0 + t) * P.place.nmw : nullptr;
                    const PlPlacement pm = pl_place_row(P.place, s_rows, (mis + t * P.place.rb) * 8, nm, s_fwd, s_rc, s_idx, n);
                    const uint32_t cnt = pm.cnt, bstrand = pm.strand;
                    const int32_t bD = pm.D;
                    if (pass == 0 && cnt) atomicAdd(&s_acc[cnt == 1 ? 3 : 4], 1u);
                    if (cnt == 1 && c_hi > c_lo) {
                        // strand 0: read base i on column D + i; strand 1: its complement on column n - 1 - D - i
                        const int32_t i0 = bD < 0 ? -bD : 0, i1 = (int32_t)L < (int32_t)n - bD ? (int32_t)L : (int32_t)n - bD;
                        int32_t lo = bstrand ? (int32_t)n - bD - (int32_t)c_hi : (int32_t)c_lo - bD;
                        int32_t hi = bstrand ? (int32_t)n - bD - (int32_t)c_lo : (int32_t)c_hi - bD;
                        lo = lo > i0 ? lo : i0;
                        hi = hi < i1 ? hi : i1;
                        const uint8_t* rowb = (const uint8_t*)s_rows + mis + t * P.place.rb;
                        for (int32_t i = lo; i < hi; ++i) {
                            if (nm && ((nm[i >> 5] >> (i & 31)) & 1u)) continue;
                            const uint32_t code = (rowb[i >> 2] >> (6 - 2 * (i & 3))) & 3u;
                            const uint32_t col = bstrand ? n - 1 - (uint32_t)(bD + i) : (uint32_t)(bD + i);
                            atomicAdd(&s_votes[(col - c_lo) * 4 + (bstrand ? 3u - code : code)], 1u);
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
                const uint32_t now = change ? bb : cur;
                changed += change;
                uncovered += (v0 | v1 | v2 | v3) == 0;
                if (fits) outp[j] = (uint8_t)(now == 0 ? 'A' : now == 1 ? 'C' : now == 2 ? 'G' : 'T');
            }
            if (changed) atomicAdd(&s_acc[1], changed);
            if (uncovered) atomicAdd(&s_acc[2], uncovered);
            __syncthreads();                     // (the votes are read: the next pass clears them)
        }
        if (fits)
            for (uint32_t i = t; i < n; i += PL_THREADS)
                if (i < b0 || i >= b1) outp[i] = (uint8_t)ctg[i];
        if (t == 0) {
            rec.off = fits ? off : 0;
            rec.len = fits ? n : 0;
            rec.flags = fits ? 0u : (uint32_t)GF_PL_F_OVERFLOW;
            rec.n_cols = n_cols;
            rec.n_changed = s_acc[1];
            rec.n_uncovered = s_acc[2];
            rec.reads_placed = s_acc[3];
            rec.reads_ambiguous = s_acc[4];
            P.out[g] = rec;
            atomicAdd(P.round.stats + GF_PL_GAPS, 1u);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PL_CHANGED), (unsigned long long)s_acc[1]);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PL_PLACED), (unsigned long long)s_acc[3]);
            atomicAdd((unsigned long long*)(P.round.stats + GF_PL_AMBIGUOUS), (unsigned long long)s_acc[4]);
            if (!fits) atomicAdd(P.round.stats + GF_PL_OVERFLOW, 1u);
        }
    }
}

}  // namespace gf

using namespace gf;

extern "C" int gf_fill_polish_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                                  int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                  const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                                  int min_overlap, int min_votes, void* d_polish, void* d_bases, size_t base_cap, void* d_stats) {
    if (base_cap && !d_bases) return GF_E_INVAL;
    PlParams P;
    memset(&P, 0, sizeof(P));
    int own = pl_place_setup(d_pool_packed, d_nmask_or_null, read_len, seed, max_mismatch, min_overlap, &P.place);
    if (min_votes < 1) own = GF_E_UNSUPPORTED;
    const FillRoundIn in = {d_pool_packed, d_pool_off, pool_rows, read_len, d_contigs, d_n_contigs, contig_cap, d_seq, d_gap_best, d_ctg_pick_or_null,
                            anchor_long, anchor_short, d_polish, d_stats};
    size_t blocks;
    const int rc = fill_round_setup(ctx, in, own, GF_PL_WORDS, 2, &P.round, &blocks);   // 2: workgroups the static LDS lets a CU hold
    if (rc || !blocks) return rc;
    P.min_votes = (uint32_t)min_votes;
    P.out = (gf_fill_polish*)d_polish;
    P.bases = (uint8_t*)d_bases;
    P.base_cap = base_cap;
    LaunchTimer tm(ctx, GF_KERNEL_POLISH);
    hipLaunchKernelGGL(fill_polish_kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, ctx->stream, P);
    GF_HIP(ctx, hipGetLastError());
    return GF_OK;
}
