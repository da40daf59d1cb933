"""The small synthetic step the GPU tests of the optional rounds share: four scaffolds of 200 kb with six gaps each, one short-insert
library of 80 000 pairs synthesised on the device, run through a Pipeline."""
SEED, SLEN, NSCF, GPS, L, N_PAIRS = 20260021, 200_000, 4, 6, 150, 80_000


def setup(gap_len, kk):
    """(gf, cfg, gaps, flanks, d_reads, d_recs, kk) of the layout with gaps of gap_len bases."""
    import torch
    from gappadder_amd.hip_api import GapFill
    gf = GapFill(0)
    cfg = GapFill.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=gap_len, read_len=L)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf.set_gaps(gaps, NSCF, flanks)
    rb = (L + 3) // 4
    d_reads = torch.empty(2 * N_PAIRS * rb + 64, dtype=torch.uint8, device="cuda")
    d_recs = torch.empty(2 * N_PAIRS * 32, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg, 0, N_PAIRS, d_reads.data_ptr(), d_recs.data_ptr())
    gf.sync()
    return gf, cfg, gaps, flanks, d_reads, d_recs, kk


def run(env, steps=1, pools=False, **kw):
    """A prepared Pipeline(**kw) over setup()'s environment and the Results of `steps` steps."""
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    pipe = Pipeline(gf, len(gaps), L, kk, **kw)
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * N_PAIRS, d_reads, d_recs))
    pipe.prepare()
    out = []
    for _ in range(steps):
        pipe.step()
        out.append(pipe.fetch(pools=pools))
    return pipe, out


def text(res, i):
    c = res.contigs[i]
    return res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])].decode()


def contigs(res):
    """[(gap, k, kv, bases)] of a Results, in the device's order."""
    return [(int(c["gap"]), int(c["k"]), int(c["kv"]), text(res, i)) for i, c in enumerate(res.contigs)]


def picks(res):
    """Pick words with the contig named by its bases (the device's contig order is unspecified)."""
    from gappadder_amd.pipeline import decode_best
    return {g: decode_best(w)[:2] + (decode_best(w)[3], text(res, decode_best(w)[2])) for g, w in enumerate(res.best.tolist()) if w}
