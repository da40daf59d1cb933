"""The picker's two flank-anchoring modes on one bench preset: `exact` anchors (the default) and `align` (seed-and-extend of the whole
flanks, gappadder_amd/pick_contigs.py::align_hits, gf_pick_aligned_dev).  Runs the preset's step through `Pipeline` once per mode and
prints one JSON line per mode: gaps closed, closed with the true sequence, the pick kernel's time per step, the align mode's overflow
counts.  --plant FRAC plants one draft mismatch within the 10 gap-side bases of one flank of that fraction of the gaps (the reads stay
true): the case exact anchors lose and bwa-grade anchoring keeps.

    python tools/anchor_modes.py --config C2RM [--plant 0.5] [--steps 3] [--reads N]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2RM", choices=sorted(bench.PRESETS))
    ap.add_argument("--plant", type=float, default=0.0, help="fraction of the gaps whose draft flank gets one mismatch next to the gap")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--modes", default="exact,align")
    args = ap.parse_args()
    seed, slen, nscf, gps, glen, dreads, kk = bench.PRESETS[args.config]
    n_reads = (args.reads or dreads) // 2 * 2
    L = 150
    rep_p, rep_c = bench.REPEATS.get(args.config, (0, 50))
    mp = bench.MATE_PAIRS.get(args.config, 0) // 2 * 2
    cfg0 = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L,
                             insert_mean=300, insert_sd=30, repeat_period=rep_p, repeat_copies=rep_c)
    gaps, flanks = GapFill.synth_layout(cfg0)
    rng = np.random.default_rng(seed)
    planted = set()
    if args.plant > 0:
        out = []
        for g, (l, r) in enumerate(flanks):
            if rng.random() < args.plant:
                planted.add(g)
                if rng.integers(0, 2):
                    i = len(l) - 1 - int(rng.integers(0, 10))
                    l = l[:i] + rng.choice([b for b in "ACGT" if b != l[i]]) + l[i + 1:]
                else:
                    i = int(rng.integers(0, 10))
                    r = r[:i] + rng.choice([b for b in "ACGT" if b != r[i]]) + r[i + 1:]
            out.append((l, r))
        flanks = out
    gf = GapFill(0)
    gf.set_gaps(gaps, nscf, flanks)
    rb = B.lib().gf_packed_read_bytes(L)
    lib_defs = [("short-insert", 300, 30, 0, n_reads, 1)] + ([("mate-pair", 5000, 500, 1, mp, 0)] if mp else [])
    data = []
    for name, is_mean, is_sd, lib_no, n, pull in lib_defs:
        cfg = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L,
                                insert_mean=is_mean, insert_sd=is_sd, library=lib_no, repeat_period=rep_p, repeat_copies=rep_c)
        d_reads = torch.empty(n * rb + 64, dtype=torch.uint8, device="cuda")
        d_recs = torch.empty(max(1, n) * 32, dtype=torch.uint8, device="cuda")
        gf.synth_pairs_dev(cfg, 0, n // 2, d_reads.data_ptr(), d_recs.data_ptr())
        data.append((name, is_mean, is_sd, n, d_reads, d_recs, pull))
    gf.sync()
    truth = {}
    for g in range(len(gaps)):
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        truth[g] = (GapFill.synth_truth(cfg0, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg0, sc, st - 6, en - st + 11))
    for mode in args.modes.split(","):
        pipe = Pipeline(gf, len(gaps), L, kk, merge_in_step=bool(mp), anchor_mode=mode)
        for name, is_mean, is_sd, n, d_reads, d_recs, pull in data:
            pipe.add_library(DeviceLibrary(name, is_mean, is_sd, n, d_reads, d_recs, pull_mates=pull))
        pipe.prepare()
        pipe.step(1)
        pipe.barrier()
        gf.timing(True)
        pipe.step(args.steps)
        pipe.barrier()
        pick_ms, launches = gf.kernel_time(B.KERNEL_PICK)
        gf.timing(False)
        res = pipe.fetch()
        seqs = pipe.picked_sequences(res)
        true = sum(1 for g, (_, body, _) in seqs.items() if body in truth[g])
        line = {"config": args.config, "mode": mode, "gaps": len(gaps), "closed": len(seqs), "equal_to_truth": true,
                "pick_ms_per_step": round(pick_ms / args.steps, 4), "pick_launches_per_step": launches / args.steps}
        if planted:
            line.update(planted=len(planted), planted_closed=sum(1 for g in planted if g in seqs),
                        planted_equal_to_truth=sum(1 for g in planted if g in seqs and seqs[g][1] in truth[g]))
        if mode == "align":
            line.update(overflow_dropped=res.align_dropped, overflow_seed_contigs=res.align_seed_overflow)
        print(json.dumps(line), flush=True)
        del pipe, res
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
