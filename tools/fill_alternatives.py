"""The fill alternatives (Pipeline(alternatives=True), gappadder_amd/fill_alternatives.py) on one bench preset.  Runs the preset's step with
the round off and on (two prepared pipelines stepped in turn) and prints one JSON object: the step's time off and on, the round's own
time (its launch repeated on the step's results, and the library's kernel timer), the statistics, and — the presets know the truth
(gf_synth_truth) — the closed gaps split into correct and wrong fills, per class: how many are contested, how many have candidates of
more than one length, how many have a rival at all levels of closeness, and how often the RIVAL's sequence is the true one.

    python tools/fill_alternatives.py C2RM [--max-dist 16] [--steps 3] [--reps 3] [--out profiles/fill_alternatives_c2rm.json]
"""
import argparse

import numpy as np

from preset_setup import emit, in_turn, preset_setup, round_ms


def main():
    import bench
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_alternatives as FA
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(bench.PRESETS))
    ap.add_argument("--max-dist", type=int, default=FA.MAX_DIST)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mp = bench.MATE_PAIRS.get(args.config, 0) // 2 * 2
    s = preset_setup(args.config, reads=args.reads, mp_reads=mp)
    flags = dict(merge_in_step=bool(mp))
    out = {"config": args.config, "gaps": len(s.gaps), "gap_len": s.gap_len, "reads": s.reads, "mp_reads": mp, "k_pairs": [list(p) for p in s.kk],
           "steps": args.steps, "alt_max_dist": args.max_dist}
    pipes, ms = in_turn(s, flags, {"off": {}, "on": dict(alternatives=True, alt_max_dist=args.max_dist)}, args.steps, args.reps)
    out.update(ms)
    pipe = pipes["on"]
    off, res = pipes["off"].fetch(), pipe.fetch()
    picked, rivals = pipe.picked_sequences(res), pipe.alternative_sequences(res)
    groups = {"correct": [], "wrong": []}
    for g in sorted(picked):
        groups["correct" if picked[g][1] in s.truth(g) else "wrong"].append(g)
    flag = lambda g, f: bool(int(res.alts[g]["flags"]) & f)
    out.update(closed=len(picked), closed_off=int((off.best != 0).sum()), alt_stats=res.alt_stats)
    for name, gs in groups.items():
        dist = [int(res.alts[g]["dist"]) for g in gs if g in rivals]
        out[name] = {"gaps": len(gs), "several_candidates": sum(1 for g in gs if int(res.alts[g]["n_candidates"]) > 1),
                     "contested": sum(1 for g in gs if g in rivals), "length_varies": sum(1 for g in gs if flag(g, B.FA_F_LENGTH_VARIES)),
                     "rival_near": sum(1 for d in dist if d != B.FA_DIST_FAR), "rival_far": sum(1 for d in dist if d == B.FA_DIST_FAR),
                     "rival_is_true": sum(1 for g in gs if g in rivals and rivals[g][1] in s.truth(g)),
                     "rival_dist": sorted(d for d in dist if d != B.FA_DIST_FAR)[:64]}
    t, k = round_ms(pipe, s.gf, pipe.alts.enqueue, B.KERNEL_ALT, args.steps, args.reps)
    out["round_ms"], out["round_kernel_ms"] = [round(x, 4) for x in t], k
    emit(out, args.out)


if __name__ == "__main__":
    main()
