"""The flank-overlap joins (Pipeline(flank_joins=True), gappadder_amd/flank_joins.py) on one bench preset.  --plant-overlap N doctors the
left flank of --sample K gaps (evenly spread) so that it ends N bases INSIDE the right flank: truth text of the same length that ends N
bases past the right flank's first base — the reads stay true, so the contigs run through the junction with the anchors out of order.
Runs the preset's step with the round off and on (two prepared pipelines stepped in turn, extended_fill on in both so that what a joined
gap was before is known) and prints one JSON object: the planted gaps joined with exactly N (and usable), the joins on gaps that were
not planted (a finding on repeat presets, not an error), what every joined gap was without the round (open / extended), the statistics,
the step's time off and on and the round's own time (its launch repeated on the step's results, and the library's kernel timer).

    python tools/flank_joins.py C2 --plant-overlap 40 [--sample 64] [--steps 3] [--reps 3] [--out profiles/flank_joins_c2.json]
"""
import argparse

import numpy as np

from preset_setup import L, emit, in_turn, preset_setup, round_ms


def main():
    import bench
    from gappadder_amd import _lib as B
    from gappadder_amd import flank_joins as FJ
    from gappadder_amd.hip_api import GapFill
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(bench.PRESETS))
    ap.add_argument("--plant-overlap", type=int, default=0, help="bases by which the doctored left flanks reach into the right flanks (0: none)")
    ap.add_argument("--sample", type=int, default=64, help="gaps to doctor")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--max-overlap", type=int, default=FJ.MAX_OVERLAP)
    ap.add_argument("--min-context", type=int, default=FJ.MIN_CONTEXT)
    ap.add_argument("--max-mismatch", type=int, default=FJ.MAX_MISMATCH)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    N = args.plant_overlap
    seed, slen, nscf, gps, glen, _, _ = bench.PRESETS[args.config]
    rep_p, rep_c = bench.REPEATS.get(args.config, (0, 50))
    cfg = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L, insert_mean=300,
                            insert_sd=30, library=0, repeat_period=rep_p, repeat_copies=rep_c)        # (preset_setup's short-insert library)
    gaps, _ = GapFill.synth_layout(cfg)
    planted = sorted(set(int(g) for g in np.linspace(0, len(gaps) - 1, min(args.sample, len(gaps))).astype(int))) if N > 0 else []

    def plant(flanks):
        out = list(flanks)
        for g in planted:
            lf, rf = flanks[g]
            at = int(gaps[g]["end"]) + 5                    # the right flank's first base
            new = GapFill.synth_truth(cfg, int(gaps[g]["scaffold"]), at + N - len(lf), len(lf))
            assert new[-N:] == rf[:N]
            out[g] = (new, rf)
        return out
    mp = bench.MATE_PAIRS.get(args.config, 0) // 2 * 2
    s = preset_setup(args.config, reads=args.reads, mp_reads=mp, edit_flanks=plant if planted else None)
    prm = dict(join_max_overlap=args.max_overlap, join_min_context=args.min_context, join_max_mismatch=args.max_mismatch)
    flags = dict(merge_in_step=bool(mp), extended_fill=True)
    out = {"config": args.config, "gaps": len(s.gaps), "gap_len": s.gap_len, "reads": s.reads, "mp_reads": mp, "plant_overlap": N,
           "planted": len(planted), "steps": args.steps, **prm}
    pipes, ms = in_turn(s, flags, {"off": {}, "on": dict(flank_joins=True, **prm)}, args.steps, args.reps)
    out.update(ms)
    off, res = pipes["off"].fetch(), pipes["on"].fetch()
    joined = [int(g) for g in np.nonzero(res.joins["overlap"])[0]]
    was = lambda g: "closed" if int(off.best[g]) else "extended" if int(off.ext[g]["len"]) else "open"
    out.update(closed=int((res.best != 0).sum()), closed_off=int((off.best != 0).sum()), join_stats=res.join_stats,
               planted_open=sum(1 for g in planted if not int(res.best[g])),
               planted_joined_with_n=sum(1 for g in planted if int(res.joins[g]["overlap"]) == N),
               planted_usable_with_n=sum(1 for g in planted if int(res.joins[g]["overlap"]) == N and FJ.usable(res.joins[g])),
               planted_joined_otherwise=sum(1 for g in planted if int(res.joins[g]["overlap"]) not in (0, N)),
               unplanted_joined=sum(1 for g in joined if g not in set(planted)),
               unplanted_usable=sum(1 for g in joined if g not in set(planted) and FJ.usable(res.joins[g])),
               unplanted_overlaps=sorted(int(res.joins[g]["overlap"]) for g in joined if g not in set(planted))[:64],
               joined_gaps_were={k: sum(1 for g in joined if was(g) == k) for k in ("open", "extended", "closed")})
    t, k = round_ms(pipes["on"], s.gf, pipes["on"].joins.enqueue, B.KERNEL_JOIN, args.steps, args.reps)
    out["round_ms"], out["round_kernel_ms"] = [round(x, 4) for x in t], k
    emit(out, args.out)


if __name__ == "__main__":
    main()
