"""The polish round (Pipeline(polish=True)) on one bench preset: the step's time with the round off and on — two prepared pipelines
stepped in turn, `--reps` timed windows each, so the spread is known before a difference is read —, the round's own time (its launch
repeated on the step's results, and the library's launch timer), and — the presets know the truth (gf_synth_truth) — the fills that equal
the truth before and after the round, the four transitions (every correct -> wrong fill with its gap, its record and its pool size), and
the distributions of `n_changed` and `reads_ambiguous` per transition group.  One JSON object on stdout, and in --out when given.

    python tools/polish_fills.py --config C5 --asm-tiebreak none [--out profiles/polish_c5_none.json]
    python tools/polish_fills.py --config C2RM --merge-in-step [--mp-reads N] [--anchor-mode exact|align|gapped]
"""
import argparse

import numpy as np

from preset_setup import emit, off_and_on, round_arguments, round_ms, round_setup


def _dist(v):
    v = np.asarray(v, dtype=np.int64)
    if not len(v):
        return {"n": 0}
    q = np.percentile(v, [50, 95])
    return {"n": int(len(v)), "zero": int((v == 0).sum()), "median": float(q[0]), "p95": float(q[1]), "max": int(v.max()), "mean": round(float(v.mean()), 3)}


def main():
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    round_arguments(ap, reps=True, placing=True)
    ap.add_argument("--min-votes", type=int, default=2)
    args = ap.parse_args()
    s, flags, out = round_setup(args)
    prm = dict(polish_seed=args.seed, polish_max_mismatch=args.max_mismatch, polish_min_overlap=args.min_overlap, polish_min_votes=args.min_votes)
    out.update(steps=args.steps, **flags, **prm)
    pipe, ms = off_and_on(s, flags, dict(polish=True, **prm), args.steps, args.reps)
    out.update(ms)
    res = pipe.fetch()
    pool_off = res.asm_off_t.cpu().numpy().astype(np.int64)
    out["closed"], out["polish_stats"] = int((res.best != 0).sum()), res.polish_stats
    ms, out["round_kernel_ms"] = round_ms(pipe, s.gf, pipe.polish.enqueue, B.KERNEL_POLISH, args.steps)
    out["round_ms"] = round(ms[0], 4)
    before, after = pipe.picked_sequences(res), pipe.polished_sequences(res)
    groups = {"wrong_to_correct": [], "wrong_to_wrong": [], "correct_to_correct": [], "correct_to_wrong": []}
    for g in before:
        t = s.truth(g)
        groups[("correct" if before[g][1] in t else "wrong") + "_to_" + ("correct" if after[g][1] in t else "wrong")].append(g)
    out["correct_before"] = len(groups["correct_to_correct"]) + len(groups["correct_to_wrong"])
    out["correct_after"] = len(groups["correct_to_correct"]) + len(groups["wrong_to_correct"])
    pol = res.polish
    for name, gs in groups.items():
        gs = np.array(gs, dtype=np.int64)
        out[name] = {"gaps": int(len(gs)), "n_changed": _dist(pol["n_changed"][gs]), "reads_ambiguous": _dist(pol["reads_ambiguous"][gs]),
                     "reads_placed": _dist(pol["reads_placed"][gs]), "n_uncovered": _dist(pol["n_uncovered"][gs])}
    out["wrong_to_wrong"]["unchanged"] = int(sum(int(pol["n_changed"][g]) == 0 for g in groups["wrong_to_wrong"]))
    out["correct_to_wrong_gaps"] = [{"gap": int(g), "pool_rows": int(pool_off[g + 1] - pool_off[g]),
                                     **{f: int(pol[g][f]) for f in ("n_cols", "n_changed", "n_uncovered", "reads_placed", "reads_ambiguous")}}
                                    for g in groups["correct_to_wrong"]]
    emit(out, args.out)


if __name__ == "__main__":
    main()
