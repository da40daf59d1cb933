"""The read-support round (Pipeline(read_support=True)) on one bench preset: the step's time with the round off and on, the round's own
time (its launch repeated on the step's results, and the library's launch timer), and — the presets know the truth (gf_synth_truth) —
the distributions of the record's `min`, `n_below` and `zero_run` over the fills that equal the truth and over those that do not.
One JSON object on stdout, and in --out when given.

    python tools/read_support.py --config C5 --asm-tiebreak none [--out profiles/read_support_c5.json]
    python tools/read_support.py --config C2RM --merge-in-step [--mp-reads N] [--support-k K] [--anchor-mode exact|align|gapped]
"""
import argparse

import numpy as np

from preset_setup import emit, release, round_arguments, round_ms, round_setup, timed_steps


def _dist(v):
    v = np.asarray(v, dtype=np.int64)
    if not len(v):
        return {"n": 0}
    q = np.percentile(v, [5, 25, 50, 75, 95])
    return {"n": int(len(v)), "zero": int((v == 0).sum()), "min": int(v.min()), "p5": float(q[0]), "p25": float(q[1]), "median": float(q[2]),
            "p75": float(q[3]), "p95": float(q[4]), "max": int(v.max()), "mean": round(float(v.mean()), 3)}


def main():
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    round_arguments(ap)
    ap.add_argument("--rescue-round", action="store_true")
    ap.add_argument("--support-k", type=int, default=0)
    args = ap.parse_args()
    s, flags, out = round_setup(args, rescue_round=args.rescue_round)
    flags["merge_in_step"] = args.merge_in_step or args.rescue_round
    out.update(flags)
    pipe = s.pipeline(**flags)
    out["ms_per_step_off"] = round(timed_steps(pipe, args.steps), 3)
    del pipe
    release()
    pipe = s.pipeline(read_support=True, support_k=args.support_k or None, **flags)
    out["ms_per_step_on"] = round(timed_steps(pipe, args.steps), 3)
    res = pipe.fetch()
    out["support_k"], out["closed"], out["windows"] = pipe.support.k, int((res.best != 0).sum()), res.support_stats["windows"]
    ms, out["round_kernel_ms"] = round_ms(pipe, s.gf, pipe.support.enqueue, B.KERNEL_SUPPORT, args.steps)
    out["round_ms"] = round(ms[0], 4)
    seqs = pipe.picked_sequences(res)
    groups = {"correct": [], "wrong": []}
    for g, (_, body, _) in seqs.items():
        groups["correct" if body in s.truth(g) else "wrong"].append(g)
    sup = res.support
    for name, gs in groups.items():
        gs = np.array(gs, dtype=np.int64)
        out[name] = {f: _dist(sup[f][gs]) for f in ("min", "n_below", "zero_run", "n_zero")}
        out[name]["gaps"] = int(len(gs))
    # what a threshold on each field would do: fills it flags, among the wrong and among the correct ones
    c, w = np.array(groups["correct"], dtype=np.int64), np.array(groups["wrong"], dtype=np.int64)
    out["flagged"] = {"n_zero>0": [int((sup["n_zero"][w] > 0).sum()), int((sup["n_zero"][c] > 0).sum())],
                      "n_below>0": [int((sup["n_below"][w] > 0).sum()), int((sup["n_below"][c] > 0).sum())],
                      "zero_run>=k": [int((sup["zero_run"][w] >= pipe.support.k).sum()), int((sup["zero_run"][c] >= pipe.support.k).sum())]}
    out["flagged_columns"] = ["of the wrong fills", "of the correct fills"]
    emit(out, args.out)


if __name__ == "__main__":
    main()
