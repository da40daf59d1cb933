"""The polish round (Pipeline(polish=True)) on one bench preset: the step's time with the round off and on — two prepared pipelines
stepped in turn, `--reps` timed windows each, so the spread is known before a difference is read —, the round's own time (its launch
repeated on the step's results, and the library's launch timer), and — the presets know the truth (gf_synth_truth) — the fills that equal
the truth before and after the round, the four transitions (every correct -> wrong fill with its gap, its record and its pool size), and
the distributions of `n_changed` and `reads_ambiguous` per transition group.  One JSON object on stdout, and in --out when given.

    python tools/polish_fills.py --config C5 --asm-tiebreak none [--out profiles/polish_c5_none.json]
    python tools/polish_fills.py --config C2RM --merge-in-step [--mp-reads N] [--anchor-mode exact|align|gapped]
"""
import argparse
import json
import time

import numpy as np

from preset_setup import preset_setup


def _dist(v):
    v = np.asarray(v, dtype=np.int64)
    if not len(v):
        return {"n": 0}
    q = np.percentile(v, [50, 95])
    return {"n": int(len(v)), "zero": int((v == 0).sum()), "median": float(q[0]), "p95": float(q[1]), "max": int(v.max()), "mean": round(float(v.mean()), 3)}


def _spread(ms):
    return {"ms": [round(x, 3) for x in ms], "median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    import bench
    import torch
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4", choices=sorted(bench.PRESETS))
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
    ap.add_argument("--reps", type=int, default=3, help="timed windows per setting, off and on in turn")
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--mp-reads", type=int, default=0, help="read records of the preset's mate-pair library (default: none)")
    ap.add_argument("--gap-len", type=int, default=0)
    ap.add_argument("--anchor-mode", default="exact")
    ap.add_argument("--asm-tiebreak", default="counts", choices=["counts", "none"])
    ap.add_argument("--merge-in-step", action="store_true")
    ap.add_argument("--seed", type=int, default=16)
    ap.add_argument("--max-mismatch", type=int, default=4)
    ap.add_argument("--min-overlap", type=int, default=48)
    ap.add_argument("--min-votes", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    s = preset_setup(args.config, reads=args.reads, gap_len=args.gap_len, mp_reads=args.mp_reads)
    s.gf.set_option("asm_tiebreak", 0 if args.asm_tiebreak == "none" else 1)
    flags = dict(anchor_mode=args.anchor_mode, merge_in_step=args.merge_in_step)
    prm = dict(polish_seed=args.seed, polish_max_mismatch=args.max_mismatch, polish_min_overlap=args.min_overlap, polish_min_votes=args.min_votes)
    out = {"config": args.config, "gaps": len(s.gaps), "gap_len": s.gap_len, "reads": s.reads, "mp_reads": args.mp_reads,
           "asm_tiebreak": args.asm_tiebreak, "steps": args.steps, **flags, **prm}
    pipes = {"off": s.pipeline(**flags), "on": s.pipeline(polish=True, **prm, **flags)}
    for pipe in pipes.values():
        pipe.prepare()
        pipe.step(1)
        pipe.barrier()
    ms = {"off": [], "on": []}
    for _ in range(args.reps):
        for name, pipe in pipes.items():
            t0 = time.perf_counter()
            pipe.step(args.steps)
            pipe.barrier()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out["ms_per_step_off"], out["ms_per_step_on"] = _spread(ms["off"]), _spread(ms["on"])
    pipe = pipes["on"]
    res = pipe.fetch()
    pool_off = res.asm_off_t.cpu().numpy().astype(np.int64)
    out["closed"], out["polish_stats"] = int((res.best != 0).sum()), res.polish_stats
    s.gf.timing(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        pipe.polish.enqueue()
    e1.record()
    pipe.barrier()
    out["round_ms"] = round(e0.elapsed_time(e1) / args.steps, 4)
    t_ms, n = s.gf.kernel_time(B.KERNEL_POLISH)
    out["round_kernel_ms"] = round(t_ms / max(1, n), 4)
    s.gf.timing(False)
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
    text = json.dumps(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
