"""The pile-up round (Pipeline(pileup=True)) on one bench preset: the step's time with the round off and on — two prepared pipelines
stepped in turn, `--reps` timed windows of `--steps` steps each after a warm-up step, so the spread is known before a difference is
read —, the round's own time (its launch repeated on the step's results, and the library's launch timer), the same for the
records-only mode, and — the presets know the truth (gf_synth_truth) — what the marks are worth: over the fills that do NOT equal the
truth, the share of their wrong columns (against the truth, aligned without gaps where the fill has the truth's length) that the round
marks low or minority, beside the share of ALL columns of the correct fills so marked.  One JSON object on stdout, and in --out.

    python tools/fill_pileup.py --config C5 --mp-reads 400000000 [--out profiles/pileup_c5_counts.json]
    python tools/fill_pileup.py --config C2RM --merge-in-step --mp-reads 32000000 [--anchor-mode exact|align|gapped]
"""
import argparse

import numpy as np

from preset_setup import emit, in_turn, round_arguments, round_ms, round_setup


def marks(s, pipe, res, min_depth, min_agree):
    """The column shares of the module docstring, from fill_confidence's oriented entries."""
    from gappadder_amd import pileup as PU
    out = {"correct_fills": 0, "correct_columns": 0, "correct_marked": 0, "wrong_fills": 0, "wrong_fills_same_length": 0, "wrong_columns": 0,
           "wrong_marked": 0, "wrong_fills_with_a_marked_column": 0, "no_track": 0}
    for g, (_, seq, entries, _) in pipe.fill_confidence(res).items():
        if entries is None:
            out["no_track"] += 1
            continue
        codes = PU._codes(seq)
        unc, thin, con, mino = PU._classes(entries, codes, min_depth, min_agree)[:4]
        marked = unc | thin | con | mino
        truths = s.truth(g)
        if any(seq in t for t in truths):
            out["correct_fills"] += 1
            out["correct_columns"] += len(seq)
            out["correct_marked"] += int(marked.sum())
            continue
        out["wrong_fills"] += 1
        out["wrong_fills_with_a_marked_column"] += bool(marked.any())
        # a fill of the truth's length: its wrong columns are where it differs from the truth at the better of the offsets it can take
        best = None
        for t in truths:
            for o in range(len(t) - len(seq) + 1):
                diff = np.frombuffer(t[o:o + len(seq)].encode(), dtype=np.uint8) != np.frombuffer(seq.encode(), dtype=np.uint8)
                if best is None or diff.sum() < best.sum():
                    best = diff
        if best is None or best.sum() > len(seq) // 4:        # another length, or no gapless alignment worth the name
            continue
        out["wrong_fills_same_length"] += 1
        out["wrong_columns"] += int(best.sum())
        out["wrong_marked"] += int((best & marked).sum())
    out["correct_share"] = round(out["correct_marked"] / max(1, out["correct_columns"]), 6)
    out["wrong_share"] = round(out["wrong_marked"] / max(1, out["wrong_columns"]), 6)
    return out


def main():
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    round_arguments(ap, reps=True, placing=True)
    ap.add_argument("--min-depth", type=int, default=3)
    ap.add_argument("--min-agree", type=int, default=80)
    args = ap.parse_args()
    s, flags, out = round_setup(args)
    prm = dict(pileup_seed=args.seed, pileup_max_mismatch=args.max_mismatch, pileup_min_overlap=args.min_overlap, pileup_min_depth=args.min_depth,
               pileup_min_agree=args.min_agree)
    out.update(steps=args.steps, **flags, **prm)
    pipes, ms = in_turn(s, flags, {"off": {}, "on": dict(pileup=True, **prm), "records_only": dict(pileup=True, pileup_track=False, **prm)},
                        args.steps, args.reps)
    out.update(ms)
    pipe = pipes["on"]
    res = pipe.fetch()
    out.update(closed=int((res.best != 0).sum()), pileup_stats=res.pileup_stats, seq_cap=pipe.seq_cap, track_bytes=pipe.seq_cap * B.PU_ENTRY_BYTES,
               passes=int(sum(-(-int(n) // 1024) for n in res.pileup["len"])))
    for name in ("on", "records_only"):
        t, k = round_ms(pipes[name], s.gf, pipes[name].pileup.enqueue, B.KERNEL_PILEUP, args.steps, args.reps)
        out["round_ms_" + name], out["round_kernel_ms_" + name] = [round(x, 4) for x in t], k
    out["marks"] = marks(s, pipe, res, args.min_depth, args.min_agree)
    emit(out, args.out)


if __name__ == "__main__":
    main()
