"""The step's second assembly round (Pipeline(second_round=True)) on one bench preset, off and on: prints one JSON line per setting with
the time per step, gaps closed, gaps closed with the true sequence (gf_synth_truth), and the round's counts (both-unmapped candidate
reads, reads recruited, gaps tried / with recruits / closed in round 2, dropped recruits).  The preset's short-insert library only.

    python tools/second_round.py --config C2 [--steps 3] [--reads N] [--gap-len G]
    python tools/second_round.py C2 --rounds 6      the round off, once (R = 1) and repeated (recruit_rounds = 6): a "rounds" list with, per
                                                    recruitment round, pairs new / gaps grown / closed / closed = truth / gated
    python tools/second_round.py C2 --rounds 4 --fills [--out FILE]
                                                    one more run with closing_pools and read support, polish, pile-up and pair span on the
                                                    closing pools: the time of the closing-pool call (and the bytes it moves) and of each
                                                    after-pick round, and the rounds' records summed by closing round (first pick, round r)
                                                    and by correct / wrong fill
"""
import argparse
import json

from preset_setup import preset_setup, release, round_ms, timed_steps

FILL_ROUNDS = dict(read_support=True, polish=True, pileup=True, pair_span=True)


def fills_report(s, pipe, res, seqs, steps):
    """The closing-pool call's and the after-pick rounds' own times, and the rounds' records by closing round and correct / wrong fill."""
    from gappadder_amd import _lib as B
    cp, r2 = res.closing_pools, pipe.round2
    ms, _ = round_ms(pipe, s.gf, pipe.closing.enqueue, B.KERNEL_POOL, steps)
    rows = cp["rows"] + sum(d["rows"] for d in cp["per_library"])
    calls = 1 + len(cp["per_library"])
    # per call: the sorted keys, their flags and scan once for the bounds and once for the gather; every row read and written
    moved = calls * r2.key_cap * 2 * 16 + 2 * rows * pipe.rb + 4 * rows + calls * 16 * (len(s.gaps) + 1)
    out = {"closing_pools": cp, "closing_pools_ms": round(ms[0], 4), "closing_pools_calls": calls, "closing_pools_bytes": moved,
           "closing_pools_GBps": round(moved / ms[0] / 1e6, 2), "rounds_ms": {}}
    for rnd in pipe.after_pick:
        ms, _ = round_ms(pipe, s.gf, rnd.enqueue, B.KERNEL_POOL, steps)
        out["rounds_ms"][rnd.WHAT] = round(ms[0], 4)
    firsts = [d["first"] for d in res.recruit_rounds]
    split = {}
    for g, (ci, body, _) in sorted(seqs.items()):
        rnd = sum(1 for f in firsts if ci >= f)
        key = "%s, %s" % ("first pick" if rnd == 0 else "round %d" % rnd, "correct" if body in s.truth(g) else "wrong")
        d = split.setdefault(key, {"gaps": 0, "pool_rows": 0, "windows": 0, "windows_without_support": 0, "polish_changed": 0,
                                   "polish_uncovered": 0, "pileup_thin": 0, "pileup_contested": 0, "pairs_placed": 0, "pairs_in_range": 0,
                                   "columns_unspanned": 0})
        d["gaps"] += 1
        d["pool_rows"] += int(res.pairs[0, g]["rows"])
        d["windows"] += int(res.support[g]["n_windows"])
        d["windows_without_support"] += int(res.support[g]["n_zero"])
        d["polish_changed"] += int(res.polish[g]["n_changed"])
        d["polish_uncovered"] += int(res.polish[g]["n_uncovered"])
        d["pileup_thin"] += int(res.pileup[g]["n_thin"])
        d["pileup_contested"] += int(res.pileup[g]["n_contested"])
        d["pairs_placed"] += int(res.pairs[:, g]["pairs_placed"].sum())
        d["pairs_in_range"] += int(res.pairs[:, g]["n_in_range"].sum())
        d["columns_unspanned"] += int(res.pairs[0, g]["n_unspanned"])
    out["records"] = split
    return out


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("preset", nargs="?", choices=sorted(bench.PRESETS), help="the same as --config")
    ap.add_argument("--config", default="C2", choices=sorted(bench.PRESETS))
    ap.add_argument("--rounds", type=int, default=0, help="recruit_rounds of a third run (and of every mode spelled rN in --modes)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--gap-len", type=int, default=0, help="gap length (default: the preset's)")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--fills", action="store_true", help="one more run: closing_pools with support, polish, pile-up and pair span (needs --rounds)")
    ap.add_argument("--out", default="", help="with --fills: the output lines as one JSON list in this file")
    args = ap.parse_args()
    config = args.preset or args.config
    s = preset_setup(config, reads=args.reads, gap_len=args.gap_len)
    if args.fills and args.rounds < 1:
        ap.error("--fills needs --rounds R")
    modes = args.modes.split(",") + (["r%d" % args.rounds] if args.rounds > 1 else []) + (["fills"] if args.fills else [])
    lines = []
    for mode in modes:
        rounds = args.rounds if mode == "fills" else int(mode[1:]) if mode.startswith("r") else 1
        pipe = s.pipeline(second_round=(mode != "off"), recruit_rounds=rounds, **(dict(FILL_ROUNDS, closing_pools=True) if mode == "fills" else {}))
        ms = timed_steps(pipe, args.steps)
        res = pipe.fetch()
        seqs = pipe.picked_sequences(res)
        true = sum(1 for g, (_, body, _) in seqs.items() if body in s.truth(g))
        line = {"config": config, "gap_len": s.gap_len, "reads": s.reads, "second_round": mode, "gaps": len(s.gaps), "ms_per_step": round(ms, 3),
                "closed": len(seqs), "equal_to_truth": true}
        if res.round2 is not None:
            line.update(res.round2)
            line["round2_equal_to_truth"] = sum(1 for g, (ci, body, _) in seqs.items() if ci >= res.round2_first and body in s.truth(g))
            firsts = [d["first"] for d in res.recruit_rounds] + [len(res.contigs)]
            line["recruit_rounds_run"] = res.recruit_rounds_run
            line["rounds"] = [{"new_pairs": d["new_pairs"], "gaps_grown": d["gaps_grown"], "closed": d["gaps_closed"], "gated": d["gated"],
                               "equal_to_truth": sum(1 for g, (ci, body, _) in seqs.items() if lo <= ci < hi and body in s.truth(g))}
                              for d, lo, hi in zip(res.recruit_rounds, firsts, firsts[1:])]
        if mode == "fills":
            line.update(fills_report(s, pipe, res, seqs, args.steps))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del pipe, res
        release()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(lines, indent=1) + "\n")


if __name__ == "__main__":
    main()
