"""The step's second assembly round (Pipeline(second_round=True)) on one bench preset, off and on: prints one JSON line per setting with
the time per step, gaps closed, gaps closed with the true sequence (gf_synth_truth), and the round's counts (both-unmapped candidate
reads, reads recruited, gaps tried / with recruits / closed in round 2, dropped recruits).  The preset's short-insert library only.

    python tools/second_round.py --config C2 [--steps 3] [--reads N] [--gap-len G]
    python tools/second_round.py C2 --rounds 6      the round off, once (R = 1) and repeated (recruit_rounds = 6): a "rounds" list with, per
                                                    recruitment round, pairs new / gaps grown / closed / closed = truth / gated
"""
import argparse
import json

from preset_setup import preset_setup, release, timed_steps


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
    args = ap.parse_args()
    config = args.preset or args.config
    s = preset_setup(config, reads=args.reads, gap_len=args.gap_len)
    modes = args.modes.split(",") + (["r%d" % args.rounds] if args.rounds > 1 else [])
    for mode in modes:
        rounds = int(mode[1:]) if mode.startswith("r") else 1
        pipe = s.pipeline(second_round=(mode != "off"), recruit_rounds=rounds)
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
        print(json.dumps(line), flush=True)
        del pipe, res
        release()


if __name__ == "__main__":
    main()
