"""The step's rescue round (Pipeline(rescue_round=True), with merge_in_step) on one bench preset, off and on: prints one JSON line per
setting with the time per step, gaps closed, gaps closed with the true sequence (gf_synth_truth), and the round's counts (gaps tried, HQ
reads, gaps with bridges, bridges, merged contigs, gaps the rescue closed, dropped reads).

    python tools/rescue_round.py --config C2 [--steps 3] [--reads N] [--mp-reads N] [--anchor-mode exact|align]

--reads thins the short-insert library; --mp-reads adds the preset's mate-pair library (IS 5000 / sd 500, bench.MATE_PAIRS) with that many
read records (default: none).
"""
import argparse
import json
import sys
import time

from preset_setup import preset_setup, release, timed_steps


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=sorted(bench.PRESETS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--mp-reads", type=int, default=0, help="read records of the mate-pair library (default: no mate-pair library)")
    ap.add_argument("--anchor-mode", default="exact", choices=("exact", "align", "gapped"))
    ap.add_argument("--modes", default="off,on")
    args = ap.parse_args()
    s = preset_setup(args.config, reads=args.reads, mp_reads=args.mp_reads)
    for mode in args.modes.split(","):
        pipe = s.pipeline(merge_in_step=True, rescue_round=(mode == "on"), anchor_mode=args.anchor_mode)
        t0 = time.perf_counter()
        ms = timed_steps(pipe, args.steps)
        sys.stderr.write("rescue_round=%s: prepared and stepped in %.1f s\n" % (mode, time.perf_counter() - t0))
        sys.stderr.flush()
        res = pipe.fetch()
        seqs = pipe.picked_sequences(res)
        true = sum(1 for g, (_, body, _) in seqs.items() if body in s.truth(g))
        line = {"config": args.config, "reads": s.reads, "mp_reads": args.mp_reads, "anchor_mode": args.anchor_mode, "rescue_round": mode,
                "gaps": len(s.gaps), "ms_per_step": round(ms, 3), "closed": len(seqs), "equal_to_truth": true}
        if res.rescue is not None:
            line["rescue"] = res.rescue
            line["rescue_equal_to_truth"] = sum(1 for g, (ci, body, _) in seqs.items() if ci >= res.rescue_first and body in s.truth(g))
        print(json.dumps(line), flush=True)
        del pipe, res
        release()


if __name__ == "__main__":
    main()
