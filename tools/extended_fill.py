"""The step's extended fill (Pipeline(extended_fill=True)) on one bench preset, off and on, per anchor mode: prints one JSON line per
setting with the time per step, the extension's own time per step (its launches repeated on the step's results), gaps closed, gaps
extended (left only, right only, both sides), fill bases, and how many parts equal the truth (gf_synth_truth): a left part the true
bases after the left anchor (from one base earlier when it keeps an anchor base), a right part the true bases before the right anchor
(up to its first base when the right side uses the left side's contig forward).  The preset's short-insert library only.

    python tools/extended_fill.py --config C4 [--steps 3] [--anchor-modes exact,align] [--reads N] [--gap-len G]
"""
import argparse
import json

from preset_setup import preset_setup, release, timed_steps


def main():
    import bench
    import torch
    from gappadder_amd.hip_api import GapFill
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4", choices=sorted(bench.PRESETS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--gap-len", type=int, default=0, help="gap length (default: the preset's)")
    ap.add_argument("--anchor-modes", default="exact,align")
    ap.add_argument("--modes", default="off,on")
    args = ap.parse_args()
    s = preset_setup(args.config, reads=args.reads, gap_len=args.gap_len)
    gaps, cfg = s.gaps, s.cfg
    for amode in args.anchor_modes.split(","):
        for mode in args.modes.split(","):
            pipe = s.pipeline(anchor_mode=amode, extended_fill=(mode == "on"))
            ms = timed_steps(pipe, args.steps)
            res = pipe.fetch()
            line = {"config": args.config, "gap_len": s.gap_len, "reads": s.reads, "anchor_mode": amode, "extended_fill": mode, "gaps": len(gaps),
                    "ms_per_step": round(ms, 3), "closed": int((res.best != 0).sum())}
            if res.extended is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    pipe.ext.enqueue()
                e1.record()
                pipe.barrier()
                line["extension_ms"] = round(e0.elapsed_time(e1) / args.steps, 4)
                line.update(res.extended)
                n_parts = n_true = 0
                for g, (li, ri, fill, _) in pipe.extended_sequences(res).items():
                    if fill is None:
                        continue
                    rec = res.ext[g]
                    ll = int(rec["l_len"])
                    lp, rp = fill[:ll], fill[ll + 2:]
                    st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
                    if lp:
                        n_parts += 1
                        n_true += GapFill.synth_truth(cfg, sc, st - 5 - int(rec["l_rev"]), len(lp)) == lp
                    if rp:
                        keep = int(rec["left"] == rec["right"] and not rec["r_rev"])
                        n_parts += 1
                        n_true += GapFill.synth_truth(cfg, sc, en + 5 + keep - len(rp), len(rp)) == rp
                line["parts"], line["parts_equal_to_truth"] = n_parts, n_true
            print(json.dumps(line), flush=True)
            del pipe, res
            release()


if __name__ == "__main__":
    main()
