"""The step's extended fill (Pipeline(extended_fill=True)) on one bench preset, off and on, per anchor mode: prints one JSON line per
setting with the time per step, the extension's own time per step (its launches repeated on the step's results), gaps closed, gaps
extended (left only, right only, both sides), fill bases, and how many parts equal the truth (gf_synth_truth): a left part the true
bases after the left anchor (from one base earlier when it keeps an anchor base), a right part the true bases before the right anchor
(up to its first base when the right side uses the left side's contig forward).  The preset's short-insert library only.

    python tools/extended_fill.py --config C4 [--steps 3] [--anchor-modes exact,align] [--reads N] [--gap-len G]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4", choices=sorted(bench.PRESETS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--gap-len", type=int, default=0, help="gap length (default: the preset's)")
    ap.add_argument("--anchor-modes", default="exact,align")
    ap.add_argument("--modes", default="off,on")
    args = ap.parse_args()
    seed, slen, nscf, gps, glen, dreads, kk = bench.PRESETS[args.config]
    glen = args.gap_len or glen
    n_reads = (args.reads or dreads) // 2 * 2
    L = 150
    rep_p, rep_c = bench.REPEATS.get(args.config, (0, 50))
    cfg = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L,
                            insert_mean=300, insert_sd=30, repeat_period=rep_p, repeat_copies=rep_c)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf = GapFill(0)
    gf.set_gaps(gaps, nscf, flanks)
    rb = B.lib().gf_packed_read_bytes(L)
    d_reads = torch.empty(n_reads * rb + 64, dtype=torch.uint8, device="cuda")
    d_recs = torch.empty(max(1, n_reads) * 32, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg, 0, n_reads // 2, d_reads.data_ptr(), d_recs.data_ptr())
    gf.sync()
    for amode in args.anchor_modes.split(","):
        for mode in args.modes.split(","):
            pipe = Pipeline(gf, len(gaps), L, kk, anchor_mode=amode, extended_fill=(mode == "on"))
            pipe.add_library(DeviceLibrary("short-insert", 300, 30, n_reads, d_reads, d_recs))
            pipe.prepare()
            pipe.step(1)
            pipe.barrier()
            t0 = time.perf_counter()
            pipe.step(args.steps)
            pipe.barrier()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            res = pipe.fetch()
            line = {"config": args.config, "gap_len": glen, "reads": n_reads, "anchor_mode": amode, "extended_fill": mode, "gaps": len(gaps),
                    "ms_per_step": round(ms, 3), "closed": int((res.best != 0).sum())}
            if res.extended is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    pipe._extend()
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
            torch.cuda.synchronize()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
