"""The step's second assembly round (Pipeline(second_round=True)) on one bench preset, off and on: prints one JSON line per setting with
the time per step, gaps closed, gaps closed with the true sequence (gf_synth_truth), and the round's counts (both-unmapped candidate
reads, reads recruited, gaps tried / with recruits / closed in round 2, dropped recruits).  The preset's short-insert library only.

    python tools/second_round.py --config C2 [--steps 3] [--reads N] [--gap-len G]
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
    ap.add_argument("--config", default="C2", choices=sorted(bench.PRESETS))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--gap-len", type=int, default=0, help="gap length (default: the preset's)")
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
    truth = {}
    for g in range(len(gaps)):
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        truth[g] = (GapFill.synth_truth(cfg, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg, sc, st - 6, en - st + 11))
    for mode in args.modes.split(","):
        pipe = Pipeline(gf, len(gaps), L, kk, second_round=(mode == "on"))
        pipe.add_library(DeviceLibrary("short-insert", 300, 30, n_reads, d_reads, d_recs))
        pipe.prepare()
        pipe.step(1)
        pipe.barrier()
        t0 = time.perf_counter()
        pipe.step(args.steps)
        pipe.barrier()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        res = pipe.fetch()
        seqs = pipe.picked_sequences(res)
        true = sum(1 for g, (_, body, _) in seqs.items() if body in truth[g])
        line = {"config": args.config, "gap_len": glen, "reads": n_reads, "second_round": mode, "gaps": len(gaps), "ms_per_step": round(ms, 3),
                "closed": len(seqs), "equal_to_truth": true}
        if res.round2 is not None:
            first = res.round2_first
            r2 = {g: v for g, v in seqs.items() if v[0] >= first}
            line.update(res.round2)
            line["round2_equal_to_truth"] = sum(1 for g, (_, body, _) in r2.items() if body in truth[g])
        print(json.dumps(line), flush=True)
        del pipe, res
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
