"""The step's rescue round (Pipeline(rescue_round=True), with merge_in_step) on one bench preset, off and on: prints one JSON line per
setting with the time per step, gaps closed, gaps closed with the true sequence (gf_synth_truth), and the round's counts (gaps tried, HQ
reads, gaps with bridges, bridges, merged contigs, gaps the rescue closed, dropped reads).

    python tools/rescue_round.py --config C2 [--steps 3] [--reads N] [--mp-reads N] [--anchor-mode exact|align]

--reads thins the short-insert library; --mp-reads adds the preset's mate-pair library (IS 5000 / sd 500, bench.MATE_PAIRS) with that many
read records (default: none).
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
    ap.add_argument("--mp-reads", type=int, default=0, help="read records of the mate-pair library (default: no mate-pair library)")
    ap.add_argument("--anchor-mode", default="exact", choices=("exact", "align"))
    ap.add_argument("--modes", default="off,on")
    args = ap.parse_args()
    seed, slen, nscf, gps, glen, dreads, kk = bench.PRESETS[args.config]
    L = 150
    rep_p, rep_c = bench.REPEATS.get(args.config, (0, 50))
    lib_defs = [("short-insert", 300, 30, 0, (args.reads or dreads) // 2 * 2, 1)]
    if args.mp_reads:
        lib_defs.append(("mate-pair", 5000, 500, 1, args.mp_reads // 2 * 2, 0))
    cfg0 = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L,
                             insert_mean=300, insert_sd=30, repeat_period=rep_p, repeat_copies=rep_c)
    gaps, flanks = GapFill.synth_layout(cfg0)
    gf = GapFill(0)
    gf.set_gaps(gaps, nscf, flanks)
    rb = B.lib().gf_packed_read_bytes(L)
    libs = []
    for name, is_mean, is_sd, lib_no, n_reads, pull in lib_defs:
        cfg = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L,
                                insert_mean=is_mean, insert_sd=is_sd, library=lib_no, repeat_period=rep_p, repeat_copies=rep_c)
        d_reads = torch.empty(n_reads * rb + 64, dtype=torch.uint8, device="cuda")
        d_recs = torch.empty(max(1, n_reads) * 32, dtype=torch.uint8, device="cuda")
        gf.synth_pairs_dev(cfg, 0, n_reads // 2, d_reads.data_ptr(), d_recs.data_ptr())
        libs.append((name, is_mean, is_sd, n_reads, d_reads, d_recs, pull))
    gf.sync()
    truth = {}
    for g in range(len(gaps)):
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        truth[g] = (GapFill.synth_truth(cfg0, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg0, sc, st - 6, en - st + 11))
    for mode in args.modes.split(","):
        pipe = Pipeline(gf, len(gaps), L, kk, merge_in_step=True, rescue_round=(mode == "on"), anchor_mode=args.anchor_mode)
        for name, is_mean, is_sd, n_reads, d_reads, d_recs, pull in libs:
            pipe.add_library(DeviceLibrary(name, is_mean, is_sd, n_reads, d_reads, d_recs, pull_mates=pull))
        t0 = time.perf_counter()
        pipe.prepare()
        sys.stderr.write("rescue_round=%s: prepared in %.1f s\n" % (mode, time.perf_counter() - t0))
        sys.stderr.flush()
        pipe.step(1)
        pipe.barrier()
        t0 = time.perf_counter()
        pipe.step(args.steps)
        pipe.barrier()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        res = pipe.fetch()
        seqs = pipe.picked_sequences(res)
        true = sum(1 for g, (_, body, _) in seqs.items() if body in truth[g])
        line = {"config": args.config, "reads": lib_defs[0][4], "mp_reads": args.mp_reads, "anchor_mode": args.anchor_mode, "rescue_round": mode,
                "gaps": len(gaps), "ms_per_step": round(ms, 3), "closed": len(seqs), "equal_to_truth": true}
        if res.rescue is not None:
            line["rescue"] = res.rescue
            line["rescue_equal_to_truth"] = sum(1 for g, (ci, body, _) in seqs.items() if ci >= res.rescue_first and body in truth[g])
        print(json.dumps(line), flush=True)
        del pipe, res
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
