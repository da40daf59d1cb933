"""The CLI's contig-merge rounds with either engine (parameters.contig_merger = "host" | "device") on one bench preset's FILES: writes
the preset's draft FASTA, BAM and FASTQ pair once (tools/synth_files), runs `python -m gappadder_amd.main -c All` as a fresh child process
once per engine (and --repeats times, engines alternated) into a working folder of its own, compares what the engines' assembly rounds wrote (merged/ and picked_seqs.fa) file by
file, and prints one JSON line per run — the GF_TIMINGS stage split, the later rounds' seconds per gap, the sets that fell back to the
host path — and a last line with the comparison.  Exit code 1 when a child fails (the runs stop there) or the folders differ.

    python tools/contig_merger.py --config C2 [--repeats 1] [--engines host,device] [--child-timeout 900] [--keep DIR]
"""
import argparse
import filecmp
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def compare_trees(a, b):
    """Relative paths that exist on one side only or differ in their bytes."""
    diff = []
    for x, y in ((a, b), (b, a)):
        for root, _, files in os.walk(x):
            for fn in files:
                p = os.path.join(root, fn)
                rel = os.path.relpath(p, x)
                q = os.path.join(y, rel)
                if not os.path.exists(q):
                    diff.append(rel)
                elif x is a and not filecmp.cmp(p, q, shallow=False):
                    diff.append(rel)
    return sorted(set(diff))


def main():
    import bench
    import synth_files_util as SF
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=sorted(bench.PRESETS))
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--engines", default="host,device")
    ap.add_argument("--child-timeout", type=int, default=900, help="seconds every child process may take")
    ap.add_argument("--keep", default="", help="write the files under this folder and keep them")
    args = ap.parse_args()
    engines = args.engines.split(",")
    seed, slen, nscf, gps, glen, dreads, kk = bench.PRESETS[args.config]
    root = args.keep or tempfile.mkdtemp(prefix="gf_merger_")
    ok = True
    try:
        cfgp, _ = SF.write_case(root, seed, slen, nscf, gps, glen, [(300, 30, dreads // 2)], kk, kmer_screen=min(a for a, _ in kk),
                                nthreads=max(1, min(16, (os.cpu_count() or 2) // 2)))
        base = json.load(open(cfgp))
        folders = {}
        for rep in range(args.repeats):
            for eng in engines:
                wf = os.path.join(root, "wf_%s" % eng)
                os.makedirs(wf, exist_ok=True)
                cfg = dict(base, parameters=dict(base["parameters"], working_folder=wf, contig_merger=eng))
                cp = os.path.join(root, "cfg_%s.json" % eng)
                json.dump(cfg, open(cp, "w"))
                tfile = os.path.join(root, "timings_%s.json" % eng)
                t0 = time.perf_counter()
                # a fresh child per run, under a time limit of its own; after a child that fails nothing more is started
                r = subprocess.run(["timeout", "-k", "10", str(args.child_timeout), sys.executable, "-m", "gappadder_amd.main", "-c", "All", "-g", cp],
                                   cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, GF_TIMINGS=tfile))
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    print(json.dumps({"engine": eng, "error": "CLI exit code %d" % r.returncode, "stderr_tail": r.stderr.decode()[-800:]}), flush=True)
                    return 1
                t = json.load(open(tfile))
                gaps = t.get("gaps") or t.get("assembly", {}).get("gaps") or 0
                later = t["stages_s"].get("assembly_rounds")
                print(json.dumps({"config": args.config, "engine": eng, "repeat": rep, "wall_s": round(wall, 3), "stages_s": t["stages_s"],
                                  "device_collect_s": t.get("seconds"), "gaps": gaps, "later_rounds_s": later,
                                  "later_rounds_ms_per_gap": round(1e3 * later / gaps, 4) if later and gaps else None,
                                  "contig_merger": t.get("contig_merger"), "assembly_rounds": t.get("assembly")}), flush=True)
                folders[eng] = wf
        if len(folders) == 2:
            a, b = (folders[e] for e in engines[:2])
            # what the merge rounds and everything behind them write: merged/ (velvet_temp/*/…) and picked_seqs.fa; the Collect stage's
            # per-library folders are listed for information (their read lists are written in the order the device found the reads)
            diff = compare_trees(a, b)
            mine = [d for d in diff if d.startswith("merged" + os.sep) or d == "picked_seqs.fa"]
            n = sum(len(f) for _, _, f in os.walk(os.path.join(a, "merged")))
            print(json.dumps({"compared": engines[:2], "files_under_merged": n, "differing": mine[:20], "n_differing": len(mine), "same": not mine,
                              "differing_outside_the_assembly_rounds": [d for d in diff if d not in mine][:20]}), flush=True)
            ok = not mine
    finally:
        if not args.keep:
            shutil.rmtree(root, ignore_errors=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
