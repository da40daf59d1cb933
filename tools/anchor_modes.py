"""The picker's three flank-anchoring modes on one bench preset: `exact` anchors (the default), `align` (seed-and-extend of the whole
flanks, gappadder_amd/pick_contigs.py::align_hits, gf_pick_aligned_dev) and `gapped` (the same with a banded affine-gap extension,
gapped_hits, gf_pick_gapped_dev).  Runs the preset's step through `Pipeline` once per mode and prints one JSON line per mode: gaps
closed, closed with the true sequence, the step's wall time and the pick kernels' time per step, the align / gapped mode's overflow
counts.  --plant FRAC plants one draft mismatch within the 10 gap-side bases of one flank of that fraction of the gaps (the reads stay
true): the case exact anchors lose and bwa-grade anchoring keeps.  --plant-indel FRAC plants a 1-3 base insertion or deletion 8-14
bases from the gap-side end of one flank instead: the case only `gapped` keeps.

    python tools/anchor_modes.py --config C2RM [--plant 0.5 | --plant-indel 0.5] [--steps 3] [--reads N] [--modes exact,align,gapped]
"""
import argparse
import json
import time

import numpy as np

from preset_setup import preset_setup, release


def main():
    import bench
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2RM", choices=sorted(bench.PRESETS))
    ap.add_argument("--plant", type=float, default=0.0, help="fraction of the gaps whose draft flank gets one mismatch next to the gap")
    ap.add_argument("--plant-indel", type=float, default=0.0,
                    help="fraction of the gaps whose draft flank gets a 1-3 base insertion or deletion 8-14 bases from the gap")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--modes", default="exact,align,gapped")
    args = ap.parse_args()
    rng = np.random.default_rng(bench.PRESETS[args.config][0])
    planted = set()

    def plant(flanks):
        out = []
        for g, (l, r) in enumerate(flanks):
            if rng.random() < args.plant_indel:
                planted.add(g)
                n, dist = int(rng.integers(1, 4)), int(rng.integers(8, 15))       # dist bases stay between the edit and the gap
                new = "".join(rng.choice(list("ACGT"), size=n)) if rng.integers(0, 2) else None      # None: a deletion
                if rng.integers(0, 2):
                    i = len(l) - dist
                    l = l[:i] + new + l[i:] if new else l[:i - n] + l[i:]
                else:
                    r = r[:dist] + new + r[dist:] if new else r[:dist] + r[dist + n:]
            elif rng.random() < args.plant:
                planted.add(g)
                if rng.integers(0, 2):
                    i = len(l) - 1 - int(rng.integers(0, 10))
                    l = l[:i] + rng.choice([b for b in "ACGT" if b != l[i]]) + l[i + 1:]
                else:
                    i = int(rng.integers(0, 10))
                    r = r[:i] + rng.choice([b for b in "ACGT" if b != r[i]]) + r[i + 1:]
            out.append((l, r))
        return out
    mp = bench.MATE_PAIRS.get(args.config, 0) // 2 * 2
    s = preset_setup(args.config, reads=args.reads, mp_reads=mp, edit_flanks=plant if args.plant > 0 or args.plant_indel > 0 else None)
    gf = s.gf
    for mode in args.modes.split(","):
        pipe = s.pipeline(merge_in_step=bool(mp), anchor_mode=mode)
        pipe.prepare()
        pipe.step(1)
        pipe.barrier()
        t0 = time.perf_counter()
        pipe.step(args.steps)
        pipe.barrier()
        step_ms = (time.perf_counter() - t0) * 1e3 / args.steps
        gf.timing(True)                    # (the same steps again with an event pair around every pick: the pick kernels' own time)
        pipe.step(args.steps)
        pipe.barrier()
        pick_ms, launches = gf.kernel_time(B.KERNEL_PICK)
        gf.timing(False)
        res = pipe.fetch()
        seqs = pipe.picked_sequences(res)
        true = sum(1 for g, (_, body, _) in seqs.items() if body in s.truth(g))
        line = {"config": args.config, "mode": mode, "gaps": len(s.gaps), "closed": len(seqs), "equal_to_truth": true, "step_ms": round(step_ms, 3),
                "pick_ms_per_step": round(pick_ms / args.steps, 4), "pick_launches_per_step": launches / args.steps}
        if planted:
            line.update(planted=len(planted), planted_closed=sum(1 for g in planted if g in seqs),
                        planted_equal_to_truth=sum(1 for g in planted if g in seqs and seqs[g][1] in s.truth(g)))
        if mode != "exact":
            line.update(overflow_dropped=res.align_dropped, overflow_seed_contigs=res.align_seed_overflow)
        print(json.dumps(line), flush=True)
        del pipe, res
        release()


if __name__ == "__main__":
    main()
