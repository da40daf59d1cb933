"""The read adjudication (Pipeline(alternatives=True, adjudicate=True), gappadder_amd/fill_adjudication.py) on one bench preset.  Runs the
preset's step with the round off (the alternatives alone) and on (two prepared pipelines stepped in turn) and prints one JSON object: the
step's time off and on, the round's own time (its launch repeated on the step's results, and the library's kernel timer), the
statistics, and — the presets know the truth (gf_synth_truth) — the contested gaps split by verdict x (winner correct, rival correct,
neither), so that one reads off whether SWITCH ever replaces a correct fill.

--plant-het N plants a heterozygous site in the first N gaps before anything runs, PLANT_AT bases into the gap: of the short-insert
library's reads whose alignment record says they cover that column (reads mapped in the left flank that run into the gap — a read
from deeper inside the gap has no position on the draft and keeps the true base, so the planted allele is the minor one; found by
position on the device; none clipped on the left, whose offset would be off), every second one gets that base substituted (on the strand the read is stored on, which the read's own base at the column tells).  The truth stays the generator's: a
fill that carries the planted allele counts as wrong.

    python tools/fill_adjudication.py C2RM --merge-in-step [--plant-het 200] [--asm-tiebreak none] [--min-votes 3] [--ratio 2]
                                      [--context N] [--steps 3] [--reps 3] [--out profiles/fill_adjudication_c2rm.json]
"""
import argparse

import numpy as np

from preset_setup import L, emit, in_turn, preset_setup, round_ms

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
PLANT_AT = 40


def plant_het(s, n_gaps, L):
    """The site in the first n_gaps gaps of preset_setup's namespace s; returns the reads changed per gap."""
    import torch
    from gappadder_amd.hip_api import GapFill
    name, is_mean, is_sd, n, d_reads, d_recs, pull = s.libs[0]
    rb = (L + 3) // 4
    recs = d_recs[:n * 32].view(torch.int32).view(-1, 8)               # gf_alnrec: pos, mate_pos, tlen, ref, mate_ref, flag | mapq | clip, read (u64)
    pos, ref, clip, read = recs[:, 0], recs[:, 3], (recs[:, 5] >> 24) & 0xFF, recs[:, 6]
    rows = d_reads[:n * rb].view(-1, rb)
    changed = []
    for g in range(min(n_gaps, len(s.gaps))):
        sc, col = int(s.gaps[g]["scaffold"]), int(s.gaps[g]["start"]) + PLANT_AT          # (0-based column of the scaffold)
        true = GapFill.synth_truth(s.cfg, sc, col, 1)
        alt = "ACGT"[("ACGT".index(true) + 1) % 4]
        hit = torch.nonzero((ref == sc) & (pos - 1 <= col) & (pos - 1 + L > col) & ((clip & 1) == 0)).flatten()
        ids, offs = read[hit].long(), (col - (pos[hit] - 1)).long()
        n_done = 0
        for x, (i, o) in enumerate(zip(ids.tolist(), offs.tolist())):
            if x % 2:
                continue
            for at, want, put in ((o, true, alt), (L - 1 - o, COMP[true], COMP[alt])):       # stored as the draft reads, or reverse-complemented
                byte, sh = at // 4, 6 - 2 * (at % 4)
                v = int(rows[i, byte])
                if "ACGT"[(v >> sh) & 3] == want:
                    rows[i, byte] = (v & ~(3 << sh)) | ("ACGT".index(put) << sh)
                    n_done += 1
                    break
        changed.append(n_done)
    torch.cuda.synchronize()
    return changed


def main():
    import bench
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_adjudication as ADJ
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(bench.PRESETS))
    ap.add_argument("--plant-het", type=int, default=0, help="gaps that get a planted heterozygous site")
    ap.add_argument("--asm-tiebreak", default="counts", choices=["counts", "none"])
    ap.add_argument("--merge-in-step", action="store_true")
    ap.add_argument("--min-votes", type=int, default=ADJ.MIN_VOTES)
    ap.add_argument("--ratio", type=int, default=ADJ.RATIO)
    ap.add_argument("--context", type=int, default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0, help="read records of the short-insert library (default: the preset's)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    mp = bench.MATE_PAIRS.get(args.config, 0) // 2 * 2
    s = preset_setup(args.config, reads=args.reads, mp_reads=mp)
    s.gf.set_option("asm_tiebreak", 0 if args.asm_tiebreak == "none" else 1)
    planted = plant_het(s, args.plant_het, L) if args.plant_het else []
    flags = dict(merge_in_step=bool(args.merge_in_step or mp), alternatives=True)
    on = dict(adjudicate=True, adj_min_votes=args.min_votes, adj_ratio=args.ratio, adj_context=args.context)
    out = {"config": args.config, "gaps": len(s.gaps), "gap_len": s.gap_len, "reads": s.reads, "mp_reads": mp, "k_pairs": [list(p) for p in s.kk],
           "steps": args.steps, "asm_tiebreak": args.asm_tiebreak, "merge_in_step": flags["merge_in_step"], "adjudicate": on,
           "planted_gaps": len(planted), "planted_reads": int(sum(planted))}
    pipes, ms = in_turn(s, flags, {"off": {}, "on": on}, args.steps, args.reps)
    out.update(ms)
    pipe = pipes["on"]
    res = pipe.fetch()
    picked, rivals = pipe.picked_sequences(res), pipe.alternative_sequences(res)
    out.update(closed=len(picked), alt_stats=res.alt_stats, adj_stats=res.adj_stats)
    tables = {}
    for name, gaps in (("all", sorted(rivals)), ("planted", [g for g in sorted(rivals) if g < len(planted)])):
        table = {v: {"winner_correct": 0, "rival_correct": 0, "neither": 0} for v in ADJ.VERDICTS}
        for g in gaps:
            truth = s.truth(g)
            which = "winner_correct" if picked[g][1] in truth else "rival_correct" if rivals[g][1] in truth else "neither"
            table[ADJ.VERDICTS[int(res.adjudication[g]["verdict"])]][which] += 1
        tables[name] = table
    out["verdict_by_truth"] = tables["all"]
    out["verdict_by_truth_planted_gaps"] = tables["planted"]
    out["switch_replaces_a_correct_fill"] = tables["all"]["switch"]["winner_correct"]
    t, k = round_ms(pipe, s.gf, lambda: pipe.adj.enqueue(None), B.KERNEL_ADJ, args.steps, args.reps)       # (None: the step passes no N masks either)
    out["round_ms"], out["round_kernel_ms"] = [round(x, 4) for x in t], k
    emit(out, args.out)


if __name__ == "__main__":
    main()
