"""The gap-span round (Pipeline(gap_span=True)) on one bench preset: the step's time with the round off and on — two
prepared pipelines stepped in turn, `--reps` timed windows each —, per library the launch timer of the span pass beside the tagger's for
the same records, the records' statistics, and the estimate against the truth: the presets' gaps are as long as the draft says, so
est - G0 is the error; its median and spread per library, and how many gaps have an estimate at all.

--shift-draft N (may be given more than once): the estimate when the draft's N-run is wrong by a known amount.  For every second gap the
draft coordinates right of the gap move right by N in the records of the pairs that straddle it — the mate's position and the template
length (torch ops on a copy of the library's records on the device; pairs that lie wholly on one side keep their coordinates, so the
neighbouring gaps are not touched) — which is what the records would look like if the true gap were G0 - N.  gf_gap_span_dev runs
off-step on the copy (record form); reported: est - (G0 - N) over the moved gaps and est - G0 over the others.
One JSON object on stdout, and in --out when given.

    python tools/gap_span.py --config C2RM --mp-reads N --merge-in-step [--shift-draft 50 --shift-draft 200] [--out profiles/gap_span_c2rm.json]
"""
import argparse

import numpy as np

from preset_setup import L, emit, off_and_on, round_arguments, round_setup


def _dist(v):
    v = np.asarray(v, dtype=np.float64)
    if not len(v):
        return {"n": 0}
    q = np.percentile(v, [5, 25, 50, 75, 95])
    return {"n": int(len(v)), "p5": round(float(q[0]), 2), "p25": round(float(q[1]), 2), "median": round(float(q[2]), 2), "p75": round(float(q[3]), 2),
            "p95": round(float(q[4]), 2), "mean": round(float(v.mean()), 2), "sd": round(float(v.std()), 2)}


def _errors(recs, gaps, truth, lb, gs):
    """est - truth, naive - truth and se over the gaps with an estimate; the gaps without one."""
    from gappadder_amd import gap_span as GS
    est, naive, se, none = [], [], [], 0
    for g in range(len(gaps)):
        g0 = int(gaps[g]["end"]) - int(gaps[g]["start"])
        e = GS.estimate(recs[g], g0, L, lb.is_mean, lb.is_sd, gs.z, gs.shift, gs.min_pairs)
        if e is None or truth[g] is None:
            none += e is None
            continue
        est.append(e.est - truth[g])
        naive.append(e.naive - truth[g])
        se.append(e.se)
    return {"est_minus_truth": _dist(est), "naive_minus_truth": _dist(naive), "se": _dist(se), "gaps_without_estimate": int(none)}


def _shifted(pipe, lb, gaps, chosen, n_shift):
    """gf_gap_span_dev on a copy of library lb's records with the coordinates right of the chosen gaps moved by n_shift (module docstring)."""
    import torch
    from gappadder_amd import _lib as B
    dev = pipe.dev
    r = lb.d_recs[:lb.n_recs * 32].clone().view(torch.int32).view(-1, 8)
    pos, mpos, tlen = r[:, 0].to(torch.int64) & 0xFFFFFFFF, r[:, 1].to(torch.int64) & 0xFFFFFFFF, r[:, 2].to(torch.int64)
    ref, mref, flag = r[:, 3].to(torch.int64) & 0xFFFFFFFF, r[:, 4].to(torch.int64) & 0xFFFFFFFF, r[:, 5].to(torch.int64) & 0xFFFF
    lo, hi = torch.minimum(pos, mpos), torch.maximum(pos, mpos)
    g_scaf = torch.from_numpy(gaps["scaffold"].astype(np.int64)).to(dev)
    g_start = torch.from_numpy(gaps["start"].astype(np.int64)).to(dev)
    g_end = torch.from_numpy(gaps["end"].astype(np.int64)).to(dev)
    g_key = (g_scaf << 32) | g_start
    nxt = torch.cat([torch.where(g_scaf[1:] == g_scaf[:-1], g_start[1:], torch.full_like(g_start[1:], 1 << 40)),
                     torch.full((1,), 1 << 40, dtype=torch.int64, device=dev)])
    pick = torch.from_numpy(np.asarray(chosen, dtype=bool)).to(dev)
    g = torch.searchsorted(g_key, (ref << 32) | (lo - 1), right=True).clamp(max=len(gaps) - 1)      # the first gap that starts behind lo
    move = (ref == mref) & ((flag & 12) == 0) & (tlen != 0) & (g_scaf[g] == ref) & (g_start[g] > lo - 1) & pick[g] & (hi - 1 >= g_end[g]) & (hi - 1 < nxt[g])
    r[:, 0] = torch.where(move & (pos == hi) & (pos != lo), pos + n_shift, pos).to(torch.int32)
    r[:, 1] = torch.where(move & (mpos == hi) & (mpos != lo), mpos + n_shift, mpos).to(torch.int32)
    r[:, 2] = torch.where(move, tlen + n_shift * torch.sign(tlen), tlen).to(torch.int32)
    d_rec = torch.zeros(max(1, pipe.n_gaps) * B.GAP_SPAN.itemsize, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(B.GS_WORDS, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    gs = pipe.gap_span
    pipe._chk(pipe.lib.gf_gap_span_dev(pipe.h, r.data_ptr(), None, lb.n_recs, pipe.L, lb.is_mean, lb.is_sd, gs.z, gs.shift, pipe.anchor_mapq,
                                       d_rec.data_ptr(), d_st.data_ptr()), "gf_gap_span_dev")
    pipe.barrier()
    return np.frombuffer(d_rec[:pipe.n_gaps * B.GAP_SPAN.itemsize].cpu().numpy().tobytes(), dtype=B.GAP_SPAN), int(move.sum())


def main():
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    round_arguments(ap, reps=True)
    ap.add_argument("--z", type=int, default=3)
    ap.add_argument("--shift", type=int, default=1000)
    ap.add_argument("--min-pairs", type=int, default=8)
    ap.add_argument("--shift-draft", type=int, action="append", default=[], help="bases the draft's N-run of every second gap is wrong by")
    args = ap.parse_args()
    s, flags, out = round_setup(args)
    on = dict(gap_span=True, span_z=args.z, span_shift=args.shift, span_min_pairs=args.min_pairs)
    out.update(steps=args.steps, **flags, **on)
    pipe, ms = off_and_on(s, flags, on, args.steps, args.reps)
    out.update(ms)
    res = pipe.fetch()
    gaps, gs = s.gaps, pipe.gap_span
    out["closed"], out["libraries"] = int((res.best != 0).sum()), [(lb.name, lb.is_mean, lb.is_sd, lb.n_recs) for lb in pipe.libs]
    out["gap_span_stats"] = res.gap_span_stats
    # the launch timers: the library's tagger pass and the span pass behind it, `steps` times each
    s.gf.timing(True)
    for lb in pipe.libs:
        for _ in range(args.steps):
            pipe.tagger(lb)
        pipe.barrier()
        (t_tag, n_tag), (t_span, n_span) = s.gf.kernel_time(B.KERNEL_TAG), s.gf.kernel_time(B.KERNEL_GAPSPAN)
        out["%s_launch_ms" % lb.name] = {"tagger": round(t_tag / max(1, n_tag), 4), "gap_span": round(t_span / max(1, n_span), 4)}
        s.gf.timing(True)           # (resets the totals)
    s.gf.timing(False)
    g0 = [int(g["end"]) - int(g["start"]) for g in gaps]
    for l, lb in enumerate(pipe.libs):
        out["%s_shift_0" % lb.name] = dict(_errors(res.gap_span[l], gaps, g0, lb, gs), n=_dist(res.gap_span[l]["n"]))
    chosen = np.arange(len(gaps)) % 2 == 0
    for n_shift in args.shift_draft:
        for l, lb in enumerate(pipe.libs):
            recs, moved = _shifted(pipe, lb, gaps, chosen, n_shift)
            out["%s_shift_%d" % (lb.name, n_shift)] = {
                "records_moved": moved,
                "moved_gaps": _errors(recs, gaps, [g0[g] - n_shift if chosen[g] else None for g in range(len(gaps))], lb, gs),
                "other_gaps": _errors(recs, gaps, [None if chosen[g] else g0[g] for g in range(len(gaps))], lb, gs),
                "other_gaps_records_equal_the_steps": bool(all(recs[g].tobytes() == res.gap_span[l, g].tobytes() for g in np.nonzero(~chosen)[0]))}
    emit(out, args.out)


if __name__ == "__main__":
    main()
