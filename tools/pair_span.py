"""The pair-span round (Pipeline(pair_span=True)) on one bench preset: the step's time with the round off and on — two prepared pipelines
stepped in turn, `--reps` timed windows each, so the spread is known before a difference is read —, the round's own time (its launches
repeated on the step's results, and the library's launch timer), and — the presets know the truth (gf_synth_truth) — the records split
by correct / wrong fill, per library: fills with n_unspanned > 0, with n_short + n_long > 0, with n_misoriented > 0, and the
distribution of span_insert_sum / n_span - is_mean.

--delete N: the round's sensitivity to a fill of the wrong length.  gf_fill_pairs_dev is called off-step on a copy of the step's
results in which every tenth closed gap's winning contig has N bases cut from the middle of its body (the word's span and any pick
entry adjusted to match), for the library with the largest insert size; reported: of those fills, how many the library's
span_insert_sum / n_span places more than 3 * is_sd / sqrt(n_span) below is_mean, and how many untouched fills cross the same line.
One JSON object on stdout, and in --out when given.

--anchored [--min-pairs N]: the anchored pair span (Pipeline(pair_anchors=True)) instead: the step with the pair-span
round alone ("off") and with the anchored pairs behind it ("on"), the pair-span round with the anchored calls repeated on the step's
results and the anchored entry's own launch timer, per library the anchored / placed / in-range pairs and the distribution of n_eval, and
with --delete N the anchored records of the edited and the untouched fills: how many have dev_min_sum / (is_sd * sqrt(dev_min_n)) below
-3, and the median dev_min_mean.

    python tools/pair_span.py --config C5 --asm-tiebreak none --mp-reads N [--delete 50] [--out profiles/pair_span_c5_none.json]
    python tools/pair_span.py --config C2RM --merge-in-step --mp-reads N [--anchor-mode exact|align|gapped]
"""
import argparse

import numpy as np

from preset_setup import emit, off_and_on, round_arguments, round_ms, round_setup, spread


def _dist(v):
    v = np.asarray(v, dtype=np.int64)
    if not len(v):
        return {"n": 0}
    q = np.percentile(v, [5, 50, 95])
    return {"n": int(len(v)), "p5": float(q[0]), "median": float(q[1]), "p95": float(q[2]), "min": int(v.min()), "max": int(v.max()),
            "mean": round(float(v.mean()), 3)}


def _low(rec, is_mean, is_sd):
    """Does the record's mean spanning insert lie more than 3 * is_sd / sqrt(n_span) below is_mean?"""
    n = int(rec["n_span"])
    return bool(n) and int(rec["span_insert_sum"]) / n < is_mean - 3.0 * is_sd / np.sqrt(n)


def _delete(pipe, res, flanks, n_cut, l, anchored=False):
    """The off-step call on the edited copy: (records of library l, edited gaps, gaps that could not take the cut).  anchored: the
    anchored entry behind it, and ITS records."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import pipeline as P
    from gappadder_amd import read_support as SUP
    ctg, best = res.contigs.copy(), res.best.copy()
    pick = res.ctg_pick.copy() if res.ctg_pick is not None else None
    seq, edited, left = bytearray(res.seq), [], []
    for g in np.nonzero(res.best)[0][::10].tolist():
        a_len, span1, ci, rev = P.decode_best(res.best[g])
        text = P.contig_text(res, ci)
        body = SUP.locate(res.best[g], text, flanks[g], pick[ci] if pick is not None else None)
        if body is None or body[1] - body[0] < n_cut + 2 or span1 >= 0xFFFFFF:
            left.append(g)
            continue
        at = (body[0] + body[1] - n_cut) // 2
        ctg[ci]["seq_off"], ctg[ci]["length"] = len(seq), len(text) - n_cut
        seq += (text[:at] + text[at + n_cut:]).encode()
        best[g] = np.uint64(int(res.best[g]) - (n_cut << 32))
        if pick is not None:                 # the alignment right of the body moves left with the bases behind the cut
            pick[ci]["lp" if rev else "rp"] -= n_cut
        edited.append(g)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(pipe.dev)
    d_ctg, d_seq, d_best = dev(ctg.view(np.uint8)), dev(np.frombuffer(bytes(seq), dtype=np.uint8)), dev(best.view(np.int64))
    d_pick = dev(pick.view(np.uint8)) if pick is not None else None
    d_n = torch.tensor([len(ctg)], dtype=torch.int32, device=pipe.dev)
    d_rec = torch.zeros(max(1, pipe.n_gaps) * B.FILL_PAIRS.itemsize, dtype=torch.uint8, device=pipe.dev)
    d_st = torch.zeros(B.PS_WORDS, dtype=torch.int32, device=pipe.dev)
    lb, ps = pipe.libs[l], pipe.pairs
    torch.cuda.synchronize()
    pipe._chk(pipe.lib.gf_fill_pairs_dev(pipe.h, pipe.pool_ptr[l], ps.masks_of(l), lb.d_pool_off.data_ptr(), lb.d_ids.data_ptr(), pipe.lib_cap, pipe.L,
                                         d_ctg.data_ptr(), d_n.data_ptr(), len(ctg), d_seq.data_ptr(), d_best.data_ptr(),
                                         d_pick.data_ptr() if d_pick is not None else None, *ps.shared_args()[6:], *ps.params[:3], lb.is_mean, lb.is_sd,
                                         ps.params[3], ps.d_scratch.data_ptr(), d_rec.data_ptr(), d_st.data_ptr()), "gf_fill_pairs_dev")
    dtype = B.FILL_PAIRS
    if anchored:
        pa, dtype = pipe.anchored, B.FILL_ANCHORS
        d_rec = torch.zeros(max(1, pipe.n_gaps) * dtype.itemsize, dtype=torch.uint8, device=pipe.dev)
        d_sa = torch.zeros(B.PA_WORDS, dtype=torch.int32, device=pipe.dev)
        pipe._chk(pipe.lib.gf_fill_pairs_anchored_dev(pipe.h, lb.d_pool_off.data_ptr(), lb.d_ids.data_ptr(), pipe.lib_cap, pipe.L, d_ctg.data_ptr(),
                                                      d_n.data_ptr(), len(ctg), d_seq.data_ptr(), d_best.data_ptr(),
                                                      d_pick.data_ptr() if d_pick is not None else None, *ps.shared_args()[6:], ps.d_scratch.data_ptr(),
                                                      lb.d_recs.data_ptr(), lb.n_recs, lb.d_thits.data_ptr(), lb.cp + 4 * P.CNT_TAG, lb.hit_cap,
                                                      lb.is_mean, lb.is_sd, ps.params[3], pa.min_pairs, pa.d_anchor.data_ptr(), d_rec.data_ptr(),
                                                      d_sa.data_ptr()), "gf_fill_pairs_anchored_dev")
    pipe.barrier()
    recs = np.frombuffer(d_rec[:pipe.n_gaps * dtype.itemsize].cpu().numpy().tobytes(), dtype=dtype)
    if int(d_st.cpu().numpy().view(np.uint32)[B.PS_MISMATCH]):
        raise RuntimeError("--delete: the edited copy does not carry its picks")
    return recs, edited, left


def _flagged(rec, is_sd):
    """Does the record's lowest column mean lie more than 3 standard errors below is_mean?"""
    from gappadder_amd.pair_anchors import z_score
    z = z_score(rec["dev_min_sum"], rec["dev_min_n"], is_sd) if int(rec["n_eval"]) else None
    return z is not None and z < -3.0


def _anchored(args, s, flags, out, prm):
    from gappadder_amd import _lib as B
    from gappadder_amd.pair_anchors import dev_means
    on = dict(pair_anchors=True, pair_min_pairs=args.min_pairs)
    out.update(anchored=True, **on)
    pipe, ms = off_and_on(s, dict(flags, pair_span=True, **prm), on, args.steps, args.reps)      # off: the pair-span round alone
    out.update(ms)
    res = pipe.fetch()
    libs = [(lb.name, lb.is_mean, lb.is_sd) for lb in pipe.libs]
    out["closed"], out["libraries"], out["pair_anchor_stats"] = int((res.best != 0).sum()), libs, res.pair_anchor_stats
    ms, out["anchored_ms_per_launch"] = round_ms(pipe, s.gf, pipe.pairs.enqueue, B.KERNEL_ANCHORS, args.steps, args.reps)
    out["pair_span_with_anchored_round_ms"] = spread(ms)
    closed = np.nonzero(res.best)[0]
    for l, (name, _, is_sd) in enumerate(libs):
        r = res.pair_anchors[l][closed]
        out["%s_records" % name] = {"n_eval": _dist(r["n_eval"]), "n_in_range": _dist(r["n_in_range"]), "with_eval": int((r["n_eval"] > 0).sum()),
                                    "flagged": int(sum(_flagged(x, is_sd) for x in r))}
    if args.delete:
        l = int(np.argmax([m for _, m, _ in libs]))
        out["delete_library"], is_sd = libs[l][0], libs[l][2]
        for n_cut in args.delete:
            recs, edited, left = _delete(pipe, res, pipe.gf.flanks, n_cut, l, anchored=True)
            ed = set(edited)
            rest = [g for g in closed.tolist() if g not in ed]
            means = [dev_means(recs[g])[0] for g in edited if int(recs[g]["n_eval"])]
            out["delete_%d" % n_cut] = {
                "edited": len(edited), "not_edited_body_too_short": len(left), "edited_with_eval": len(means),
                "edited_flagged": int(sum(_flagged(recs[g], is_sd) for g in edited)), "untouched": len(rest),
                "untouched_with_eval": int(sum(int(recs[g]["n_eval"]) > 0 for g in rest)),
                "untouched_flagged": int(sum(_flagged(recs[g], is_sd) for g in rest)),
                "untouched_records_equal_the_steps": bool(all(recs[g].tobytes() == res.pair_anchors[l, g].tobytes() for g in rest)),
                "edited_dev_min_mean": _dist(means)}
    emit(out, args.out)


def main():
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    round_arguments(ap, reps=True, placing=True)
    ap.add_argument("--z", type=int, default=3)
    ap.add_argument("--delete", type=int, action="append", default=[], help="bases cut from every tenth closed fill (may be given more than once)")
    ap.add_argument("--anchored", action="store_true", help="the anchored pair span behind the pair-span round (DESIGN.md §20)")
    ap.add_argument("--min-pairs", type=int, default=8)
    args = ap.parse_args()
    s, flags, out = round_setup(args)
    prm = dict(pair_seed=args.seed, pair_max_mismatch=args.max_mismatch, pair_min_overlap=args.min_overlap, pair_z=args.z)
    out.update(steps=args.steps, **flags, **prm)
    if args.anchored:
        return _anchored(args, s, flags, out, prm)
    pipe, ms = off_and_on(s, flags, dict(pair_span=True, **prm), args.steps, args.reps)
    out.update(ms)
    res = pipe.fetch()
    libs = [(lb.name, lb.is_mean, lb.is_sd) for lb in pipe.libs]
    out["closed"], out["libraries"], out["pair_stats"] = int((res.best != 0).sum()), libs, res.pair_stats
    ms, out["round_kernel_ms_per_launch"] = round_ms(pipe, s.gf, pipe.pairs.enqueue, B.KERNEL_PAIRS, args.steps, args.reps)
    out["round_ms"] = spread(ms)
    picked = pipe.picked_sequences(res)
    groups = {"correct": [], "wrong": []}
    for g in picked:
        groups["correct" if picked[g][1] in s.truth(g) else "wrong"].append(g)
    out["correct"], out["wrong"] = len(groups["correct"]), len(groups["wrong"])
    for l, (name, is_mean, is_sd) in enumerate(libs):
        for kind, gs in groups.items():
            r = res.pairs[l][np.array(gs, dtype=np.int64)]
            sp = r[r["n_span"] > 0]
            out["%s_%s" % (name, kind)] = {
                "gaps": int(len(r)), "unspanned": int((r["n_unspanned"] > 0).sum()), "short_or_long": int((r["n_short"] + r["n_long"] > 0).sum()),
                "misoriented": int((r["n_misoriented"] > 0).sum()), "with_spanning_pairs": int(len(sp)), "n_span": _dist(sp["n_span"]),
                "span_mean_minus_is": _dist(sp["span_insert_sum"] // np.maximum(1, sp["n_span"].astype(np.int64)) - is_mean),
                "low": int(sum(_low(x, is_mean, is_sd) for x in sp))}
        if groups["wrong"]:
            out["%s_wrong_records" % name] = [{"gap": int(g), **{f: int(res.pairs[l, g][f]) for f in B.FILL_PAIRS.names}} for g in groups["wrong"][:16]]
    if args.delete:
        l = int(np.argmax([m for _, m, _ in libs]))
        _, is_mean, is_sd = libs[l]
        out["delete_library"] = libs[l][0]
        for n_cut in args.delete:
            recs, edited, left = _delete(pipe, res, pipe.gf.flanks, n_cut, l)
            ed = set(edited)
            rest = [g for g in np.nonzero(res.best)[0].tolist() if g not in ed]
            same = all(recs[g].tobytes() == res.pairs[l, g].tobytes() for g in rest)
            out["delete_%d" % n_cut] = {
                "edited": len(edited), "not_edited_body_too_short": len(left), "edited_with_spanning_pairs": int(sum(int(recs[g]["n_span"]) > 0 for g in edited)),
                "edited_low": int(sum(_low(recs[g], is_mean, is_sd) for g in edited)), "untouched": len(rest),
                "untouched_with_spanning_pairs": int(sum(int(recs[g]["n_span"]) > 0 for g in rest)),
                "untouched_low": int(sum(_low(recs[g], is_mean, is_sd) for g in rest)), "untouched_records_equal_the_steps": bool(same),
                "edited_span_mean_minus_is": _dist([int(recs[g]["span_insert_sum"]) // int(recs[g]["n_span"]) - is_mean for g in edited if int(recs[g]["n_span"])])}
    emit(out, args.out)


if __name__ == "__main__":
    main()
