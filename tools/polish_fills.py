"""The polish round (Pipeline(polish=True)) on one bench preset: the step's time with the round off and on — two prepared pipelines
stepped in turn, `--reps` timed windows each, so the spread is known before a difference is read —, the round's own time (its launch
repeated on the step's results, and the library's launch timer), and — the presets know the truth (gf_synth_truth) — the fills that equal
the truth before and after the round, the four transitions (every correct -> wrong fill with its gap, its record and its pool size), and
the distributions of `n_changed` and `reads_ambiguous` per transition group.  One JSON object on stdout, and in --out when given.

--indels: three pipelines in turn — off, the plain round, the indel-aware round (polish_indels, polish_gapped.py) — and everything above
once per round ("plain", "indels"), from the same run.
--plant-indel N (with --indels; exact anchors): after the step, on the fetched results, one seeded indel of 1..N bases is planted in the body
of every closed fill that equals the truth — half of them lose bases, half gain random ones —, the contig list and the pick words' spans
are rewritten, both entries are called on the edited list with the step's pools, and the fills are counted: restored (the polished
contig is the step's again), unchanged (still the edited one) or broken (anything else).  The entries get no N masks, as the
step of a preset gets none (the synthetic reads have no N).

    python tools/polish_fills.py --config C5 --asm-tiebreak none [--out profiles/polish_c5_none.json]
    python tools/polish_fills.py --config C2RM --merge-in-step [--mp-reads N] [--anchor-mode exact|align|gapped]
    python tools/polish_fills.py --config C5 --indels --plant-indel 8 [--out profiles/polish_gapped_c5.json]
"""
import argparse

import numpy as np

from preset_setup import L, emit, in_turn, round_arguments, round_ms, round_setup


def _dist(v):
    v = np.asarray(v, dtype=np.int64)
    if not len(v):
        return {"n": 0}
    q = np.percentile(v, [50, 95])
    return {"n": int(len(v)), "zero": int((v == 0).sum()), "median": float(q[0]), "p95": float(q[1]), "max": int(v.max()), "mean": round(float(v.mean()), 3)}


def effect(s, pipe, res, kernel, steps):
    """The round's own time and what it did to the fills: the transition table with its distributions."""
    out = {"closed": int((res.best != 0).sum()), "polish_stats": res.polish_stats}
    pool_off = res.asm_off_t.cpu().numpy().astype(np.int64)
    ms, out["round_kernel_ms"] = round_ms(pipe, s.gf, pipe.polish.enqueue, kernel, steps)
    out["round_ms"] = round(ms[0], 4)
    before, after = pipe.picked_sequences(res), pipe.polished_sequences(res)
    groups = {"wrong_to_correct": [], "wrong_to_wrong": [], "correct_to_correct": [], "correct_to_wrong": []}
    for g in before:
        t = s.truth(g)
        groups[("correct" if before[g][1] in t else "wrong") + "_to_" + ("correct" if after[g][1] in t else "wrong")].append(g)
    out["correct_before"] = len(groups["correct_to_correct"]) + len(groups["correct_to_wrong"])
    out["correct_after"] = len(groups["correct_to_correct"]) + len(groups["wrong_to_correct"])
    pol = res.polish
    fields = ("n_cols", "n_changed", "n_uncovered", "reads_placed", "reads_ambiguous") + tuple(f for f in ("n_events", "n_inserted", "n_deleted", "reads_split")
                                                                                               if f in pol.dtype.names)
    for name, gs in groups.items():
        gs = np.array(gs, dtype=np.int64)
        out[name] = {"gaps": int(len(gs)), **{f: _dist(pol[f][gs]) for f in fields[1:]}}
    events = pol["n_events"] if "n_events" in pol.dtype.names else np.zeros(len(pol), dtype=np.uint32)
    out["wrong_to_wrong"]["unchanged"] = int(sum(int(pol["n_changed"][g]) == 0 and int(events[g]) == 0 for g in groups["wrong_to_wrong"]))
    out["correct_to_wrong_gaps"] = [{"gap": int(g), "pool_rows": int(pool_off[g + 1] - pool_off[g]), **{f: int(pol[g][f]) for f in fields}}
                                    for g in groups["correct_to_wrong"]]
    return out, groups


def planted_list(res, before, gaps, flanks, n_max, rng):
    """The contig list of --plant-indel: for every gap of `gaps` (closed, exact anchors; before: picked_sequences) whose body has room, the
    winning contig with one indel of 1..n_max bases planted in its body — bases taken out or random bases put in, by the toss of a coin.
    Returns (the records as a CONTIG array, their bases, the pick words with the spans rewritten — zero for every other gap —,
    {gap: (contig, edited contig)})."""
    from gappadder_amd import _lib as B
    from gappadder_amd import read_support as SUP
    from gappadder_amd.pipeline import contig_text, decode_best
    recs, texts, words, planted = [], [], np.zeros(len(res.best), dtype=np.uint64), {}
    for g in gaps:
        ci = before[g][0]
        contig = contig_text(res, ci)
        body = SUP.locate(res.best[g], contig, flanks[g], None)
        glen = int(rng.integers(1, n_max + 1))
        if body is None or body[1] - body[0] < glen + 4 or len(contig) + glen > B.PL_MAX_CONTIG:
            continue
        at = int(rng.integers(body[0] + 1, body[1] - glen - 1))
        edited = contig[:at] + contig[at + glen:] if rng.integers(0, 2) else contig[:at] + "".join("ACGT"[i] for i in rng.integers(0, 4, glen)) + contig[at:]
        a_len, span1, _, rev = decode_best(res.best[g])
        words[g] = (a_len << 56) | ((span1 + len(edited) - len(contig)) << 32) | ((0x7FFFFFFF - len(recs)) << 1) | rev
        rec = res.contigs[ci].copy()
        rec["length"], rec["seq_off"] = len(edited), sum(len(t) for t in texts)
        recs.append(rec)
        texts.append(edited)
        planted[g] = (contig, edited)
    return np.array(recs, dtype=B.CONTIG), "".join(texts).encode(), words, planted


def run_entry(pipe, entry, record, own, n_words, recs, seq, words):
    """One polish entry (gf_fill_polish_dev / gf_fill_polish_gapped_dev; own: its parameters) on a contig list of the caller's, with the
    pools of the stepped pipeline `pipe` (exact anchors).  The N-mask argument is null, as in the step of a pipeline whose libraries
    carry no mask — the synthetic presets'; on reads with N the counts would be taken with N read as A.
    Returns (the records, the base buffer's bytes, the statistics words)."""
    import torch
    from gappadder_amd import _lib as B
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_ctg, d_seq = dev(recs.view(np.uint8)), dev(np.frombuffer(seq, dtype=np.uint8))
    d_n, d_best = torch.tensor([len(recs)], dtype=torch.int32, device="cuda"), dev(words.view(np.int64))
    cap = len(seq) + B.PLG_MAX_INSERTED * len(recs)
    d_rec = torch.zeros(len(words) * record.itemsize, dtype=torch.uint8, device="cuda")
    d_bases, d_st = torch.zeros(cap, dtype=torch.uint8, device="cuda"), torch.zeros(n_words, dtype=torch.int32, device="cuda")
    pipe._chk(entry(pipe.h, pipe.asm_ptr, None, pipe.asm_off, pipe.asm_rows, L, d_ctg.data_ptr(), d_n.data_ptr(), len(recs), d_seq.data_ptr(),
                    d_best.data_ptr(), None, *pipe.anchor_pair, *own, d_rec.data_ptr(), d_bases.data_ptr(), cap, d_st.data_ptr()), "polish entry")
    pipe.barrier()
    return np.frombuffer(d_rec.cpu().numpy().tobytes(), dtype=record), d_bases.cpu().numpy().tobytes(), d_st.cpu().numpy()


def plant_indels(s, pipe, res, groups, n_max, prm, max_indel, seed=1):
    """--plant-indel: see the module docstring.  pipe: a stepped pipeline in exact anchor mode (its pools are the entries' pools)."""
    from gappadder_amd import _lib as B
    recs, seq, words, planted = planted_list(res, pipe.picked_sequences(res), sorted(groups["correct_to_correct"] + groups["correct_to_wrong"]),
                                             s.gf.flanks, n_max, np.random.default_rng(seed))
    out = {"planted": len(planted), "max": n_max, "seed": seed}
    if not planted:
        return out
    for name, entry, record, own, n_words in (("plain", pipe.lib.gf_fill_polish_dev, B.FILL_POLISH, prm, B.PL_WORDS),
                                              ("indels", pipe.lib.gf_fill_polish_gapped_dev, B.FILL_POLISH_GAPPED, prm + (max_indel,), B.PLG_WORDS)):
        rec, bases, st = run_entry(pipe, entry, record, own, n_words, recs, seq, words)
        count = {"restored": 0, "unchanged": 0, "broken": 0, "mismatches": int(st[B.PL_MISMATCH])}
        for g, (contig, edited) in planted.items():
            text = bases[int(rec[g]["off"]):int(rec[g]["off"]) + int(rec[g]["len"])].decode()
            count["restored" if text == contig else "unchanged" if text == edited else "broken"] += 1
        out[name] = count
    return out


def main():
    from gappadder_amd import _lib as B
    ap = argparse.ArgumentParser()
    round_arguments(ap, reps=True, placing=True)
    ap.add_argument("--min-votes", type=int, default=2)
    ap.add_argument("--indels", action="store_true", help="off / plain / indel-aware in turn")
    ap.add_argument("--max-indel", type=int, default=8)
    ap.add_argument("--plant-indel", type=int, default=0, metavar="N", help="with --indels: plant an indel of 1..N bases in every correct fill")
    args = ap.parse_args()
    if args.plant_indel and not (args.indels and args.anchor_mode == "exact"):
        raise SystemExit("--plant-indel needs --indels and exact anchors")
    s, flags, out = round_setup(args)
    prm = dict(polish_seed=args.seed, polish_max_mismatch=args.max_mismatch, polish_min_overlap=args.min_overlap, polish_min_votes=args.min_votes)
    out.update(steps=args.steps, **flags, **prm)
    settings = {"off": {}, "on": dict(polish=True, **prm)}
    if args.indels:
        out["polish_max_indel"] = args.max_indel
        settings = {"off": {}, "plain": settings["on"], "indels": dict(polish=True, polish_indels=True, polish_max_indel=args.max_indel, **prm)}
    pipes, ms = in_turn(s, flags, settings, args.steps, args.reps)
    out.update(ms)
    if not args.indels:
        out.update(effect(s, pipes["on"], pipes["on"].fetch(), B.KERNEL_POLISH, args.steps)[0])
    else:
        res = pipes["plain"].fetch()
        out["plain"], groups = effect(s, pipes["plain"], res, B.KERNEL_POLISH, args.steps)
        out["indels"] = effect(s, pipes["indels"], pipes["indels"].fetch(), B.KERNEL_POLISH_GAPPED, args.steps)[0]
        if args.plant_indel:
            out["plant_indel"] = plant_indels(s, pipes["plain"], res, groups, args.plant_indel, tuple(prm.values()), args.max_indel)
    emit(out, args.out)


if __name__ == "__main__":
    main()
