"""The picker's "gapped" mode on the device (gf_pick_gapped_dev, the gapped instantiation of csrc/pick_align.hip) against its host
twin (gappadder_amd/pick_contigs.py::gapped_hits + select_per_contig), through Pipeline(anchor_mode="gapped") on a synthetic step whose
draft flanks carry a planted indel next to the gap, and in the extended fill."""
import numpy as np
import pytest

import pick_util as PK

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _edit(s, i, rng, kinds=(0, 1, 2)):
    """One edit at s[i]: a substitution, or an insertion / a deletion of 1-3 bases.  Returns (edited, is an indel)."""
    kind = int(rng.choice(kinds))
    if kind == 0:
        return s[:i] + str(rng.choice([b for b in "ACGT" if b != s[i]])) + s[i + 1:], False
    n = int(rng.integers(1, 4))
    if kind == 1:
        return s[:i] + PK.rand_seq(rng, n) + s[i:], True
    return s[:i] + s[i + n:], True


def _cases(seed):
    """picker_cases plus 160 gaps with flanks of 12 ... 1 024 bases whose contigs carry the flanks with 0-3 edits (substitutions and 1-3
    base indels) 1 ... 40 bases from either flank's gap-side end, a few indels of 32 and more bases, both strands, N in flanks and
    contigs, contigs that end inside a flank, and a repeat beyond the cap.  Returns (cases, the (gap, contig number) with an indel)."""
    rng = np.random.default_rng(seed)
    out = PK.picker_cases(seed, 160)
    indel = set()
    for g in range(160):
        nl = 1024 if g % 40 == 3 else [120, 12, 300, 80, 60][g % 5]
        nr = 700 if g % 40 == 9 else [150, 200, 16, 90, 64][(g // 5) % 5]
        l, r, mid = PK.rand_seq(rng, nl), PK.rand_seq(rng, nr), PK.rand_seq(rng, int(rng.integers(0, 250)))
        if g % 11 == 3:
            l = l[:40] + "N" + l[41:]
        if g % 13 == 4:
            r = r[:-30] + "NN" + r[-28:]
        contigs = []
        for _ in range(int(rng.integers(1, 4))):
            lm, rm = l, r
            planted = False
            for _ in range(int(rng.integers(0, 4))):
                dist = int(rng.integers(1, 41))
                if rng.integers(0, 2) and len(lm) > dist + 3:
                    lm, ind = _edit(lm, len(lm) - dist, rng)
                elif len(rm) > dist + 3:
                    rm, ind = _edit(rm, dist - 1, rng)
                else:
                    ind = False
                planted |= ind
            if g % 16 == 6 and len(lm) > 100:             # outside the band: 32 and more bases
                n = int(rng.integers(32, 41))
                lm = lm[:-60] + (PK.rand_seq(rng, n) if rng.integers(0, 2) else "") + lm[-60 + (0 if rng.integers(0, 2) else n):]
            a, b = int(rng.integers(0, len(lm) + 1)), int(rng.integers(0, len(rm) + 1))
            s = PK.rand_seq(rng, int(rng.integers(0, 30))) + lm[a // 3 if g % 2 else 0:] + mid + rm[:len(rm) - b // 3 if g % 3 else len(rm)] + PK.rand_seq(rng, 20)
            if g % 7 == 2:
                s = s[:25] + "N" + s[26:]
            if planted:
                indel.add((g + 160, len(contigs)))
            contigs.append(PK._rc(s) if rng.integers(0, 2) else s)
        if g % 9 == 5 and len(l) >= 60:                   # a repeat of the left flank's end beyond the cap of 64 alignments
            unit = l[-40:]
            contigs.append("".join(unit + PK.rand_seq(rng, 7) for _ in range(80)) + mid + r)
        out.append((l, r, contigs))
    return out, indel


def _host_expect(cases, contigs, first, scores):
    """Host twin of the device words: per gap the best word, per contig (index >= first) its selection, and the dropped count."""
    from gappadder_amd.pick_contigs import gapped_hits, select_per_contig
    n_gaps = len(cases)
    best = np.zeros(n_gaps, dtype=np.uint64)
    picks = {}
    dropped = 0
    for g, (l, r, _) in enumerate(cases):
        idx = [i for i, (gg, _) in enumerate(contigs) if gg == g and i >= first]
        mine = [("c%d" % i, contigs[i][1]) for i in idx]
        st = {}
        for t in scores:
            per = select_per_contig(gapped_hits(mine, l, r, t, stats=st if t == scores[0] else None))
            for j, (span, lp, rp, lm, rm, rc) in per.items():
                ci = idx[j]
                if span < 0 or ci in picks:
                    continue
                picks[ci] = (lp, rp, lm, rm, int(rc), t)
                w = (t << 56) | (min(span + 1, 0xFFFFFF) << 32) | ((0x7FFFFFFF - ci) << 1) | int(rc)
                best[g] = max(int(best[g]), w)
        dropped += st.get("dropped", 0)
    return best, picks, dropped


def _gapped_share(cases, indel):
    """Of the contigs with a planted indel, how many yield a selected hit (score 15) whose contig span differs from its query span."""
    from gappadder_amd.pick_contigs import ALIGN_CAP, _gapped_alignments, _queries, select_per_contig, gapped_hits
    n = 0
    for g, j in sorted(indel):
        l, r, seqs = cases[g]
        per = select_per_contig(gapped_hits([("c", seqs[j])], l, r, 15))
        if 0 not in per:
            continue
        _, lp, rp, lm, rm, _ = per[0]
        qs, index = _queries(l, r)
        al = _gapped_alignments(seqs[j], qs, index, ALIGN_CAP, {})
        spans = {(cb + 1, ce - cb): qe - qb for q in al for qb, qe, cb, ce, _ in q}
        n += spans[lp, lm] != lm or spans[rp, rm] != rm
    return n


SEED = 23


def test_device_gapped_pick_equals_the_host_twin():
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    cases, indel = _cases(SEED)
    n_gaps = len(cases)
    gaps = np.zeros(n_gaps, dtype=B.GAP)
    for g in range(n_gaps):
        gaps[g] = (0, 2000 * (g + 1), 2000 * (g + 1) + 100, g + 1)
    rng = np.random.default_rng(22)
    contigs = [(g, s) for g, (_, _, seqs) in enumerate(cases) for s in seqs]
    contigs = [contigs[i] for i in rng.permutation(len(contigs))]
    ctg = np.zeros(len(contigs), dtype=B.CONTIG)
    o = 0
    for i, (g, s) in enumerate(contigs):
        ctg[i] = (g, 31, 29, max(1, len(s) - 28), len(s), 0, 0, o)
        o += len(s)
    n = len(contigs)
    first = n // 3
    want_all = _host_expect(cases, contigs, 0, (30, 15))
    want_from = _host_expect(cases, contigs, first, (30, 15))
    # what keeps the test honest, from the twin alone
    assert want_all[2] > 0, "no case reaches the cap"
    n_closed_want = int((want_all[0] != 0).sum())
    assert n_gaps / 4 < n_closed_want < 3 * n_gaps / 4, n_closed_want
    assert len(indel) >= 60 and 3 * _gapped_share(cases, indel) >= len(indel), (_gapped_share(cases, indel), len(indel))
    gf = GapFill(0)
    gf.set_gaps(gaps, 1, [(l, r) for l, r, _ in cases])
    lib = B.lib()
    d_ctg, d_seq = _dev(ctg.view(np.uint8)), _dev(np.frombuffer("".join(s for _, s in contigs).encode(), dtype=np.uint8))
    d_n = torch.tensor([n, first], dtype=torch.int32, device="cuda")
    for how in ("one launch", (30, 15), (15, 30), "from"):
        d_best = torch.zeros(n_gaps, dtype=torch.int64, device="cuda")
        d_closed = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_pick = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(2, dtype=torch.int32, device="cuda")
        args = (d_best.data_ptr(), d_closed.data_ptr(), d_pick.data_ptr(), d_st.data_ptr())
        if how == "one launch":
            assert lib.gf_pick_gapped_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), 30, 15, *args) == 0
        elif how == "from":
            assert lib.gf_pick_gapped_from_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), 30, 15, d_n.data_ptr() + 4, *args) == 0
        else:
            for t in how:
                assert lib.gf_pick_gapped_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), t, 0, *args) == 0
        gf.sync()
        best_w, picks_w, dropped_w = want_from if how == "from" else want_all
        best = d_best.cpu().numpy().view(np.uint64)
        bad = [g for g in range(n_gaps) if int(best[g]) != int(best_w[g])]
        assert not bad, (how, [(g, hex(int(best[g])), hex(int(best_w[g]))) for g in bad[:5]])
        pk = np.frombuffer(d_pick.cpu().numpy().tobytes(), dtype=B.CTG_PICK)
        got = {i: (int(p["lp"]), int(p["rp"]), int(p["lm"]), int(p["rm"]), int(p["reverse"]), int(p["threshold"])) for i, p in enumerate(pk)
               if p["threshold"]}
        assert got == picks_w, (how, sorted(set(got.items()) ^ set(picks_w.items()))[:6])
        assert int(d_closed[0]) == int((best_w != 0).sum())
        st = d_st.cpu().numpy()
        assert int(st[1]) == 0
        assert int(st[0]) == dropped_w * (1 if isinstance(how, str) else 2), how      # (every launch counts its own)


def test_device_gapped_pick_rejects_flanks_beyond_1024_bases():
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    gaps = np.zeros(1, dtype=B.GAP)
    gaps[0] = (0, 2000, 2100, 1)
    gf = GapFill(0)
    gf.set_gaps(gaps, 1, [("A" * 1025, "C" * 300)])
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    ctg = np.zeros(1, dtype=B.CONTIG)
    ctg[0] = (0, 31, 29, 1, 40, 0, 0, 0)
    d_ctg, d_seq = _dev(ctg.view(np.uint8)), _dev(np.frombuffer(b"A" * 40, dtype=np.uint8))
    p = z.data_ptr()
    assert B.lib().gf_pick_gapped_dev(gf.handle, d_ctg.data_ptr(), p, 1, d_seq.data_ptr(), 30, 15, p + 8, p + 16, p + 32, p + 64) == B.GF_E_UNSUPPORTED


def _plant_indels(flanks):
    """Every other gap gets a 1-2 base draft indel 8-14 bases from a flank's gap-side end (that many true bases stay between the edit
    and the gap), alternating sides and insertion / deletion.  Returns (flanks, the planted gaps)."""
    rng = np.random.default_rng(5)
    out, planted = [], set()
    for g, (l, r) in enumerate(flanks):
        if g % 2 == 0:
            planted.add(g)
            n, dist = int(rng.integers(1, 3)), int(rng.integers(8, 15))
            new = PK.rand_seq(rng, n) if (g // 4) % 2 == 0 else None        # None: a deletion
            if g % 4 == 0:
                i = len(l) - dist
                l = l[:i] + new + l[i:] if new else l[:i - n] + l[i:]
            else:
                r = r[:dist] + new + r[dist:] if new else r[:dist] + r[dist + n:]
        out.append((l, r))
    return out, planted


def _step(flanks_fn, anchor_mode=None):
    import torch
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    seed, slen, nscf, gps, glen, L, n_pairs = 20260011, 200_000, 3, 4, 120, 150, 60_000
    gf = GapFill(0)
    cfg = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L)
    gaps, flanks = GapFill.synth_layout(cfg)
    flanks = flanks_fn(flanks)
    gf.set_gaps(gaps, nscf, flanks)
    kw = {} if anchor_mode is None else {"anchor_mode": anchor_mode}
    pipe = Pipeline(gf, len(gaps), L, [(31, 29)], **kw)
    d_reads = torch.empty(2 * n_pairs * 38 + 64, dtype=torch.uint8, device="cuda")
    d_recs = torch.empty(2 * n_pairs * 32, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg, 0, n_pairs, d_reads.data_ptr(), d_recs.data_ptr())
    gf.sync()
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * n_pairs, d_reads, d_recs))
    pipe.prepare()
    pipe.step()
    res = pipe.fetch()
    return pipe, res, gaps, cfg


def test_gapped_mode_closes_gaps_whose_flanks_carry_an_indel_next_to_the_gap():
    """Half of the gaps get a 1-2 base draft indel 8-14 bases from a flank's gap-side end: exact mode closes none of those the clean
    run closes, gapped mode closes every one of them with the clean run's sequence, the true one for all but at most one (a gap whose
    boundary base is ambiguous); on clean flanks gapped closes what exact closes with the identical sequence."""
    from gappadder_amd.hip_api import GapFill
    planted = set()

    def plant(flanks):
        out, p = _plant_indels(flanks)
        planted.update(p)
        return out

    p_ex, r_ex, gaps, cfg = _step(lambda f: f)
    p_gp, r_gp, _, _ = _step(lambda f: f, "gapped")
    seq_ex, seq_gp = p_ex.picked_sequences(r_ex), p_gp.picked_sequences(r_gp)
    assert len(seq_ex) >= 6
    for g, (ci, body, rev) in seq_ex.items():
        assert g in seq_gp and seq_gp[g][1] == body, g
    pm_ex, rm_ex, _, _ = _step(plant, "exact")
    pm_gp, rm_gp, _, _ = _step(plant, "gapped")
    closed_clean = set(seq_ex)
    assert len(planted & closed_clean) >= 3
    assert not (set(np.nonzero(rm_ex.best)[0].tolist()) & planted & closed_clean)
    got = pm_gp.picked_sequences(rm_gp)
    n_true = 0
    for g in planted & closed_clean:
        assert g in got, g
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        truth = (GapFill.synth_truth(cfg, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg, sc, st - 6, en - st + 11))
        assert got[g][1] == seq_ex[g][1], g
        n_true += got[g][1] in truth
    assert n_true >= len(planted & closed_clean) - 1
    assert rm_gp.align_dropped == 0 and rm_gp.align_seed_overflow == 0
    assert r_gp.align_dropped == 0 and r_gp.align_seed_overflow == 0


def test_pipeline_refuses_an_unknown_anchor_mode():
    from gappadder_amd.pipeline import Pipeline
    with pytest.raises(ValueError, match="anchor_mode"):
        Pipeline(None, 1, 150, [(31, 29)], anchor_mode="banded")


def test_extended_fill_in_gapped_mode_equals_the_twin_on_planted_flanks():
    """On a layout whose gaps stay open (900 bases, k 31), with an indel planted in every other gap's flank.  The synthetic contigs
    cover a whole 300-base flank — an unclipped hit, which the extended pick does not use — so every flank also gets 40 foreign
    bases at its far end: the hits are clipped there, as the extended pick wants them."""
    from step_util import NSCF, contigs as _contigs, run as _run, setup as _setup
    from test_gpu_extended_fill import twin_expect
    env = _setup(900, [(31, 29)])
    gf, cfg, gaps, flanks = env[:4]
    flanks, planted = _plant_indels(flanks)
    rng = np.random.default_rng(8)
    flanks = [(PK.rand_seq(rng, 40) + l, r + PK.rand_seq(rng, 40)) for l, r in flanks]
    gf.set_gaps(gaps, NSCF, flanks)
    env = (gf, cfg, gaps, flanks) + env[4:]
    pipe, (res,) = _run(env, extended_fill=True, anchor_mode="gapped")
    open_gaps = [g for g in range(len(flanks)) if not res.best[g]]
    assert len(open_gaps) >= len(flanks) - 2 and set(open_gaps) & planted
    want = twin_expect(flanks, _contigs(res), pipe.kk, "gapped", open_gaps)
    got = pipe.extended_sequences(res)
    assert got == want, sorted(g for g in set(got) | set(want) if got.get(g) != want.get(g))[:5]
    fills = {g for g, v in got.items() if v[2] is not None}
    print("extended fill, gapped: %d open gaps, %d fills, %d of them on planted flanks" % (len(open_gaps), len(fills), len(fills & planted)))
    assert len(fills) == res.extended["gaps_extended"] >= len(open_gaps) // 2 and len(fills & planted) >= len(planted) // 2
    assert res.extended["align_dropped"] == 0 and res.extended["align_seed_overflow"] == 0
