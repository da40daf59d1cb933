"""The picker's "align" mode on the device (gf_pick_aligned_dev, csrc/pick_align.hip) against its host twin
(gappadder_amd/pick_contigs.py::align_hits + select_full), and through Pipeline(anchor_mode="align") on a synthetic step whose draft
flanks carry a planted mismatch next to the gap."""
import numpy as np
import pytest

import pick_util as PK

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _mutate(s, i, rng):
    return s[:i] + rng.choice([b for b in "ACGT" if b != s[i]]) + s[i + 1:]


def _cases(seed):
    """picker_cases plus whole-flank contigs with 0-3 mismatches near either flank end (both strands), repeats beyond the cap,
    flanks shorter than a seed and longer than 300, non-ACGT in flanks and contigs."""
    rng = np.random.default_rng(seed)
    out = PK.picker_cases(seed, 160)
    for g in range(160):
        nl = [300, 12, 700, 1024, 150][g % 5]
        nr = [300, 300, 16, 900, 1000][(g // 5) % 5]
        l, r, mid = PK.rand_seq(rng, nl), PK.rand_seq(rng, nr), PK.rand_seq(rng, int(rng.integers(0, 250)))
        if g % 11 == 3:
            l = l[:40] + "N" + l[41:]
        if g % 13 == 4:
            r = r[:-30] + "NN" + r[-28:]
        contigs = []
        for _ in range(int(rng.integers(1, 4))):
            lm, rm = l, r
            for _ in range(int(rng.integers(0, 4))):      # mismatches within the 12 gap-side bases of either flank
                if rng.integers(0, 2) and len(lm) > 12:
                    lm = _mutate(lm, len(lm) - 1 - int(rng.integers(0, 12)), rng)
                elif len(rm) > 12:
                    rm = _mutate(rm, int(rng.integers(0, 12)), rng)
            a, b = int(rng.integers(0, len(lm) + 1)), int(rng.integers(0, len(rm) + 1))
            s = PK.rand_seq(rng, int(rng.integers(0, 30))) + lm[a // 3 if g % 2 else 0:] + mid + rm[:len(rm) - b // 3 if g % 3 else len(rm)] + PK.rand_seq(rng, 20)
            if g % 7 == 2:
                s = s[:25] + "N" + s[26:]
            contigs.append(PK._rc(s) if rng.integers(0, 2) else s)
        if g % 9 == 5 and len(l) >= 60:                   # a repeat of the left flank's end beyond the cap of 64 alignments
            unit = l[-40:]
            contigs.append("".join(unit + PK.rand_seq(rng, 7) for _ in range(80)) + mid + r)
        out.append((l, r, contigs))
    return out


def _host_expect(cases, contigs, first, scores):
    """Host twin of the device words: per gap the best word, per contig (index >= first) its selection, and the dropped count."""
    from gappadder_amd.pick_contigs import align_hits, select_per_contig
    n_gaps = len(cases)
    best = np.zeros(n_gaps, dtype=np.uint64)
    picks = {}
    dropped = 0
    for g, (l, r, _) in enumerate(cases):
        idx = [i for i, (gg, _) in enumerate(contigs) if gg == g and i >= first]
        mine = [("c%d" % i, contigs[i][1]) for i in idx]
        st = {}
        for t in scores:
            per = select_per_contig(align_hits(mine, l, r, t, stats=st if t == scores[0] else None))
            for j, (span, lp, rp, lm, rm, rc) in per.items():
                ci = idx[j]
                if span < 0 or ci in picks:
                    continue
                picks[ci] = (lp, rp, lm, rm, int(rc), t)
                w = (t << 56) | (min(span + 1, 0xFFFFFF) << 32) | ((0x7FFFFFFF - ci) << 1) | int(rc)
                best[g] = max(int(best[g]), w)
        dropped += st.get("dropped", 0)
    return best, picks, dropped


def test_device_align_pick_equals_the_host_twin():
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    cases = _cases(21)
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
    gf = GapFill(0)
    gf.set_gaps(gaps, 1, [(l, r) for l, r, _ in cases])
    lib = B.lib()
    n = len(contigs)
    d_ctg, d_seq = _dev(ctg.view(np.uint8)), _dev(np.frombuffer("".join(s for _, s in contigs).encode(), dtype=np.uint8))
    first = n // 3
    d_n = torch.tensor([n, first], dtype=torch.int32, device="cuda")
    want_all = _host_expect(cases, contigs, 0, (30, 15))
    want_from = _host_expect(cases, contigs, first, (30, 15))
    assert want_all[2] > 0, "no case reaches the cap"
    n_closed_want = int((want_all[0] != 0).sum())
    assert 150 < n_closed_want < n_gaps - 30
    for how in ("one launch", (30, 15), (15, 30), "from"):
        d_best = torch.zeros(n_gaps, dtype=torch.int64, device="cuda")
        d_closed = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_pick = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(2, dtype=torch.int32, device="cuda")
        args = (d_best.data_ptr(), d_closed.data_ptr(), d_pick.data_ptr(), d_st.data_ptr())
        if how == "one launch":
            assert lib.gf_pick_aligned_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), 30, 15, *args) == 0
        elif how == "from":
            assert lib.gf_pick_aligned_from_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), 30, 15, d_n.data_ptr() + 4, *args) == 0
        else:
            for t in how:
                assert lib.gf_pick_aligned_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), t, 0, *args) == 0
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
        if how == "one launch":
            assert int(st[0]) == dropped_w


def test_device_align_pick_rejects_flanks_beyond_1024_bases():
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
    assert B.lib().gf_pick_aligned_dev(gf.handle, d_ctg.data_ptr(), p, 1, d_seq.data_ptr(), 30, 15, p + 8, p + 16, p + 32, p + 64) == B.GF_E_UNSUPPORTED


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


def _picks(res):
    """Pick words with the contig named by its bases (the device's contig order is unspecified)."""
    from gappadder_amd.pipeline import decode_best
    out = []
    for g, w in enumerate(res.best.tolist()):
        if w:
            t, span1, ci, rev = decode_best(w)
            c = res.contigs[ci]
            out.append((g, t, span1, rev, res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])]))
    return out


def test_align_mode_closes_gaps_whose_flanks_carry_a_mismatch_next_to_the_gap():
    """Half of the gaps get one draft mismatch within the 10 gap-side bases of a flank: exact mode closes none of them, align mode
    closes every one the unmutated run closes, with the true sequence; on error-free flanks align closes what exact closes with the
    identical sequence; anchor_mode="exact" passed explicitly gives the default's words (threshold, span, strand, contig) exactly."""
    from gappadder_amd.hip_api import GapFill
    rng = np.random.default_rng(5)
    mutated = set()

    def plant(flanks):
        out = []
        for g, (l, r) in enumerate(flanks):
            if g % 2 == 0:
                mutated.add(g)
                if g % 4 == 0:
                    l = _mutate(l, len(l) - 1 - int(rng.integers(0, 10)), rng)
                else:
                    r = _mutate(r, int(rng.integers(0, 10)), rng)
            out.append((l, r))
        return out

    p_ex, r_ex, gaps, cfg = _step(lambda f: f)
    p_ex2, r_ex2, _, _ = _step(lambda f: f, "exact")
    assert _picks(r_ex) == _picks(r_ex2)
    p_al, r_al, _, _ = _step(lambda f: f, "align")
    seq_ex, seq_al = p_ex.picked_sequences(r_ex), p_al.picked_sequences(r_al)
    assert len(seq_ex) >= 6
    for g, (ci, body, rev) in seq_ex.items():
        assert g in seq_al and seq_al[g][1] == body, g
    pm_ex, rm_ex, _, _ = _step(plant, "exact")
    pm_al, rm_al, _, _ = _step(plant, "align")
    closed_clean = set(seq_ex)
    assert mutated & closed_clean
    assert not (set(np.nonzero(rm_ex.best)[0].tolist()) & mutated & closed_clean)
    got = pm_al.picked_sequences(rm_al)
    n_true = 0
    for g in mutated & closed_clean:
        assert g in got, g
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        truth = (GapFill.synth_truth(cfg, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg, sc, st - 6, en - st + 11))
        assert got[g][1] == seq_ex[g][1], g
        n_true += got[g][1] in truth
    assert n_true >= len(mutated & closed_clean) - 1
    assert rm_al.align_dropped == 0 and rm_al.align_seed_overflow == 0
