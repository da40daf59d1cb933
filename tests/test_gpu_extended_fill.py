"""The extended fill on the device (gf_pick_extended_dev / gf_pick_extended_aligned_dev, csrc/pick_ext.hip) against its host twin
(pick_contigs.pick_extended_sequence on the contigs in pick_contigs.extension_order), called directly on hand-built and random contig
sets, and through Pipeline(extended_fill=True) on synthetic steps whose gaps the picks leave open: alone, with merge_in_step and with
second_round, in both anchor modes."""
import numpy as np
import pytest

import pick_util as PK
from step_util import contigs as _contigs, picks as _picks, run as _run, setup as _setup

pytestmark = pytest.mark.gpu

KK = [(31, 29), (41, 39), (51, 49)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _random_cases(seed, n_gaps):
    """Per gap (left flank, right flank, [contig]): clipped and unclipped flanks, N in an anchor, flanks shorter than 15, repeated
    anchors, contigs shorter than 30 with one anchor, several contigs with a hit per side, equal lengths, duplicates, both strands."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n_gaps):
        nl, nr = [100, 15, 60, 10, 300][g % 5], [100, 100, 15, 40, 12][(g // 5) % 5]
        l, r = PK.rand_seq(rng, nl), PK.rand_seq(rng, nr)
        if g % 11 == 3:
            l = l[:-4] + "N" + l[-3:]
        if g % 13 == 4:
            r = r[:6] + "N" + r[7:]
        contigs = []
        for _ in range(int(rng.integers(1, 7))):
            kind = int(rng.integers(0, 8))
            into, out_ = PK.rand_seq(rng, int(rng.integers(0, 120))), PK.rand_seq(rng, int(rng.integers(0, 120)))
            ls, rs = l[len(l) - int(rng.integers(15, 61)):] if len(l) >= 15 else l, r[:int(rng.integers(15, 61))]
            if kind == 0:
                s = PK.rand_seq(rng, int(rng.integers(0, 20))) + ls + into
            elif kind == 1:
                s = out_ + rs + PK.rand_seq(rng, int(rng.integers(0, 20)))
            elif kind == 2:                                   # shorter than 30, one anchor
                s = (l[-15:] + PK.rand_seq(rng, int(rng.integers(0, 12)))) if rng.integers(0, 2) else (PK.rand_seq(rng, int(rng.integers(0, 12))) + r[:15])
            elif kind == 3:                                   # repeated anchors
                s = l[-15:] + PK.rand_seq(rng, 7) + ls + into + rs + PK.rand_seq(rng, 5) + r[:15]
            elif kind == 4:                                   # both anchors out of order: one contig on both sides
                s = out_ + rs + PK.rand_seq(rng, 20) + ls + into
            elif kind == 5 and contigs:                       # a duplicate, or a same-length rival
                s = contigs[-1] if rng.integers(0, 2) else PK.rand_seq(rng, len(contigs[-1]))
            elif kind == 6:
                s = ls + into + PK.rand_seq(rng, 5) + rs
            else:
                s = PK.rand_seq(rng, int(rng.integers(5, 80)))
            contigs.append(PK._rc(s) if rng.integers(0, 3) == 0 else s)
        out.append((l, r, contigs))
    return out


def _hand_cases():
    """The hand-built cases of the host layer's quirk test (extended part), one gap each."""
    rng = np.random.default_rng(3)
    left, right = PK.rand_seq(rng, 100), PK.rand_seq(rng, 100)
    into, out_ = PK.rand_seq(rng, 120), PK.rand_seq(rng, 90)
    cl, cr = left[-40:] + into, out_ + right[:50]
    both = out_[:25] + right[:15] + PK.rand_seq(rng, 30) + left[-15:] + into[:10]
    return [(left, right, [cl, cr]), (left, right, [cl]), (left, right, [cr]), (left, right, [left[-15:] + "ACGTA", cl]),
            (left, right, [PK._rc(cr)]), (left, right, [PK._rc(cl)]), (left, right, [both]), (left, right, [PK.rand_seq(rng, 300)]),
            (left, right, [left[-15:]]), (left, right, [cl, PK._rc(cl), cr, PK._rc(cr)])]


def twin_expect(flanks, contigs, k_pairs, mode, open_gaps, first=0):
    """Per open gap the twin's (left index or -1, right index or -1, fill, text) on the gap's contigs (index >= first) in extension
    order; contigs: [(gap, k, kv, bases)]."""
    from gappadder_amd.pick_contigs import extension_order, pick_extended_sequence
    per = {}
    for i, (g, k, kv, s) in enumerate(contigs):
        if i >= first:
            per.setdefault(g, []).append(i)
    want = {}
    for g in open_gaps:
        idx = per.get(g, [])
        order = [idx[j] for j in extension_order([contigs[i][1:] for i in idx], k_pairs)]
        l, r = flanks[g]
        res = pick_extended_sequence([("%d" % i, contigs[i][3]) for i in order], l, r, 15, mode)
        if res is not None:
            want[g] = (int(res[0]) if res[0] else -1, int(res[1]) if res[1] else -1, res[2], res[3])
    return want


def _decode_all(ext, bases, contigs):
    from gappadder_amd import _lib as B
    from gappadder_amd.pick_contigs import decode_extended
    got = {}
    for g, rec in enumerate(ext):
        d = decode_extended(rec, lambda i: contigs[i][3])
        if d is None:
            assert int(rec["len"]) == 0
            continue
        assert bases[int(rec["off"]):int(rec["off"]) + int(rec["len"])].decode() == (d[2] or ""), g
        got[g] = d
    return got


@pytest.mark.parametrize("mode", ["exact", "align"])
def test_device_extension_equals_the_host_twin(mode):
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    cases = PK.picker_cases(21, 200) + _hand_cases() + _random_cases(5, 400)
    n_gaps = len(cases)
    gaps = np.zeros(n_gaps, dtype=B.GAP)
    for g in range(n_gaps):
        gaps[g] = (0, 2000 * (g + 1), 2000 * (g + 1) + 100, g + 1)
    rng = np.random.default_rng(7)
    pairs = KK + [(0, 0), (21, 19)]
    contigs = [(g, *pairs[int(rng.integers(0, len(pairs)))], s) for g, (_, _, seqs) in enumerate(cases) for s in seqs]
    contigs = [contigs[i] for i in rng.permutation(len(contigs))]
    ctg = np.zeros(len(contigs), dtype=B.CONTIG)
    o = 0
    for i, (g, k, kv, s) in enumerate(contigs):
        ctg[i] = (g, k, kv, 1, len(s), 0, 0, o)
        o += len(s)
    gf = GapFill(0)
    flanks = [(l, r) for l, r, _ in cases]
    gf.set_gaps(gaps, 1, flanks)
    lib = B.lib()
    n = len(contigs)
    d_ctg, d_seq = _dev(ctg.view(np.uint8)), _dev(np.frombuffer("".join(c[3] for c in contigs).encode(), dtype=np.uint8))
    first = n // 4
    d_n = torch.tensor([n, first], dtype=torch.int32, device="cuda")
    best = np.zeros(n_gaps, dtype=np.uint64)
    best[rng.choice(n_gaps, n_gaps // 10, replace=False)] = 1 << 56          # closed gaps: never extended
    d_best = _dev(best.view(np.int64))
    k_arr, kv_arr = (np.array([a for a, _ in KK], dtype=np.int32), np.array([b for _, b in KK], dtype=np.int32))
    fn = lib.gf_pick_extended_aligned_dev if mode == "align" else lib.gf_pick_extended_dev
    open_gaps = [g for g in range(n_gaps) if not best[g]]
    for first_p, f0 in ((None, 0), (d_n.data_ptr() + 4, first)):
        want = twin_expect(flanks, contigs, KK, mode, open_gaps, f0)
        n_fill = sum(w[2] is not None for w in want.values())
        assert n_fill > 150 and sum(w[0] >= 0 and w[1] >= 0 for w in want.values()) > 50
        total = sum(len(w[2]) for w in want.values() if w[2] is not None)
        d_ext = torch.full((n_gaps * B.EXT_PICK.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
        d_bases = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        d_st = torch.full((B.EXT_WORDS,), 7, dtype=torch.int32, device="cuda")
        assert fn(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), 15, B._p(k_arr), B._p(kv_arr), len(KK), first_p,
                  d_best.data_ptr(), d_ext.data_ptr(), d_bases.data_ptr(), total + 64, d_st.data_ptr()) == 0
        gf.sync()
        ext = np.frombuffer(d_ext.cpu().numpy().tobytes(), dtype=B.EXT_PICK)
        got = _decode_all(ext, d_bases.cpu().numpy().tobytes(), contigs)
        bad = sorted(g for g in set(got) | set(want) if got.get(g) != want.get(g))
        assert not bad, (mode, f0, [(g, got.get(g), want.get(g)) for g in bad[:3]])
        st = d_st.cpu().numpy().view(np.uint32)
        fills = [w for w in want.values() if w[2] is not None]
        assert int(st[B.EXT_EXTENDED]) == n_fill
        assert int(st[B.EXT_BOTH]) == sum(w[0] >= 0 and w[1] >= 0 for w in fills)
        assert int(st[B.EXT_LEFT_ONLY]) == sum(w[1] < 0 for w in fills) and int(st[B.EXT_RIGHT_ONLY]) == sum(w[0] < 0 for w in fills)
        assert int(st[B.EXT_BASES]) + (int(st[B.EXT_BASES + 1]) << 32) == total and int(st[B.EXT_OVERFLOW]) == 0
        # a base buffer one byte short: flagged, the fills that do not fit are not written
        d_small = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        assert fn(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), 15, B._p(k_arr), B._p(kv_arr), len(KK), first_p,
                  d_best.data_ptr(), d_ext.data_ptr(), d_small.data_ptr(), total - 1, d_st.data_ptr()) == 0
        gf.sync()
        assert int(d_st[B.EXT_OVERFLOW]) == 1 and int(d_small[total - 1:].sum()) == 0


# ---- Pipeline(extended_fill=True) on synthetic steps ----------------------------------------------------------------------------------

# name -> (gap length, k pairs): round 1 reaches about one insert (300 bp) past each flank; 900 bp / k 31 closes none of the 24 gaps,
# 550 bp / k 31 closes 3 (a second round closes all 24 of both); 2 000 bp stays open after two rounds
CONFIGS = {"open900_k31": (900, [(31, 29)]), "mixed550_k31": (550, [(31, 29)]), "open2000_k31": (2000, [(31, 29)])}
SETTINGS = {"plain": {}, "merge": {"merge_in_step": True}, "round2": {"second_round": True}}


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def layout(request):
    return (request.param,) + _setup(*CONFIGS[request.param])


def _true_parts(layout, fills):
    """(parts, parts equal to the truth): a left part equals the true bases after the left anchor (from one base earlier when a reverse
    part keeps an anchor base), a right part the true bases before the right anchor (up to its first base when the right side uses the
    left side's contig forward)."""
    from gappadder_amd.hip_api import GapFill
    _, gf, cfg, gaps, flanks, _, _, _ = layout
    n = ok = 0
    for g, lp, rp, l_keep, r_keep in fills:
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        if lp:
            n += 1
            ok += GapFill.synth_truth(cfg, sc, st - 5 - l_keep, len(lp)) == lp
        if rp:
            n += 1
            ok += GapFill.synth_truth(cfg, sc, en + 5 + r_keep - len(rp), len(rp)) == rp
    return n, ok


@pytest.fixture(scope="module")
def runs(layout):
    """(setting, anchor mode) -> (pipeline, Results) with the extension on; and the same with it off."""
    on, off = {}, {}
    for name, kw in SETTINGS.items():
        for mode in ("exact", "align"):
            on[name, mode] = _run(layout[1:], steps=2, extended_fill=True, anchor_mode=mode, **kw)
            off[name, mode] = _run(layout[1:], anchor_mode=mode, **kw)
    return on, off


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", ["exact", "align"])
def test_pipeline_fills_equal_the_twin(layout, runs, setting, mode):
    pipe, (res, res2) = runs[0][setting, mode]
    flanks = layout[4]
    contigs = _contigs(res)
    first = res.round2_first if setting == "round2" else 0
    open_gaps = [g for g in range(len(flanks)) if not res.best[g]]
    want = twin_expect(flanks, contigs, pipe.kk, mode, open_gaps, first)
    got = pipe.extended_sequences(res)
    assert got == want, sorted(g for g in set(got) | set(want) if got.get(g) != want.get(g))[:5]
    closed = np.nonzero(res.best)[0]
    assert (res.ext["left"][closed] == 0xFFFFFFFF).all() and (res.ext["right"][closed] == 0xFFFFFFFF).all() and not res.ext["len"][closed].any()
    if setting == "round2":
        assert all(i < 0 or i >= first for v in got.values() for i in v[:2])
    fills = [v for v in got.values() if v[2] is not None]
    assert res.extended["gaps_extended"] == len(fills) and res.extended["bases"] == sum(len(v[2]) for v in fills)
    if layout[0] == "open900_k31" and setting == "plain":
        assert not res.best.any()
    if layout[0] == "open900_k31" and setting == "plain" and mode == "exact":
        assert res.extended["both_sides"] == len(flanks) == len(fills)
    # parts against the truth
    parts = []
    for g, v in got.items():
        rec = res.ext[g]
        if v[2] is not None:
            ll = int(rec["l_len"])
            parts.append((g, v[2][:ll], v[2][ll + 2:], int(rec["l_rev"]), int(rec["left"] == rec["right"] and not rec["r_rev"])))
    n, ok = _true_parts(layout, parts)
    print("%s %s %s: %d open gaps, %d extended, %d of %d parts true" % (layout[0], setting, mode, len(open_gaps), len(fills), ok, n))
    if mode == "exact":
        # (align mode: the synthetic contigs mostly cover a whole 300-base flank, an unclipped hit that never extends)
        assert ok >= 0.9 * n, (ok, n)
        if setting != "round2" or layout[0] == "open2000_k31":
            assert len(fills) >= len(open_gaps) // 2 > 0
    # two consecutive steps: the same fills (the contig indices may differ: the device's contig order is unspecified)
    assert {g: v[2:] for g, v in pipe.extended_sequences(res2).items()} == {g: v[2:] for g, v in got.items()}
    assert res2.ext_bases == res.ext_bases


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", ["exact", "align"])
def test_extension_changes_nothing_else(runs, setting, mode):
    _, (res, _) = runs[0][setting, mode]
    _, (ref,) = runs[1][setting, mode]
    assert ref.ext is None and ref.extended is None
    assert _picks(res) == _picks(ref)
    assert sorted(_contigs(res)) == sorted(_contigs(ref))
    assert res.merge == ref.merge and res.round2 == ref.round2 and res.round2_first == ref.round2_first


def test_too_small_fill_buffer_is_reported(layout):
    pipe, _ = _run(layout[1:], steps=0, extended_fill=True, ext_base_cap=64)
    pipe.step()
    with pytest.raises(RuntimeError, match="extended fill overflow"):
        pipe.fetch()
