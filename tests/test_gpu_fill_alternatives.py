"""gf_fill_alts_dev (csrc/fill_alt.hip) called directly on a hand-built contig list: the cases of tests/fill_alt_cases.py —
whose records are derived by hand — and, beside them, the cases that are the device's own: differing windows of 63, 64, 65 and 8 192
columns with exactly B and B + 1 edits for B in {1, 16, 31}, the first and the last of them in the window's first and last column; fills
that start at contig offsets 63 and 64; two unrelated fills of 8 192 bases; 300 peers of one gap; every gap's contigs between decoys of
other gaps; a list handed over at its capacity with the counter beyond it; `first` pointing into the list; no per-contig buffer.  The pick
words come from gf_pick_anchored2_dev on the same list (and must be the hand-written ones), then the doctored words replace theirs.
Records, per-contig records and statistics equal the twin (tobytes())."""
import random

import numpy as np
import pytest

import fill_alt_cases as AC

pytestmark = pytest.mark.gpu

BOUNDS = (AC.B, 1, 31)


def edited(W, n_edits, indels):
    """W, a text without the letter C, with n_edits edits, the first in its first column and the last in its last, the others spread
    evenly between: substitutions by C, or with `indels` (n_edits >= 4) the second a deleted base and the second but last an inserted C.
    Every edit changes the number of Cs by at most one, so n_edits substitutions are at distance n_edits exactly; with the two indels
    n_edits - 1 edits would all have to be substitutions, which the shifted stretch between the indels rules out."""
    cols = [round(x * (len(W) - 1) / max(1, n_edits - 1)) for x in range(n_edits)]
    assert "C" not in W and len(set(cols)) == n_edits
    t = list(W)
    for x, c in enumerate(cols):
        t[c] = "C"
        if indels and n_edits >= 4 and x == n_edits - 2:
            t[c] = W[c] + "C"
        if indels and n_edits >= 4 and x == 1:
            t[c] = ""
    return "".join(t)


def device_cases(seed=25):
    """(cases without hand-derived answers: the twin is their reference)"""
    rng = random.Random(seed)
    out = []

    def add(name, contigs, lf=None, rf=None):
        lf, rf = lf or AC.rnd(rng, 400), rf or AC.rnd(rng, 400)
        out.append(dict(name=name, lf=lf, rf=rf, contigs=[c(lf, rf) if callable(c) else c for c in contigs], tombstones=[], best=None, doctored=False,
                        want=None, per=None))

    ctg = lambda F, cl=40, cr=40, turn=False: (lambda lf, rf: AC.rc(lf[-cl:] + F + rf[:cr]) if turn else lf[-cl:] + F + rf[:cr])
    for cols in (63, 64, 65, 8192):
        for b in BOUNDS:
            for n_edits in (b, b + 1):
                pre, W, post = AC.rnd(rng, 10), "".join(rng.choice("AGT") for _ in range(cols)), AC.rnd(rng, 10)
                rivals = [ctg(pre + edited(W, n_edits, indels) + post, turn=indels and cols != 8192) for indels in (False, True)]
                add("window %d, %d edits" % (cols, n_edits), [ctg(pre + W + post)] + rivals[:1 if cols == 8192 and b != AC.B else 2])
    for cl in (63, 64):
        F = AC.rnd(rng, 130)
        add("fill at offset %d" % cl, [ctg(F, cl=cl), ctg(AC.flip(F, 0, 64, 129), cl=cl + 1), ctg(AC.flip(F, 63), cl=cl, turn=True)])
    add("unrelated 8192", [ctg(AC.rnd(rng, 8192)), ctg(AC.rnd(rng, 8192)), ctg(AC.rnd(rng, 8190), turn=True)])
    F = AC.rnd(rng, 100)
    peers = [ctg(F)]
    for x in range(300):
        kind = x % 4
        peers.append(ctg(F if kind == 0 else AC.flip(F, x % 100) if kind == 1 else AC.flip(F, *range(x % 50, x % 50 + 40, 2)) if kind == 2 else F[:x % 90] + F[x % 90 + 3:],
                         cl=30 + x % 30, turn=bool(x & 4)))
    add("300 peers", peers)
    return out


@pytest.fixture(scope="module")
def world():
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    shared = AC.cases()
    cs = shared + device_cases()
    contigs, flanks, hand, index = AC.assemble(cs)
    n = len(contigs)
    ctg = np.zeros(n, dtype=B.CONTIG)
    off = 0
    for i, (g, s) in enumerate(contigs):
        ctg[i] = (g, 31, 29, 1, len(s), 0, 0, off)
        off += len(s)
    gaps = np.zeros(len(cs), dtype=B.GAP)
    for g in range(len(cs)):
        gaps[g] = (0, 20000 * (g + 1), 20000 * (g + 1) + 100, g + 1)
    gf = GapFill(0)
    gf.set_gaps(gaps, 1, flanks)
    lib = B.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_ctg, d_seq = dev(ctg.view(np.uint8)), dev(np.frombuffer("".join(s for _, s in contigs).encode(), dtype=np.uint8))

    def pick(a_l, a_s):
        """the pick's own words on this list"""
        d_best = torch.zeros(len(cs), dtype=torch.int64, device="cuda")
        d_n = torch.tensor([n, 0], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = lib.gf_pick_anchored2_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), a_l, a_s, d_best.data_ptr(), d_n.data_ptr() + 4)
        assert rc == 0, (rc, lib.gf_last_error(gf.handle))
        gf.sync()
        return [int(x) for x in d_best.cpu().numpy().view(np.uint64)]

    best = pick(30, 15)
    for g, c in enumerate(shared):
        if c["doctored"]:
            best[g] = hand[g]
        else:
            assert best[g] == hand[g], (c["name"], hex(best[g]), hex(hand[g]))
    assert all(best[g] for g in range(len(shared), len(cs)))
    w = dict(cs=cs, n_shared=len(shared), contigs=contigs, flanks=flanks, best=best, index=index, n=n, gf=gf, lib=lib, d_ctg=d_ctg, d_seq=d_seq, dev=dev,
             pick=pick)
    yield w
    gf.close()


def _call(w, anchors=AC.ANCHORS, bound=AC.B, counter=None, cap=None, first=None, per_contig=True, best=None):
    """(records, per-contig records or None, statistics dictionary) of one call; the outputs are pre-filled with junk: the call writes
    every record and word."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_alternatives as FA
    n_gaps = len(w["cs"])
    cap = w["n"] if cap is None else cap
    d_n = torch.tensor([w["n"] if counter is None else counter], dtype=torch.int32, device="cuda")
    d_first = torch.tensor([first], dtype=torch.int32, device="cuda") if first is not None else None
    d_rec = torch.full((n_gaps * B.FILL_ALT.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    d_per = torch.full((max(1, cap) * B.FILL_ALT_CONTIG.itemsize,), 0x55, dtype=torch.uint8, device="cuda") if per_contig else None
    d_st = torch.full((B.FA_WORDS,), 7, dtype=torch.int32, device="cuda")
    d_best = w["dev"](np.array(w["best"] if best is None else best, dtype=np.uint64).view(np.int64))
    torch.cuda.synchronize()
    a_l, a_s = FA.check_anchors(anchors)
    rc = w["lib"].gf_fill_alts_dev(w["gf"].handle, w["d_ctg"].data_ptr(), d_n.data_ptr(), cap, w["d_seq"].data_ptr(), a_l, a_s, bound,
                                   d_first.data_ptr() if d_first is not None else None, d_best.data_ptr(), d_rec.data_ptr(),
                                   d_per.data_ptr() if per_contig else None, d_st.data_ptr())
    assert rc == 0, (rc, w["lib"].gf_last_error(w["gf"].handle))
    w["gf"].sync()
    words = d_st.cpu().numpy().view(np.uint32)
    assert not words[B.FA_LOST + 1:].any()
    n_listed = min(cap, w["n"] if counter is None else counter)
    per = np.frombuffer(d_per.cpu().numpy().tobytes(), dtype=B.FILL_ALT_CONTIG) if per_contig else None
    if per is not None:          # (the records beyond the list are not the call's)
        assert per[n_listed:].tobytes() == b"\x55" * (8 * (len(per) - n_listed))
        per = per[:n_listed]
    return np.frombuffer(d_rec.cpu().numpy().tobytes(), dtype=B.FILL_ALT), per, FA.stats_dict(words)


def _same(got, want, cs):
    bad = [g for g in range(len(cs)) if got[0][g].tobytes() != want[0][g].tobytes()]
    assert not bad, [(cs[g]["name"], got[0][g], want[0][g]) for g in bad[:4]]
    if got[1] is not None:
        bad = [i for i in range(len(want[1])) if got[1][i].tobytes() != want[1][i].tobytes()]
        assert not bad and len(got[1]) == len(want[1]), [(i, got[1][i], want[1][i]) for i in bad[:4]]
    assert got[2] == want[2]


@pytest.mark.parametrize("anchors, bound", [(AC.ANCHORS, AC.B), (AC.ANCHORS, 1), (AC.ANCHORS, 31), ((30,), 5), ((32, 8), 16)])
def test_records_and_statistics_equal_the_twin(world, anchors, bound):
    from gappadder_amd import fill_alternatives as FA
    w = world
    # (the doctored words belong to the cases' own anchors; at other anchors every word is that pick's)
    best = w["best"] if anchors == AC.ANCHORS else w["pick"](*FA.check_anchors(anchors))
    want = FA.alts_host(w["contigs"], w["flanks"], best, anchors, bound)
    got = _call(w, anchors, bound, best=best)
    print(anchors, bound, got[2])
    _same(got, want, w["cs"])
    assert want[2]["lost"] == (4 if anchors == AC.ANCHORS else 0) and want[2]["contested"] >= 30
    names = [c["name"] for c in w["cs"]]
    if anchors == AC.ANCHORS:
        # the planted windows: exactly `bound` edits are near at that distance, one more is far; lcp and lcs frame the window
        for cols in (63, 64, 65, 8192):
            for n_edits, near in ((bound, True), (bound + 1, False)):
                r = got[0][names.index("window %d, %d edits" % (cols, n_edits))]
                assert (int(r["n_near"]) >= 1) == near and (int(r["lcp"]), int(r["fill_len"])) == (10, cols + 20), (cols, n_edits, r)
                assert int(r["n_near"]) + int(r["n_far"]) == int(r["n_candidates"]) - 1 >= 1
        r = got[0][names.index("unrelated 8192")]
        assert (int(r["n_far"]), int(r["dist"]), int(r["fill_len"]), int(r["rival_len"])) == (2, 0xFFFF, 8192, 8192)
        r = got[0][names.index("300 peers")]
        assert int(r["n_candidates"]) == 301 and int(r["n_identical"]) == 75 and int(r["len_min"]) == 97 and int(r["len_max"]) == 100
        assert int(r["n_near"]) + int(r["n_far"]) == 225 and int(r["flags"]) & AC.LENGTH_VARIES
    if (anchors, bound) == (AC.ANCHORS, AC.B):
        # the hand-derived answers of the shared cases
        from test_fill_alternatives_host import record
        recs, per, _ = AC.expected(w["cs"][:w["n_shared"]], w["index"])
        for g, r in enumerate(recs):
            assert got[0][g].tobytes() == record(r).tobytes(), (names[g], got[0][g], r)
        for at, p in per.items():
            assert tuple(int(x) for x in got[1][at]) == p, (at, got[1][at], p)
        assert got[2]["lost"] == 4 and got[2]["outranked"] == 4


def test_without_a_per_contig_buffer(world):
    from gappadder_amd import fill_alternatives as FA
    w = world
    want = FA.alts_host(w["contigs"], w["flanks"], w["best"])
    got = _call(w, per_contig=False)
    assert got[1] is None
    _same(got, want, w["cs"])
    assert int(want[0]["dist"].max()) == 0xFFFF and ((want[0]["dist"] > 0) & (want[0]["dist"] <= 16)).sum() >= 10


def test_a_counter_beyond_the_capacity_and_a_capacity_below_the_list(world):
    from gappadder_amd import fill_alternatives as FA
    w = world
    full = FA.alts_host(w["contigs"], w["flanks"], w["best"])
    _same(_call(w, counter=w["n"] + 5), full, w["cs"])                 # an overflowed producer: the records up to the capacity
    cap = w["n"] - 150                                                 # (cuts into the 300 peers)
    cut = FA.alts_host(w["contigs"][:cap], w["flanks"], w["best"])
    assert cut[0].tobytes() != full[0].tobytes()
    _same(_call(w, cap=cap), cut, w["cs"])
    _same(_call(w, counter=w["n"] + 5, cap=cap), cut, w["cs"])
    empty = FA.alts_host([], w["flanks"], w["best"])
    assert empty[2]["lost"] == empty[2]["closed_gaps"] > 0
    _same(_call(w, counter=0), empty, w["cs"])


def test_first_points_into_the_list(world):
    from gappadder_amd import fill_alternatives as FA
    w = world
    n_gaps = len(w["cs"])
    below = None
    for first in (0, n_gaps + 3, w["n"] - 3, w["n"], w["n"] + 4):
        want = FA.alts_host(w["contigs"], w["flanks"], w["best"], first=first)
        _same(_call(w, first=first), want, w["cs"])
        if first == n_gaps + 3:
            below = want
    # the winners below `first` are found all the same: no gap is lost that was not lost before, the per-contig record names them
    full = FA.alts_host(w["contigs"], w["flanks"], w["best"])
    assert below[2]["lost"] == full[2]["lost"] and below[2]["candidates"] < full[2]["candidates"]
    winners_below = [int(r["contig"]) for r in below[0] if int(r["n_candidates"]) and int(r["contig"]) < n_gaps + 3]
    assert len(winners_below) >= 20 and all(int(below[1][c]["cls"]) == AC.WINNER for c in winners_below)


def test_arguments_out_of_range_are_refused(world):
    import torch
    from gappadder_amd import _lib as B
    w = world
    d_n = torch.tensor([w["n"]], dtype=torch.int32, device="cuda")
    d_rec = torch.zeros(len(w["cs"]) * 48, dtype=torch.uint8, device="cuda")
    d_per = torch.zeros(w["n"] * 8, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(B.FA_WORDS, dtype=torch.int32, device="cuda")
    d_best = w["dev"](np.array(w["best"], dtype=np.uint64).view(np.int64))

    def call(a_l=30, a_s=15, bound=16, rec=d_rec, best=d_best, st=d_st, cap=w["n"]):
        ptr = lambda t: t.data_ptr() if t is not None else None
        return w["lib"].gf_fill_alts_dev(w["gf"].handle, w["d_ctg"].data_ptr(), d_n.data_ptr(), cap, w["d_seq"].data_ptr(), a_l, a_s, bound, None, ptr(best),
                                         ptr(rec), d_per.data_ptr(), ptr(st))
    for kw in (dict(bound=0), dict(bound=32), dict(bound=-1), dict(a_l=33), dict(a_l=7, a_s=0), dict(a_s=30), dict(a_s=7), dict(rec=None), dict(best=None),
               dict(st=None), dict(cap=0x80000000)):
        assert call(**kw) == B.GF_E_INVAL, kw
    assert call(a_s=0) == 0 and call(bound=1) == 0 and call(bound=31) == 0 and call(a_l=32, a_s=8) == 0
    w["gf"].sync()
