"""gf_pick_joins_dev (csrc/pick_join.hip) called directly on a hand-built contig list: the cases of
tests/flank_join_cases.py — whose records are derived by hand — and, beside them, the cases that are the device's own: anchors at
contig positions 63 and 64 (the wave's stride), at 0 and at the contig's end, a contig of the smallest length that can be accepted, a
contig of 8 192 bases, on both strands, every gap's contigs between decoys of other gaps; a list handed over at its capacity with the
counter beyond it; `first` pointing into the list.  Every record and every statistics word equals the twin (tobytes())."""
import random

import numpy as np
import pytest

import flank_join_cases as FC

pytestmark = pytest.mark.gpu

PARAMS = [(FC.ANCHORS, FC.X, FC.C, FC.M), ((30, 15), 64, 0, 0), ((32, 8), 1024, 255, 15), ((20,), 100, 10, 1)]


def device_cases(seed=24):
    """(cases without hand-derived answers: the twin is their reference; the names of those the twin must join at the default parameters)"""
    rng = random.Random(seed)
    out, joined = [], []

    def add(name, lf, rf, contigs, join=True):
        out.append(dict(name=name, lf=lf, rf=rf, contigs=contigs, closed=False, tombstones=[], want=None, stats={}))
        if join:
            joined.append(name)

    for cl in (63, 64, 81, 82):                  # j = cl, i = cl + 12 - 30: the right anchor at 63 / 64, then the left one
        lf, rf, s = FC.junction(rng, 12, cl=cl)
        add("stride %d" % cl, lf, rf, [s])
        lf, rf, s = FC.junction(rng, 12, cl=40, cr=cl)
        add("stride %d reverse" % cl, lf, rf, [FC.rc(s)])
    for o in (30, 40):                           # the right anchor at 0, the left one ending at the contig's end: no context unless C = 0
        lf, rf, s = FC.junction(rng, o, cl=0, cr=0)
        add("edges o=%d" % o, lf, rf, [s, FC.rc(s)], join=False)
    lf, rf, s = FC.junction(rng, 12, cl=FC.C, cr=FC.C)       # C + o + C bases: the smallest contig the defaults accept
    add("minimal contig", lf, rf, [s, s[1:], s[:-1]])
    lf, rf, s = FC.junction(rng, 100, cl=4000, cr=4092, size=9400, r=4500)
    assert len(s) == 8192
    add("8192 bases", lf, rf, [s])
    lf, rf, s = FC.junction(rng, 100, cl=4092, cr=4000, size=9400, r=4500)
    add("8192 bases reverse", lf, rf, [FC.rc(s)])
    return out, joined


@pytest.fixture(scope="module")
def world():
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    extra, must_join = device_cases()
    cs = FC.cases() + extra
    contigs, flanks, best, index = FC.assemble(cs)
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
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    w = dict(cs=cs, contigs=contigs, flanks=flanks, best=best, index=index, n=n, gf=gf, lib=B.lib(), must_join=must_join,
             d_ctg=dev(ctg.view(np.uint8)), d_seq=dev(np.frombuffer("".join(s for _, s in contigs).encode(), dtype=np.uint8)),
             d_best=dev(np.array(best, dtype=np.uint64).view(np.int64)))
    yield w
    gf.close()


def _call(w, anchors, X, C, M, counter=None, cap=None, first=None):
    """(records, statistics dictionary) of one call; the outputs are pre-filled with junk: the call writes every record and word."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import flank_joins as FJ
    n_gaps = len(w["cs"])
    d_n = torch.tensor([w["n"] if counter is None else counter], dtype=torch.int32, device="cuda")
    d_first = torch.tensor([first], dtype=torch.int32, device="cuda") if first is not None else None
    d_rec = torch.full((n_gaps * B.FLANK_JOIN.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B.FJ_WORDS,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a_l, a_s = FJ.check_anchors(anchors)
    rc = w["lib"].gf_pick_joins_dev(w["gf"].handle, w["d_ctg"].data_ptr(), d_n.data_ptr(), w["n"] if cap is None else cap, w["d_seq"].data_ptr(), a_l, a_s,
                                    X, C, M, d_first.data_ptr() if d_first is not None else None, w["d_best"].data_ptr(), d_rec.data_ptr(),
                                    d_st.data_ptr())
    assert rc == 0, (rc, w["lib"].gf_last_error(w["gf"].handle))
    w["gf"].sync()
    words = d_st.cpu().numpy().view(np.uint32)
    assert not words[B.FJ_NO_ANCHORS + 1:].any()
    return np.frombuffer(d_rec.cpu().numpy().tobytes(), dtype=B.FLANK_JOIN), FJ.stats_dict(words)


def _same(got, want, cs):
    bad = [g for g in range(len(cs)) if got[0][g].tobytes() != want[0][g].tobytes()]
    assert not bad, [(cs[g]["name"], got[0][g], want[0][g]) for g in bad[:4]]
    assert got[1] == want[1]


@pytest.mark.parametrize("anchors, X, C, M", PARAMS)
def test_records_and_statistics_equal_the_twin(world, anchors, X, C, M):
    from gappadder_amd import flank_joins as FJ
    w = world
    want = FJ.joins_host(w["contigs"], w["flanks"], w["best"], anchors, X, C, M)
    got = _call(w, anchors, X, C, M)
    print(anchors, X, C, M, got[1])
    _same(got, want, w["cs"])
    assert want[1]["joined"] >= (10 if C <= 30 else 2)         # (C = 255: only the long contigs have that much context)
    if (anchors, X, C, M) == PARAMS[0]:
        # the hand-derived answers of the shared cases, and the device's own cases the twin must join
        n0 = len(FC.cases())
        recs, _ = FC.expected(w["cs"][:n0], w["index"])
        for g, r in enumerate(recs):
            if r is None:
                assert got[0][g].tobytes() == bytes(32), w["cs"][g]["name"]
            else:
                assert {k: int(got[0][g][k]) for k in r} == r, w["cs"][g]["name"]
        names = [c["name"] for c in w["cs"]]
        for name in w["must_join"]:
            assert int(got[0][names.index(name)]["overlap"]) in (12, 100), name
    if C == 0:          # anchors at 0 and at the contig's end are accepted without context
        names = [c["name"] for c in w["cs"]]
        for o in (30, 40):
            r = got[0][names.index("edges o=%d" % o)]
            assert int(r["overlap"]) == o and int(r["right_pos"]) == 0 and int(r["n_accepted"]) == 2 and not int(r["flags"]) & FC.REVERSE


def test_a_counter_beyond_the_capacity_and_a_capacity_below_the_list(world):
    from gappadder_amd import flank_joins as FJ
    w = world
    full = FJ.joins_host(w["contigs"], w["flanks"], w["best"])
    _same(_call(w, *PARAMS[0], counter=w["n"] + 5), full, w["cs"])                 # an overflowed producer: the records up to the capacity
    cap = w["n"] - 7
    cut = FJ.joins_host(w["contigs"][:cap], w["flanks"], w["best"])
    assert cut[0].tobytes() != full[0].tobytes()
    _same(_call(w, *PARAMS[0], cap=cap), cut, w["cs"])
    _same(_call(w, *PARAMS[0], counter=w["n"] + 5, cap=cap), cut, w["cs"])
    _same(_call(w, *PARAMS[0], counter=0), FJ.joins_host([], w["flanks"], w["best"]), w["cs"])


def test_first_points_into_the_list(world):
    from gappadder_amd import flank_joins as FJ
    w = world
    for first in (0, 9, w["n"] - 3, w["n"], w["n"] + 4):
        want = FJ.joins_host(w["contigs"], w["flanks"], w["best"], first=first)
        _same(_call(w, *PARAMS[0], first=first), want, w["cs"])
    assert FJ.joins_host(w["contigs"], w["flanks"], w["best"], first=9)[0].tobytes() != FJ.joins_host(w["contigs"], w["flanks"], w["best"])[0].tobytes()


def test_arguments_out_of_range_are_refused(world):
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    w = world
    d_n = torch.tensor([w["n"]], dtype=torch.int32, device="cuda")
    d_rec = torch.zeros(len(w["cs"]) * 32, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(B.FJ_WORDS, dtype=torch.int32, device="cuda")

    def call(gf, a_l=30, a_s=15, X=256, C=30, M=2, rec=d_rec):
        return w["lib"].gf_pick_joins_dev(gf.handle, w["d_ctg"].data_ptr(), d_n.data_ptr(), w["n"], w["d_seq"].data_ptr(), a_l, a_s, X, C, M, None,
                                          w["d_best"].data_ptr(), rec.data_ptr() if rec is not None else None, d_st.data_ptr())
    for kw in (dict(X=0), dict(X=1025), dict(C=-1), dict(C=256), dict(M=-1), dict(M=16), dict(a_l=33), dict(a_l=7, a_s=0), dict(a_s=30), dict(a_s=7),
               dict(rec=None)):
        assert call(w["gf"], **kw) == B.GF_E_INVAL, kw
    assert call(w["gf"], a_s=0) == 0 and call(w["gf"], X=1, C=0, M=0) == 0 and call(w["gf"], X=1024, C=255, M=15) == 0
    # a flank of 65 536 bases: unsupported, nothing is truncated
    gf2 = GapFill(0)
    gaps = np.zeros(1, dtype=B.GAP)
    gaps[0] = (0, 100000, 100100, 1)
    gf2.set_gaps(gaps, 1, [("ACGT" * 16384, "ACGT" * 100)])
    d_best1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = w["lib"].gf_pick_joins_dev(gf2.handle, w["d_ctg"].data_ptr(), d_n.data_ptr(), w["n"], w["d_seq"].data_ptr(), 30, 15, 256, 30, 2, None,
                                    d_best1.data_ptr(), d_rec.data_ptr(), d_st.data_ptr())
    assert rc == B.GF_E_UNSUPPORTED
    gf2.close()
