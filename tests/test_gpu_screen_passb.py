"""The partitioned screen filter (csrc/screen_pf4.hip) against twins written from its definitions (screen_cand_twin.py), at sizes of a few
seconds that reach what the other screen tests reach only at bench size: parts of several pass-B trips with a tail trip behind full ones, the
short pair list with many groups, a part that runs full after the first iteration, and full home groups of the grouped exact set.  Asserted
on what the device dumps (gf_screen_debug_view): pass A's state pair for pair, and the candidate list read for read — every planted read is a
candidate through ONE pair, so a pair lost anywhere loses a candidate.  The inputs and their preconditions: screen_passb_cases.py (checked
without a GPU in test_screen_cand_twin_host.py); the preconditions are asserted here again, on the dumped counts and fills."""
import numpy as np
import pytest

import screen_cand_twin as W
import screen_passb_cases as K
from oracle import c_oracle as CO
from screen_state_util import build_column, dev, screen

pytestmark = pytest.mark.gpu

L = K.L
COL, ROWS, RUNS = "pf4_scatter_col_kernel<", "pf4_scatter_lines_kernel<", "pf4_scatter_kernel<"
FORMS = ((18, False, ROWS), (16, True, COL), (17, False, RUNS))     # (screen_variant, from the probe column, pass A's kernel)


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


@pytest.fixture()
def forced(gf, monkeypatch):
    """The partitioned filter on small inputs (2^27-bit level-1 bitmap, variant 16), its workspace and candidate list readable; every
    option back at its default afterwards."""
    monkeypatch.setenv("GF_DIAGNOSTICS", "1")
    try:
        gf.set_option("screen_keep_cand", 1)
        gf.set_option("bitmap_log2", 27)
        gf.set_option("screen_variant", 16)
        yield gf
    finally:
        gf.set_option("screen_variant", 0)
        gf.set_option("bitmap_log2", 0)
        gf.set_option("screen_ext", 1)
        gf.set_option("screen_pf4_cap8", 0)
        gf.set_option("screen_pf4_writers", 0)
        gf.set_option("screen_keep_cand", 0)


def _upload(packed):
    import torch
    return torch.cat([dev(packed), torch.zeros(64, dtype=torch.uint8, device="cuda")])


def _oracle(blob, flanks, k):
    from gappadder_amd import _lib as B
    return np.sort(CO.screen_reads(blob, L, flanks, k).astype(B.HIT), order=("gap", "read"))


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _forms(gf, d_reads, n, k, forms):
    """One screen per form of pass A, from the same reads: (variant, result of screen_state_util.screen)."""
    d_col = geom = None
    for variant, col, kernel in forms:
        gf.set_option("screen_variant", 16)
        if col and d_col is None:
            d_col, geom = build_column(gf, d_reads, n, L, k)
            assert geom.use == 1, geom.key()
        gf.set_option("screen_variant", variant)
        res = screen(gf, d_reads, n, L, k, d_col if col else None, geom if col else None)
        assert res[3].startswith(kernel) and res[2] == 0, (variant, res[3], res[2])
        yield variant, res


def _same_state(st, tw, what):
    assert st["shape"][3] == tw["n_groups"], (what, st["shape"])
    for name in ("count", "fills", "runs", "pairs"):
        assert np.array_equal(st[name], tw[name]), (what, name)


def _same_cand(cand, r, what):
    lost, extra = np.setdiff1d(r["cand"], cand), np.setdiff1d(cand, r["cand"])
    assert not len(lost) and not len(extra), (what, "lost %d of %d, (read, part, group) of the first: %s; not candidates: %s" % (
        len(lost), len(r["cand"]), W.homes(r["state"], r["qual"], lost[:12]) if r["state"] else lost[:12], extra[:12]))


def test_writer_cap_is_a_diagnostic_and_leaves_the_default_plan_alone(forced, monkeypatch):
    """Option screen_pf4_writers: refused without GF_DIAGNOSTICS; 0 and a cap above the automatic number of writers give the plan of
    plan_screen without it (n_writers, cap, gs, n_groups of the workspace view against the twin's plan) and the same state and candidates
    before and after a capped run; a cap below it is the number of writers."""
    from gappadder_amd._lib import GapFillError
    gf = forced
    monkeypatch.delenv("GF_DIAGNOSTICS")
    with pytest.raises(GapFillError):
        gf.set_option("screen_pf4_writers", 1)
    gf.set_option("screen_pf4_writers", 0)
    monkeypatch.setenv("GF_DIAGNOSTICS", "1")
    with pytest.raises(GapFillError):
        gf.set_option("screen_pf4_writers", 257)
    r = K.crowded_case()
    n = r["case"]["packed"].shape[0]
    gf.set_gaps(r["draft"]["gaps"], r["draft"]["n_scaffolds"], r["draft"]["flanks"])
    d_reads = _upload(r["case"]["packed"])
    got = []
    for writers in (0, 256, 3, 0):
        gf.set_option("screen_pf4_writers", writers)
        st = screen(gf, d_reads, n, L, 51, None, None)[4]
        p = W.plan(n, L, 51, _n_cu(), writers)
        assert st["shape"].tolist() == [p["n_writers"], p["cap"], p["gs"], p["n_groups"]], (writers, st["shape"], p)
        got.append(st)
    assert got[2]["shape"][0] == 3 < got[0]["shape"][0] == (n + 2047) // 2048
    for other in (got[1], got[3]):
        for name in ("shape", "count", "fills", "runs", "pairs", "cand"):
            assert np.array_equal(got[0][name], other[name]), name


@pytest.mark.parametrize("n,writers", K.TRIP_RUNS)
def test_parts_of_several_trips(forced, n, writers):
    """Case (a): k = 51 under one or two writers.  Nearly every part takes two or three trips of pass B — full trips with a prefetch, then a
    tail trip whose mask is built at i0 > 0 — and in most parts the LAST group, which lies in the tail trip, holds a planted pair."""
    gf = forced
    c = K.draft()
    gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
    gf.set_option("screen_pf4_writers", writers)
    for ext in (1, 0):
        r = K.trip_run(n, writers, ext)
        exp = _oracle(r["case"]["blob"], c["flanks"], 51)
        gf.set_option("screen_ext", ext)
        d_reads = _upload(r["case"]["packed"])
        for variant, res in _forms(gf, d_reads, n, 51, FORMS):
            st, what = res[4], (n, writers, ext, variant)
            # the preconditions, on the dumped counts and fills
            f = W.tail_facts(st["count"], st["fills"])
            print("trips: reads %d writers %d ext %d variant %d: count %d..%d, tail classes %s, parts over 1024: %d of %d" % (
                n, writers, ext, variant, f["min"], f["max"], sorted(f["tails"]), (st["count"] > 1024).sum(), len(st["count"])))
            assert st["shape"][0] == writers and st["shape"][3] == (n + 2048 * writers - 1) // (2048 * writers), what
            assert (st["count"] > 1024).mean() > 0.9 and (st["count"] < st["shape"][1]).all(), what
            assert K.TRIP_WANT[n][0] <= f["tails"] and f["mod4"] == {0, 1, 2, 3} and (f["max"] > 2048) == K.TRIP_WANT[n][1], (what, f)
            assert len(r["confirmed"]) > 0.2 * n and W.planted_in_last_group(r["state"], st["count"], st["fills"], r["confirmed"], r["qual"]) >= 0.5, what
            # pass A's state, the candidates, the hits
            _same_state(st, r["state"], what)
            _same_cand(st["cand"], r, what)
            assert np.array_equal(res[0], exp) and res[1] == len(exp) > 0.005 * n, what


@pytest.mark.parametrize("k", [51, 31, 41])
def test_short_pair_list_with_many_groups(forced, k):
    """Case (b): a pair list of 256 / 1 024 entries against tens of thousands of pairs of the exact set, 25 iterations under one writer, one
    (k = 51) or two (k = 31, 41) groups each: what does not fit the list is resolved by its lane — the octet from the fill history
    (pf4_octet), no neighbour check — so the candidates lie between the twin's with and without that check."""
    gf = forced
    c, r = K.draft(), K.short_list_run(k)
    n = r["case"]["packed"].shape[0]
    gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
    gf.set_option("screen_pf4_writers", 1)
    exp = _oracle(r["case"]["blob"], c["flanks"], k)
    d_reads = _upload(r["case"]["packed"])
    for cap8 in (256, 1024):
        gf.set_option("screen_pf4_cap8", cap8)
        for variant, res in _forms(gf, d_reads, n, k, ((16, False, ROWS), (17, False, RUNS))):
            st, what = res[4], (k, cap8, variant)
            assert st["shape"][0] == 1 and st["shape"][3] == 25 * (1 if k == 51 else 2), (what, st["shape"])
            on_list = W.exact_set_pairs(st["pairs"], st["runs"], 1, int(st["shape"][3]), K.seeds(k)[0])
            assert on_list > 4 * cap8, (what, on_list)
            _same_state(st, r["state"], what)
            lost, extra = np.setdiff1d(r["cand"], st["cand"]), np.setdiff1d(st["cand"], r["loose"])
            assert not len(lost) and not len(extra), (what, W.homes(r["state"], r["qual"], lost[:12]), extra[:12])
            assert np.array_equal(res[0], exp) and res[1] == len(exp) > 0.005 * n, what


@pytest.mark.parametrize("variant,kernel", [(16, ROWS), (17, RUNS)])
def test_part_that_runs_full_after_the_first_iteration(forced, variant, kernel):
    """Case (c): 60 000 poly-A reads, none in the first iteration of the two writers: bucket 0's parts run full in a later group, and what
    spills is tested on the spot and resolved through the octet of ITS iteration."""
    gf = forced
    r = K.spill_case()
    gf.set_gaps(r["gaps"], r["n_scaffolds"], r["flanks"])
    gf.set_option("screen_pf4_writers", 2)
    d_reads = _upload(r["packed"])
    (_, res), = _forms(gf, d_reads, r["n"], 31, ((variant, False, kernel),))
    st = res[4]
    n_writers, cap, _, n_groups = st["shape"].tolist()
    assert n_writers == 2 and n_groups == r["state"]["n_groups"] > r["state"]["n_grp"] == 2, st["shape"]
    assert K.spill_facts(r["state"], cap)["first_full_group"] >= 2 and (st["count"][:2] == cap).all()
    lost, extra = np.setdiff1d(r["cand"], st["cand"]), np.setdiff1d(st["cand"], r["loose"])
    assert not len(lost) and not len(extra), (variant, W.homes(r["state"], W.candidates(r["packed"], L, 31, r["flanks"])[1], lost[:12]), extra[:12])
    exp = _oracle(r["blob"], r["flanks"], 31)
    assert np.array_equal(res[0], exp) and res[1] == len(exp) > 60000, variant


def test_full_home_groups_of_the_grouped_exact_set(forced):
    """Case (d): every 16-mer whose home group of four slots is the home of more than four keys is planted: at least one per such group
    lies in a later group and is found by the walk behind a full group of foreign keys."""
    gf = forced
    r = K.crowded_case()
    assert len(r["keys"]) >= 32
    n = r["case"]["packed"].shape[0]
    gf.set_gaps(r["draft"]["gaps"], r["draft"]["n_scaffolds"], r["draft"]["flanks"])
    exp = _oracle(r["case"]["blob"], r["draft"]["flanks"], 51)
    d_reads = _upload(r["case"]["packed"])
    for variant, res in _forms(gf, d_reads, n, 51, FORMS):
        _same_cand(res[4]["cand"], r, variant)
        assert np.array_equal(res[0], exp) and res[1] == len(exp) > 0.005 * n, variant
