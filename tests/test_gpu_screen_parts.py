"""A library's resident parts on the GPU (gf_screen_parts_build_dev, gf_screen_reads_parts_dev): pass A alone leaves what a screen's pass A
leaves, a screen from the parts returns what a screen from the rows returns, nothing writes the parts, parts that do not fit the plan of a
call are refused, and the pipeline keeps and uses them.  Pair order inside a run differs from launch to launch: states are compared in
screen_state_util.filter_state's sorted-per-run form."""
import ctypes as C

import numpy as np
import pytest

import screen_cand_twin as W
import screen_parts_cases as P
import screen_passb_cases as K
from oracle import c_oracle as CO
from screen_state_util import build_column, dev, filter_state, screen

pytestmark = pytest.mark.gpu

L = K.L
PASS_A, COL, ROWS = "pf4_scatter", "pf4_scatter_col_kernel<", "pf4_scatter_lines_kernel<"
LATER = "pf4_probe_kernel,pf4_resolve_kernel,pf4_list_kernel"


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


def _build(gf, d_reads, n, k, d_col=None, geom=None):
    """(parts buffer, what it was built for, the kernel of the build) of gf_screen_parts_build_dev, from the column when one is given."""
    import torch
    from gappadder_amd import _lib as B
    want = B.ScreenPartsGeom()
    assert B.lib().gf_screen_parts_geometry(gf.handle, n, L, k, C.byref(want)) == 0
    d_parts = torch.full((max(1, B.lib().gf_screen_parts_bytes(C.byref(want)) // 4),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = B.ScreenPartsGeom()
    assert B.lib().gf_screen_parts_build_dev(gf.handle, d_reads.data_ptr(), d_col.data_ptr() if d_col is not None else None,
                                             C.byref(geom) if d_col is not None else None, n, L, k, d_parts.data_ptr(), C.byref(got)) == 0
    gf.sync()
    assert got.key() == want.key() and got.use <= want.use
    return d_parts, got, B.lib().gf_screen_kernels(gf.handle).decode()


def _parts_state(d_parts, g):
    """The parts buffer in filter_state's form: count, fills, and the pairs sorted inside every (part, group) run."""
    words = d_parts.cpu().numpy().view(np.uint32)
    parts = W.NB * g.n_writers
    at_fills, at_pairs, n_words = P.parts_layout(g.n_writers, g.cap, g.gs)
    assert len(words) == n_words
    count = words[:parts].copy()
    assert (count <= g.cap).all()
    fills = words[at_fills:at_fills + parts * g.gs].reshape(parts, g.gs)[:, :g.n_groups + 1].copy()
    pairs = words[at_pairs:at_pairs + parts * g.cap].reshape(parts, g.cap)
    part, pos = np.nonzero(np.arange(g.cap)[None, :] < count[:, None])
    big = np.int64(2 * g.cap + 2)
    bounds = (np.arange(parts, dtype=np.int64)[:, None] * big + fills[:, 1:]).ravel()
    run = np.searchsorted(bounds, part.astype(np.int64) * big + pos, side="right")
    pairs = pairs[part, pos]
    return {"shape": np.array([g.n_writers, g.cap, g.gs, g.n_groups]), "count": count, "fills": fills, "pairs": pairs[np.lexsort((pairs, run))], "runs": run}


def _screen_parts(gf, d_reads, n, k, d_parts, pgeom, d_col=None, geom=None, cap=1 << 21):
    """screen_state_util.screen through gf_screen_reads_parts_dev."""
    import torch
    from gappadder_amd import _lib as B
    d_out = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert B.lib().gf_screen_reads_parts_dev(gf.handle, d_reads.data_ptr(), None, d_col.data_ptr() if d_col is not None else None,
                                             C.byref(geom) if d_col is not None else None, d_parts.data_ptr() if d_parts is not None else None,
                                             C.byref(pgeom) if d_parts is not None else None, n, L, k, 1, d_out.data_ptr(), cap, d_n.data_ptr()) == 0
    gf.sync()
    dropped = C.c_size_t(0)
    assert B.lib().gf_screen_last_overflow(gf.handle, C.byref(dropped)) == 0
    n_hits = int(d_n[0].item())
    assert n_hits <= cap
    hits = d_out[:n_hits * 8].cpu().numpy().view(B.HIT)
    kernels = B.lib().gf_screen_kernels(gf.handle).decode()
    return np.sort(hits, order=("gap", "read")), n_hits, dropped.value, kernels, filter_state(gf) if "pf4_" in kernels else None


def _same_state(a, b, what, names=("shape", "count", "fills", "runs", "pairs")):
    for name in names:
        assert np.array_equal(a[name], b[name]), (what, name)


def _same_screen(got, rows, what, between=None):
    """Hits sorted, hit count, dropped count, and the candidate list.  between: (the twin's candidates, the twin's without the neighbour
    check) — with a short pair list, which pairs miss the list (and are then resolved without that check) is decided by the order of the
    waves' atomics, launch by launch: both lists lie between the twin's two."""
    assert np.array_equal(got[0], rows[0]) and got[1:3] == rows[1:3], (what, got[1:3], rows[1:3])
    if between is None:
        assert np.array_equal(got[4]["cand"], rows[4]["cand"]), what
    else:
        for res in (got, rows):
            lost, extra = np.setdiff1d(between[0], res[4]["cand"]), np.setdiff1d(res[4]["cand"], between[1])
            assert not len(lost) and not len(extra), (what, lost[:12], extra[:12])


def _from_parts(gf, d_reads, n, k, what, with_column=True, between=None):
    """Rows screen; parts built from the rows and from the column equal its state; the screen from either equals it and launches no pass A.
    Returns the rows screen and the parts built from the column."""
    rows = screen(gf, d_reads, n, L, k, None, None)
    assert rows[3].startswith(ROWS) and rows[2] == 0, (what, rows[3])
    d_col, geom = build_column(gf, d_reads, n, L, k)
    assert geom.use == 1, what
    built = []
    for col in ((False, True) if with_column else (False,)):
        d_parts, g, kernel = _build(gf, d_reads, n, k, d_col if col else None, geom if col else None)
        assert g.use == 1 and kernel.startswith(COL if col else ROWS), (what, col, kernel, g.use)
        _same_state(_parts_state(d_parts, g), rows[4], (what, col))
        got = _screen_parts(gf, d_reads, n, k, d_parts, g, d_col if col else None, geom if col else None)
        assert got[3] == LATER, (what, got[3])
        _same_state(got[4], rows[4], (what, col))      # (the view points at the resident parts)
        _same_screen(got, rows, (what, col), between)
        built.append((d_parts, g))
    return rows, built[-1]


@pytest.mark.parametrize("n", P.COUNTS)
def test_built_parts_equal_a_screens_parts_and_screen_alike(forced, n):
    gf = forced
    c, r = K.draft(), P.reads_for_both_drafts()
    gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
    d_reads = _upload(r["packed"][:n])
    rows, _ = _from_parts(gf, d_reads, n, 51, n)
    tw = W.pass_a_state(r["packed"][:n], L, 51, int(rows[4]["shape"][0]))
    _same_state(rows[4], tw, n, ("count", "fills", "runs", "pairs"))
    exp = _oracle(r["blob"][:n * L], c["flanks"], 51)
    assert np.array_equal(rows[0], exp) and (n < 2047 or len(exp) > 0), n


@pytest.mark.parametrize("n,writers", K.TRIP_RUNS)
def test_parts_of_several_trips(forced, n, writers):
    """Parts that take several trips of pass B with a tail trip (screen_passb_cases), with and without the neighbour check."""
    gf = forced
    c = K.draft()
    gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
    gf.set_option("screen_pf4_writers", writers)
    for ext in (1, 0):
        r = K.trip_run(n, writers, ext)
        gf.set_option("screen_ext", ext)
        rows, _ = _from_parts(gf, _upload(r["case"]["packed"]), n, 51, (n, writers, ext), with_column=ext == 1)
        assert rows[4]["shape"][0] == writers and (rows[4]["count"] > 1024).mean() > 0.9
        assert np.array_equal(rows[0], _oracle(r["case"]["blob"], c["flanks"], 51)) and rows[1] > 0.005 * n


@pytest.mark.parametrize("cap8", [256, 1024])
def test_short_pair_list_on_the_resident_fill_history(forced, cap8):
    """What does not fit a short pair list is resolved by its lane: the octet from the RESIDENT fill history (pf4_octet)."""
    gf = forced
    c, r = K.draft(), K.short_list_run(51)
    n = r["case"]["packed"].shape[0]
    gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
    gf.set_option("screen_pf4_writers", 1)
    gf.set_option("screen_pf4_cap8", cap8)
    rows, _ = _from_parts(gf, _upload(r["case"]["packed"]), n, 51, cap8, with_column=False, between=(r["cand"], r["loose"]))
    assert W.exact_set_pairs(rows[4]["pairs"], rows[4]["runs"], 1, int(rows[4]["shape"][3]), K.seeds(51)[0]) > 4 * cap8
    assert np.array_equal(rows[0], _oracle(r["case"]["blob"], c["flanks"], 51))


def test_one_set_of_parts_two_gap_sets(forced):
    """Built once, screened under draft A, draft B and A again: each screen equals the row-form screen under that draft, and the buffer is
    byte-identical before and after — nothing writes it."""
    import torch
    gf = forced
    a, b, r = K.draft(), P.draft_b(), P.reads_for_both_drafts()
    n = 40_003
    d_reads = _upload(np.concatenate([r["packed"][:n // 2], r["packed"][-(n - n // 2):]]))
    gf.set_gaps(a["gaps"], a["n_scaffolds"], a["flanks"])
    d_parts, g, _ = _build(gf, d_reads, n, 51)
    assert g.use == 1
    before = d_parts.clone()
    hits = []
    for c in (a, b, a):
        gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
        rows = screen(gf, d_reads, n, L, 51, None, None)
        got = _screen_parts(gf, d_reads, n, 51, d_parts, g)
        assert got[3] == LATER and rows[3].startswith(ROWS) and rows[1] > 0, (got[3], rows[3])
        _same_screen(got, rows, len(hits))
        hits.append(got[0])
    assert np.array_equal(hits[0], hits[2]) and not np.array_equal(hits[0], hits[1])
    assert torch.equal(before, d_parts)


def test_two_libraries_in_turn_on_one_context(forced):
    gf = forced
    c, r = K.draft(), P.reads_for_both_drafts()
    gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
    libs = []
    for lo, n in ((0, 30_011), (30_011, 10_002)):
        d_reads = _upload(r["packed"][lo:lo + n])
        rows = screen(gf, d_reads, n, L, 51, None, None)
        libs.append((d_reads, n, rows) + _build(gf, d_reads, n, 51)[:2])
    assert not np.array_equal(libs[0][2][0], libs[1][2][0])
    for _ in range(2):                                     # in turn: nothing of one library's screen is left for the other's
        for d_reads, n, rows, d_parts, g in libs:
            got = _screen_parts(gf, d_reads, n, 51, d_parts, g)
            assert got[3] == LATER, got[3]
            _same_screen(got, rows, n)


def test_stale_parts_are_refused_and_the_hits_are_right(forced):
    gf = forced
    c, r = K.draft(), P.reads_for_both_drafts()
    n = P.N_MAX
    gf.set_gaps(c["gaps"], c["n_scaffolds"], c["flanks"])
    d_reads = _upload(r["packed"])
    rows = screen(gf, d_reads, n, L, 51, None, None)
    assert rows[4]["shape"][0] > 2
    p61 = _build(gf, d_reads, n, 61)
    short = _build(gf, d_reads, n - 64, 51)
    gf.set_option("screen_pf4_writers", 2)
    two = _build(gf, d_reads, n, 51)
    gf.set_option("screen_pf4_writers", 0)
    for what, (d_parts, g, _) in (("k = 61", p61), ("n - 64 reads", short), ("two writers", two)):
        assert g.use == 1, what
        got = _screen_parts(gf, d_reads, n, 51, d_parts, g)
        assert PASS_A in got[3] and got[3].startswith(ROWS), (what, got[3])
        _same_screen(got, rows, what)
    # (and the same parts are taken where they fit)
    gf.set_option("screen_pf4_writers", 2)
    assert _screen_parts(gf, d_reads, n, 51, two[0], two[1])[3] == LATER


def test_a_part_that_runs_full(forced):
    """Poly-A reads under two writers at k = 51: bucket 0's parts run full.  The build has no index to test such a pair against: it counts
    them and reports use == 0; a screen handed those parts all the same takes today's path, and its hits are the oracle's."""
    gf = forced
    r = P.full_part_case()
    gf.set_gaps(r["gaps"], r["n_scaffolds"], r["flanks"])
    gf.set_option("screen_pf4_writers", 2)
    d_reads = _upload(r["packed"])
    d_parts, g, kernel = _build(gf, d_reads, r["n"], 51)
    assert kernel.startswith(ROWS) and g.n_writers == 2 and g.use == 0
    assert (r["state"]["count"][:2] > g.cap).all()                       # the twin's bucket 0: more pairs than a part holds
    got = _screen_parts(gf, d_reads, r["n"], 51, d_parts, g)
    assert got[3].startswith(ROWS) and (got[4]["count"][:2] == g.cap).all(), got[3]
    from gappadder_amd import _lib as B
    exp = np.sort(r["exp"].astype(B.HIT), order=("gap", "read"))
    assert np.array_equal(got[0], exp) and got[1] == len(exp) >= 6000 and got[2] == 0


def _canonical(res):
    """A fetched step in a form two runs can be compared by: the device lists contigs in no fixed order, so the contigs (record fields and
    bases) sorted, and every closed gap's pick word with the picked contig itself in place of its index."""
    ctg, seq = res.contigs, res.seq
    rows = [(int(c["gap"]), int(c["k"]), int(c["kv"]), int(c["n_nodes"]), int(c["cov_sum"]), seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])])
            for c in ctg]
    picks = []
    for g in np.nonzero(res.best)[0]:
        b = int(res.best[g])
        picks.append((int(g), b >> 56, (b >> 32) & 0xFFFFFF, b & 1, rows[0x7FFFFFFF - ((b >> 1) & 0x7FFFFFFF)]))
    return sorted(rows), picks, (res.best != 0).tobytes(), len(seq)


def test_pipeline_keeps_and_uses_the_parts(forced):
    """The C3-sized draft of test_gpu_probe_column.py: pipelines with and without screen_parts give the same contigs, bases and pick words."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    gf = forced
    cfg = GapFill.synth_cfg(seed=20260003, scaffold_len=4_600_000, n_scaffolds=1, gaps_per_scaffold=200, gap_len=1000)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf.set_gaps(gaps, 1, flanks)
    n = 2_000_000
    d_reads = torch.empty(n * B.lib().gf_packed_read_bytes(150) + 64, dtype=torch.uint8, device="cuda")
    d_recs = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg, 0, n // 2, d_reads.data_ptr(), d_recs.data_ptr())
    gf.sync()
    out = {}
    for on in (True, False):
        pipe = Pipeline(gf, len(gaps), 150, [(51, 49)], screen_parts=on)
        lb = pipe.add_library(DeviceLibrary("lib0", 300, 30, n, d_reads, d_recs))
        assert (lb.d_parts is not None) == on and lb.d_probes is not None and lb.probe_geom.k == 51 and lb.probe_geom.use == 1
        assert not on or (lb.parts_geom.use == 1 and 4 * lb.d_parts.numel() == B.lib().gf_screen_parts_bytes(C.byref(lb.parts_geom)))
        pipe.prepare()
        pipe.step(2)
        res = pipe.fetch()
        assert (B.lib().gf_screen_kernels(gf.handle).decode() == LATER) == on
        out[on] = _canonical(res) + (lb.counts["screen_hits"],)
        assert res.n_contigs > 0 and len(res.seq) > 0 and lb.counts["screen_hits"] > 0      # (1-kb gaps under a 300-base insert: none closes)
    assert out[True] == out[False]
    assert Pipeline(gf, len(gaps), 150, [(51, 49)]).add_library(DeviceLibrary("lib0", 300, 30, n, d_reads, d_recs)).d_parts is not None      # the default
