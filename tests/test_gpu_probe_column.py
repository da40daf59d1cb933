"""The reads' probe column on the GPU: the stand-alone producer against the numpy twin, and the screen from the column against the screen
from the packed rows — same process, same inputs, identical hits, counts and overflow counters."""
import ctypes as C

import numpy as np
import pytest

import probe_column_twin as T
import synth_small as S
from screen_state_util import build_column as _build, dev as _dev, screen as _screen

pytestmark = pytest.mark.gpu

COL, ROWS = "pf4_scatter_col_kernel<", "pf4_scatter_lines_kernel<"


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


@pytest.fixture(autouse=True)
def diagnostics(gf, monkeypatch):
    """The filter's workspace and a copy of its candidate list are readable (gf_screen_debug_view)."""
    monkeypatch.setenv("GF_DIAGNOSTICS", "1")
    gf.set_option("screen_keep_cand", 1)
    yield
    gf.set_option("screen_keep_cand", 0)


@pytest.fixture()
def forced(gf):
    """The partitioned filter on small inputs too (2^27-bit level-1 bitmap, variant 16); the defaults afterwards."""
    gf.set_option("bitmap_log2", 27)
    gf.set_option("screen_variant", 16)
    yield gf
    gf.set_option("screen_variant", 0)
    gf.set_option("bitmap_log2", 0)
    gf.set_option("screen_ext", 1)


def _both_forms_agree(gf, d_reads, n, L, k, want_col=True, cap=1 << 21):
    d_col, geom = _build(gf, d_reads, n, L, k)
    assert bool(geom.use) == want_col, (L, k, geom.key())
    rows = _screen(gf, d_reads, n, L, k, None, None, cap)
    col = _screen(gf, d_reads, n, L, k, d_col, geom, cap)
    assert (COL in col[3]) == want_col and COL not in rows[3], (col[3], rows[3])
    assert not geom.use or col[3].startswith(COL), col[3]      # `use` and the screen read the same plan: a wanted column, handed over, is streamed
    assert np.array_equal(rows[0], col[0]) and rows[1:3] == col[1:3], (L, k, n, rows[1:3], col[1:3])
    assert (rows[4] is None) == (col[4] is None)
    if rows[4] is not None:      # pass A's pairs and fill history, and the candidate list: the same arrays from both forms
        for name in ("shape", "count", "fills", "runs", "pairs", "cand"):
            assert np.array_equal(rows[4][name], col[4][name]), (L, k, n, name)
        assert len(rows[4]["cand"]) >= len(np.unique(rows[0]["read"])) and rows[4]["count"].sum() == len(rows[4]["pairs"]) > 0
    return rows, d_col, geom


@pytest.mark.parametrize("L", [100, 150, 151])
@pytest.mark.parametrize("k", [41, 51, 63])
def test_standalone_column_equals_the_twin(gf, L, k):
    """gf_read_probes_dev against the definition, word for word, pad included: read counts that are no multiple of 64, of the producer's
    256-read tile or of pass A's 2 048-read batch, and a single read."""
    import torch
    rb = (L + 3) // 4
    rng = np.random.default_rng(1000 * L + k)
    for n in (1, 63, 64, 257, 2048 + 65, 10_007):
        packed = rng.integers(0, 256, size=(n, rb), dtype=np.uint8)
        d_reads = torch.cat([_dev(packed), torch.zeros(64, dtype=torch.uint8, device="cuda")])
        d_col, geom = _build(gf, d_reads, n, L, k)
        assert (geom.first, geom.stride, geom.np, geom.ext) == T.geometry(L, k)
        got = d_col.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, T.column(packed, L, k)), (L, k, n)


def _synth(gf, cfg, n_pairs, L):
    import torch
    from gappadder_amd import _lib as B
    rb = B.lib().gf_packed_read_bytes(L)
    d_reads = torch.empty(2 * n_pairs * rb + 64, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg, 0, n_pairs, d_reads.data_ptr())
    gf.sync()
    return d_reads


def test_c3_sized_library_both_forms(forced):
    """BASELINE configs[2]'s draft and 5 M reads.  At its own k = 41 a read has five probes (20 of 38 bytes): no column, the rows as before;
    at k = 51 and 61 (three and two probes) the column form runs and returns what the row form returns."""
    from gappadder_amd.hip_api import GapFill
    gf = forced
    cfg = GapFill.synth_cfg(seed=20260003, scaffold_len=4_600_000, n_scaffolds=1, gaps_per_scaffold=200, gap_len=1000)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf.set_gaps(gaps, 1, flanks)
    n = 5_000_000
    d_reads = _synth(gf, cfg, n // 2, 150)
    rows41, _, _ = _both_forms_agree(gf, d_reads, n, 150, 41, want_col=False)
    assert rows41[1] > 50_000
    for k in (51, 61):
        rows, _, _ = _both_forms_agree(gf, d_reads, n, 150, k)
        assert rows[1] > 10_000
    _both_forms_agree(gf, d_reads, n - 2049, 150, 51)          # ends inside a tile, an octet and a batch
    gf.set_option("screen_ext", 0)                              # 16-base seeds: another stride, another column
    _both_forms_agree(gf, d_reads, n, 150, 51)


def test_c2_sized_library_and_planted_repeats_both_forms(forced):
    """BASELINE configs[1]'s draft (1 000 gaps) with 6 M of its reads, then the same draft with planted repeats (reads that hit up to 50
    gaps: the verification's large lists and overflow counters)."""
    from gappadder_amd.hip_api import GapFill
    gf = forced
    for period in (0, 8):
        cfg = GapFill.synth_cfg(seed=20260002, scaffold_len=5_000_000, n_scaffolds=50, gaps_per_scaffold=20, gap_len=2000, repeat_period=period)
        gaps, flanks = GapFill.synth_layout(cfg)
        gf.set_gaps(gaps, 50, flanks)
        n = 6_000_000
        d_reads = _synth(gf, cfg, n // 2, 150)
        rows, _, _ = _both_forms_agree(gf, d_reads, n, 150, 51, cap=1 << 23)
        assert rows[1] > 10_000, period


def test_small_key_set_under_the_automatic_choice_keeps_no_column(gf):
    """Without the forced filter a C2-sized key set takes the pipelined kernel: the geometry says so (`use` = 0), the pipeline builds no
    column, and a column handed in all the same is not streamed."""
    from gappadder_amd.hip_api import GapFill
    cfg = GapFill.synth_cfg(seed=20260002, scaffold_len=5_000_000, n_scaffolds=50, gaps_per_scaffold=20, gap_len=2000)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf.set_gaps(gaps, 50, flanks)
    n = 2_000_000
    d_reads = _synth(gf, cfg, n // 2, 150)
    rows, _, _ = _both_forms_agree(gf, d_reads, n, 150, 51, want_col=False)
    assert "pf4_" not in rows[3]


def test_sparse_key_set_with_a_large_bitmap_keeps_no_column(gf):
    """A 2^27-bit level-1 bitmap and 2^20 reads make the partitioned filter eligible, yet a key set this sparse (100 gaps) takes the
    pipelined kernel all the same.  `use` says so — no column is built for a screen that would never stream it — and a column handed in all
    the same is not streamed; the hits are those of the rows."""
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    gf.set_option("bitmap_log2", 27)
    try:
        cfg = GapFill.synth_cfg(seed=20260005, scaffold_len=5_000_000, n_scaffolds=5, gaps_per_scaffold=20, gap_len=2000)
        gaps, flanks = GapFill.synth_layout(cfg)
        gf.set_gaps(gaps, 5, flanks)
        n = (1 << 20) + 130
        d_reads = _synth(gf, cfg, n // 2, 150)
        g = B.ProbeColumnGeom()
        assert B.lib().gf_probe_geometry(gf.handle, n, 150, 51, C.byref(g)) == 0
        assert g.use == 0 and (g.first, g.stride, g.np, g.ext) == T.geometry(150, 51)
        rows, _, _ = _both_forms_agree(gf, d_reads, n, 150, 51, want_col=False)
        assert rows[3].startswith("screen_filter_pipe_kernel<") and rows[1] > 0, rows[3]
    finally:
        gf.set_option("bitmap_log2", 0)


def test_two_libraries_and_a_column_built_for_another_k(forced):
    """Two libraries of different sizes screened in turn on one context, each from its own column; then library 0's column for k = 61 handed to
    a k = 51 screen: refused (the rows are read, the hits are right), and Pipeline.add_library replaces it by one for its own k."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    gf = forced
    cfg = GapFill.synth_cfg(seed=20260003, scaffold_len=4_600_000, n_scaffolds=1, gaps_per_scaffold=200, gap_len=1000)
    cfg1 = GapFill.synth_cfg(seed=20260003, scaffold_len=4_600_000, n_scaffolds=1, gaps_per_scaffold=200, gap_len=1000, library=1,
                             insert_mean=5000, insert_sd=500)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf.set_gaps(gaps, 1, flanks)
    n0, n1 = 3_000_000, 1_000_002
    d0, d1 = _synth(gf, cfg, n0 // 2, 150), _synth(gf, cfg1, n1 // 2, 150)
    rows0, col0, g0 = _both_forms_agree(gf, d0, n0, 150, 51)
    rows1, col1, g1 = _both_forms_agree(gf, d1, n1, 150, 51)
    assert not np.array_equal(rows0[0], rows1[0])
    for _ in range(2):                                     # in turn: nothing of one library's pass is left for the other's
        a, b = _screen(gf, d0, n0, 150, 51, col0, g0), _screen(gf, d1, n1, 150, 51, col1, g1)
        assert COL in a[3] and COL in b[3]
        assert np.array_equal(a[0], rows0[0]) and a[1:3] == rows0[1:3] and np.array_equal(b[0], rows1[0]) and b[1:3] == rows1[1:3]
    # a column of another k, and one of another read count
    col61, g61 = _build(gf, d0, n0, 150, 61)
    stale = _screen(gf, d0, n0, 150, 51, col61, g61)
    assert ROWS in stale[3] and COL not in stale[3] and np.array_equal(stale[0], rows0[0]) and stale[1:3] == rows0[1:3]
    short = _screen(gf, d0, n0 - 64, 150, 51, col0, g0)
    assert ROWS in short[3] and COL not in short[3]
    # the pipeline: a library that brings the k = 61 column gets one for the pipeline's k
    recs = torch.zeros(32 * n0, dtype=torch.uint8, device="cuda")
    pipe = Pipeline(gf, len(gaps), 150, [(51, 49)])
    lb = pipe.add_library(DeviceLibrary("lib0", 300, 30, n0, d0, recs, d_probes=col61, probe_geom=g61))
    assert lb.probe_geom.k == 51 and lb.probe_geom.use == 1
    assert np.array_equal(lb.d_probes.cpu().numpy(), col0.cpu().numpy())
    lb2 = Pipeline(gf, len(gaps), 150, [(51, 49)], probe_column=False).add_library(DeviceLibrary("lib0", 300, 30, n0, d0, recs))
    assert lb2.d_probes is None


def test_column_beyond_4_GiB_on_the_device(gf):
    """A library whose column passes a 4 GiB byte offset: 600 M + 37 synthetic reads at k = 51 (three planes of 2.4 GB; plane 2 starts beyond
    4 GiB, plane 1 passes it, the packed rows pass it five times).  Stripes of the column against the twin — the first and last tiles of every plane, and
    the words on both sides of the 4 GiB offset."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    L, k, n = 150, 51, 600_000_000 + 38
    rb = B.lib().gf_packed_read_bytes(L)
    cfg = GapFill.synth_cfg(seed=20260004, scaffold_len=5_000_000, n_scaffolds=620, gaps_per_scaffold=32, gap_len=2000)
    d_reads = _synth(gf, cfg, n // 2, L)
    n -= 1                                                  # an odd read count: the planes end inside a tile
    d_col, geom = _build(gf, d_reads, n, L, k)
    plane = T.plane_words(n)
    assert geom.np == 3 and 2 * plane * 4 > 1 << 32 and d_col.numel() == 3 * plane
    col = d_col.view(3, plane)
    r4g = (1 << 32) // 4 - plane                            # the read of plane 1 whose word starts at byte 4 GiB
    assert 0 < r4g < n
    for r0 in (0, r4g - 640, (1 << 32) // rb - 320, n - 700):
        r0 -= r0 % 64
        r1 = min(n, r0 + 1280)
        packed = d_reads[r0 * rb:r1 * rb].cpu().numpy().reshape(-1, rb)
        want = T.column(packed, L, k).reshape(3, -1)[:, :r1 - r0]
        assert np.array_equal(col[:, r0:r1].cpu().numpy().view(np.uint32), want), r0
    assert (col[:, n:] == 0).all()
