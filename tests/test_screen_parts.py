"""A library's resident parts (pass A's output kept across screens) without a GPU: the exports, the geometry against the twin's plan, the
size of the buffer, and where parts are kept."""
import ctypes as C
import os
import re

import pytest

import screen_cand_twin as W
import screen_parts_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("gf_screen_parts_geometry", "gf_screen_parts_bytes", "gf_screen_parts_build_dev", "gf_screen_reads_parts_dev")
N_CU = 256          # a null context plans for 256 CUs (include/gapfill_hip.h)


def _geom(n, L, k):
    from gappadder_amd import _lib as B
    g = B.ScreenPartsGeom()
    assert B.lib().gf_screen_parts_geometry(None, n, L, k, C.byref(g)) == 0
    return g


def test_the_parts_entry_points_are_declared_and_exported():
    from gappadder_amd import _lib as B
    text = open(os.path.join(ROOT, "include", "gapfill_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\(" % name, text), name
        assert getattr(B.lib(), name).argtypes is not None, name
    assert C.sizeof(B.ScreenPartsGeom) == 72 and B.ScreenPartsGeom.probe.offset == 0 and B.ScreenPartsGeom.n_writers.offset == 40
    assert B.ScreenPartsGeom.use.offset == 64


@pytest.mark.parametrize("n", [1, 2048, 2049, 3_000_000, 900_000_000])
def test_geometry_of_the_library_equals_the_twins_plan(n):
    from gappadder_amd import _lib as B
    g = _geom(n, 150, 51)
    p = W.plan(n, 150, 51, N_CU, 0)
    assert (g.n_writers, g.cap, g.gs, g.n_groups) == (p["n_writers"], p["cap"], p["gs"], p["n_groups"]), (n, p)
    assert (g.n_grp, g.tiles_wg) == (p["n_grp"], 32) and g.use == 1
    pg = B.ProbeColumnGeom()
    assert B.lib().gf_probe_geometry(None, n, 150, 51, C.byref(pg)) == 0
    assert g.probe.key() == pg.key() and g.probe.use == pg.use == 1
    # one buffer: the counts (rounded up to 256 bytes), the fill history, the pairs and the 64 words behind them
    count_b, fill_b, pair_b = (256 * g.n_writers * 4 + 255) // 256 * 256, 256 * g.n_writers * g.gs * 4, 256 * g.n_writers * g.cap * 4 + 256
    assert B.lib().gf_screen_parts_bytes(C.byref(g)) == count_b + fill_b + pair_b == 4 * P.parts_layout(g.n_writers, g.cap, g.gs)[2]


def test_the_parts_of_the_default_benchmark_pass_4_GiB():
    from gappadder_amd import _lib as B
    g = _geom(900_000_000, 150, 51)
    nbytes = B.lib().gf_screen_parts_bytes(C.byref(g))
    assert g.n_writers == 256 and nbytes > 1 << 32
    assert 11.0e9 < 256 * 256 * g.cap * 4 < 12.5e9 and nbytes < 13.0e9
    assert 256 * g.n_writers * (g.cap >> 5) + 1 < 0xFFFFFFFF     # a line's index in the pairs fits 32 bits


@pytest.mark.parametrize("k,use", [(31, 0), (41, 0), (51, 1), (61, 1)])
def test_parts_are_kept_where_a_column_is(k, use):
    from gappadder_amd import _lib as B
    g = _geom(3_000_000, 150, k)
    assert g.use == use == g.probe.use, (k, g.use, g.probe.use)
    assert g.probe.np == W.T.geometry(150, k)[2]
    assert (B.lib().gf_screen_parts_bytes(C.byref(g)) > 0) == bool(g.n_writers)
