"""The reads' probe column without a GPU: the exports, the geometry (library against the numpy twin) and the index arithmetic of a
column that passes 4 GiB."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import probe_column_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("gf_probe_geometry", "gf_probe_column_bytes", "gf_read_probes_dev", "gf_screen_reads_probes_dev")


def test_the_probe_column_entry_points_are_declared_and_exported():
    from gappadder_amd import _lib as B
    text = open(os.path.join(ROOT, "include", "gapfill_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\(" % name, text), name
        assert getattr(B.lib(), name).argtypes is not None, name
    assert C.sizeof(B.ProbeColumnGeom) == 40 and B.ProbeColumnGeom.n_reads.offset == 0 and B.ProbeColumnGeom.use.offset == 32


@pytest.mark.parametrize("L", [100, 101, 125, 150, 151, 250])
def test_geometry_of_the_library_equals_the_twin(L):
    from gappadder_amd import _lib as B
    for k in range(16, min(64, L) + 1):
        g = B.ProbeColumnGeom()
        assert B.lib().gf_probe_geometry(None, 1000, L, k, C.byref(g)) == 0
        assert (g.first, g.stride, g.np, g.ext) == T.geometry(L, k), (L, k)
        assert (g.n_reads, g.read_len, g.k) == (1000, L, k)
        rb = (L + 3) // 4
        assert bool(g.use) == (g.np <= 4 and 8 * g.np <= rb and rb <= 38), (L, k)     # at most half the row; rows the whole-line filter takes (these lengths: up to 38 bytes)
        assert B.lib().gf_probe_column_bytes(C.byref(g)) == 1024 * g.np * 4


def test_the_benchmark_geometries():
    assert T.geometry(150, 51) == (32, 34, 3, 2)          # 12 of 38 bytes: the column is taken
    assert T.geometry(150, 31)[2] == 8 and T.geometry(150, 41)[2] == 5     # 32 / 20 of 38 bytes: no column


def test_twin_words_on_known_reads():
    L, k = 150, 51
    rb = (L + 3) // 4
    packed = np.zeros((3, rb), dtype=np.uint8)            # poly-A: canonical form of AAAA... is itself (0)
    packed[1] = 0xFF                                      # poly-T: its reverse complement is poly-A
    packed[2] = 0x1B                                      # ACGT x n: its own reverse complement
    col = T.column(packed, L, k).reshape(3, 64)
    assert (col[:, 0] == 0).all() and (col[:, 1] == 0).all()
    assert (col[[0, 2], 2] == (0x1B1B1B1B * T.S16_MUL) & 0xFFFFFFFF).all()      # probes at bases 32 and 100: whole ACGT units
    assert (col[:, 3:] == 0).all()                        # the pad of the planes


def test_a_column_that_passes_4_GiB_is_indexed_in_64_bits():
    """C4's library: 900 M reads, three planes of 3.6 GB.  Plane 1 passes 4 GiB, plane 2 lies wholly beyond it; 32-bit arithmetic would wrap."""
    from gappadder_amd import _lib as B
    n = 900_000_000 + 37
    g = B.ProbeColumnGeom()
    assert B.lib().gf_probe_geometry(None, n, 150, 51, C.byref(g)) == 0 and g.np == 3 and g.use == 1
    plane = T.plane_words(n)
    assert plane % 64 == 0 and 0 <= plane - n < 64
    assert B.lib().gf_probe_column_bytes(C.byref(g)) == 3 * plane * 4 > 2 * (1 << 32)
    seen = set()
    for j in range(3):
        for r in (0, 63, 64, n - 1, (1 << 29) - 1, 1 << 29):
            w = T.word_index(n, r, j)
            assert w < 3 * plane and w not in seen
            seen.add(w)
            if j == 2:
                assert 4 * w >= 1 << 32 and (4 * w) & 0xFFFFFFFF != 4 * w     # a 32-bit byte offset would alias another word
    # a tile of 64 consecutive reads is 256 aligned contiguous bytes of every plane
    for t in (0, 1, (n - 1) // 64):
        for j in range(3):
            assert 4 * T.word_index(n, 64 * t, j) % 256 == 0
            assert T.word_index(n, 64 * t + 63, j) - T.word_index(n, 64 * t, j) == 63


def test_column_loads_are_not_touched_before_their_wait(tmp_path):
    """The column form of pass A loads its words with inline asm one iteration ahead; the compiler takes such a load for complete where
    it is issued.  tools/check_asm_load_wait.py reads the device assembly of all four instantiations: no load destination is read, copied
    or overwritten before the next counted wait.  The checker itself is shown a copy in front of the wait."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_asm_load_wait as CK
    bad = tmp_path / "bad.s"
    bad.write_text("pf4_scatter_col_kernel_x:\n\t;;#ASMSTART\n\tglobal_load_dword v29, v13, s[0:1]\n\t;;#ASMEND\n\tv_add_u32_e32 v1, v2, v3\n"
                   "\tv_mov_b32_e32 v3, v29\n\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n\tv_mov_b32_e32 v4, v29\n")
    n, _, found = CK.check(str(bad), "pf4_scatter_col_kernel")
    assert n == 1 and len(found) == 1 and "v29" in found[0]
    csrc = os.path.join(ROOT, "gappadder_amd", "csrc")
    out = tmp_path / "screen_pf4.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                           os.path.join(csrc, "screen_pf4.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    n, kernels, found = CK.check(str(out), "pf4_scatter_col_kernel")
    assert len(kernels) == 4 and n == 2 * 2 * (1 + 2 + 3 + 4), (n, kernels)      # prologue + loop, two tiles, G words each
    assert not found, found
