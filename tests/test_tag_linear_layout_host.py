"""The tagger's linear layout (gf_tag_layout): gf_tag_layout_from_ends against a numpy twin written from the header's words, and the
linearisation of records under it (no GPU: the layout is host arithmetic, the twin is numpy)."""
import ctypes as C

import numpy as np
import pytest

import tag_linear_twin as T


def _native(ends, n_recs):
    from gappadder_amd import _lib as B
    ends = np.ascontiguousarray(ends, dtype=np.uint32)
    lay = B.TagLayout()
    base = np.full(len(ends) + 1, 0x55555555, dtype=np.uint32)
    assert B.lib().gf_tag_layout_from_ends(B._p(ends) if len(ends) else None, len(ends), n_recs, C.byref(lay), B._p(base)) == 0
    return lay, base


def _same(lay, base, want):
    assert lay.use == want["use"] and lay.n_recs == want["n_recs"] and lay.n_scaffolds == want["n_scaffolds"]
    if want["use"]:
        assert (lay.granule_log2, lay.span, lay.checksum) == (want["granule_log2"], want["span"], want["checksum"])
        assert (base == want["base"]).all()


def test_struct_matches_the_header():
    from gappadder_amd import _lib as B
    assert C.sizeof(B.TagLayout) == 40 and B.TagLayout.checksum.offset == 16 and B.TagLayout.use.offset == 32
    for n, ns in ((0, 1), (1, 3), (255, 3), (256, 620), (257, 1), (1025, 2049)):
        assert B.lib().gf_alnrec_linkeys_bytes(n, ns) == 4 * T.parts(n, ns)[4] == 4 * B.linkeys_layout(n, ns)[4]
        assert B.linkeys_layout(n, ns) == T.parts(n, ns)


def test_bases_are_the_prefix_sums_of_the_ends_rounded_up_to_a_granule():
    """Ends of 1 base, one granule plus 1, and a non-multiple of the granule: 1, 2 and 4 granules of 2^20."""
    g = 1 << 20
    ends = [1, g + 1, 3 * g + 12345]
    lay, base = _native(ends, 77)
    _same(lay, base, T.layout(ends, 77))
    assert lay.use == 1 and lay.granule_log2 == 20 and base.tolist() == [0, g, 3 * g, 7 * g] and lay.span == 7 * g
    # an end that is a whole number of granules takes exactly that many; a scaffold without records takes none
    lay, base = _native([g, 0, 2 * g, 0], 5)
    assert base.tolist() == [0, g, g, 3 * g, 3 * g]
    _same(lay, base, T.layout([g, 0, 2 * g, 0], 5))
    lay, base = _native([], 0)
    assert lay.use == 1 and lay.span == 0 and base[0] == 0


def test_sentinel_for_what_takes_no_part_and_no_key_reaches_it():
    from gappadder_amd import _lib as B
    ns = 3
    recs = np.zeros(7, dtype=B.ALNREC)
    recs["ref"] = [0, 1, 2, 0xFFFFFFFF, ns, 2, ns + 5]
    recs["pos"] = [0, 9, (1 << 20) + 3, 4, 5, 0, 6]
    recs["mapq"] = [0, 30, 0, 0, 0, 7, 0]
    ends = T.ends_of(recs, ns)
    assert ends.tolist() == [1, 10, (1 << 20) + 4]
    want = T.layout(ends, len(recs))
    lay, base = _native(ends, len(recs))
    _same(lay, base, want)
    keys, plane = T.column(recs, ns, base)
    g = 1 << 20
    assert keys.tolist() == [0, g + 9, 2 * g + g + 3, T.SENTINEL, T.SENTINEL, 2 * g, T.SENTINEL] + [T.SENTINEL] * 5       # 7 -> 8 keys + 4
    assert plane.tolist() == [0b101] + [0] * 7                                                                             # records 0 and 2
    # every key lies below the line's end, and the line ends a granule short of 2^32: the sentinel's bin is behind every bin of every map
    assert int(keys[keys != T.SENTINEL].max()) < lay.span < (1 << 32) - (1 << lay.granule_log2)


def test_a_draft_beyond_32_bits_keeps_no_linear_column():
    """Three scaffolds with one record each near position 2^31: no granule fits the line into 32 bits."""
    ends = [(1 << 31) - 5, (1 << 31) + 1, (1 << 31) - 100]
    lay, _ = _native(ends, 3)
    assert lay.use == 0 and T.layout(ends, 3)["use"] == 0
    # at the bound itself: the line must stay BELOW 2^32 - 2^A
    g = 1 << 20
    lay, _ = _native([(1 << 32) - 2 * g], 1)              # span 2^32 - 2 g < 2^32 - g
    assert lay.use == 1 and lay.granule_log2 == 20 and lay.span == (1 << 32) - 2 * g
    for end in ((1 << 32) - 2 * g + 1, 0xFFFFFFFF):        # span 2^32 - g with A = 20, and as little short of 2^32 with every smaller A
        lay, _ = _native([end], 1)
        assert lay.use == T.layout([end], 1)["use"]
        assert lay.use == 0 or lay.span < (1 << 32) - (1 << lay.granule_log2)
    assert _native([0xFFFFFFFF], 1)[0].use == 0


@pytest.mark.parametrize("n_scaf,end,granule", [(5000, 100_000, 19), (100_000, 3000, 15), (620, 5_000_000, 20)])
def test_many_small_scaffolds_take_a_smaller_granule(n_scaf, end, granule):
    ends = [end] * n_scaf
    lay, base = _native(ends, 10)
    want = T.layout(ends, 10)
    _same(lay, base, want)
    assert lay.use == 1 and lay.granule_log2 == granule
    assert n_scaf << (granule + 1) >= (1 << 32) - (2 << granule) or granule == 20       # the next larger granule does not fit
    assert lay.span < (1 << 32) - (1 << granule) and (base[:-1].astype(np.int64) % (1 << granule) == 0).all()
    assert (lay.span >> granule) + 1 <= 1 << 17                                          # 2^17 bins no wider than a granule cover the line
