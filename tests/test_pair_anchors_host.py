"""The host twin of the anchored pair span (gappadder_amd/pair_anchors.py) against expectations written out by hand from
planted coordinates: a random contig of 1 200 bases with the body [400, 800), a gap at [10 000, 10 400) of the draft, reads of 100 bases
that are exact windows of the contig (strand 0) or their reverse complements (strand 1), and anchors given as draft coordinates.  Nothing
here goes through the twin's own helpers: every expected number is a literal derived in the comment next to it."""
import numpy as np
import pytest

L, N, B0, B1, START, END = 100, 1200, 400, 800, 10000, 10400
_RNG = np.random.default_rng(20)
CONTIG = "".join("ACGT"[i] for i in _RNG.integers(0, 4, N))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _row(strand, d, contig=CONTIG):
    """The row that places at (strand, d): the window as stored, or its reverse complement."""
    w = contig[d:d + L]
    assert len(w) == L
    return _rc(w) if strand else w


def _run(pairs, rev=0, is_mean=1000, is_sd=10, z=3, min_pairs=1, contig=CONTIG, body=(B0, B1)):
    """pairs: (A0, sA, strand of B, diagonal of B) or (None, read text): the twin's record."""
    from gappadder_amd import pair_anchors as PA
    reads = [p[1] if p[0] is None else _row(p[2], p[3], contig) for p in pairs]
    anchors = [None if p[0] is None else (p[0], p[1]) for p in pairs]
    ids = [2 * i + 1 for i in range(len(pairs))]
    return PA.anchors_host(reads, ids, anchors, contig, body[0], body[1], rev, (START, END), is_mean, is_sd, z=z, min_pairs=min_pairs, L=L)


def _is(rec, **want):
    got = {k: int(rec[k]) for k in want}
    assert got == want


def test_left_and_right_anchors_forward_word():
    rec = _run([
        (START - 300, 0, 1, 1000),   # left, forward: column 400 - 300 = 100; B reverse at 1000: insert 1000 + 100 - 100 = 1000, dev 0; spans; covers [100, 1100)
        (END + 500, 1, 0, 390),      # right, reverse: column 800 + 500 = 1300 > n; B forward at 390: insert 1300 + 100 - 390 = 1010, dev 10; spans; covers [390, 1200)
        (START - 300, 1, 1, 1000),   # left, reverse and B reverse: same strand, misoriented
        (START - 100, 0, 1, 700),    # column 300, B reverse at 700: insert 500, short; 300 <= 400 and 800 <= 800: spans
        (START - 390, 0, 1, 1100),   # column 10, B reverse at 1100 (ends at n): insert 1190, long; spans
        (END + 10, 0, 1, 900),       # right, forward: column 810, B reverse at 900: proper (810 <= 900), insert 190, short; 810 > 400: no span
        (END + 600, 0, 1, 900),      # right, forward: column 1400 > 900 = d_r: misoriented
    ])
    _is(rec, flags=0, rows=7, n_anchored=7, n_placed=7, n_proper=5, n_misoriented=2, n_in_range=2, n_short=2, n_long=1, n_left=1, n_span=4,
        span_insert_sum=1000 + 1010 + 500 + 1190, dev_sum=10, n_cols=400, min_cover=2, min_col=400, n_unspanned=0, n_eval=400,
        # both in-range pairs cover every body column: the mean is 10 / 2 everywhere, and the smallest column wins either extreme
        dev_min_col=400, dev_min_n=2, dev_min_sum=10, dev_max_col=400, dev_max_n=2, dev_max_sum=10)


def test_left_and_right_anchors_reverse_word():
    rec = _run([
        (START - 300, 0, 0, 100),    # left, forward -> strand 1, column 800 + 300 - 100 = 1000; B forward at 100: insert 1000 + 100 - 100 = 1000; covers [100, 1100)
        (END + 290, 1, 1, 920),      # right, reverse -> strand 0, column 400 - 290 - 100 = 10; B reverse at 920: insert 920 + 100 - 10 = 1010; covers [10, 1020)
        (START - 300, 0, 1, 100),    # left, forward -> strand 1, B on strand 1 too: misoriented
        (END + 290, 1, 0, 920),      # right -> strand 0, B on strand 0: misoriented
    ], rev=1)
    _is(rec, n_anchored=4, n_placed=4, n_proper=2, n_misoriented=2, n_in_range=2, n_left=1, n_span=2, span_insert_sum=2010, dev_sum=10,
        min_cover=2, min_col=400, n_unspanned=0, n_eval=400, dev_min_col=400, dev_min_n=2, dev_min_sum=10, dev_max_col=400, dev_max_sum=10)


def test_columns_far_outside_the_contig():
    rec = _run([
        (START - 1500, 0, 1, 800),   # column 400 - 1500 = -1100 < -1024; B reverse at 800: insert 800 + 100 + 1100 = 2000; covers [0, 900)
        (END + 1100, 1, 0, 0),       # column 800 + 1100 = 1900 > n; B forward at 0: insert 1900 + 100 - 0 = 2000; covers [0, 1200)
        (END + 1000, 1, 0, 0),       # column 1800: insert 1900 <= lo = 1970: short, spans
    ], is_mean=2000)
    _is(rec, n_placed=3, n_proper=3, n_in_range=2, n_short=1, n_long=0, n_left=1, n_span=3, span_insert_sum=5900, dev_sum=0, min_cover=2,
        min_col=400, n_unspanned=0, n_eval=400, dev_min_col=400, dev_min_n=2, dev_min_sum=0)


def test_strict_bounds():
    # lo = 970, hi = 1030; the left anchor at column 100
    rec = _run([(START - 300, 0, 1, 970 - 100 + 100), (START - 300, 0, 1, 971), (START - 300, 0, 1, 1029), (START - 300, 0, 1, 1030)])
    # inserts 970 + 100 - 100 = 970 (short: not above lo), 971, 1029 (in range), 1030 (long: not below hi)
    _is(rec, n_proper=4, n_short=1, n_in_range=2, n_long=1, dev_sum=(971 - 1000) + (1029 - 1000), n_span=4, min_cover=2)


def _deleted(delta):
    """Seven pairs whose true insert is exactly 1 000 on a fill that is `delta` bases short (delta < 0: long) at column 600: three of them
    have B left of the defect (B reverse at 450, ends at 550: insert 1 000 from column -450), four have B right of it (B reverse at 700,
    ends at 800: the anchor's column is 800 - 1 000 + delta)."""
    return [(START - 850, 0, 1, 450)] * 3 + [(START - (400 - (800 - 1000 + delta)), 0, 1, 700)] * 4


def test_sixty_bases_deleted():
    rec = _run(_deleted(60), z=7, min_pairs=4)
    # [400, 550): 7 pairs with a sum of 4 * -60; [550, 800): the 4 pairs over the defect alone, every one 60 short
    _is(rec, n_in_range=7, n_left=7, dev_sum=-240, min_cover=4, min_col=550, n_unspanned=0, n_eval=400, dev_min_col=550, dev_min_n=4,
        dev_min_sum=-60 * 4, dev_max_col=400, dev_max_n=7, dev_max_sum=-240)
    assert int(rec["dev_min_sum"]) == -60 * int(rec["dev_min_n"])
    # a cover of min_pairs counts, a cover of min_pairs - 1 does not
    rec = _run(_deleted(60), z=7, min_pairs=5)
    _is(rec, n_eval=150, dev_min_col=400, dev_min_n=7, dev_min_sum=-240, dev_max_col=400, dev_max_n=7)
    rec = _run(_deleted(60), z=7, min_pairs=8)
    _is(rec, n_in_range=7, n_eval=0, dev_min_col=0, dev_min_n=0, dev_min_sum=0, dev_max_col=0, dev_max_n=0, dev_max_sum=0)
    # z = 3: the four pairs over the defect are short (940 <= 970) and the columns behind 550 are not covered
    rec = _run(_deleted(60), z=3, min_pairs=1)
    _is(rec, n_in_range=3, n_short=4, min_cover=0, min_col=550, n_unspanned=250, n_eval=150, dev_min_sum=0)


def test_forty_bases_inserted():
    rec = _run(_deleted(-40), z=7, min_pairs=4)
    _is(rec, n_in_range=7, dev_sum=160, n_eval=400, dev_max_col=550, dev_max_n=4, dev_max_sum=40 * 4, dev_min_col=400, dev_min_n=7, dev_min_sum=160)


def test_equal_means_the_smaller_column_wins():
    # is_mean 400: the anchors at column 100 with B reverse at 390 and 410: inserts 390 and 410, dev -10 and +10, covers [100, 490) and
    # [100, 510); a third anchor at column 400 - 200 = 200 with B at 1000: insert 900, long
    rec = _run([(START - 300, 0, 1, 390), (START - 300, 0, 1, 410), (START - 200, 0, 1, 1000)], min_pairs=1, is_mean=400)
    # the columns 400..489 hold both pairs (mean 0: the first of them is the smallest mean), 490..509 the second alone (mean 10), 510.. none
    _is(rec, n_in_range=2, n_long=1, n_eval=110, dev_min_col=400, dev_min_n=2, dev_min_sum=0, dev_max_col=490, dev_max_n=1, dev_max_sum=10,
        min_cover=0, min_col=510, n_unspanned=290)
    rec = _run([(START - 300, 0, 1, 390), (START - 300, 0, 1, 410), (START - 300, 0, 1, 400)], min_pairs=3, is_mean=400)
    # a third pair with dev 0 over [100, 500): cover 3 and mean 0 on [400, 490) only: both extremes at 400
    _is(rec, n_in_range=3, n_eval=90, dev_min_col=400, dev_min_n=3, dev_min_sum=0, dev_max_col=400, dev_max_n=3, dev_max_sum=0)


def test_ambiguous_unplaced_and_unanchored_rows():
    rng = np.random.default_rng(21)
    seq = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    rep = seq(200)
    contig = seq(300) + rep + rep + seq(500)
    rec = _run([
        (START - 300, 0, 1, 1000),           # placed: insert 1000
        (START - 300, 0, 0, 320),            # a window of the repeat: two placements, ambiguous
        (None, _row(1, 1000, contig)),       # a placed row without an anchor
        (START - 300, 0, 1, 1000),
    ], contig=contig)
    _is(rec, rows=4, n_anchored=3, n_placed=2, n_proper=2, n_in_range=2)
    from gappadder_amd import pair_anchors as PA
    reads = [seq(100), _row(1, 1000, contig)]         # a read that lies nowhere: unplaced
    rec = PA.anchors_host(reads, [1, 3], [(START - 300, 0), None], contig, B0, B1, 0, (START, END), 1000, 10, min_pairs=1)
    _is(rec, rows=2, n_anchored=1, n_placed=0, n_proper=0, n_unspanned=400, n_eval=0)


def test_empty_body_and_empty_pool():
    rec = _run([(START - 400, 0, 1, 1000)], body=(500, 500))       # column 500 - 400 = 100: insert 1000
    _is(rec, n_in_range=1, n_span=1, n_cols=0, min_cover=0, min_col=0, n_unspanned=0, n_eval=0, dev_min_n=0)
    rec = _run([])
    _is(rec, rows=0, n_anchored=0, n_cols=400, min_cover=0, min_col=400, n_unspanned=400, n_eval=0)


def test_long_and_non_acgt_contigs():
    from gappadder_amd import _lib as B
    rng = np.random.default_rng(22)
    long = CONTIG + "".join("ACGT"[i] for i in rng.integers(0, 4, B.PL_MAX_CONTIG + 1 - N))
    rec = _run([(START - 300, 0, 1, 1000)], contig=long)
    assert len(long) == 8193 and rec.tobytes() == np.array((B.PS_F_LONG, 1) + (0,) * 22, dtype=B.FILL_ANCHORS).tobytes()
    rec = _run([(START - 300, 0, 1, 1000)], contig=CONTIG[:50] + "N" + CONTIG[51:])
    assert rec.tobytes() == np.array((B.PS_F_NON_ACGT, 1) + (0,) * 22, dtype=B.FILL_ANCHORS).tobytes()
    assert int(_run([(START - 300, 0, 1, 1000)], contig=long[:8192])["flags"]) == 0


def test_scatter_filters_duplicates_and_counts():
    from gappadder_amd import _lib as B
    from gappadder_amd import pair_anchors as PA
    gaps = np.zeros(2, dtype=B.GAP)
    gaps[0], gaps[1] = (0, 10000, 10400, 1), (0, 50000, 50100, 2)
    off = np.array([0, 3, 5])
    ids = np.array([10, 7, 21, 4, 31], dtype=np.uint32)       # gap 0: rows 0..2 (side 0: 10; side 1: 7, 21); gap 1: rows 3, 4
    rec = lambda pos, flag, clip, read: (pos, 0, 0, 0, 0, flag, 60, clip, read)
    recs = np.array([
        rec(9701, 0x00, 0, 11),     # 0: mate 10 -> row 0; A0 = 9700, forward
        rec(9651, 0x10, 0, 11),     # 1: the same read again, further left, reverse: (9650, 1) is smaller and wins
        rec(9651, 0x00, 0, 11),     # 2: ... and (9650, 0) is smaller still
        rec(10901, 0x10, 0, 6),     # 3: mate 7 -> row 1; right anchor
        rec(9701, 0x00, 1, 20),     # 4: clipped
        rec(9701, 0x100, 0, 20),    # 5: secondary
        rec(9701, 0x800, 0, 20),    # 6: supplementary
        rec(9701, 0x04, 0, 20),     # 7: unmapped
        rec(10001, 0x00, 0, 20),    # 8: A0 = 10000 = start: inside the gap
        rec(10400, 0x00, 0, 20),    # 9: A0 = 10399 = end - 1: inside the gap
        rec(10401, 0x00, 0, 20),    # 10: A0 = 10400 = end: a right anchor; mate 21 -> row 2
        rec(9701, 0x00, 0, 40),     # 11: mate 41 is not in gap 0's slice: absent
        rec(49001, 0x00, 0, 5),     # 12: gap 1, mate 4 -> row 3
        rec(49001, 0x00, 0, 0xFFFFFFFF),   # 13: no read
        rec(10000, 0x00, 0, 30),    # 14: gap 0, A0 = 9999 = start - 1: left; mate 31 is in gap 1's slice only: absent
    ], dtype=B.ALNREC)
    D, U, C = B.KIND_DISCORDANT, B.KIND_UNMAP, B.KIND_CLIP
    hits = np.array([(0, 0, D, 1), (1, 0, U, 1), (2, 0, D, 1), (3, 0, U, 1), (4, 0, D, 1), (5, 0, D, 1), (6, 0, U, 1), (7, 0, U, 1), (8, 0, D, 1),
                     (9, 0, D, 1), (10, 0, D, 1), (11, 0, D, 1), (12, 1, U, 1), (13, 1, U, 1), (14, 0, D, 1),
                     (0, 0, D, 0),           # to_mate = 0
                     (0, 0, C, 1),           # another kind
                     (0, 0, B.KIND_LOWMAPQ, 1), (99, 0, D, 1), (0, 7, D, 1)], dtype=B.TAGHIT)       # ..., a record and a gap out of range
    want_at = {0: (9650, 0), 1: (10900, 1), 2: (10400, 0), 3: (49000, 0)}
    want_st = {"kept": 6, "dropped_clipped": 1, "dropped_in_gap": 2, "dropped_secondary": 2, "absent": 2, "dropped_other": 7}
    for order in (np.arange(len(hits)), np.arange(len(hits))[::-1], np.random.default_rng(5).permutation(len(hits))):
        at, st = PA.scatter_host(hits[order], recs, gaps, off, ids)
        assert at == want_at and st == want_st
    at, st = PA.scatter_host(hits, recs, gaps, off, ids, hit_cap=1)
    assert at == {0: (9700, 0)} and st["kept"] == 1 and sum(st.values()) == 1


def test_parameters():
    from gappadder_amd import pair_anchors as PA
    assert PA.check_params(150, min_pairs=1)[4] == 1 and PA.check_params(150)[4] == 8
    for kw in (dict(min_pairs=0), dict(min_pairs=-1), dict(min_pairs=2.5), dict(z=3, is_sd=349526), dict(z=1, is_sd=1 << 20), dict(z=0)):
        with pytest.raises(ValueError):
            PA.check_params(150, **kw)
    PA.check_params(150, z=3, is_sd=349525)       # 3 * 349 525 = 2^20 - 1
    assert PA.dev_means(np.zeros((), dtype=PA.B.FILL_ANCHORS)) == (None, None)
    assert abs(PA.z_score(-240, 4, 10) + 12.0) < 1e-12 and PA.z_score(0, 0, 10) is None
