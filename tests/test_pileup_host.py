"""The definition of the per-base pile-up (gappadder_amd/pileup.py: the host twin and its helpers) on hand-made rows: every class at its
boundary, strands and ambiguity, the run analysis, oriented / phred / is_low, and the parameter refusals.  No GPU."""
import numpy as np
import pytest

L, SEED, MM, MO = 24, 12, 1, 12     # two seeds a read, one mismatch allowed
PRM = dict(seed=SEED, max_mismatch=MM, min_overlap=MO)


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _contig(n, seed=5):
    """A contig whose 12-mers are all different, on either strand."""
    rng = np.random.default_rng(seed)
    while True:
        c = "".join("ACGT"[i] for i in rng.integers(0, 4, n))
        k = [c[i:i + SEED] for i in range(n - SEED + 1)]
        if len(set(k) | {_rc(x) for x in k}) == 2 * len(k):
            return c


def _read(c, at, rev=False, sub=None):
    """The read of c[at : at + L] (sub: a contig column whose base is replaced), as it is or reverse-complemented."""
    r = c[at:at + L]
    if sub is not None:
        r = r[:sub - at] + "ACGT"[("ACGT".index(r[sub - at]) + 1) % 4] + r[sub - at + 1:]
    return _rc(r) if rev else r


def _host(reads, c, b0, b1, **kw):
    from gappadder_amd import pileup as PU
    return PU.pileup_host(reads, c, b0, b1, **dict(PRM, **kw))


def test_depth_boundaries_thin_and_uncovered():
    c = _contig(100)
    # columns 30..39: depth 2 = min_depth - 1; 40..53: depth 3 = min_depth; 54..63: depth 1; 64..69: nothing
    reads = [_read(c, 30), _read(c, 30, rev=True), _read(c, 40)]
    e, rec = _host(reads, c, 30, 70)
    assert e.shape == (100, 8) and e.dtype == np.uint16 and int(rec["len"]) == 100 and int(rec["n_cols"]) == 40
    assert [int(e[j].sum()) for j in (29, 30, 39, 40, 53, 54, 63, 64)] == [0, 2, 2, 3, 3, 1, 1, 0]
    assert (int(rec["n_thin"]), int(rec["n_uncovered"]), int(rec["n_contested"]), int(rec["n_minority"])) == (20, 6, 0, 0)
    assert int(rec["depth_sum"]) == 2 * 10 + 3 * 14 + 10 and (int(rec["min_depth_seen"]), int(rec["min_depth_col"])) == (0, 34)
    assert (int(rec["reads_placed"]), int(rec["reads_ambiguous"])) == (3, 0)
    # both strands vote the base as it reads on the stored contig
    b = "ACGT".index(c[35])
    assert int(e[35][b]) == 1 and int(e[35][4 + b]) == 1
    # at min_depth 2 the depth-2 columns are no longer thin, at 4 the depth-3 columns are
    assert int(_host(reads, c, 30, 70, min_depth=2)[1]["n_thin"]) == 10 and int(_host(reads, c, 30, 70, min_depth=4)[1]["n_thin"]) == 34


def test_agreement_boundary_is_not_contested():
    from gappadder_amd import pileup as PU
    c = _contig(100)
    reads = [_read(c, 40), _read(c, 40), _read(c, 40, rev=True), _read(c, 40, rev=True), _read(c, 40, sub=45)]
    e, rec = _host(reads, c, 30, 70, min_agree=80)            # column 45: depth 5, agree 4: 100 * 4 == 80 * 5
    assert int(e[45].sum()) == 5 and int(rec["n_contested"]) == 0 and int(rec["n_minority"]) == 0
    assert int(_host(reads, c, 30, 70, min_agree=81)[1]["n_contested"]) == 1
    assert not PU.is_low(e[45], c[45], 3, 80) and PU.is_low(e[45], c[45], 3, 81) and PU.is_low(e[45], c[45], 6, 1)
    # a contested column is low; with as many votes against as for it is not minority, with more it is
    reads2 = reads[:2] + [_read(c, 40, sub=45), _read(c, 40, sub=45)]
    e2, rec2 = _host(reads2, c, 30, 70)
    assert (int(rec2["n_contested"]), int(rec2["n_minority"])) == (1, 0) and not PU.is_minority(e2[45], c[45])
    e3, rec3 = _host(reads2[1:], c, 30, 70)
    assert (int(rec3["n_contested"]), int(rec3["n_minority"])) == (1, 1) and PU.is_minority(e3[45], c[45])


def test_minority_below_min_depth():
    c = _contig(100)
    e, rec = _host([_read(c, 40, sub=50)], c, 30, 70)         # one read: every column thin, column 50 minority as well
    assert (int(rec["n_thin"]), int(rec["n_minority"]), int(rec["n_contested"]), int(rec["n_one_strand"])) == (24, 1, 0, 0)
    assert int(e[50]["ACGT".index(c[50])]) == 0 and int(e[50].sum()) == 1


def test_one_strand_columns():
    c = _contig(100)
    fwd = [_read(c, 36)] * 3
    _, rec = _host(fwd, c, 30, 70)
    assert int(rec["n_one_strand"]) == 24
    e, rec = _host([_read(c, 36, rev=True)] * 3, c, 30, 70)
    assert int(rec["n_one_strand"]) == 24 and int(e[40][:4].sum()) == 0 and int(e[40][4:].sum()) == 3
    _, rec = _host(fwd + [_read(c, 48, rev=True)], c, 30, 70)                      # 48..59 have both strands, 60..71 are thin
    assert int(rec["n_one_strand"]) == 12
    _, rec = _host(fwd[:2], c, 30, 70)                                              # below min_depth no column is one_strand
    assert int(rec["n_one_strand"]) == 0 and int(rec["n_thin"]) == 24


def test_ambiguous_row_does_not_vote():
    c0 = _contig(100)
    c = c0[:60] + c0[20:60] + c0[60:]                          # c0[20:60] twice: a read inside it has two best placements
    reads = [_read(c0, 25), _read(c0, 62), _read(c0, 62)]
    e, rec, where, _ = _host(reads, c, 10, 120, detail=True)
    assert where[0] == "ambiguous" and (int(rec["reads_placed"]), int(rec["reads_ambiguous"])) == (2, 1)
    assert int(e[:100].sum()) == 0 and int(e.sum()) == 2 * L


def test_low_runs():
    c = _contig(130)
    cover = lambda at: [_read(c, at), _read(c, at, rev=True), _read(c, at)]
    # body 30..89: nothing on 30..34 and on 59..63 — two runs of five, the first wins —, and on 88, 89
    _, rec = _host(cover(35) + cover(64), c, 30, 90)
    assert (int(rec["low_run"]), int(rec["low_run_col"]), int(rec["n_uncovered"])) == (5, 0, 12)
    # a run that ends on the last body column; the uncovered flank columns behind it do not count
    _, rec = _host(cover(30), c, 30, 60)
    assert (int(rec["low_run"]), int(rec["low_run_col"]), int(rec["n_uncovered"])) == (6, 24, 6)
    # a thin column between two uncovered ones belongs to the run
    _, rec = _host(cover(30) + [_read(c, 56)], c, 30, 90)
    assert (int(rec["low_run"]), int(rec["low_run_col"]), int(rec["n_thin"]), int(rec["n_uncovered"])) == (36, 24, 24, 12)
    # no low column, and an empty body
    _, rec = _host(cover(30), c, 30, 54)
    assert (int(rec["low_run"]), int(rec["low_run_col"]), int(rec["min_depth_seen"])) == (0, 0, 3)
    _, rec = _host(cover(30), c, 40, 40)
    assert int(rec["n_cols"]) == 0 and (int(rec["low_run"]), int(rec["min_depth_seen"]), int(rec["min_depth_col"]), int(rec["depth_sum"])) == (0, 0, 0, 0)


def test_oriented_is_an_involution_that_swaps_the_strands():
    from gappadder_amd import pileup as PU
    c = _contig(110)
    reads = [_read(c, 20), _read(c, 31, rev=True), _read(c, 40, sub=50), _read(c, 70, rev=True, sub=80), _read(c, 86)]
    e, _ = _host(reads, c, 30, 80)
    flipped = PU.oriented(e, True)
    assert (PU.oriented(flipped, True) == e).all() and (PU.oriented(e, False) == e).all() and not (flipped == e).all()
    # the same rows on the reverse-complemented contig: what lay on the reverse strand votes forward, on the mirrored column
    e_rc, _ = _host(reads, _rc(c), 30, 80)
    assert (e_rc == flipped).all()
    assert (PU.oriented(e[30:80], True) == e_rc[110 - 80:110 - 30]).all()
    one = np.array([[1, 2, 3, 4, 5, 6, 7, 8]], dtype=np.uint16)
    assert PU.oriented(one, True).tolist() == [[8, 7, 6, 5, 4, 3, 2, 1]]


def test_phred_corners():
    from gappadder_amd import pileup as PU
    E = lambda f, r: np.array(list(f) + list(r), dtype=np.uint16)
    assert PU.phred(E((0, 0, 0, 0), (0, 0, 0, 0)), "A") == 0                         # depth 0
    assert PU.phred(E((2, 1, 0, 0), (0, 0, 0, 0)), "A") == 0                         # agree - 2 other = 0
    assert PU.phred(E((1, 0, 0, 0), (0, 0, 0, 2)), "A") == 0                         # ... below 0
    assert PU.phred(E((4, 0, 0, 0), (3, 0, 0, 0)), "A") == 35                        # 7
    assert PU.phred(E((4, 0, 0, 0), (4, 0, 0, 0)), "A") == 40                        # 8
    assert PU.phred(E((0, 0, 9, 0), (0, 0, 1, 1)), "G") == 40 and PU.phred(E((0, 0, 9, 0), (0, 0, 1, 1)), 2) == 40
    assert PU.phred(E((65535, 0, 0, 0), (0, 0, 0, 0)), "A") == 40 and PU.phred(E((0, 5, 0, 0), (0, 0, 0, 0)), "A") == 0
    with pytest.raises(ValueError):
        PU.phred(E((1, 0, 0, 0), (0, 0, 0, 0)), "N")


def test_skipped_contigs_and_records_only():
    from gappadder_amd import _lib as B
    c = _contig(100)
    e, rec = _host([_read(c, 40)], c[:50] + "N" + c[51:], 30, 70)
    assert e is None and int(rec["flags"]) == B.PU_F_NON_ACGT and int(rec["n_cols"]) == 40 and int(rec["len"]) == 0 and int(rec["reads_placed"]) == 0
    e, rec = _host([], "ACGT" * 2049, 30, 70)
    assert e is None and int(rec["flags"]) == B.PU_F_LONG and int(rec["n_cols"]) == 40
    e, rec = _host([_read(c, 40)], c, 30, 70, track=False)
    full = _host([_read(c, 40)], c, 30, 70)[1]
    assert e is None and int(rec["len"]) == 0 and int(full["len"]) == 100 and int(rec["flags"]) == 0
    assert all(int(rec[f]) == int(full[f]) for f in B.FILL_PILEUP.names if f != "len")
    assert B.FILL_PILEUP.itemsize == 72 and B.FILL_PILEUP.fields["depth_sum"][1] == 56


def test_parameter_refusals():
    from gappadder_amd import pileup as PU
    from gappadder_amd.pipeline import Pipeline
    assert PU.check_params(150) == (16, 4, 48, 3, 80) and PU.check_params(100, 12, 7, 12, 1, 100) == (12, 7, 12, 1, 100)
    for kw in (dict(seed=11), dict(seed=33), dict(max_mismatch=-1), dict(max_mismatch=16), dict(min_overlap=15), dict(min_overlap=151),
               dict(min_depth=0), dict(min_agree=0), dict(min_agree=101), dict(seed=32, max_mismatch=4), dict(seed=20, max_mismatch=7)):
        with pytest.raises(ValueError, match="pileup"):
            PU.check_params(150, **kw)
    with pytest.raises(ValueError, match="pileup"):
        PU.pileup_host(["A" * 150], "ACGT" * 100, 10, 20, min_agree=0)
    with pytest.raises(ValueError, match="pileup with second_round"):
        Pipeline(None, 4, 150, [(31, 29)], pileup=True, second_round=True)
    with pytest.raises(ValueError, match="pileup runs on a single rank"):
        Pipeline(None, 4, 150, [(31, 29)], pileup=True, world=2)
