"""Known answers, derived by hand, for the picker's "gapped" mode (gappadder_amd/pick_contigs.py::gapped_hits: seed-and-extend of the
whole flanks with a banded affine-gap extension, gap of g bases = 6 + g) and its use by the full and extended picks.

The layout of every case: contig c = a (50) + l (300) + gap (200) + r (300) + b (40), so the clean left flank l lies at contig bases
[50, 350) and the right flank r at [550, 850); the draft's flank is l or r with an edit.  Every derivation below assumes that the random
bases next to an edit do not happen to continue a match; the assertions on the sequences at the top of each test say so."""
import os

import numpy as np
import pytest

import pick_util as PK
from gappadder_amd.pick_contigs import (ALIGN_CAP, GAP_BAND, ContigsSelection, align_hits, gapped_hits, pick_extended_sequence,
                                        pick_gap_sequence, revcomp, stand_in_hits)

BOTH, LEFT, RIGHT, NONE = 1, 2, 3, 4


def _flanks(seed=3, nl=300, nr=300, gap=200):
    rng = np.random.default_rng(seed)
    return PK.rand_seq(rng, nl), PK.rand_seq(rng, nr), PK.rand_seq(rng, gap), PK.rand_seq(rng, 50), PK.rand_seq(rng, 40)


def _other(*bases):
    return next(x for x in "ACGT" if x not in bases)


def _ins(s, i, n=1):
    """n bases inserted in front of s[i], the first of them different from both neighbours."""
    return s[:i] + _other(s[i - 1], s[i]) + "ACGT"[:n - 1] + s[i:]


def _del(s, i, n=1):
    return s[:i] + s[i + n:]


def _left(hits):
    return [h for h in hits if h[0] == "left"]


def test_a_one_base_indel_ten_bases_from_the_gap_side_end_is_aligned_through_on_both_strands():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    assert l[289] != l[290] != l[291] and r[8] != r[9] != r[10]
    # insertion in the draft: the seed is l[:290] (score 290, at the query's start); to the right the inserted base is a gap of one
    # query base (-7) and the 10 bases behind it match: 293 in the query's last column, the maximum -> unclipped.  The alignment covers
    # the 300 contig bases of l with 301 query bases: pos 51, M = 300
    # deletion: a gap of one contig base (-7), 9 matches: 292 -> unclipped, 299 query bases over the same 300 contig bases
    for lf in (_ins(l, 290), _del(l, 290)):
        assert _left(gapped_hits([("c", c)], lf, r, 30)) == [("left", False, 0, 51, NONE, 300)], lf
        # reverse strand: revcomp(c) holds rc(l) at [890 - 350, 890 - 50); the indel is now LEFT of the seed
        assert _left(gapped_hits([("c", revcomp(c))], lf, r, 30)) == [("left", True, 0, 541, NONE, 300)], lf
    # the right flank: the indel is 10 bases behind the flank's first base, the seed is r[10:] and the left extension crosses it
    for rf in (_ins(r, 10), _del(r, 9)):
        h = gapped_hits([("c", c)], l, rf, 30)
        assert h == [("left", False, 0, 51, NONE, 300), ("right", False, 0, 551, NONE, 300)], rf
        h = gapped_hits([("c", revcomp(c))], l, rf, 30)
        assert h == [("left", True, 0, 541, NONE, 300), ("right", True, 0, 41, NONE, 300)], rf
    # the ungapped mode clips these on the gap side: 290 bases, the flank's tail stays outside
    assert _left(align_hits([("c", c)], _ins(l, 290), r, 30)) == [("left", False, 0, 51, RIGHT, 290)]


def test_the_same_indel_one_base_from_the_end_is_not_aligned_through():
    """An indel one base from the end costs 7 and regains 1: 6 below the maximum, and the end rule wants less than CLIP_PEN = 5.  The
    insertion is therefore clipped.  For the deletion the DP has a cheaper way to the query's end than the gap — the last base as ONE
    MISMATCH (-4, within the 5) — so that hit is unclipped but UNGAPPED: 299 query bases on 299 contig bases, not the 300 a gap would
    cover.  (The issue's text expects a clip in both cases; its own end rule gives this.)"""
    l, r, gap, a, b = _flanks()
    gap = _other(l[299]) + gap[1:]
    c = a + l + gap + r + b
    assert l[298] != l[299] and gap[0] != l[299]
    # insertion X before the last base: seed l[:299] = 299.  Query tail X, l[299]; contig l[299], gap[0].  Through the gap: 299 - 7 + 1 =
    # 293; ungapped: X/l[299] -4, l[299]/gap[0] -4 = 291.  g = 293 <= 299 - 5: clipped at the seed's end
    assert _left(gapped_hits([("c", c)], _ins(l, 299), r, 30)) == [("left", False, 0, 51, RIGHT, 299)]
    # deletion of l[298]: seed l[:298] = 298, query tail l[299], contig l[298], l[299].  Last column: (1, 1) = 298 - 4 = 294 (mismatch),
    # (2, 1) = 298 - 7 + 1 = 292 (gap).  g = 294 > 293: to the end through the mismatch, 299 contig bases
    assert _left(gapped_hits([("c", c)], _del(l, 298), r, 30)) == [("left", False, 0, 51, NONE, 299)]


def test_a_three_base_deletion_five_bases_from_the_end_goes_through():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    lf = _del(l, 292, 3)                                 # seed l[:292] = 292; gap of 3 contig bases -9, 5 matches: 288 > 292 - 5
    assert l[292] != l[295]
    assert _left(gapped_hits([("c", c)], lf, r, 30)) == [("left", False, 0, 51, NONE, 300)]
    assert _left(gapped_hits([("c", revcomp(c))], lf, r, 30)) == [("left", True, 0, 541, NONE, 300)]
    lf4 = _del(l, 293, 3)                                # 4 matches behind it: 287 <= 287, clipped at the seed's end
    assert l[293] != l[296]
    assert _left(gapped_hits([("c", c)], lf4, r, 30)) == [("left", False, 0, 51, RIGHT, 293)]
    ins3 = _ins(l, 290, 3)                               # three inserted bases, 10 behind: 290 - 9 + 10 = 291: through, 303 query bases
    assert _left(gapped_hits([("c", c)], ins3, r, 30)) == [("left", False, 0, 51, NONE, 300)]


def test_an_indel_of_32_bases_is_outside_the_band():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    assert GAP_BAND == 31
    # a deletion of l[p:p + 32], p near 228, where the bases next to the cut do not continue either match
    p = next(p for p in range(225, 240) if l[p] != l[p + 32] and l[p - 1] != l[p + 31] and l[p] != l[p + 31] and l[p - 1] != l[p + 30])
    lf = _del(l, p, 32)                                  # l[:p] + l[p + 32:]: two seeds, diagonals 50 and 82, 32 apart
    # the first cannot reach the second (|i - j| would be 32) and ends at its own end; the second (268 - p bases) neither: two clipped
    # hits, the higher score first
    assert _left(gapped_hits([("c", c)], lf, r, 30)) == [("left", False, 0, 51, RIGHT, p), ("left", False, 0, 50 + p + 32 + 1, LEFT, 268 - p)]
    lf31 = _del(l, p, 31)                                # 31 bases: inside the band, -37, then 269 - p > 37 matches: through
    assert _left(gapped_hits([("c", c)], lf31, r, 30)) == [("left", False, 0, 51, NONE, 300)]


def test_a_seed_behind_an_indel_inside_a_produced_alignment_is_skipped():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    # 40 bases behind the indel are a seed of their own.  Deletion: diagonal 51, after the first seed's alignment (diagonal 50), which
    # ran through the gap over it; insertion: diagonal 49, BEFORE the long seed, and its own left extension takes the long one in
    for lf in (_del(l, 259), _ins(l, 260)):
        st = {}
        assert _left(gapped_hits([("c", c)], lf, r, 15, stats=st)) == [("left", False, 0, 51, NONE, 300)]
        assert st == {}
    # a second copy of the 40 bases elsewhere in the contig is NOT inside the alignment's contig interval: a hit of its own
    c2 = c + l[260:]
    assert _left(gapped_hits([("c", c2)], _del(l, 259), r, 15)) == [("left", False, 0, 51, NONE, 300), ("left", False, 0, 891, LEFT, 40)]


def test_non_acgt_bases_score_minus_one_and_do_not_seed():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    lf = _ins(l, 290)
    ln = lf[:150] + "N" + lf[151:]                       # seeds l[:150] and l[151:290] on one diagonal; the N is crossed at -1
    assert _left(gapped_hits([("c", c)], ln, r, 30)) == [("left", False, 0, 51, NONE, 300)]
    cn = c[:50 + 295] + "N" + c[50 + 296:]               # an N in the contig behind the indel: 290 - 7 + 9 - 1 = 291, still through
    assert _left(gapped_hits([("c", cn)], lf, r, 30)) == [("left", False, 0, 51, NONE, 300)]
    assert _left(gapped_hits([("c", revcomp(cn))], lf, r, 30)) == [("left", True, 0, 541, NONE, 300)]
    assert gapped_hits([("c", "N" * 400)], l, r, 15) == []


def test_the_cap_counts_what_is_not_extended():
    l, r, _, _, _ = _flanks()
    rng = np.random.default_rng(4)
    unit = l[-40:]
    c = "".join(unit + PK.rand_seq(rng, 7) for _ in range(ALIGN_CAP + 10))
    st = {}
    h = [x for x in gapped_hits([("c", c)], l, r, 30, stats=st) if x[0] == "left" and not x[1]]
    assert len(h) == ALIGN_CAP and st["dropped"] == 10 and all(x[4] == LEFT and x[5] >= 40 for x in h)


def test_gapped_mode_closes_the_gap_where_align_keeps_the_flank_tail_and_exact_finds_nothing():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    for ctg in (c, revcomp(c)):
        clean = pick_gap_sequence([("c", ctg)], l, r, 30)
        assert clean is not None and clean[1] == (gap + r[0] if ctg == c else l[-1] + gap)
        assert pick_gap_sequence([("c", ctg)], l, r, 30, "gapped") == clean
        for lf, rf in ((_ins(l, 290), r), (_del(l, 290), r), (l, _ins(r, 10)), (l, _del(r, 9))):
            assert pick_gap_sequence([("c", ctg)], lf, rf, 30) is None and pick_gap_sequence([("c", ctg)], lf, rf, 15) is None
            assert pick_gap_sequence([("c", ctg)], lf, rf, 30, "gapped") == clean
            wrong = pick_gap_sequence([("c", ctg)], lf, rf, 30, "align")
            assert wrong is not None and len(wrong[1]) == len(clean[1]) + 10 and (clean[1][1:-1] in wrong[1])
    # the extended fill reads the gapped hits, too: contigs that end inside the flanks give clipped hits
    left_only, right_only = l[100:] + gap[:80], gap[120:] + r[:200]
    want = pick_extended_sequence([("x", left_only), ("y", right_only)], l, r, 15)
    assert want is not None and want[2] == gap[:80] + "NN" + gap[120:]
    assert pick_extended_sequence([("x", left_only), ("y", right_only)], _ins(l, 290), _del(r, 9), 15) is None
    assert pick_extended_sequence([("x", left_only), ("y", right_only)], _ins(l, 290), _del(r, 9), 15, "gapped") == want


def test_stand_in_hits_takes_the_third_mode_and_refuses_a_fourth(tmp_path):
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    assert stand_in_hits("gapped", [("c", c)], l, r, 30) == gapped_hits([("c", c)], l, r, 30) == align_hits([("c", c)], l, r, 30)
    for call in (lambda: stand_in_hits("banded", [("c", c)], l, r, 30), lambda: ContigsSelection("x/", "banded")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        gapped_hits([("c", c)], "A" * 1025, r, 30)
    wf = str(tmp_path) + "/wf/"
    os.makedirs(wf + "velvet_temp/0_1")
    os.makedirs(str(tmp_path) + "/flank_regions")
    open(str(tmp_path) + "/flank_regions/0_1.fa", "w").write(">0_1_left\n%s\n>0_1_right\n%s\n" % (_del(l, 290), r))
    open(wf + "velvet_temp/0_1/contigs.fa", "w").write(">NODE_1\n%s\n" % c)
    for mode, n in (("exact", 0), ("gapped", 1)):
        sf = str(tmp_path) + "/picked_%s.fa" % mode
        assert ContigsSelection(wf, mode).pick_full_constructed_contigs(30, ["0_1"], sf) == n
        if n:
            assert open(sf).read() == ">0_1_NODE_1\n%s\n" % (gap + r[0])
