"""Known answers, derived by hand, for the picker's "align" mode (gappadder_amd/pick_contigs.py::align_hits: ungapped
seed-and-extend of the whole flanks with bwa mem's default scores) and its use by the full and extended picks."""
import numpy as np

import pick_util as PK
from gappadder_amd.pick_contigs import (ALIGN_CAP, ContigsSelection, align_hits, pick_extended_sequence, pick_gap_sequence, revcomp,
                                        select_full)

BOTH, LEFT, RIGHT, NONE = 1, 2, 3, 4


def _flanks(seed=3, nl=300, nr=300, gap=200):
    rng = np.random.default_rng(seed)
    return PK.rand_seq(rng, nl), PK.rand_seq(rng, nr), PK.rand_seq(rng, gap), PK.rand_seq(rng, 50), PK.rand_seq(rng, 40)


def _mut(s, i):
    return s[:i] + ("A" if s[i] != "A" else "C") + s[i + 1:]


def test_one_mismatch_near_the_gap_side_end_is_aligned_through():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    for k in range(1, 7):                               # last 6 positions: -4 then up to +5 back: g > best - 5, never clipped
        h = align_hits([("c", c)], _mut(l, len(l) - k), r, 30)
        assert h[0] == ("left", False, 0, 51, NONE, 300), (k, h)
        h = align_hits([("c", c)], l, _mut(r, k - 1), 30)
        assert h[1] == ("right", False, 0, 551, NONE, 300), (k, h)


def test_mismatches_at_the_last_two_positions_clip():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    lm = _mut(_mut(l, 299), 298)                        # g = best - 8 <= best - 5: clipped at the maximum
    assert align_hits([("c", c)], lm, r, 30)[0] == ("left", False, 0, 51, RIGHT, 298)
    rm = _mut(_mut(r, 0), 1)
    assert align_hits([("c", c)], l, rm, 30)[1] == ("right", False, 0, 553, LEFT, 298)


def test_whole_flanks_inside_a_contig_and_contig_ends_inside_the_flanks_on_both_strands():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    assert align_hits([("c", c)], l, r, 30) == [("left", False, 0, 51, NONE, 300), ("right", False, 0, 551, NONE, 300)]
    rc = revcomp(c)                                     # SAM frame: forward contig positions, revcomp(flank) as the query
    assert align_hits([("c", rc)], l, r, 30) == [("left", True, 0, 541, NONE, 300), ("right", True, 0, 41, NONE, 300)]
    c2 = l[100:] + gap + r[:250]                        # the contig starts inside the left flank and ends inside the right one
    assert align_hits([("c", c2)], l, r, 30) == [("left", False, 0, 1, LEFT, 200), ("right", False, 0, 401, RIGHT, 250)]
    assert align_hits([("c", revcomp(c2))], l, r, 30) == [("left", True, 0, 451, RIGHT, 200), ("right", True, 0, 1, LEFT, 250)]


def test_seed_length_19_and_the_score_threshold():
    l, r, _, _, _ = _flanks()
    rng = np.random.default_rng(9)
    for n, want in ((18, 0), (19, 1)):                  # a shared stretch shorter than a seed is never found
        c = PK.rand_seq(rng, 30) + l[-n:] + "T" * 0 + PK.rand_seq(rng, 30)
        h = [x for x in align_hits([("c", c)], l, r, 15) if x[0] == "left" and x[5] == n]
        assert len(h) == want, (n, h)
    base = l[-40:]
    for n in (29, 30):                                  # a match of n bases scores n (flanked by random bases: nothing to extend)
        c = "ACGTTGCA" + base[-n:] + "TTTT"
        got = [x for x in align_hits([("c", c)], l, r, 30) if x[0] == "left" and not x[1]]
        assert (len(got) == 1) == (n == 30), (n, got)


def test_two_alignments_on_one_diagonal_and_n_bases():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    # 30 mismatches in a row (-120, beyond z-drop 100) split the diagonal into two alignments; 6 of them do not
    l2 = l[:100] + "".join("A" if x != "A" else "C" for x in l[100:130]) + l[130:]
    h = [x for x in align_hits([("c", c)], l2, r, 30) if x[0] == "left"]
    assert h == [("left", False, 0, 181, LEFT, 170), ("left", False, 0, 51, RIGHT, 100)]
    l3 = l[:100] + "".join("A" if x != "A" else "C" for x in l[100:106]) + l[106:]
    assert [x for x in align_hits([("c", c)], l3, r, 30) if x[0] == "left"] == [("left", False, 0, 51, NONE, 300)]
    ln = l[:150] + "N" + l[151:]                        # an N in the flank scores -1: aligned through
    assert align_hits([("c", c)], ln, r, 30)[0] == ("left", False, 0, 51, NONE, 300)
    cn = c[:60] + "N" + c[61:]                          # an N in the contig, too
    assert align_hits([("c", cn)], l, r, 30)[0] == ("left", False, 0, 51, NONE, 300)


def test_tie_order_and_the_cap():
    l, r, gap, _, _ = _flanks()
    rng = np.random.default_rng(4)
    unit = l[-40:]
    c = "".join(unit + PK.rand_seq(rng, 7) for _ in range(3)) + revcomp(unit)
    h = [x for x in align_hits([("c", c)], l, r, 30) if x[0] == "left"]
    # equal scores (40): forward before reverse, then by position
    assert [(x[1], x[3]) for x in h] == [(False, 1), (False, 48), (False, 95), (True, 142)], h
    assert all(x[4] == (RIGHT if x[1] else LEFT) and x[5] == 40 for x in h)
    c = "".join(unit + PK.rand_seq(rng, 7) for _ in range(ALIGN_CAP + 10))
    st = {}
    h = [x for x in align_hits([("c", c)], l, r, 30, stats=st) if x[0] == "left" and not x[1]]
    assert len(h) == ALIGN_CAP and st["dropped"] == 10
    assert max(x[3] for x in h) < 47 * ALIGN_CAP                       # the first 64 diagonals in production order are kept
    # the highest score first: a longer match on the reverse strand comes before the shorter forward one
    c = l[-35:] + PK.rand_seq(rng, 9) + revcomp(l[-60:])
    h = [x for x in align_hits([("c", c)], l, r, 30) if x[0] == "left"]
    assert [(x[1], x[5]) for x in h] == [(True, 60), (False, 35)]


def test_align_mode_closes_a_gap_exact_mode_leaves_open_with_the_same_slice():
    l, r, gap, a, b = _flanks()
    c = a + l + gap + r + b
    for ctg in (c, revcomp(c)):
        clean = pick_gap_sequence([("c", ctg)], l, r, 30)
        assert clean is not None and clean[1] == (gap + r[0] if ctg == c else l[-1] + gap)
        for lm, rm in ((_mut(l, 297), r), (l, _mut(r, 4))):
            assert pick_gap_sequence([("c", ctg)], lm, rm, 30) is None and pick_gap_sequence([("c", ctg)], lm, rm, 15) is None
            assert pick_gap_sequence([("c", ctg)], lm, rm, 30, "align") == clean
    # the extended fill reads the align hits, too
    left_only, right_only = l[100:] + gap[:80], gap[120:] + r[:200]        # contigs that end inside the flanks: clipped hits
    want = pick_extended_sequence([("x", left_only), ("y", right_only)], l, r, 15)
    assert want is not None and want[2] is not None
    assert pick_extended_sequence([("x", left_only), ("y", right_only)], _mut(l, 296), _mut(r, 3), 15) is None
    assert pick_extended_sequence([("x", left_only), ("y", right_only)], _mut(l, 296), _mut(r, 3), 15, "align") == want


def test_exact_mode_is_the_default_and_select_full_is_unchanged():
    cases = PK.picker_cases(11, 60)
    for l, r, contigs in cases:
        named = [("c%d" % i, s) for i, s in enumerate(contigs)]
        for a in (30, 15):
            assert pick_gap_sequence(named, l, r, a) == pick_gap_sequence(named, l, r, a, "exact")
    assert ContigsSelection("x/").mode == "exact" and ContigsSelection("x/", "align").mode == "align"
    assert select_full([]) is None


def test_contigs_selection_in_align_mode_writes_the_picked_sequence(tmp_path):
    l, r, gap, a, b = _flanks()
    wf = str(tmp_path) + "/wf/"
    import os
    os.makedirs(wf + "velvet_temp/0_1")
    os.makedirs(str(tmp_path) + "/flank_regions")
    lm = _mut(l, 298)
    open(str(tmp_path) + "/wf/../flank_regions/0_1.fa", "w").write(">0_1_left\n%s\n>0_1_right\n%s\n" % (lm, r))
    open(wf + "velvet_temp/0_1/contigs.fa", "w").write(">NODE_1\n%s\n" % (a + l + gap + r + b))
    for mode, n in (("exact", 0), ("align", 1)):
        sf = str(tmp_path) + "/picked_%s.fa" % mode
        assert ContigsSelection(wf, mode).pick_full_constructed_contigs(30, ["0_1"], sf) == n
        if n:
            assert open(sf).read() == ">0_1_NODE_1\n%s\n" % (gap + r[0])
