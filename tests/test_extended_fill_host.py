"""The extended fill's host side: the contig order the device step uses for pick_extended_sequence's "first contig"
(pick_contigs.extension_order), the decoding of its per-gap records (pick_contigs.decode_extended, Pipeline.extended_sequences) against
the host twin on hand-built records, and the constructor's refusal of a multi-rank run."""
import numpy as np
import pytest

from gappadder_amd import _lib as B
from gappadder_amd.pick_contigs import decode_extended, extension_order, pick_extended_sequence, revcomp

NONE = B.EXT_NONE


def _rnd(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def test_extension_order_key():
    kk = [(51, 49), (31, 29), (61, 59)]
    contigs = [(31, 29, "CCCC"), (0, 0, "AAAAAAAAAA"), (51, 49, "GG"), (31, 29, "ACGTA"), (61, 59, "TTTTTTTT"), (31, 29, "AAAA"),
               (51, 49, "GGG"), (31, 29, "AAAA"), (17, 15, "A")]
    # pair rank 0: 51/49 longest first; rank 1: 31/29 length 5, then length 4 by bases (equal bases: by index); rank 2: 61/59;
    # after every pair: the merged contig (0, 0) and a pair not in the list, longest first
    assert extension_order(contigs, kk) == [6, 2, 3, 5, 7, 0, 4, 1, 8]
    assert extension_order([(0, 0, "T"), (0, 0, "A"), (31, 29, "G")], [(31, 29)]) == [2, 1, 0]
    assert extension_order([], kk) == []


def _rec(**kw):
    r = np.zeros(1, dtype=B.EXT_PICK)[0]
    r["left"] = r["right"] = NONE
    for k, v in kw.items():
        r[k] = v
    return r


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(11)
    left, right = _rnd(rng, 60), _rnd(rng, 60)
    la, ra = left[-15:], right[:15]
    into, out = _rnd(rng, 40), _rnd(rng, 30)
    cl = _rnd(rng, 5) + la + into               # the left anchor at 1-based 6, then 40 bases into the gap
    cr = out + ra + _rnd(rng, 5)                # 30 bases out of the gap, then the right anchor at 31
    return left, right, la, ra, into, out, cl, cr


def _check(contigs, left, right, rec):
    twin = pick_extended_sequence([("%d" % i, s) for i, s in enumerate(contigs)], left, right, 15)
    got = decode_extended(rec, lambda i: contigs[i])
    want = (int(twin[0]) if twin[0] else -1, int(twin[1]) if twin[1] else -1, twin[2], twin[3])
    assert got == want, (got, want)
    return got


def test_decode_left_only(case):
    left, right, la, ra, into, out, cl, cr = case
    got = _check([cl], left, right, _rec(left=0, l_beg=cl.find(la) + 15, l_len=len(into)))
    assert got[2] == into + "NN"


def test_decode_right_only(case):
    left, right, la, ra, into, out, cl, cr = case
    got = _check([cr], left, right, _rec(right=0, r_beg=0, r_len=cr.rfind(ra)))
    assert got[2] == "NN" + out and got[3] == "NN" + cr


def test_decode_both_sides_on_two_contigs(case):
    left, right, la, ra, into, out, cl, cr = case
    got = _check([cl, cr], left, right, _rec(left=0, right=1, l_beg=20, l_len=40, r_beg=0, r_len=30))
    assert got[2] == into + "NN" + out and got[3] == cl + "NN" + cr


def test_decode_same_contig_on_both_sides(case):
    left, right, la, ra, into, out, cl, cr = case
    rng = np.random.default_rng(12)
    both = out[:25] + ra + _rnd(rng, 30) + la + into[:10]       # anchors out of order: the right side only, with the anchor's first base
    p = both.find(ra)
    got = _check([both], left, right, _rec(left=0, right=0, r_beg=0, r_len=p + 1))
    assert got[:3] == (0, 0, "NN" + out[:25] + ra[0]) and got[3] == both


def test_decode_reverse_parts(case):
    left, right, la, ra, into, out, cl, cr = case
    rl, rr = revcomp(cl), revcomp(cr)
    pl = rl.rfind(revcomp(la)) + 1            # 1-based position of rc(left anchor): the part is [0, pl), one anchor base kept
    pr = rr.find(revcomp(ra)) + 1             # rc(right anchor): the part starts at its last base
    got = _check([rl, rr], left, right, _rec(left=0, right=1, l_beg=0, l_len=pl, l_rev=1, r_beg=pr + 14, r_len=len(rr) - (pr + 14), r_rev=1))
    assert got[2] == left[-1] + into + "NN" + out


def test_decode_nothing_but_nn(case):
    left, right, la, ra, into, out, cl, cr = case
    c = "ACGTA" + la                           # the left anchor at the contig's end: an empty part
    got = _check([c], left, right, _rec(left=0, l_beg=20, l_len=0))
    assert got == (0, -1, None, c)
    assert decode_extended(_rec(), lambda i: "") is None


def test_extended_fill_is_single_rank():
    from gappadder_amd.pipeline import Pipeline
    with pytest.raises(ValueError):
        Pipeline(None, 4, 150, [(31, 29)], world=2, extended_fill=True)
    with pytest.raises(ValueError):
        Pipeline(None, 4, 150, [(31, 29)], force_exchange=True, extended_fill=True)
