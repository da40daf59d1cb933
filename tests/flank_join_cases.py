"""Hand-built cases of the flank-overlap joins (gappadder_amd/flank_joins.py), one gap each, shared by the host test and the
device test.  A case is built from a random truth T around a junction r: the right flank is T[r : r + n_r], the left flank ends o bases
PAST the right flank's first base, T[r + o - n_l : r + o], and a contig T[r - cl : r + o + cr] runs through it — so on the contig the
right anchor lies at j = cl and the left anchor (length a) at i = cl + o - a.  `want` is the record derived by hand from that (None: the
all-zero record), `stats` the statistics words the case adds.  Parameters of the expectations: anchors (30, 15), X = 256, C = 30, M = 2."""
import random

ANCHORS, X, C, M = (30, 15), 256, 30, 2
REVERSE, AMBIGUOUS, MULTI = 1, 2, 4
_COMP = str.maketrans("ACGT", "TGCA")
_NEXT = str.maketrans("ACGT", "CGTA")


def rc(s):
    return s.translate(_COMP)[::-1]


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def flip(s, *positions):
    """s with the bases at `positions` replaced by another base."""
    t = list(s)
    for p in positions:
        t[p] = t[p].translate(_NEXT)
    return "".join(t)


def junction(rng, o, n_l=400, n_r=400, cl=40, cr=40, size=1200, r=600):
    """(left flank, right flank, contig) of the module docstring."""
    T = rnd(rng, size)
    return T[r + o - n_l:r + o], T[r:r + n_r], T[r - cl:r + o + cr]


def want(o, level, i, j, contig=0, m_left=0, m_right=0, m_flanks=0, flags=0, n_candidates=1, n_accepted=1, o_min=None, o_max=None):
    return dict(contig=contig, left_pos=i, right_pos=j, overlap=o, m_left=m_left, m_right=m_right, m_flanks=m_flanks, n_candidates=n_candidates,
                n_accepted=n_accepted, o_min=o if o_min is None else o_min, o_max=o if o_max is None else o_max, level=level, flags=flags)


def homopolymer(rng):
    """Flanks that meet in a run of 12 A: P + A12 and A12 + Q.  A contig with 12 A between P and Q joins with o = 12, one with 14 A with
    o = 10 (the anchors of 30: P[-18:] + A12 at 42, A12 + Q[:18] at 60 / 62), both agreeing with the flanks in every compared column."""
    P, Q = rnd(rng, 199) + "C", "G" + rnd(rng, 199)
    return P + "A" * 12, "A" * 12 + Q, P[-60:] + "A" * 12 + Q[:60], P[-60:] + "A" * 14 + Q[:60]


def cases(seed=20260024):
    """[{name, lf, rf, contigs: [text], closed, tombstones: [text], want, stats}]"""
    out = []

    def add(name, lf, rf, contigs, want_=None, closed=False, tombstones=(), **stats):
        if want_ is not None:
            usable = not want_["flags"] & (AMBIGUOUS | MULTI)
            stats = dict(dict(joined=1, usable=int(usable)), **stats)
        if not closed:
            stats = dict(dict(open_gaps=1), **stats)
        out.append(dict(name=name, lf=lf, rf=rf, contigs=list(contigs), closed=closed, tombstones=list(tombstones), want=want_, stats=stats))

    rng = random.Random(seed)
    # the overlap itself: 1, around the anchor length, long, at X and beyond
    for o in (1, 29, 30, 31, 100, 256):
        lf, rf, s = junction(rng, o)
        add("o=%d" % o, lf, rf, [s], want(o, 30, 40 + o - 30, 40), candidates=1)
    lf, rf, s = junction(rng, 257)
    add("o=X+1 is far", lf, rf, [s], candidates=1, far=1)
    # the reverse strand: the oriented positions are those of the forward case
    lf, rf, s = junction(rng, 12)
    add("strand 1", lf, rf, [rc(s)], want(12, 30, 22, 40, flags=REVERSE), candidates=1)
    # one base of the long left anchor broken on the contig (outside the short anchor): the short level, the base counts on both sides
    lf, rf, s = junction(rng, 40)
    add("short level only", lf, rf, [flip(s, 40 + 40 - 30 + 5)], want(40, 15, 40 + 40 - 15, 40, m_left=1, m_right=1), candidates=1)
    # context of exactly C and of C - 1, on either side
    for name, cl, cr, ok in (("left context C", 30, 40, True), ("left context C-1", 29, 40, False), ("right context C", 40, 30, True),
                             ("right context C-1", 40, 29, False)):
        lf, rf, s = junction(rng, 40, cl=cl, cr=cr)
        if ok:
            add(name, lf, rf, [s], want(40, 30, cl + 10, cl), candidates=1)
        else:
            add(name, lf, rf, [s], candidates=1, no_context=1)
    # M and M + 1 differences in the left context (columns the right comparison does not see; outside both anchors)
    lf, rf, s = junction(rng, 12)
    add("m_l = M", lf, rf, [flip(s, 40 - 20, 40 - 25)], want(12, 30, 22, 40, m_left=2), candidates=1)
    lf, rf, s = junction(rng, 12)
    add("m_l = M+1", lf, rf, [flip(s, 40 - 20, 40 - 25, 40 - 28)], candidates=1, mismatch=1)
    # two contigs with different o
    lf, rf, c12, c10 = homopolymer(rng)
    add("ambiguous", lf, rf, [c12, c10], want(10, 30, 42, 62, contig=1, flags=AMBIGUOUS, n_candidates=2, n_accepted=2, o_min=10, o_max=12), candidates=2)
    # the right anchor a second time, further left on the winner: the rightmost stays j
    lf, rf, s = junction(rng, 12)
    add("multi", lf, rf, [rf[:30] + rnd(rng, 20) + s], want(12, 30, 50 + 22, 50 + 40, flags=MULTI), candidates=1)
    # the word's order: a clean o = 12 beats an o = 10 with one difference (left context, outside the anchors) ...
    lf, rf, c12, c10 = homopolymer(rng)
    add("fewer mismatches beat the smaller overlap", lf, rf, [flip(c10, 35), c12],
        want(12, 30, 42, 60, contig=1, flags=AMBIGUOUS, n_candidates=2, n_accepted=2, o_min=10, o_max=12), candidates=2)
    # ... and of two equal contigs the earlier wins
    lf, rf, s = junction(rng, 12)
    add("the earlier contig wins ties", lf, rf, [s, s], want(12, 30, 22, 40, contig=0, n_candidates=2, n_accepted=2), candidates=2)
    # a closed gap and a tombstone are not looked at
    lf, rf, s = junction(rng, 12)
    add("closed gap", lf, rf, [s], closed=True)
    lf, rf, s = junction(rng, 12)
    add("tombstone", lf, rf, [], tombstones=[s])
    # a flank of o + C - 1 bases, and of exactly o + C
    lf, rf, s = junction(rng, 12, n_r=41)
    add("right flank shorter than o + C", lf, rf, [s], candidates=1, short_flank=1)
    lf, rf, s = junction(rng, 12, n_l=41)
    add("left flank shorter than o + C", lf, rf, [s], candidates=1, short_flank=1)
    lf, rf, s = junction(rng, 12, n_l=42, n_r=42)
    add("flanks of exactly o + C", lf, rf, [s], want(12, 30, 22, 40), candidates=1)
    # an N in the long left anchor only: the short level, and the N differs from the contig's base; an N in the short anchor: no anchors
    lf, rf, s = junction(rng, 12)
    add("N in the long anchor", lf[:-20] + "N" + lf[-19:], rf, [s], want(12, 15, 40 + 12 - 15, 40, m_left=1), candidates=1)
    lf, rf, s = junction(rng, 12)
    add("N in the short anchor", lf[:-5] + "N" + lf[-4:], rf, [s], no_anchors=1)
    # a true gap of 50 bases filled by a contig stored on the other strand: an in-order pair, the pick's, no candidate
    T = rnd(rng, 1200)
    add("in-order pair on the other strand", T[200:600], T[650:1050], [rc(T[540:710])])
    return out


def assemble(cs, interleave=True):
    """The cases as one contig list: ([(gap, text)], [(lf, rf)], best words, {case index: list index of its relative contig 0, 1, ..}).
    interleave: the contigs of the gaps alternate (every gap's contigs keep their order), so that each gap's neighbours in the list are
    decoys of other gaps; a tombstone carries gap 0xFFFFFFFF."""
    items = []
    for g, c in enumerate(cs):
        items += [(n, g, g, t) for n, t in enumerate(c["contigs"])] + [(len(c["contigs"]) + n, g, 0xFFFFFFFF, t) for n, t in enumerate(c["tombstones"])]
    if interleave:
        items.sort(key=lambda x: (x[0], -x[1]))
    else:
        items.sort(key=lambda x: (x[1], x[0]))
    index = {}
    for at, (n, g, gap, _) in enumerate(items):
        if gap == g:
            index[(g, n)] = at
    contigs = [(gap, t) for _, _, gap, t in items]
    flanks = [(c["lf"], c["rf"]) for c in cs]
    best = [(30 << 56 | 1 << 32 | 1) if c["closed"] else 0 for c in cs]
    return contigs, flanks, best, index


def expected(cs, index):
    """(records as dictionaries, None for the zero record; the statistics dictionary) the cases' hand-derived answers add up to."""
    from gappadder_amd import flank_joins as FJ
    recs, st = [], dict.fromkeys(FJ.STAT_KEYS, 0)
    for g, c in enumerate(cs):
        recs.append(None if c["want"] is None else dict(c["want"], contig=index[(g, c["want"]["contig"])]))
        for k, v in c["stats"].items():
            st[k] += v
    return recs, st
