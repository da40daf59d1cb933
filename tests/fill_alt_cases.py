"""Hand-built cases of the fill alternatives (gappadder_amd/fill_alternatives.py), one gap each, shared by the host test and
the device test.  A gap has random flanks LF, RF of 400 bases; a contig ctg(F) = LF[-40:] + F + RF[:40] carries both anchors of 30 (and of
15) around the fill F, so it is a candidate of level 30, span len(F), strand 0, and rc(ctg(F)) the same on strand 1; broken(F) has the
sixth base of the long left anchor changed (outside the short anchor): level 15.  `best` is the gap's pick word written by hand as
(level, span, contig, strand), the contig relative to the case's own (None: the gap is open); `doctored` marks the words the device's pick
would not give (they name another contig than the longest span of the highest level).  `want` is the record derived by hand (None: all
zero), `per` the per-contig records (length, dist, class, strand).  Parameters of the expectations: anchors (30, 15), B = 16."""
import random

ANCHORS, B = (30, 15), 16
REVERSE, RIVAL_REVERSE, HAS_RIVAL, LENGTH_VARIES, OUTRANKED, LOST = 1, 2, 4, 8, 16, 32
NONE, WINNER, IDENTICAL, NEAR, FAR, LOWER = range(6)
DIST_FAR = 0xFFFF
ZERO = (0, 0, NONE, 0)
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


def cut(rng, n, at, d):
    """(F, F without its d bases from `at` on) for a random F of n bases whose deleted block differs from its neighbours at both ends, so
    that the common prefix is exactly `at` and the common suffix everything behind the block."""
    while True:
        F = rnd(rng, n)
        if F[at] != F[at + d] and F[at + d - 1] != F[at - 1]:
            return F, F[:at] + F[at + d:]


def want(fill_len, contig=0, rival=None, rival_len=0, lcp=0, lcs=0, len_min=None, len_max=None, n=1, lower=0, identical=0, near=0, far=0, dist=0,
         level=30, flags=0):
    return dict(contig=contig, rival=0 if rival is None else rival, fill_len=fill_len, rival_len=rival_len, lcp=lcp, lcs=lcs,
                len_min=fill_len if len_min is None else len_min, len_max=fill_len if len_max is None else len_max, n_candidates=n, n_lower=lower,
                n_identical=identical, n_near=near, n_far=far, dist=dist, level=level, flags=flags | (HAS_RIVAL if rival is not None else 0))


def cases(seed=20260025):
    """[{name, lf, rf, contigs: [text], tombstones: [text], best, doctored, want, per}]"""
    out = []
    rng = random.Random(seed)

    def gap(n_l=400, n_r=400):
        return rnd(rng, n_l), rnd(rng, n_r)

    def add(name, lf, rf, contigs, best, want_, per, tombstones=(), doctored=False):
        assert len(per) == len(contigs)
        out.append(dict(name=name, lf=lf, rf=rf, contigs=list(contigs), tombstones=list(tombstones), best=best, doctored=doctored, want=want_, per=list(per)))

    def ctg(lf, rf, F, cl=40, cr=40):
        return lf[-cl:] + F + rf[:cr]

    def broken(lf, rf, F):
        return flip(ctg(lf, rf, F), 40 - 30 + 5)

    W = lambda n, strand=0: (n, DIST_FAR, WINNER, strand)

    # one candidate only
    lf, rf = gap()
    F = rnd(rng, 120)
    add("one candidate", lf, rf, [ctg(lf, rf, F)], (30, 120, 0, 0), want(120), [W(120)])
    # identical fills: in another context, the same contig twice, on the other strand
    lf, rf = gap()
    F = rnd(rng, 120)
    add("identical fill, longer context", lf, rf, [ctg(lf, rf, F), ctg(lf, rf, F, 55, 61)], (30, 120, 0, 0), want(120, n=2, identical=1),
        [W(120), (120, DIST_FAR, IDENTICAL, 0)])
    lf, rf = gap()
    F = rnd(rng, 77)
    add("the same contig twice", lf, rf, [ctg(lf, rf, F)] * 2, (30, 77, 0, 0), want(77, n=2, identical=1), [W(77), (77, DIST_FAR, IDENTICAL, 0)])
    lf, rf = gap()
    F = rnd(rng, 131)
    add("identical on the other strand", lf, rf, [ctg(lf, rf, F), rc(ctg(lf, rf, F))], (30, 131, 0, 0), want(131, n=2, identical=1),
        [W(131), (131, DIST_FAR, IDENTICAL, 1)])
    # substitutions: one, B and B + 1 (every tenth column from 7 on)
    lf, rf = gap()
    F = rnd(rng, 200)
    add("one substitution", lf, rf, [ctg(lf, rf, F), ctg(lf, rf, flip(F, 61))], (30, 200, 0, 0),
        want(200, rival=1, rival_len=200, lcp=61, lcs=138, n=2, near=1, dist=1), [W(200), (200, 1, NEAR, 0)])
    for k in (B, B + 1):
        lf, rf = gap()
        F = rnd(rng, 200)
        cols = [7 + 10 * x for x in range(k)]
        near = k <= B
        add("%d substitutions" % k, lf, rf, [ctg(lf, rf, F), ctg(lf, rf, flip(F, *cols))], (30, 200, 0, 0),
            want(200, rival=1, rival_len=200, lcp=7, lcs=199 - cols[-1], n=2, near=int(near), far=int(not near), dist=k if near else DIST_FAR),
            [W(200), (200, k, NEAR, 0) if near else (200, DIST_FAR, FAR, 0)])
    # a rival shorter by 1, B and B + 1 bases: a pure deletion, the windows are d / 0; the rival comes first in the list
    for d in (1, B, B + 1):
        lf, rf = gap()
        F, P = cut(rng, 150, 60, d)
        near = d <= B
        add("rival shorter by %d" % d, lf, rf, [ctg(lf, rf, P), ctg(lf, rf, F)], (30, 150, 1, 0),
            want(150, contig=1, rival=0, rival_len=150 - d, lcp=60, lcs=150 - d - 60, len_min=150 - d, len_max=150, n=2, near=int(near), far=int(not near),
                 dist=d if near else DIST_FAR, flags=LENGTH_VARIES),
            [(150 - d, d, NEAR, 0) if near else (150 - d, DIST_FAR, FAR, 0), W(150)])
    # a pure insertion in the rival, windows 0 / 5: the word names the shorter contig, so the longer one outranks it
    lf, rf = gap()
    F, P = cut(rng, 90, 33, 5)
    add("pure insertion in the rival", lf, rf, [ctg(lf, rf, P), ctg(lf, rf, F)], (30, 85, 0, 0),
        want(85, rival=1, rival_len=90, lcp=33, lcs=52, len_min=85, len_max=90, n=2, near=1, dist=5, flags=LENGTH_VARIES | OUTRANKED),
        [W(85), (90, 5, NEAR, 0)], doctored=True)
    # the suffix is capped by what the prefix leaves: AAAA against AAAAA
    lf, rf = gap()
    lf, rf = lf[:-1] + "C", "G" + rf[1:]
    add("capped suffix", lf, rf, [ctg(lf, rf, "AAAA"), ctg(lf, rf, "AAAAA")], (30, 4, 0, 0),
        want(4, rival=1, rival_len=5, lcp=4, lcs=0, len_min=4, len_max=5, n=2, near=1, dist=1, flags=LENGTH_VARIES | OUTRANKED),
        [W(4), (5, 1, NEAR, 0)], doctored=True)
    # adjacent anchors: span 0 as the winner (doctored) and as the rival
    lf, rf = gap()
    add("span 0 wins", lf, rf, [ctg(lf, rf, ""), ctg(lf, rf, "ACG")], (30, 0, 0, 0),
        want(0, rival=1, rival_len=3, len_min=0, len_max=3, n=2, near=1, dist=3, flags=LENGTH_VARIES | OUTRANKED), [W(0), (3, 3, NEAR, 0)], doctored=True)
    lf, rf = gap()
    add("span 0 is the rival", lf, rf, [ctg(lf, rf, ""), ctg(lf, rf, "ACGTTGCA")], (30, 8, 1, 0),
        want(8, contig=1, rival=0, rival_len=0, len_min=0, len_max=8, n=2, near=1, dist=8, flags=LENGTH_VARIES), [(0, 8, NEAR, 0), W(8)])
    # strands: the rival reverse under a forward winner, and the other way round
    lf, rf = gap()
    F = rnd(rng, 140)
    add("rival on the reverse strand", lf, rf, [ctg(lf, rf, F), rc(ctg(lf, rf, flip(F, 20)))], (30, 140, 0, 0),
        want(140, rival=1, rival_len=140, lcp=20, lcs=119, n=2, near=1, dist=1, flags=RIVAL_REVERSE), [W(140), (140, 1, NEAR, 1)])
    lf, rf = gap()
    F = rnd(rng, 140)
    add("winner on the reverse strand", lf, rf, [rc(ctg(lf, rf, F)), ctg(lf, rf, flip(F, 0, 139))], (30, 140, 0, 1),
        want(140, rival=1, rival_len=140, lcp=0, lcs=0, n=2, near=1, dist=2, flags=REVERSE), [W(140, 1), (140, 2, NEAR, 0)])
    # two rivals: the runner-up is the longer span (one base deleted at 50 and four substituted: 5 edits), not the closer one (3 deleted)
    lf, rf = gap()
    F, A = cut(rng, 160, 50, 1)
    A = flip(A, 20, 89, 99, 109)                       # (F's columns 20, 90, 100, 110)
    _, C3 = F, F[:70] + F[73:]
    add("the runner-up is the longer span", lf, rf, [ctg(lf, rf, F), ctg(lf, rf, C3), ctg(lf, rf, A)], (30, 160, 0, 0),
        want(160, rival=2, rival_len=159, lcp=20, lcs=160 - 111, len_min=157, len_max=160, n=3, near=2, dist=5, flags=LENGTH_VARIES),
        [W(160), (157, 3, NEAR, 0), (159, 5, NEAR, 0)])
    # three peers: identical, far (every column differs), near; far and near have the winner's span, the earlier one is the rival
    lf, rf = gap()
    F = rnd(rng, 180)
    add("identical, far and near", lf, rf, [ctg(lf, rf, F), ctg(lf, rf, F, 31, 30), ctg(lf, rf, F.translate(_NEXT)), ctg(lf, rf, flip(F, 90))],
        (30, 180, 0, 0), want(180, rival=2, rival_len=180, lcp=0, lcs=0, n=4, identical=1, near=1, far=1, dist=DIST_FAR),
        [W(180), (180, DIST_FAR, IDENTICAL, 0), (180, DIST_FAR, FAR, 0), (180, 1, NEAR, 0)])
    # levels: a short-level candidate under a long-level winner; a winner at the short level only; a long-level candidate over a word of
    # the short level
    lf, rf = gap()
    F = rnd(rng, 100)
    add("lower", lf, rf, [broken(lf, rf, flip(F, 5)), ctg(lf, rf, F)], (30, 100, 1, 0), want(100, contig=1, n=2, lower=1), [(100, DIST_FAR, LOWER, 0), W(100)])
    lf, rf = gap()
    F = rnd(rng, 100)
    add("short level only", lf, rf, [broken(lf, rf, F), broken(lf, rf, flip(F, 99))], (15, 100, 0, 0),
        want(100, rival=1, rival_len=100, lcp=99, lcs=0, n=2, near=1, dist=1, level=15), [W(100), (100, 1, NEAR, 0)])
    lf, rf = gap()
    F = rnd(rng, 100)
    add("outranked by a higher level", lf, rf, [broken(lf, rf, F), ctg(lf, rf, F)], (15, 100, 0, 0), want(100, n=2, level=15, flags=OUTRANKED),
        [W(100), ZERO], doctored=True)
    # lost: the word names a contig of another gap (the first case's), a tombstone, or has the wrong span
    lf, rf = gap()
    F = rnd(rng, 60)
    add("lost: another gap's contig", lf, rf, [ctg(lf, rf, F)], (30, 60, ("one candidate", 0), 0), dict(level=30, flags=LOST), [ZERO], doctored=True)
    lf, rf = gap()
    add("lost: a tombstone", lf, rf, [ctg(lf, rf, F)], (30, 60, 1, 0), dict(level=30, flags=LOST), [ZERO], tombstones=[ctg(lf, rf, F)], doctored=True)
    lf, rf = gap()
    add("lost: the wrong span", lf, rf, [ctg(lf, rf, F)], (30, 61, 0, 0), dict(level=30, flags=LOST), [ZERO], doctored=True)
    lf, rf = gap()
    add("lost: the wrong strand", lf, rf, [ctg(lf, rf, F)], (30, 60, 0, 1), dict(level=30, flags=LOST), [ZERO], doctored=True)
    # an open gap
    lf, rf = gap()
    add("open gap", lf, rf, [ctg(lf, rf, F), ctg(lf, rf, flip(F, 3))], None, None, [ZERO, ZERO], doctored=True)
    # an N in the fill is a byte like any other, and its own complement
    lf, rf = gap()
    F = rnd(rng, 110)
    F = F[:10] + "N" + F[11:]
    add("N in the fill", lf, rf, [ctg(lf, rf, F), rc(ctg(lf, rf, flip(F, 70))), ctg(lf, rf, F[:10] + "A" + F[11:])], (30, 110, 0, 0),
        want(110, rival=1, rival_len=110, lcp=70, lcs=39, n=3, near=2, dist=1, flags=RIVAL_REVERSE), [W(110), (110, 1, NEAR, 1), (110, 1, NEAR, 0)])
    # a left flank exactly as long as the long anchor: a contig with the left anchor forward and the whole pair reverse has no pair at 30
    # (the forward hit hides the reverse one) but one at 15, where the flank is longer than the anchor; with a longer flank it is a peer
    for n_l, name in ((30, "whole flank"), (400, "flank longer than the anchor")):
        lf, rf = gap(n_l=n_l)
        F = rnd(rng, 90)
        odd = lf[-30:] + rnd(rng, 20) + rc(lf[-30:] + flip(F, 44) + rf[:40])
        if n_l == 30:
            add(name, lf, rf, [lf + F + rf[:40], odd], (30, 90, 0, 0), want(90, n=2, lower=1), [W(90), (90, DIST_FAR, LOWER, 1)])
        else:
            add(name, lf, rf, [ctg(lf, rf, F), odd], (30, 90, 0, 0), want(90, rival=1, rival_len=90, lcp=44, lcs=45, n=2, near=1, dist=1, flags=RIVAL_REVERSE),
                [W(90), (90, 1, NEAR, 1)])
    # the right anchor a second time, 60 bases further right: the rightmost counts, that contig has the longer span and wins
    lf, rf = gap()
    F = rnd(rng, 50)
    add("an anchor twice", lf, rf, [ctg(lf, rf, F), ctg(lf, rf, F) + rnd(rng, 20) + rf[:30]], (30, 110, 1, 0),
        want(110, contig=1, rival=0, rival_len=50, lcp=50, lcs=0, len_min=50, len_max=110, n=2, far=1, dist=DIST_FAR, flags=LENGTH_VARIES),
        [(50, DIST_FAR, FAR, 0), W(110)])
    return out


def assemble(cs, interleave=True):
    """The cases as one contig list: ([(gap, text)], [(lf, rf)], best words, {(case index, relative contig): list index}).  interleave: the
    contigs of the gaps alternate (every gap's contigs keep their order), so that each gap's neighbours in the list are decoys of other
    gaps; a tombstone carries gap 0xFFFFFFFF and follows its case's contigs in the relative numbering."""
    items = []
    for g, c in enumerate(cs):
        items += [(n, g, g, t) for n, t in enumerate(c["contigs"])] + [(len(c["contigs"]) + n, g, 0xFFFFFFFF, t) for n, t in enumerate(c["tombstones"])]
    items.sort(key=(lambda x: (x[0], -x[1])) if interleave else (lambda x: (x[1], x[0])))
    index = {(g, n): at for at, (n, g, _, _) in enumerate(items)}
    names = {c["name"]: g for g, c in enumerate(cs)}
    best = []
    for g, c in enumerate(cs):
        if c["best"] is None:
            best.append(0)
            continue
        level, span, rel, strand = c["best"]
        ci = index[(names[rel[0]], rel[1])] if isinstance(rel, tuple) else index[(g, rel)]
        best.append(level << 56 | (span + 1) << 32 | (0x7FFFFFFF - ci) << 1 | strand)
    return [(gap, t) for _, _, gap, t in items], [(c["lf"], c["rf"]) for c in cs], best, index


def expected(cs, index):
    """(records as dictionaries with list indices, None for the zero record; per-contig records {list index: tuple}; the statistics the
    records add up to)"""
    recs, per = [], {}
    st = dict.fromkeys(("closed_gaps", "contested", "length_varies", "candidates", "lower", "identical", "near", "far", "outranked", "lost"), 0)
    for g, c in enumerate(cs):
        w = c["want"]
        for n, p in enumerate(c["per"]):
            per[index[(g, n)]] = p
        for n in range(len(c["tombstones"])):
            per[index[(g, len(c["contigs"]) + n)]] = ZERO
        if w is None:
            recs.append(None)
            continue
        st["closed_gaps"] += 1
        if w["flags"] & LOST:
            st["lost"] += 1
            recs.append(dict(w))
            continue
        recs.append(dict(w, contig=index[(g, w["contig"])], rival=index[(g, w["rival"])] if w["flags"] & HAS_RIVAL else 0))
        st["contested"] += bool(w["flags"] & HAS_RIVAL)
        st["length_varies"] += bool(w["flags"] & LENGTH_VARIES)
        st["outranked"] += bool(w["flags"] & OUTRANKED)
        for k, f in (("candidates", "n_candidates"), ("lower", "n_lower"), ("identical", "n_identical"), ("near", "n_near"), ("far", "n_far")):
            st[k] += w[f]
    return recs, per, st
