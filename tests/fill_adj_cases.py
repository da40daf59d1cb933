"""Hand-built cases of the read adjudication (gappadder_amd/fill_adjudication.py), one contested gap each, shared by the
host test and the device test.  A gap has random flanks LF, RF (400 bases unless the case says otherwise) and two oriented fills F_w
(the winner's) and F_r (the rival's); G_w = LF + F_w + RF and G_r = LF + F_r + RF are the two haplotypes, and every pool row is an exact
copy of L bases of one of them at a stated start (a coordinate of G; the fill begins at len(LF)), given as it is or reverse-complemented
(`turned`), with the stated read positions replaced by N (a masked base).  The locus of a fill is G[len(LF) - C : len(LF) + len(F) + C]
with C = L (the default context).  Parameters of the expectations: seed 16, max_mismatch 4, min_overlap 48, min_votes 3, ratio 2.

What makes the answers derivable by hand: the sequences are random, so a row fits a locus only on its own diagonal (and, in a tandem
repeat, on the diagonals a whole number of units away); on that diagonal the mismatches are the differing columns the row covers —
one for a substitution; for an all-different rival fill (`unlike`) the number of fill columns covered; at the edge of a repeat array
whose neighbours differ from the unit in EVERY column, the number of columns the row reaches beyond the shorter array.  A row whose
overlap with the locus is below 48 bases, or that has a masked base in every one of its L // 16 seed windows, has no accepted pair."""
import random

import fill_alt_cases as AC

rc, rnd, flip = AC.rc, AC.rnd, AC.flip
SEED, MAX_MISMATCH, MIN_OVERLAP, MIN_VOTES, RATIO = 16, 4, 48, 3, 2
KEEP, SWITCH, UNDECIDED = 1, 2, 3
LONG, NON_ACGT, RIVAL_FAR, NO_ROWS = 1, 2, 4, 8
MAX_LOCUS = 8192
COUNTERS = ("votes_w", "votes_r", "votes_w_s0", "votes_r_s0", "ties", "unplaced", "only")
_NEXT = str.maketrans("ACGT", "CGTA")


def unlike(s):
    """A text that differs from s in every column."""
    return s.translate(_NEXT)


def want(locus_w, locus_r, verdict, flags=0, **counters):
    out = dict(locus_w=locus_w, locus_r=locus_r, verdict=verdict, flags=flags)
    out.update({k: counters.get(k, 0) for k in COUNTERS})
    return out


def rows(G, L, starts, turned=(), masked=None):
    """The rows G[s : s + L] for s in starts; the x-th is reverse-complemented when x is in `turned`, and has N at the read positions
    masked[x] (positions of the row as it is cut from G, before it is turned)."""
    out = []
    for x, s in enumerate(starts):
        r = list(G[s:s + L])
        assert len(r) == L
        for p in (masked or {}).get(x, ()):
            r[p] = "N"
        r = "".join(r)
        out.append(rc(r) if x in turned else r)
    return out


def cases(seed=20260026):
    """[{name, L, lf, rf, fill_w, fill_r, turn_w, turn_r (the contig is stored reverse-complemented), reads, rival_far, want}]"""
    rng = random.Random(seed)
    out = []

    def add(name, L, lf, rf, fill_w, fill_r, reads, want_, turn_w=False, turn_r=False, rival_far=False):
        out.append(dict(name=name, L=L, lf=lf, rf=rf, fill_w=fill_w, fill_r=fill_r, reads=list(reads), want=want_, turn_w=turn_w, turn_r=turn_r,
                        rival_far=rival_far))

    # ---- L = 150, C = 150: the locus is G[250 : 550 + len(F)], 420 bases for a fill of 120
    # a substitution at fill column 60 = G column 460.  A row [s, s + 150) covers it for 311 <= s <= 460: it has 0 mismatches on its own
    # haplotype's locus and 1 on the other, the same overlap on both: a vote.  A row that does not cover it has equal keys: a tie (240:
    # overlap 140 on both; 600: overlap 70 on both).  640: overlap 30 < 48, 100: overlap 0: unplaced on both.
    starts = [240, 300, 311, 350, 400, 459, 460, 461, 520, 600, 640, 100]
    sub = want(420, 420, KEEP, votes_w=5, votes_w_s0=3, ties=5, unplaced=2)       # votes: 311, 350, 400, 459, 460; turned: 350, 459
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("substitution, the winner's allele in the pool", 150, lf, rf, F, flip(F, 60), rows(lf + F + rf, 150, starts, turned=(3, 5)), sub)
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("substitution, the rival's allele in the pool", 150, lf, rf, F, flip(F, 60), rows(lf + flip(F, 60) + rf, 150, starts, turned=(3, 5)),
        want(420, 420, SWITCH, votes_r=5, votes_r_s0=3, ties=5, unplaced=2))
    # two votes only: below min_votes
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("votes below min_votes", 150, lf, rf, F, flip(F, 60), rows(lf + F + rf, 150, [300, 350, 400, 520]), want(420, 420, UNDECIDED, votes_w=2, votes_w_s0=2, ties=2))
    # four rows of the winner's allele and three of the rival's over the column: 4 >= 3 but 4 < 2 * 3, and 3 < 2 * 4
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("votes below the ratio", 150, lf, rf, F, flip(F, 60),
        rows(lf + F + rf, 150, [320, 360, 400, 440]) + rows(lf + flip(F, 60) + rf, 150, [330, 370, 410], turned=(0,)),
        want(420, 420, UNDECIDED, votes_w=4, votes_w_s0=4, votes_r=3, votes_r_s0=2))
    # a tandem repeat: A (40) + n units U (10) + B (40), n = 6 in the longer fill (array G[440:500)) and 5 in the shorter (G[440:490));
    # the 10 bases before the array and the 10 behind it differ from U in every column.  Rows of the LONGER haplotype on the SHORTER
    # locus: one that enters the array from the left and ends x columns behind the shorter array (x = s + 150 - 490) has x mismatches
    # there: 340: x = 0, a tie; 341: x = 1, a vote (placed on both); 346: x = 6 > 4: no pair on the shorter locus.  One that starts x
    # columns before the place where the shorter array would begin (x = 450 - s), the same: 450: a tie; 449: 1 mismatch; 380 and 430
    # span the whole array: on either diagonal of the shorter locus a whole unit lies on 10 differing columns: no pair.  300 (10 columns
    # into the array) and 520 (behind it) fit both: ties.
    starts = [300, 340, 341, 346, 380, 430, 449, 450, 520]
    for name, longer_wins in (("an inserted repeat unit, its reads in the pool", True), ("a deleted repeat unit, the longer allele in the pool", False)):
        lf, rf, U = rnd(rng, 400), rnd(rng, 400), rnd(rng, 10)
        A, Bt = rnd(rng, 30) + unlike(U), unlike(U) + rnd(rng, 30)
        longer, shorter = A + U * 6 + Bt, A + U * 5 + Bt
        votes = dict(ties=4, only=3)                                             # ties: 300, 340, 450, 520; only: 346, 380, 430
        if longer_wins:
            add(name, 150, lf, rf, longer, shorter, rows(lf + longer + rf, 150, starts, turned=(4,)),
                want(440, 430, KEEP, votes_w=5, votes_w_s0=4, **votes))
        else:
            add(name, 150, lf, rf, shorter, longer, rows(lf + longer + rf, 150, starts, turned=(4,)),
                want(430, 440, SWITCH, votes_r=5, votes_r_s0=4, **votes))
    # a FAR rival: a fill that differs from the winner's in every column.  A row of the winner's haplotype has as many mismatches on the
    # rival's locus as fill columns it covers: 254 covers 4 (G[400:404)): placed on both, a vote; 255 covers 5: no pair there; 300 and 400
    # likewise; 517 covers 3 (G[517:520)): a vote; 520 covers none: a tie
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("a FAR rival", 150, lf, rf, F, unlike(F), rows(lf + F + rf, 150, [254, 255, 300, 400, 517, 520], turned=(1,)),
        want(420, 420, KEEP, RIVAL_FAR, votes_w=5, votes_w_s0=4, ties=1, only=3), rival_far=True)
    # both contigs stored reverse-complemented: the oriented fills, so everything, as in the first case
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("reverse-strand winner and rival", 150, lf, rf, F, flip(F, 60), rows(lf + F + rf, 150, [240, 300, 311, 350, 400, 459, 460, 461, 520, 600, 640, 100], turned=(3, 5)),
        sub, turn_w=True, turn_r=True)
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("a reverse-strand rival, every row reverse-complemented", 150, lf, rf, F, flip(F, 60), rows(lf + F + rf, 150, [300, 311, 350, 400, 460, 461], turned=range(6)),
        want(420, 420, KEEP, votes_w=4, ties=2), turn_r=True)
    # a left flank of 60 bases: used whole, the locus is G[0 : 60 + 120 + 150]; the substitution at fill column 30 = G column 90 is
    # covered by the rows at 0, 20 and 60, not by 91 and 180
    lf, rf, F = rnd(rng, 60), rnd(rng, 400), rnd(rng, 120)
    add("a flank shorter than the context", 150, lf, rf, F, flip(F, 30), rows(lf + F + rf, 150, [0, 20, 60, 91, 180]),
        want(330, 330, KEEP, votes_w=3, votes_w_s0=3, ties=2))
    # an N in the left flank, 50 bases before the gap: inside the context, outside the anchors: skipped; 160 bases before it: outside
    for at, w in ((50, want(420, 420, 0, NON_ACGT)), (160, want(420, 420, KEEP, votes_w=3, votes_w_s0=3, ties=1))):
        lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
        G = lf + F + rf
        lf = lf[:400 - at] + "N" + lf[400 - at + 1:]
        add("an N in the left flank, %d bases before the gap" % at, 150, lf, rf, F, flip(F, 60), rows(G, 150, [320, 380, 440, 520]), w)
    # loci of exactly 8 192 bases (a substitution at fill column 4 000 = G column 4 400), and a rival one base longer: 8 193, skipped
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, MAX_LOCUS - 300)
    add("loci of 8192 bases", 150, lf, rf, F, flip(F, 4000), rows(lf + F + rf, 150, [4251, 4300, 4400, 4401, 8000], turned=(1,)),
        want(MAX_LOCUS, MAX_LOCUS, KEEP, votes_w=3, votes_w_s0=2, ties=2))
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, MAX_LOCUS - 300)
    add("a rival's locus of 8193 bases", 150, lf, rf, F, F[:4000] + unlike(F[4000]) + F[4000:], rows(lf + F + rf, 150, [4300, 4400]),
        want(MAX_LOCUS, MAX_LOCUS + 1, 0, LONG))
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("an empty pool", 150, lf, rf, F, flip(F, 60), [], want(420, 420, UNDECIDED, NO_ROWS))

    # ---- L = 100, C = 100: the locus is G[300 : 500 + len(F)], 320 bases for a fill of 120; six seed windows [16 j, 16 j + 16), j < 6
    # masked bases, the substitution at G column 460: 380 covers it at read position 80, which is masked: 0 mismatches on both loci, a
    # tie.  400: one N in the first seed window, the column unmasked: a vote.  420: an N in every seed window: no pair on either
    # locus.  430, 440 (turned), 450: votes.  300: does not cover the column: a tie
    lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 120)
    add("masked bases", 100, lf, rf, F, flip(F, 60),
        rows(lf + F + rf, 100, [380, 400, 420, 430, 440, 450, 300], turned=(4,), masked={0: (80,), 1: (5,), 2: (0, 16, 32, 48, 64, 80)}),
        want(320, 320, KEEP, votes_w=4, votes_w_s0=3, ties=2, unplaced=1))
    # a repeat array longer than a read: 7 units of 20 (G[440:580)) against 6 (G[440:560)).  450 lies inside the array: it fits both
    # loci without a mismatch, on two diagonals of the longer (450, 470) and one of the shorter: a tie, whatever the multiplicity.  460
    # likewise; 420 and 370 enter the array from the left and cover 80 and 30 of its columns: ties.  No read spans 120 columns of
    # array: nothing votes.  The fills differ by 20 bases in length, more than the alternatives' max_dist of 16: a FAR rival.
    lf, rf, U = rnd(rng, 400), rnd(rng, 400), rnd(rng, 20)
    A, Bt = rnd(rng, 20) + unlike(U), unlike(U) + rnd(rng, 20)
    add("rows inside a repeat longer than a read", 100, lf, rf, A + U * 7 + Bt, A + U * 6 + Bt, rows(lf + A + U * 7 + Bt + rf, 100, [420, 450, 460, 370], turned=(1,)),
        want(420, 400, UNDECIDED, RIVAL_FAR, ties=4), rival_far=True)
    return out


def assemble(cs):
    """The cases of one read length as a contig list: per case its winner lf[-40:] + F_w + rf[:40] and its rival, each stored as it is or
    reverse-complemented; between the cases an OPEN gap with one contig and an UNCONTESTED gap with two contigs of one fill.
    Returns (contigs [(gap, text)], flanks, best words, reads per gap, {case index: gap})."""
    rng = random.Random(len(cs))
    contigs, flanks, best, reads, gap_of = [], [], [], [], {}
    ctg = lambda lf, rf, F, turn=False: rc(lf[-40:] + F + rf[:40]) if turn else lf[-40:] + F + rf[:40]
    for x, c in enumerate(cs):
        lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 90)
        flanks.append((lf, rf))                                   # open: its contig carries both anchors, its word is zero
        contigs.append((len(flanks) - 1, ctg(lf, rf, F)))
        best.append(0)
        reads.append(rows(lf + F + rf, c["L"], [350, 400]))
        g = len(flanks)
        gap_of[x] = g
        flanks.append((c["lf"], c["rf"]))
        best.append(word(30, len(c["fill_w"]), len(contigs), int(c["turn_w"])))
        contigs += [(g, ctg(c["lf"], c["rf"], c["fill_w"], c["turn_w"])), (g, ctg(c["lf"], c["rf"], c["fill_r"], c["turn_r"]))]
        reads.append(c["reads"])
        lf, rf, F = rnd(rng, 400), rnd(rng, 400), rnd(rng, 90)
        g = len(flanks)
        flanks.append((lf, rf))                                   # uncontested: two contigs, one fill
        best.append(word(30, 90, len(contigs), 0))
        contigs += [(g, ctg(lf, rf, F)), (g, ctg(lf, rf, F, True))]
        reads.append(rows(lf + F + rf, c["L"], [350, 400, 420]))
    return contigs, flanks, best, reads, gap_of


def word(level, span, contig, strand):
    return level << 56 | min(span + 1, 0xFFFFFF) << 32 | (0x7FFFFFFF - contig) << 1 | strand
