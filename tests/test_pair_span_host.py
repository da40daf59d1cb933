"""The host twin of the pair-span round (gappadder_amd/pair_span.py: pair_span_host) on seeded cases built from a truth sequence: read
pairs are sampled FR at KNOWN coordinates with inserts drawn around (mean, sd), every row's place on the contig under test follows from
where it was planted, and the expected record is a brute-force restatement of the definition over those planted places (_expect) that
never calls polish.placements.  (a) contig = truth, one pair exactly at lo and one exactly at hi; (b) 60 bases deleted from the body;
(c) a chimeric contig; (d) an inverted segment; (e) a mate absent from the pool, a mate ambiguous in a tandem repeat, N-masked rows, an
empty pool, an empty body, both mates overhanging the contig's ends; skipped contigs; parameter validation."""
import numpy as np
import pytest

from gappadder_amd import _lib as B
from gappadder_amd import pair_span as PS
from gappadder_amd.pick_contigs import revcomp

L, MEAN, SD, Z = 150, 400, 20, 3
LO, HI = MEAN - Z * SD, MEAN + Z * SD


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _pair(truth, p_f, insert):
    """The two reads of an FR pair on `truth`: the forward mate at p_f, the reverse mate ending at p_f + insert."""
    return truth[p_f:p_f + L], revcomp(truth[p_f + insert - L:p_f + insert])


class Pool:
    """Rows with their ids and, per row, where the row was planted on the contig under test: (strand, d), "ambiguous" or None."""

    def __init__(self, rng):
        self.rng, self.reads, self.ids, self.where, self.inserts, self.next_pair = rng, [], [], [], {}, 0

    def add(self, truth, p_f, insert, place, keep=(True, True)):
        """One pair from `truth`; place(p, strand) -> the row's planted place on the contig for a read at truth[p:p + L] read on
        `strand`; the forward mate is mate 0 or mate 1 at random; keep: which of the two reads are in the pool."""
        fwd, rev = _pair(truth, p_f, insert)
        pair, flip = self.next_pair, int(self.rng.integers(0, 2))
        self.next_pair += 1 + int(self.rng.integers(0, 3))            # (ids with holes)
        for read, side, at in ((fwd, flip, place(p_f, 0)), (rev, flip ^ 1, place(p_f + insert - L, 1))):
            if keep[0 if read is fwd else 1]:
                self.reads.append(read)
                self.ids.append(2 * pair + side)
                self.where.append(at)
        self.inserts[pair] = insert
        return pair

    def rows(self):
        """(reads, ids, where) in the pool's order: by (mate side, pair)."""
        order = sorted(range(len(self.ids)), key=lambda i: (self.ids[i] & 1, self.ids[i] >> 1))
        return [self.reads[i] for i in order], [self.ids[i] for i in order], [self.where[i] for i in order]


def _expect(ids, where, n, b0, b1, mean=MEAN, sd=SD, z=Z):
    """The record from the planted places alone: the definition, column by column."""
    rec = np.zeros((), dtype=B.FILL_PAIRS)
    rec["rows"], rec["n_cols"] = len(ids), b1 - b0
    lo, hi = mean - z * sd, mean + z * sd
    cover = [0] * n
    at = dict(zip(ids, where))
    for r in ids:
        if r % 2 == 1 or r + 1 not in at:
            continue
        rec["pairs_complete"] += 1
        a, b = at[r], at[r + 1]
        if not isinstance(a, tuple) or not isinstance(b, tuple):
            continue
        rec["pairs_placed"] += 1
        fwd = [x for x in (a, b) if x[0] == 0]
        back = [x for x in (a, b) if x[0] == 1]
        if len(fwd) != 1 or fwd[0][1] > back[0][1]:
            rec["n_misoriented"] += 1
            continue
        rec["n_proper"] += 1
        first, end = fwd[0][1], back[0][1] + L
        size = end - first
        if size <= lo:
            rec["n_short"] += 1
        elif size >= hi:
            rec["n_long"] += 1
        else:
            rec["n_in_range"] += 1
            for c in range(max(0, first), min(n, end)):
                cover[c] += 1
        if first <= b0 and b1 <= end:
            rec["n_span"] += 1
            rec["span_insert_sum"] += size
    if b1 > b0:
        body = cover[b0:b1]
        rec["min_cover"], rec["min_col"], rec["n_unspanned"] = min(body), b0 + body.index(min(body)), body.count(0)
    return rec


def _same(got, want):
    assert got.tobytes() == want.tobytes(), (got, want)


def _inserts(rng, k):
    return [int(x) for x in np.clip(np.rint(rng.normal(MEAN, SD, k)), 2 * L, MEAN + 6 * SD)]


def test_contig_equals_truth_classes_by_the_strict_bounds():
    rng = np.random.default_rng(101)
    truth = _seq(rng, 1200)
    pool = Pool(rng)
    same = lambda p, strand: (strand, p)
    for ins in _inserts(rng, 80):
        pool.add(truth, int(rng.integers(0, len(truth) - ins + 1)), ins, same)
    at_lo = pool.add(truth, 300, LO, same)
    at_hi = pool.add(truth, 310, HI, same)
    pool.add(truth, 320, LO + 1, same)
    pool.add(truth, 330, HI - 1, same)
    reads, ids, where = pool.rows()
    b0, b1 = 500, 700
    rec, placed = PS.pair_span_host(reads, ids, truth, b0, b1, MEAN, SD, detail=True)
    assert [w[:2] for w in placed] == where                           # every row where it was planted
    _same(rec, _expect(ids, where, len(truth), b0, b1))
    assert int(rec["pairs_complete"]) == int(rec["pairs_placed"]) == int(rec["n_proper"]) == 84 and int(rec["n_misoriented"]) == 0
    others = [i for p, i in pool.inserts.items() if p not in (at_lo, at_hi)]
    assert int(rec["n_short"]) == 1 + sum(i <= LO for i in others) and int(rec["n_long"]) == 1 + sum(i >= HI for i in others)
    assert int(rec["n_in_range"]) == 84 - int(rec["n_short"]) - int(rec["n_long"]) and int(rec["n_span"]) > 0
    assert int(rec["min_cover"]) > 0 and int(rec["n_unspanned"]) == 0
    # the bounds move with z: at z = 4 the two pairs at the old bounds are in range
    wide = PS.pair_span_host(reads, ids, truth, b0, b1, MEAN, SD, z=4)
    _same(wide, _expect(ids, where, len(truth), b0, b1, z=4))
    assert int(wide["n_in_range"]) >= int(rec["n_in_range"]) + 2


def test_a_deletion_lowers_the_spanning_inserts_by_its_length():
    rng = np.random.default_rng(202)
    truth = _seq(rng, 1400)
    x, cut = 700, 60
    contig = truth[:x] + truth[x + cut:]
    b0, b1 = 620, 760
    place = lambda p, strand: (strand, p if p + L <= x else p - cut)
    pool = Pool(rng)
    for ins in _inserts(rng, 400):
        p = int(rng.integers(0, len(truth) - ins + 1))
        q = p + ins - L
        if all(a + L <= x or a >= x + cut for a in (p, q)):           # no read holds a deleted base or straddles the cut
            pool.add(truth, p, ins, place)
    reads, ids, where = pool.rows()
    rec, placed = PS.pair_span_host(reads, ids, contig, b0, b1, MEAN, SD, detail=True)
    assert [w[:2] for w in placed] == where
    _same(rec, _expect(ids, where, len(contig), b0, b1))
    at = dict(zip(ids, where))
    spanning = [p for p in pool.inserts if min(at[2 * p][1], at[2 * p + 1][1]) <= b0 and b1 <= max(at[2 * p][1], at[2 * p + 1][1]) + L]
    assert len(spanning) == int(rec["n_span"]) > 10
    assert int(rec["span_insert_sum"]) == sum(pool.inserts[p] for p in spanning) - cut * len(spanning)
    pushed = [p for p in spanning if pool.inserts[p] > LO and pool.inserts[p] - cut <= LO]
    on_truth = PS.pair_span_host(*_on_truth(pool, truth), truth, b0, b1 + cut, MEAN, SD)
    assert pushed and int(rec["n_short"]) == int(on_truth["n_short"]) + len(pushed)


def _on_truth(pool, truth):
    """The pool's rows and ids (the reads are the truth's own: they place where they were sampled)."""
    reads, ids, _ = pool.rows()
    return reads, ids


def test_a_chimeric_contig_is_unspanned_at_the_join():
    rng = np.random.default_rng(303)
    ta, tb = _seq(rng, 1300), _seq(rng, 1300)
    h = 650
    contig = ta[:h] + tb[h:]
    b0, b1 = h - 150, h + 150
    pool = Pool(rng)
    left = lambda p, strand: (strand, p) if p + L <= h else None      # a read of A right of the join has no place on the contig
    right = lambda p, strand: (strand, p) if p >= h else None
    pool.add(ta, h - 3 - 380, 380, left)                              # the last pair before the join ends at h - 3,
    pool.add(tb, h + 2, 410, right)                                   # the first after it starts at h + 2
    for ins in _inserts(rng, 300):
        p = int(rng.integers(0, len(ta) - ins + 1))
        q = p + ins - L
        if p + L <= h - 3 and q + L <= h - 3:
            pool.add(ta, p, ins, left)
        elif p >= h + 2:
            pool.add(tb, p, ins, right)
        elif p + L <= h - 3 and q >= h + 2 and len(pool.ids) % 3 == 0:
            pool.add(ta, p, ins, left)                                # a pair of A across the join: its reverse mate is not placed
    reads, ids, where = pool.rows()
    rec, placed = PS.pair_span_host(reads, ids, contig, b0, b1, MEAN, SD, detail=True)
    assert [None if w is None else w[:2] for w in placed] == where
    _same(rec, _expect(ids, where, len(contig), b0, b1))
    assert int(rec["pairs_complete"]) > int(rec["pairs_placed"]) and int(rec["n_span"]) == 0
    assert int(rec["min_cover"]) == 0 and int(rec["min_col"]) == h - 3 and int(rec["n_unspanned"]) == 5


def test_an_inverted_segment_gives_misoriented_pairs():
    rng = np.random.default_rng(404)
    truth = _seq(rng, 1500)
    x, y = 500, 1000
    contig = truth[:x] + revcomp(truth[x:y]) + truth[y:]
    place = lambda p, strand: (strand, p) if p + L <= x or p >= y else (1 - strand, x + y - p - L)
    pool = Pool(rng)
    for ins in _inserts(rng, 300):
        p = int(rng.integers(0, len(truth) - ins + 1))
        if all(a + L <= x or a >= y or (x <= a and a + L <= y) for a in (p, p + ins - L)):
            pool.add(truth, p, ins, place)
    reads, ids, where = pool.rows()
    b0, b1 = 450, 1050
    rec, placed = PS.pair_span_host(reads, ids, contig, b0, b1, MEAN, SD, detail=True)
    assert [w[:2] for w in placed] == where
    _same(rec, _expect(ids, where, len(contig), b0, b1))
    assert int(rec["n_misoriented"]) > 5 and int(rec["n_proper"]) > 5 and int(rec["pairs_placed"]) == int(rec["pairs_complete"])


def test_edges_absent_ambiguous_masked_empty_and_overhanging():
    rng = np.random.default_rng(505)
    unit = _seq(rng, 200)
    wide = _seq(rng, 300) + _seq(rng, 400) + unit * 3 + _seq(rng, 500) + _seq(rng, 300)
    off, n = 300, 1500
    contig = wide[off:off + n]                                        # the repeat at [400, 1000) of the contig
    rep0, rep1 = 400, 1000
    pool = Pool(rng)

    def place(p, strand):
        d = p - off
        if min(L, n - d) - max(0, -d) < PS.MIN_OVERLAP:
            return None
        inside = rep0 <= d and d + L <= rep1
        return "ambiguous" if inside else (strand, d)
    pool.add(wide, off + 20, 390, place, keep=(True, False))          # a mate absent from the pool
    pool.add(wide, off + 30, 405, place, keep=(False, True))
    pool.add(wide, off + 1100, 395, place)                            # a plain pair right of the repeat
    amb = pool.add(wide, off + 100, 400 + 150, place)                 # forward mate unique, reverse mate inside the repeat
    pool.add(wide, off + 450, 380, place)                             # both mates inside the repeat
    over = pool.add(wide, off - 40, 410, place)                       # the forward mate overhangs the contig's start,
    over2 = pool.add(wide, off + n + 30 - 395, 395, place)            # the reverse mate its end
    both = pool.add(wide, off - 60, 420, place)
    gone = pool.add(wide, off - 120, 400, place)                      # 30 bases of overlap: unplaced
    masked = pool.add(wide, off + 1150, 402, place)
    dead = pool.add(wide, off + 1160, 398, place)
    reads, ids, where = pool.rows()
    for r, how in ((2 * masked, [5]), (2 * dead + 1, list(range(8, L, 16)))):
        i = ids.index(r)
        reads[i] = "".join("N" if k in how else c for k, c in enumerate(reads[i]))
    where[ids.index(2 * dead + 1)] = None                             # an N in every seed window: no clean seed, unplaced
    b0, b1 = 0, n                                                     # the whole contig: the clipped spans reach column 0 and column n - 1
    rec, placed = PS.pair_span_host(reads, ids, contig, b0, b1, MEAN, SD, detail=True)
    assert [w if not isinstance(w, tuple) else w[:2] for w in placed] == where
    _same(rec, _expect(ids, where, n, b0, b1))
    at = dict(zip(ids, where))
    assert at[2 * over][1] == -40 or at[2 * over + 1][1] == -40
    assert max(at[2 * over2][1], at[2 * over2 + 1][1]) + L == n + 30 and None in (at[2 * gone], at[2 * gone + 1])
    assert "ambiguous" in (at[2 * amb], at[2 * amb + 1]) and min(at[2 * both][1], at[2 * both + 1][1]) == -60
    assert int(rec["pairs_complete"]) == 9 and int(rec["pairs_placed"]) == 5 and int(rec["n_in_range"]) == 5
    assert int(rec["n_span"]) == 0 and int(rec["min_cover"]) == 0 and int(rec["n_unspanned"]) > 0
    # an empty body: the three coverage fields are 0, a pair over the point spans it
    empty = PS.pair_span_host(reads, ids, contig, 1250, 1250, MEAN, SD)
    _same(empty, _expect(ids, where, n, 1250, 1250))
    assert int(empty["n_cols"]) == int(empty["min_cover"]) == int(empty["min_col"]) == int(empty["n_unspanned"]) == 0 and int(empty["n_span"]) >= 1
    # an empty pool
    none = PS.pair_span_host([], [], contig, 100, 300, MEAN, SD)
    _same(none, _expect([], [], n, 100, 300))
    assert int(none["n_cols"]) == 200 and int(none["n_unspanned"]) == 200 and int(none["min_col"]) == 100 and int(none["rows"]) == 0


def test_skipped_contigs_carry_a_flag_and_the_rows():
    rng = np.random.default_rng(606)
    truth = _seq(rng, 600)
    pool = Pool(rng)
    pool.add(truth, 50, 400, lambda p, s: (s, p))
    reads, ids, _ = pool.rows()
    for contig, flag in ((truth[:200] + "N" + truth[201:], B.PS_F_NON_ACGT), (_seq(rng, PS.MAX_CONTIG + 1), B.PS_F_LONG)):
        rec = PS.pair_span_host(reads, ids, contig, 100, 300, MEAN, SD)
        want = np.zeros((), dtype=B.FILL_PAIRS)
        want["flags"], want["rows"] = flag, 2
        _same(rec, want)
    assert int(PS.pair_span_host(reads, ids, _seq(rng, PS.MAX_CONTIG), 100, 300, MEAN, SD)["flags"]) == 0


def test_parameters_out_of_range_raise():
    ok = dict(seed=16, max_mismatch=4, min_overlap=48, z=3, is_sd=30)
    assert PS.check_params(150, **ok) == (16, 4, 48, 3)
    for bad in (dict(seed=11), dict(seed=33), dict(max_mismatch=-1), dict(max_mismatch=16), dict(min_overlap=15), dict(min_overlap=151),
                dict(z=0), dict(z=-2), dict(z=2.5), dict(is_sd=-1), dict(seed=32, max_mismatch=4), dict(seed=20, max_mismatch=7)):
        with pytest.raises(ValueError, match="pair_span"):
            PS.check_params(150, **dict(ok, **bad))
    with pytest.raises(ValueError, match="pair_span"):
        PS.pair_span_host(["A" * 150], [0], "ACGT" * 100, 10, 20, 400, -5)
    with pytest.raises(ValueError, match="pair_span"):
        PS.pair_span_host(["A" * 150], [0], "ACGT" * 100, 10, 20, 400, 20, z=0)
    assert PS.span_mean_minus_is({"span_insert_sum": -7, "n_span": 2}, 10) == -14 and PS.span_mean_minus_is({"span_insert_sum": 0, "n_span": 0}, 10) is None
