"""The host twin of the polish round (gappadder_amd/polish.py: polish_host and what it is made of): four seeded cases with sampled reads
(L = 100, 0.5 % substitution errors), hand-derived answers for every clause of the definition, and the twin's seed-indexed search for
placements against a brute-force restatement of the definition over all diagonals."""
import types

import numpy as np
import pytest

from gappadder_amd import _lib as B
from gappadder_amd import polish as PL
from gappadder_amd.pick_contigs import revcomp


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def _sub(text, at, step=1):
    return text[:at] + _other(text[at], step) + text[at + 1:]


def _sample(rng, truth, n_reads, L=100, err=0.005):
    out = []
    for _ in range(n_reads):
        o = int(rng.integers(0, len(truth) - L + 1))
        r = list(truth[o:o + L])
        for i in np.nonzero(rng.random(L) < err)[0]:
            r[i] = _other(r[i], int(rng.integers(1, 4)))
        r = "".join(r)
        out.append(revcomp(r) if rng.integers(0, 2) else r)
    return out


# ---- the four seeded cases ------------------------------------------------------------------------------------------------------------
def test_planted_substitutions_are_repaired():
    rng = np.random.default_rng(11)
    truth = _seq(rng, 600)
    contig = truth
    for at in (200, 301, 455):
        contig = _sub(contig, at)
    text, rec = PL.polish_host(_sample(rng, truth, 90), contig, 100, 500)
    assert text == truth
    assert int(rec["n_cols"]) == 400 and int(rec["n_changed"]) == 3 and int(rec["n_uncovered"]) == 0 and int(rec["len"]) == 600


def _near_repeat(rng):
    """150 unique + copy 1 + 100 unique + copy 2 + 150 unique; the 150-base copies differ at their positions 50 and 99, which every read
    of 100 bases inside a copy covers."""
    rep = _seq(rng, 150)
    rep2 = _sub(_sub(rep, 50), 99)
    return _seq(rng, 150) + rep + _seq(rng, 100) + rep2 + _seq(rng, 150)


def test_a_near_repeat_is_not_homogenised():
    rng = np.random.default_rng(12)
    truth = _near_repeat(rng)
    text, rec = PL.polish_host(_sample(rng, truth, 200), truth, 100, 600)
    assert text == truth and int(rec["n_changed"]) == 0 and int(rec["n_uncovered"]) == 0
    # a read is ambiguous or unplaced only through its own errors (one on each differing column it covers; more than four): a handful at most
    assert int(rec["reads_placed"]) + int(rec["reads_ambiguous"]) <= 200 and int(rec["reads_placed"]) >= 190


def test_an_error_in_one_copy_of_a_near_repeat_is_repaired_from_its_own_reads():
    rng = np.random.default_rng(13)
    truth = _near_repeat(rng)
    contig = _sub(truth, 150 + 50)             # copy 1 takes copy 2's base at the first differing position
    assert contig[200] == truth[400 + 50]
    text, rec = PL.polish_host(_sample(rng, truth, 200), contig, 100, 600)
    assert text == truth and int(rec["n_changed"]) == 1


def test_an_exact_tandem_repeat_stays_as_it_is():
    rng = np.random.default_rng(14)
    unit = _seq(rng, 120)
    truth = _seq(rng, 150) + unit * 3 + _seq(rng, 150)
    text, rec = PL.polish_host(_sample(rng, truth, 200), truth, 100, 560)
    assert text == truth and int(rec["n_changed"]) == 0
    # a read inside the repeat fits one unit further as well: ambiguous, and the columns only such reads cover have no vote
    assert int(rec["reads_ambiguous"]) > 0 and int(rec["reads_placed"]) > 0 and int(rec["n_uncovered"]) > 0


# ---- hand-derived answers: reads of 48 bases, four seeds of 12 ---------------------------------------------------------------------------
L, S, MM, MO = 48, 12, 3, 24
KW = dict(seed=S, max_mismatch=MM, min_overlap=MO)


@pytest.fixture(scope="module")
def contig():
    return _seq(np.random.default_rng(5), 160)


def _run(reads, contig, b0=30, b1=130, min_votes=2, **kw):
    text, rec, where = PL.polish_host(reads, contig, b0, b1, min_votes=min_votes, detail=True, **dict(KW, **kw))
    return text, rec, where


def test_a_tie_with_the_current_base_changes_nothing(contig):
    alt = _sub(contig, 70)
    reads = [alt[40:88], alt[50:98], contig[45:93], contig[60:108]]
    text, rec, where = _run(reads, contig)
    assert where == [(0, 40, 1, 48), (0, 50, 1, 48), (0, 45, 0, 48), (0, 60, 0, 48)]
    assert text == contig and int(rec["n_changed"]) == 0 and int(rec["reads_placed"]) == 4
    # one more vote for the other base decides it
    text, rec, _ = _run(reads + [alt[30:78]], contig)
    assert text == alt and int(rec["n_changed"]) == 1


def test_min_votes(contig):
    alt = _sub(contig, 70)
    text, rec, _ = _run([alt[40:88]], contig)
    assert text == contig and int(rec["n_changed"]) == 0                       # one vote against none: below min_votes = 2
    text, rec, _ = _run([alt[40:88]], contig, min_votes=1)
    assert text == alt and int(rec["n_changed"]) == 1
    assert int(rec["n_uncovered"]) == 100 - 48 and int(rec["n_cols"]) == 100


def test_a_masked_base_neither_mismatches_nor_votes(contig):
    r = contig[40:88]
    r = r[:30] + "N" + r[31:]
    text, rec, where = _run([r], contig, max_mismatch=0)
    assert where == [(0, 40, 0, 48)]                                            # no mismatch although the contig has a base there
    assert int(rec["n_uncovered"]) == 100 - 47 and text == contig              # and column 70 got no vote
    # a seed with a masked base is no seed: masks in all four windows leave nothing to accept the row by
    r4 = "".join("N" if i % 12 == 5 else c for i, c in enumerate(contig[40:88]))
    assert _run([r4], contig)[2] == [None]


def test_the_mismatch_budget(contig):
    at3, at4 = (45, 57, 69), (45, 57, 69, 70)        # read positions 5, 17, 29(, 30): seed 3 stays clean
    r3, r4 = contig, contig
    for a in at3:
        r3 = _sub(r3, a)
    for a in at4:
        r4 = _sub(r4, a)
    _, rec, where = _run([r3[40:88]], contig)
    assert where == [(0, 40, 3, 48)] and int(rec["reads_placed"]) == 1
    _, rec, where = _run([r4[40:88]], contig)
    assert where == [None] and int(rec["reads_placed"]) == 0


@pytest.mark.parametrize("dirty,clean", [((1, 2, 3), 0), ((0, 1, 2), 3)])
def test_one_clean_seed_is_enough_first_or_last(contig, dirty, clean):
    r = contig
    for j in dirty:
        r = _sub(r, 40 + 12 * j + 6)
    assert r[40 + 12 * clean:52 + 12 * clean] == contig[40 + 12 * clean:52 + 12 * clean]
    assert _run([r[40:88]], contig)[2] == [(0, 40, 3, 48)]
    assert _run([revcomp(r[40:88])], contig)[2] == [(1, 40, 3, 48)]


def test_clean_seeds_outside_the_overlap_do_not_count(contig):
    rng = np.random.default_rng(6)
    head = _seq(rng, 24)                              # overhangs the contig's left end: seeds 0 and 1 lie outside the overlap
    body = contig[:24]
    assert _run([head + body], contig)[2] == [(0, -24, 0, 24)]
    dirty = _sub(_sub(body, 6), 18)                   # one mismatch in seed 2, one in seed 3: two mismatches, within the budget, no clean seed inside
    assert _run([head + dirty], contig)[2] == [None]
    assert _run([head + _sub(body, 6)], contig)[2] == [(0, -24, 1, 24)]


def test_read_length_not_a_multiple_of_the_seed(contig):
    rng = np.random.default_rng(7)
    kw = dict(min_overlap=12)
    # 50 bases: seeds [0, 12) .. [36, 48); two more bases belong to no seed
    left = _seq(rng, 38) + contig[:12]                # overlap [38, 50): 12 equal bases, but seed 3 = [36, 48) is not wholly inside
    assert _run([left], contig, **kw)[2] == [None]
    right = contig[148:] + _seq(rng, 38)              # overlap [0, 12) = seed 0
    assert _run([right], contig, **kw)[2] == [(0, 148, 0, 12)]
    inner = _sub(_sub(_sub(contig, 46), 58), 70)[40:90]       # read positions 6, 18, 30
    assert _run([inner], contig, **kw)[2] == [(0, 40, 3, 50)]


def test_overhanging_rows_vote_at_both_ends(contig):
    rng = np.random.default_rng(8)
    n = len(contig)
    alt = _sub(_sub(contig, 6), n - 7)
    reads = [_seq(rng, 20) + alt[:28], _seq(rng, 10) + alt[:38], alt[n - 30:] + _seq(rng, 18), revcomp(alt[n - 40:] + _seq(rng, 8))]
    text, rec, where = _run(reads, contig, b0=5, b1=n - 5)
    assert where == [(0, -20, 1, 28), (0, -10, 1, 38), (0, n - 30, 1, 30), (1, n - 40, 1, 40)]
    assert text == alt and int(rec["n_changed"]) == 2
    # outside the body nothing changes, whatever the votes
    text, rec, _ = _run(reads, contig, b0=7, b1=n - 7)
    assert text == contig and int(rec["n_changed"]) == 0


def test_a_palindromic_row_is_ambiguous():
    rng = np.random.default_rng(9)
    half = _seq(rng, 24)
    pal = half + revcomp(half)
    assert revcomp(pal) == pal
    c = _seq(rng, 50) + pal + _seq(rng, 50)
    text, rec, where = _run([pal, pal, pal], c, b0=20, b1=120)
    assert where == ["ambiguous"] * 3 and text == c
    assert int(rec["reads_ambiguous"]) == 3 and int(rec["reads_placed"]) == 0 and int(rec["n_uncovered"]) == 100


def test_a_row_in_an_exact_repeat_is_ambiguous_and_best_of_decides_a_near_repeat():
    rng = np.random.default_rng(10)
    rep = _seq(rng, 48)
    c = _seq(rng, 30) + rep + _seq(rng, 20) + rep + _seq(rng, 30)
    assert _run([rep], c)[2] == ["ambiguous"]
    c2 = _seq(rng, 30) + rep + _seq(rng, 20) + _sub(rep, 20) + _seq(rng, 30)
    assert _run([rep, _sub(rep, 20)], c2)[2] == [(0, 30, 0, 48), (0, 98, 0, 48)]


def test_a_reverse_pick_is_the_forward_pick_on_the_reverse_complement():
    rng = np.random.default_rng(15)
    truth = _seq(rng, 600)
    contig = _sub(_sub(truth, 210), 390)
    reads = _sample(rng, truth, 90)
    fwd, rec_f = PL.polish_host(reads, contig, 100, 480)
    rev, rec_r = PL.polish_host(reads, revcomp(contig), 600 - 480, 600 - 100)
    assert rev == revcomp(fwd) and fwd == truth
    assert rec_f.tobytes() == rec_r.tobytes() and int(rec_f["n_changed"]) == 2


def test_an_empty_body_and_an_empty_pool(contig):
    alt = _sub(contig, 70)
    text, rec, _ = _run([alt[40:88]] * 3, contig, b0=70, b1=70)
    assert text == contig and int(rec["n_cols"]) == 0 and int(rec["n_changed"]) == 0 and int(rec["reads_placed"]) == 3
    text, rec = PL.polish_host([], contig, 30, 130)
    assert text == contig and int(rec["n_uncovered"]) == 100 and int(rec["reads_placed"]) == 0


def test_skipped_contigs_come_out_unchanged_with_a_flag(contig):
    alt = _sub(contig, 70)
    text, rec = PL.polish_host([alt[40:88]] * 3, contig[:60] + "N" + contig[61:], 30, 130, **KW)
    assert text == contig[:60] + "N" + contig[61:] and int(rec["flags"]) == B.PL_F_NON_ACGT and int(rec["n_changed"]) == 0
    long = _seq(np.random.default_rng(16), PL.MAX_CONTIG + 1)
    text, rec = PL.polish_host([_sub(long, 500)[480:528]] * 3, long, 100, 8000, **KW)
    assert text == long and int(rec["flags"]) == B.PL_F_LONG and int(rec["len"]) == PL.MAX_CONTIG + 1 and int(rec["n_cols"]) == 7900
    text, rec = PL.polish_host([_sub(long, 500)[480:528]] * 3, long[:-1], 100, 8000, **KW)
    assert text == _sub(long, 500)[:-1] and int(rec["flags"]) == 0 and int(rec["n_changed"]) == 1
    assert PL.MAX_CONTIG >= 8192


def _pack(reads, L):
    rows = np.zeros((len(reads), (L + 3) // 4), dtype=np.uint8)
    for r, text in enumerate(reads):
        for i, c in enumerate(text):
            rows[r, i // 4] |= "ACGT".index(c) << (6 - 2 * (i % 4))
    return rows


def test_a_whole_step_open_gaps_and_mismatches(contig):
    """polish_of_results on a hand-made Results: a closed gap (exact anchors), an open gap, and a word whose span the contig does not carry."""
    rng = np.random.default_rng(17)
    lf, rf = _seq(rng, 60), _seq(rng, 60)
    stored = lf[-40:] + contig + rf[:40]
    alt = _sub(stored, 100)
    reads = [alt[70:118], alt[80:128], revcomp(alt[90:138])]
    word = lambda span: (30 << 56) | ((span + 1) << 32) | ((0x7FFFFFFF - 0) << 1)
    res = types.SimpleNamespace(ctg_pick=None, seq=stored.encode(), pool_rows=_pack(reads, L))
    res.contigs = np.zeros(1, dtype=B.CONTIG)
    res.contigs[0] = (1, 31, 29, 1, len(stored), 0, 0, 0)
    flanks = [("A" * 60, "C" * 60), (lf, rf), ("G" * 60, "T" * 60)]
    res.best = np.array([0, word(len(contig)), 0], dtype=np.uint64)
    res.pool_off = np.array([0, 0, 3, 3], dtype=np.int64)
    rec, texts, stats = PL.polish_of_results(res, flanks, L, **KW)
    assert texts == {1: alt} and not rec[0].tobytes().strip(b"\0") and not rec[2].tobytes().strip(b"\0")
    assert (int(rec[1]["n_cols"]), int(rec[1]["n_changed"]), int(rec[1]["reads_placed"]), int(rec[1]["len"])) == (160, 1, 3, 240)
    assert stats == dict(dict.fromkeys(PL.STAT_KEYS, 0), gaps=1, changed=1, placed=3, bases=240)
    res.best = np.array([0, word(len(contig) + 3), 0], dtype=np.uint64)
    rec, texts, stats = PL.polish_of_results(res, flanks, L, **KW)
    assert texts == {} and stats["mismatches"] == 1 and stats["gaps"] == 0 and not rec.tobytes().strip(b"\0")


def test_parameters_are_validated():
    ok = PL.check_params(150)
    assert ok == (16, 4, 48, 2)
    assert PL.check_params(100, 12, 7, 12, 1) == (12, 7, 12, 1) and PL.check_params(100, 32, 2, 100, 9) == (32, 2, 100, 9)
    for kw in (dict(seed=11), dict(seed=33), dict(max_mismatch=-1), dict(max_mismatch=16), dict(min_overlap=15), dict(min_overlap=151),
               dict(min_votes=0), dict(seed=32, max_mismatch=4), dict(seed=20, max_mismatch=7)):
        with pytest.raises(ValueError, match="polish"):
            PL.check_params(150, **kw)
    with pytest.raises(ValueError, match="polish"):
        PL.polish_host(["A" * 150], "ACGT" * 100, 10, 20, seed=40)


# ---- the seed-indexed search against the definition over all diagonals ----------------------------------------------------------------
def _brute(reads, contig, s, mm_max, mo):
    n, out = len(contig), []
    for r in reads:
        acc = []
        for strand, q in ((0, r), (1, "".join({"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}[c] for c in reversed(r)))):
            Lr = len(q)
            for d in range(-(Lr - mo), n - mo + 1):
                i0, i1 = max(0, -d), min(Lr, n - d)
                if i1 - i0 < mo:
                    continue
                mm = sum(q[i] != "N" and q[i] != contig[d + i] for i in range(i0, i1))
                seeds = [j for j in range(Lr // s) if j * s >= i0 and j * s + s <= i1 and "N" not in q[j * s:j * s + s]
                         and q[j * s:j * s + s] == contig[d + j * s:d + j * s + s]]
                if mm <= mm_max and seeds:
                    acc.append((mm, -(i1 - i0), strand, d))
        if not acc:
            out.append(None)
            continue
        key = min(a[:2] for a in acc)
        best = [a for a in acc if a[:2] == key]
        out.append((best[0][2], best[0][3], best[0][0], -best[0][1]) if len(best) == 1 else "ambiguous")
    return out


@pytest.mark.parametrize("s,mm_max,mo,Lr", [(12, 3, 24, 50), (16, 2, 20, 48)])
def test_placements_equal_the_definition_over_all_diagonals(s, mm_max, mo, Lr):
    rng = np.random.default_rng(100 + s)
    unit = _seq(rng, 80)
    truth = _seq(rng, 60) + unit + unit + _sub(unit, 9) + _seq(rng, 60)
    padded = _seq(rng, 30) + truth + _seq(rng, 30)               # reads that overhang either end
    reads = []
    for r in _sample(rng, padded, 120, L=Lr, err=0.03):
        if rng.integers(0, 3) == 0:
            p = int(rng.integers(0, Lr))
            r = r[:p] + "N" + r[p + 1:]
        reads.append(r)
    got = PL.placements(reads, truth, s, mm_max, mo)
    want = _brute(reads, truth, s, mm_max, mo)
    assert got == want
    kinds = [("none" if w is None else w if w == "ambiguous" else "placed") for w in want]
    assert all(kinds.count(k_) >= 3 for k_ in ("none", "ambiguous", "placed"))
    assert any(w not in (None, "ambiguous") and w[1] < 0 for w in want) and any(w not in (None, "ambiguous") and w[1] + Lr > len(truth) for w in want)
