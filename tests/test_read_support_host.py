"""The host twin of the read-support round (gappadder_amd/read_support.py: support_host and what it is made of) on hand-derived answers,
and its counting rule against oracle.gp_oracle.count_kmers — an independent restatement — on a random pool."""
import numpy as np
import pytest

from gappadder_amd import read_support as RS
from gappadder_amd.pick_contigs import revcomp

KS = [31, 51]
L = 150


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _tile(text, cov, step=1):
    """Reads of L bases at every `step`-th offset of text, each `cov` times: every k-window at least L - k bases from both ends of the
    text lies in (L - k + 1) / step reads x cov."""
    return [text[o:o + L] for o in range(0, len(text) - L + 1, step) for _ in range(cov)]


def _case(seed, body_len=200, flank=150, pad=200):
    """A contig = flank + body + flank inside a longer true text that the reads tile."""
    rng = np.random.default_rng(seed)
    text = _seq(rng, 2 * pad + 2 * flank + body_len)
    contig = text[pad:pad + 2 * flank + body_len]
    return text, contig, flank, flank + body_len


def _naive(reads, k):
    cnt = {}
    for r in reads:
        for p in range(len(r) - k + 1):
            w = r[p:p + k]
            if all(c in "ACGT" for c in w):
                key = min(w, revcomp(w))
                cnt[key] = cnt.get(key, 0) + 1
    return cnt


def _naive_supports(reads, contig, b0, b1, k):
    cnt = _naive(reads, k)
    lo, hi = max(0, b0 - k + 1), min(len(contig) - k, max(b1, b0) - 1)
    return [cnt.get(min(contig[s:s + k], revcomp(contig[s:s + k])), 0) if all(c in "ACGT" for c in contig[s:s + k]) else 0 for s in range(lo, hi + 1)]


@pytest.mark.parametrize("k", KS)
def test_a_covered_fill_has_the_planted_support(k):
    text, contig, b0, b1 = _case(1)
    # 10 identical copies of the whole text cut into L-base reads at every offset: every window of the contig lies in L - k + 1 reads
    reads = _tile(text, 10)
    rec = RS.support_host(reads, contig, b0, b1, k, 2)
    planted = 10 * (L - k + 1)
    assert int(rec["n_windows"]) == (b1 - b0) + k - 1
    assert int(rec["n_zero"]) == 0 and int(rec["n_below"]) == 0 and int(rec["zero_run"]) == 0
    assert int(rec["min"]) == int(rec["max"]) == planted and int(rec["sum"]) == planted * int(rec["n_windows"])


@pytest.mark.parametrize("k", KS)
def test_b_one_wrong_base_gives_k_zero_windows(k):
    text, contig, b0, b1 = _case(2)
    at = b0 + 100
    bad = contig[:at] + "ACGT"[("ACGT".index(contig[at]) + 1) % 4] + contig[at + 1:]
    rec = RS.support_host(_tile(text, 3), bad, b0, b1, k, 2)
    assert int(rec["n_windows"]) == 200 + k - 1
    assert int(rec["n_zero"]) == k and int(rec["zero_run"]) == k and int(rec["n_below"]) == k
    assert int(rec["min"]) == 0 and int(rec["max"]) == 3 * (L - k + 1)
    assert int(rec["sum"]) == 3 * (L - k + 1) * (200 - 1)


@pytest.mark.parametrize("k", KS)
def test_c_wrong_base_near_the_contig_end_is_clipped(k):
    rng = np.random.default_rng(3)
    text = _seq(rng, 900)
    contig = text[200:500]                       # the body runs to the contig's end: b1 = 300 (a pick whose right hit is empty is not
    at = len(contig) - 3                         # produced by the picks; the twin takes any body) — two bases from the end
    bad = contig[:at] + "ACGT"[("ACGT".index(contig[at]) + 1) % 4] + contig[at + 1:]
    rec = RS.support_host(_tile(text, 2), bad, 100, 300, k, 2)
    assert int(rec["n_windows"]) == 300 - k - (100 - k + 1) + 1
    # windows that hold base `at` and fit the contig: starts at - k + 1 .. len - k: 3 of them
    assert int(rec["n_zero"]) == 3 and int(rec["zero_run"]) == 3


@pytest.mark.parametrize("k", KS)
def test_d_empty_body_gives_the_junction_windows(k):
    text, contig, b0, _ = _case(4, body_len=0)
    sup = RS.window_supports(_tile(text, 1), contig, b0, b0, k)
    assert len(sup) == k - 1 and set(sup) == {L - k + 1}
    # a junction at the contig's first base has no window over it
    assert RS.window_supports(_tile(text, 1), contig, 0, 0, k) == []
    # a contig shorter than k: no windows, the zero record
    rec = RS.support_host(_tile(text, 1), contig[:k - 1], 5, 9, k, 2)
    assert rec.tobytes() == bytes(32)


@pytest.mark.parametrize("k", KS)
def test_e_orientation_does_not_matter(k):
    text, contig, b0, b1 = _case(5)
    at = b0 + 30
    bad = contig[:at] + "ACGT"[("ACGT".index(contig[at]) + 2) % 4] + contig[at + 1:]
    reads = _tile(text, 2, step=7)
    fwd = RS.support_host(reads, bad, b0, b1, k, 2)
    n = len(bad)
    rev = RS.support_host(reads, revcomp(bad), n - b1, n - b0, k, 2)
    assert fwd.tobytes() == rev.tobytes() and int(fwd["zero_run"]) == k
    # through the hits: a forward exact pick and the reverse pick on the reverse-complemented contig give the same body, mirrored
    lf, rf = contig[b0 - 60:b0], contig[b1:b1 + 60]
    assert RS.locate_exact(bad, lf, rf, 30, False) == (b0, b1)
    assert RS.locate_exact(revcomp(bad), lf, rf, 30, True) == (n - b1, n - b0)
    assert RS.locate_exact(bad, lf, rf, 30, True) is None
    pick = {"lp": b0 - 40 + 1, "lm": 40, "rp": b1 + 1, "rm": 35, "threshold": 30}
    assert RS.locate_pick(pick, False) == (b0, b1)
    rpick = {"lp": n - b0 + 1, "lm": 40, "rp": n - b1 - 35 + 1, "rm": 35, "threshold": 30}
    assert RS.locate_pick(rpick, True) == (n - b1, n - b0)


@pytest.mark.parametrize("k", KS)
def test_f_a_masked_read_base_hides_its_windows(k):
    text, contig, b0, b1 = _case(6)
    o = 300                                      # one read at text offset 300 (the contig starts at text offset 200): over the first body bases
    reads = [text[o:o + L]]
    clean = RS.window_supports(reads, contig, b0, b1, k)
    assert sum(clean) == sum(1 for s in range(b0 - k + 1, b1) if o <= 200 + s and 200 + s + k <= o + L)
    masked = [reads[0][:120] + "N" + reads[0][121:]]
    sup = RS.window_supports(masked, contig, b0, b1, k)
    lost = [i for i, (x, y) in enumerate(zip(clean, sup)) if x != y]
    # exactly the windows over read base 120 (text offset 420) go from 1 to 0
    lo = b0 - k + 1
    assert lost == [s - lo for s in range(lo, b1) if 200 + s <= 420 < 200 + s + k and o <= 200 + s and 200 + s + k <= o + L]
    assert all(sup[i] == 0 and clean[i] == 1 for i in lost) and lost
    # the same through packed rows and mask words
    codes, valid = RS.codes_of(masked)
    rows = np.zeros((1, (L + 3) // 4), dtype=np.uint8)
    for i in range(L):
        rows[0, i // 4] |= int(codes[0, i]) << (6 - 2 * (i % 4))
    nm = np.zeros((1, (L + 31) // 32), dtype=np.uint32)
    nm[0, 120 // 32] = 1 << (120 % 32)
    assert RS.window_supports(RS.codes_of_rows(rows, L, nm), contig, b0, b1, k) == sup
    # without the mask the N reads as A
    assert RS.window_supports(RS.codes_of_rows(rows, L, None), contig, b0, b1, k) == (clean if text[420] == "A" else sup)


@pytest.mark.parametrize("k", KS)
def test_g_a_repeated_kmer_counts_occurrences_in_both_windows(k):
    rng = np.random.default_rng(7)
    unit = _seq(rng, k)
    body = unit + _seq(rng, 40) + revcomp(unit) + _seq(rng, 30)        # the k-mer twice in the fill, once per strand
    left, right = _seq(rng, 160), _seq(rng, 160)
    contig = left + body + right
    reads = _tile(_seq(rng, 200) + contig + _seq(rng, 200), 2)
    sup = RS.window_supports(reads, contig, len(left), len(left) + len(body), k)
    lo = len(left) - k + 1
    first, second = sup[len(left) - lo], sup[len(left) + k + 40 - lo]
    # every read window over either copy counts for both: twice the support of a window that occurs once
    assert first == second == 2 * 2 * (L - k + 1)
    assert sup[len(left) + k + 5 - lo] == 2 * (L - k + 1)
    assert sup == _naive_supports(reads, contig, len(left), len(left) + len(body), k)


@pytest.mark.parametrize("k", [32, 33])
def test_h_one_word_and_two_word_keys_agree_with_a_string_count(k):
    rng = np.random.default_rng(8)
    text = _seq(rng, 700)
    contig = text[100:600]
    reads = _tile(text, 1, step=3) + [revcomp(r) for r in _tile(text, 1, step=5)] + ["T" * L, "A" * 75 + "T" * 75]
    contig = contig[:250] + "T" * 70 + contig[250:]
    sup = RS.window_supports(reads, contig, 120, 400, k)
    assert sup == _naive_supports(reads, contig, 120, 400, k) and max(sup) > 0 and min(sup) == 0
    keys, ok = RS.canonical_keys(*RS.codes_of(reads), k)
    assert keys.shape == ((len(reads), L - k + 1) if k <= 32 else (len(reads), L - k + 1, 2)) and ok.all()


def test_support_k_outside_16_64_is_refused():
    for k in (15, 65, 0):
        with pytest.raises(ValueError):
            RS.support_host(["A" * L], "ACGT" * 50, 50, 60, k)


@pytest.mark.parametrize("k", [16, 31, 32, 33, 51, 64])
def test_counts_equal_the_oracles_kmer_counter(k):
    from oracle import gp_oracle as O
    rng = np.random.default_rng(100 + k)
    base = _seq(rng, 400)
    reads = []
    for _ in range(60):
        o = int(rng.integers(0, len(base) - 100))
        r = list(base[o:o + 100])
        for _ in range(int(rng.integers(0, 3))):
            r[int(rng.integers(0, 100))] = "ACGTN"[int(rng.integers(0, 5))]
        r = "".join(r)
        reads.append(revcomp(r).replace("n", "N") if rng.integers(0, 2) else r)
    got = RS.kmer_counts(*RS.codes_of(reads), k)
    want = O.count_kmers(reads, k, min_count=1)
    as_int = {(key << 64 if k <= 32 else (key[0] << 64) | key[1]): n for key, n in got.items()}
    assert sorted(as_int.items()) == want and len(want) > 100
