"""The host pieces the three after-pick rounds share (gappadder_amd/fill_rounds.py) on one hand-made Results of four gaps — one open, one
closed and correct, one whose word names a contig beyond the list, one whose word names another gap's contig: the shared walk, and the
three twins over the whole step, with exact anchors and with a gf_ctg_pick whose threshold is 0 (align mode's mismatch)."""
import types

import numpy as np
import pytest

from gappadder_amd import _lib as B
from gappadder_amd import fill_rounds as FR
from gappadder_amd import pair_span as PS
from gappadder_amd import polish as PL
from gappadder_amd import read_support as RS
from gappadder_amd.pick_contigs import revcomp

L, A, K = 100, 30, 31


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _pack(reads):
    rows = np.zeros((len(reads), (L + 3) // 4), dtype=np.uint8)
    for r, text in enumerate(reads):
        for i, c in enumerate(text):
            rows[r, i // 4] |= "ACGT".index(c) << (6 - 2 * (i % 4))
    return rows


def _word(ci, span):
    return (A << 56) | ((span + 1) << 32) | ((0x7FFFFFFF - ci) << 1)


@pytest.fixture(scope="module")
def step():
    """Gap 0 is open.  Gap 1: contig 0 = the last 40 flank bases, a body of 200, the first 40 flank bases, so the
    anchors of A bases are there and the span is the word's; its pool: 20 read pairs (ids 2 p, 2 p + 1; FR, insert 260) over the contig,
    rows ordered by (mate side, pair) as gf_build_pools_dev leaves them.  Gap 2's word names contig 5 of a list of 2; gap 3's names
    contig 0, which is gap 1's."""
    rng = np.random.default_rng(36)
    lf, rf, body = _seq(rng, 60), _seq(rng, 60), _seq(rng, 200)
    stored = lf[-40:] + body + rf[:40]
    other = _seq(rng, 250)
    starts = [int(x) for x in rng.integers(0, len(stored) - 260 + 1, 20)]
    reads = [stored[s:s + L] for s in starts] + [revcomp(stored[s + 160:s + 260]) for s in starts]
    ids = np.array([2 * p for p in range(20)] + [2 * p + 1 for p in range(20)], dtype=np.uint32)
    res = types.SimpleNamespace(ctg_pick=None, seq=(stored + other).encode(), pool_rows=_pack(reads))
    res.contigs = np.zeros(2, dtype=B.CONTIG)
    res.contigs[0] = (1, K, 29, 1, len(stored), 0, 0, 0)
    res.contigs[1] = (2, K, 29, 1, len(other), 0, 0, len(stored))
    res.best = np.array([0, _word(0, len(body)), _word(5, len(body)), _word(0, len(body))], dtype=np.uint64)
    res.pool_off = np.array([0, 0, 40, 40, 40], dtype=np.int64)
    res.lib_pool_off, res.lib_pool_rows, res.lib_pool_ids = [res.pool_off], [res.pool_rows], [ids]
    flanks = [("A" * 60, "C" * 60), (lf, rf), (_seq(rng, 60), _seq(rng, 60)), (lf, rf)]
    return res, flanks, stored, (40, 240)


def _with_picks(res, threshold, own_contig=False):
    """The same step in align mode: contig 0 carries a selection whose alignments end at base 40 and start at base 241 (1-based), with
    the given threshold.  own_contig: gap 3's word names contig 1, which is then gap 3's own — and carries a selection with threshold 0."""
    out = types.SimpleNamespace(**vars(res))
    out.ctg_pick = np.zeros(2, dtype=B.CTG_PICK)
    out.ctg_pick[0] = (1, 241, 40, 40, 0, threshold, 0)
    if own_contig:
        out.contigs, out.best = res.contigs.copy(), res.best.copy()
        out.contigs[1]["gap"] = 3
        out.best[3] = _word(1, 200)
        out.ctg_pick[1] = (1, 241, 40, 40, 0, 0, 0)
    return out


def _check(res, flanks, want):
    """want: what the shared walk yields.  The twins count its bodiless entries as mismatches and examine the others."""
    assert [(int(g), contig, b) for g, contig, b in FR.closed_fills(res, flanks)] == want              # nothing for the open gap 0
    good = [g for g, _, b in want if b is not None]
    n_bad = len(want) - len(good)
    sup, s_stats = RS.support_of_results(res, flanks, L, K)
    pol, texts, p_stats = PL.polish_of_results(res, flanks, L)
    prs, r_stats = PS.pair_span_of_results(res, flanks, L, [(260, 10)])
    assert s_stats["mismatches"] == p_stats["mismatches"] == r_stats[0]["mismatches"] == n_bad
    assert s_stats["gaps"] == p_stats["gaps"] == r_stats[0]["gaps"] == len(good) and sorted(texts) == good
    for rec in (sup, pol, prs[0]):
        assert len(rec) == 4 and [g for g in range(4) if rec[g].tobytes().strip(b"\0")] == good
    if good:
        assert good == [1] and int(sup[1]["n_windows"]) == 200 + K - 1 and int(pol[1]["n_cols"]) == 200 and texts[1] == want[0][1]
        assert (int(prs[0, 1]["rows"]), int(prs[0, 1]["pairs_complete"]), int(prs[0, 1]["n_in_range"])) == (40, 20, 20)
    return n_bad


def test_exact_anchors_one_fill_two_mismatches_and_nothing_for_the_open_gap(step):
    res, flanks, stored, body = step
    assert _check(res, flanks, [(1, stored, body), (2, "", None), (3, "", None)]) == 2


def test_align_mode_a_selection_with_threshold_zero_is_a_mismatch(step):
    res, flanks, stored, body = step
    other = res.seq[len(stored):].decode()
    assert _check(_with_picks(res, 30), flanks, [(1, stored, body), (2, "", None), (3, "", None)]) == 2
    assert _check(_with_picks(res, 30, own_contig=True), flanks, [(1, stored, body), (2, "", None), (3, other, None)]) == 2
    assert _check(_with_picks(res, 0), flanks, [(1, stored, None), (2, "", None), (3, "", None)]) == 3
