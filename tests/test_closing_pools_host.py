"""The closing pools without a device: second_round.closing_pools_host against a key-by-key brute force on hand-made inputs, the
one accessor the host twins read their pool through, and what Pipeline accepts and refuses with closing_pools."""
import types

import numpy as np
import pytest

KK = [(31, 29)]


def _brute(n_src, best, keys, library=None):
    """Key by key, no sets: a pair goes in when no equal key came before it; then ordered by (library, pair) by insertion."""
    out = []
    for g in range(len(best)):
        if not best[g]:
            out.append([])
            continue
        mine = []
        for i, (kg, l, q) in enumerate(keys):
            if kg != g or (library is not None and l != library):
                continue
            if any(keys[j] == (kg, l, q) for j in range(i)):
                continue
            at = 0
            while at < len(mine) and (mine[at][0] < l or (mine[at][0] == l and mine[at][1] < q)):
                at += 1
            mine.insert(at, (l, q))
        out.append([(-1, j) for j in range(n_src[g])] + [(l, 2 * q + m) for l, q in mine for m in (0, 1)])
    return out


def _hand_made():
    n_src = [3, 2, 0, 4, 1]
    best = [7, 9, 1 << 56, 0, 5]          # gap 3 is open
    keys = [(0, 1, 9), (0, 0, 9), (0, 1, 2), (0, 0, 9), (0, 1, 9),      # closed, two libraries, the same pair id in both, repeats
            (2, 0, 4), (2, 2, 1), (2, 0, 4),                           # closed, no step rows
            (3, 0, 1), (3, 1, 1),                                      # open, with recruits: empty
            (4, 2, 0),
            (5, 0, 3), (-1, 0, 3)]                                     # beyond the gaps: ignored
    return n_src, best, keys                                           # (gap 1: closed, no recruits)


def test_twin_equals_brute_force_on_hand_made_inputs():
    from gappadder_amd.second_round import closing_pools_host
    n_src, best, keys = _hand_made()
    got = closing_pools_host(n_src, best, keys)
    assert got == _brute(n_src, best, keys)
    assert got[0] == [(-1, 0), (-1, 1), (-1, 2), (0, 18), (0, 19), (1, 4), (1, 5), (1, 18), (1, 19)]
    assert got[1] == [(-1, 0), (-1, 1)]                      # closed by the first pick: the step's rows alone
    assert got[2] == [(0, 8), (0, 9), (2, 2), (2, 3)]        # no step rows
    assert got[3] == []                                      # open: empty, whatever keys it holds
    assert got[4] == [(-1, 0), (2, 0), (2, 1)]
    for l in (0, 1, 2):
        assert closing_pools_host(n_src, best, keys, library=l) == _brute(n_src, best, keys, l)
    assert closing_pools_host(n_src, best, keys, library=1)[0] == [(-1, 0), (-1, 1), (-1, 2), (1, 4), (1, 5), (1, 18), (1, 19)]
    assert closing_pools_host(n_src, best, keys, library=1)[2] == []


def test_twin_equals_brute_force_on_random_inputs():
    from gappadder_amd.second_round import closing_pools_host
    rng = np.random.default_rng(11)
    for _ in range(20):
        n = int(rng.integers(1, 9))
        n_src = rng.integers(0, 5, size=n).tolist()
        best = (rng.integers(0, 2, size=n) * 77).tolist()
        keys = [(int(rng.integers(0, n + 1)), int(rng.integers(0, 3)), int(rng.integers(0, 6))) for _ in range(int(rng.integers(0, 60)))]
        for l in (None, 0, 2):
            assert closing_pools_host(n_src, best, keys, l) == _brute(n_src, best, keys, l)


def test_the_twins_accessor_prefers_the_closing_pool():
    from gappadder_amd import fill_rounds as FR
    step = types.SimpleNamespace(pool_off="o", pool_rows="r", lib_pool_off=["lo"], lib_pool_rows=["lr"], lib_pool_ids=["li"])
    assert FR.fill_pool(step, "m") == ("o", "r", "m") and FR.fill_lib_pool(step, 0, "m") == ("lo", "lr", "li", "m")
    both = types.SimpleNamespace(pool_off="o", pool_rows="r", closing_pool_off="co", closing_pool_rows="cr", closing_pool_nmask=None,
                                 lib_pool_off=["lo"], lib_pool_rows=["lr"], lib_pool_ids=["li"], closing_lib_pool_off=["clo"],
                                 closing_lib_pool_rows=["clr"], closing_lib_pool_ids=["cli"], closing_lib_pool_nmask=None)
    assert FR.fill_pool(both, "m") == ("co", "cr", None) and FR.fill_lib_pool(both, 0, "m") == ("clo", "clr", "cli", None)


def _constructed(**kw):
    """The constructor's refusals come before anything touches gf: with gf = None, getting past them ends at the first use of gf."""
    from gappadder_amd.pipeline import Pipeline
    try:
        Pipeline(None, 24, 150, KK, **kw)
    except AttributeError:
        pass
    return True


def test_closing_pools_needs_second_round():
    with pytest.raises(ValueError, match="closing_pools needs second_round"):
        _constructed(closing_pools=True)
    with pytest.raises(ValueError, match="closing_pools needs second_round"):
        _constructed(closing_pools=True, polish=True)


@pytest.mark.parametrize("kw, what", [(dict(read_support=True), "read_support"), (dict(polish=True), "polish"),
                                      (dict(polish=True, polish_indels=True), "polish"), (dict(pileup=True), "pileup"),
                                      (dict(pair_span=True), "pair_span"), (dict(alternatives=True, adjudicate=True), "adjudicate")])
def test_without_the_flag_the_rounds_are_refused_as_before_and_accepted_with_it(kw, what):
    old = "%s with second_round: the second round assembles a pool of its own, not the step's" % what
    with pytest.raises(ValueError, match=old):
        _constructed(second_round=True, **kw)
    with pytest.raises(ValueError, match=old):
        _constructed(second_round=True, recruit_rounds=4, **kw)
    assert _constructed(second_round=True, closing_pools=True, **kw)
    assert _constructed(second_round=True, recruit_rounds=4, closing_pools=True, **kw)


def test_pair_anchors_stays_refused_and_the_other_refusals_hold():
    with pytest.raises(ValueError, match="pair_anchors with second_round"):
        _constructed(second_round=True, closing_pools=True, pair_span=True, pair_anchors=True)
    with pytest.raises(ValueError, match="single rank"):
        _constructed(second_round=True, closing_pools=True, world=2)
    with pytest.raises(ValueError, match="merge_in_step"):
        _constructed(second_round=True, closing_pools=True, merge_in_step=True)
