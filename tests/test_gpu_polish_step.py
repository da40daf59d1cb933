"""Pipeline(polish=True) on the shared synthetic step (step_util): Results.polish and the polished bases against the host twin on the
step's own pools, contigs and picks — exact anchors, behind the merge round, and in align mode; nothing else of the step changes;
polished_sequences against picked_sequences; what the constructor refuses."""
import numpy as np
import pytest

from step_util import L, contigs as _contigs, picks as _picks, run as _run, setup as _setup

pytestmark = pytest.mark.gpu

# name -> (gap length, k pairs, Pipeline options): 300-base gaps are closed by the first pick; of the 550-base gaps most stay open for the merge round
RUNS = {"exact": (300, [(31, 29), (41, 39)], {"anchor_mode": "exact"}),
        "align": (300, [(31, 29), (41, 39)], {"anchor_mode": "align"}),
        "merge": (550, [(31, 29)], {"merge_in_step": True})}
_ENVS = {}


def _env(gap_len, kk):
    key = (gap_len, tuple(kk))
    if key not in _ENVS:
        _ENVS[key] = _setup(gap_len, kk)
    return _ENVS[key]


@pytest.fixture(scope="module", params=sorted(RUNS))
def pair(request):
    gap_len, kk, kw = RUNS[request.param]
    env = _env(gap_len, kk)
    on = _run(env, pools=True, polish=True, **kw)
    off = _run(env, **kw)
    return request.param, env, on, off


def test_polish_equals_the_twin_on_the_steps_own_pools(pair):
    from gappadder_amd import polish as PL
    name, env, (pipe, (res,)), _ = pair
    flanks = env[3]
    assert pipe.polish.params == (16, 4, 48, 2)
    want, texts, stats = PL.polish_of_results(res, flanks, L)
    closed = np.nonzero(res.best)[0]
    assert len(closed) and sorted(texts) == closed.tolist() and stats["mismatches"] == 0
    bad, spans = [], []
    for g in range(len(want)):
        a = res.polish[g].copy()
        o, n = int(a["off"]), int(a["len"])
        a["off"] = 0
        if a.tobytes() != want[g].tobytes() or (g in texts and PL.polished_text(res, g) != texts[g]) or (g not in texts and (o or n)):
            bad.append(g)
        if g in texts:
            spans.append((o, o + n))
    assert not bad, [(g, res.polish[g], want[g]) for g in bad[:4]]
    assert res.polish_stats == stats
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == len(res.polish_bases) and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    print("%s: %d of %d gaps closed, columns %d, changed %d, uncovered %d, rows placed %d, ambiguous %d"
          % (name, len(closed), len(res.best), int(res.polish["n_cols"].sum()), stats["changed"], int(res.polish["n_uncovered"].sum()),
             stats["placed"], stats["ambiguous"]))
    assert stats["placed"] > 0
    if name == "merge":
        assert res.merge is not None


def test_polished_sequences_are_the_picked_ones_where_nothing_changed(pair):
    from gappadder_amd import polish as PL
    from gappadder_amd.pipeline import contig_text
    _, _, (pipe, (res,)), _ = pair
    picked, polished = pipe.picked_sequences(res), pipe.polished_sequences(res)
    assert sorted(picked) == sorted(polished) == np.nonzero(res.best)[0].tolist()
    for g, (ci, body, rev) in picked.items():
        assert polished[g][0] == ci and polished[g][2] == rev and len(polished[g][1]) == len(body)
        diff = sum(x != y for x, y in zip(polished[g][1], body))
        assert diff <= int(res.polish[g]["n_changed"])            # (the cut may leave a changed column of the body out; it adds none)
        if int(res.polish[g]["n_changed"]) == 0:
            assert polished[g][1] == body and PL.polished_text(res, g) == contig_text(res, ci)


def _records(res):
    """Every contig record with its bases, order-free: two runs of the SAME step list the same records in different orders."""
    return sorted((int(c["gap"]), int(c["k"]), int(c["kv"]), int(c["n_nodes"]), int(c["length"]), int(c["cov_sum"]), s)
                  for c, (_, _, _, s) in zip(res.contigs, _contigs(res)))


def test_the_round_changes_nothing_else(pair):
    """`contigs`, `seq` and `best` of the step with the round on against the step with it off, order-free (the step lists its contigs in
    no fixed order, and a pick word names its contig by index), and the bytes wherever the two lists do come in one order."""
    _, _, (pipe, (res,)), (pipe_off, (ref,)) = pair
    assert ref.polish is None and ref.polish_bases is None and ref.polish_stats is None and pipe_off.polish is None
    assert _records(res) == _records(ref) and len(res.seq) == len(ref.seq)
    assert _picks(res) == _picks(ref) and (res.best != 0).tobytes() == (ref.best != 0).tobytes()
    assert res.merge == ref.merge
    assert {g: v[1:] for g, v in pipe.picked_sequences(res).items()} == {g: v[1:] for g, v in pipe_off.picked_sequences(ref).items()}
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()


def test_constructor_refuses_what_the_round_excludes():
    from gappadder_amd.pipeline import Pipeline
    gf = _env(300, [(31, 29), (41, 39)])[0]
    with pytest.raises(ValueError, match="second_round"):
        Pipeline(gf, 24, L, [(31, 29)], polish=True, second_round=True)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, [(31, 29)], polish=True, world=2)
    with pytest.raises(ValueError, match="polish"):
        Pipeline(gf, 24, L, [(31, 29)], polish=True, polish_seed=40)
    with pytest.raises(ValueError, match="polish"):
        Pipeline(gf, 24, L, [(31, 29)], polish=True, polish_seed=32, polish_max_mismatch=4)
