"""Pipeline(read_support=True) on the shared synthetic step (step_util): Results.support against the host twin on the step's own pools,
contigs and picks in every anchor mode and behind the merge and rescue rounds; nothing else of the step changes; what the constructor
refuses."""
import numpy as np
import pytest

from step_util import L, contigs as _contigs, picks as _picks, run as _run, setup as _setup

pytestmark = pytest.mark.gpu

# name -> (gap length, k pairs, Pipeline options): 300-base gaps are closed by the first pick; of the 550-base gaps most stay open for
# the merge and rescue rounds
RUNS = {"exact": (300, [(31, 29), (41, 39)], {"anchor_mode": "exact"}),
        "align": (300, [(31, 29), (41, 39)], {"anchor_mode": "align"}),
        "gapped": (300, [(31, 29), (41, 39)], {"anchor_mode": "gapped"}),
        "merge_rescue": (550, [(31, 29)], {"merge_in_step": True, "rescue_round": True})}
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
    on = _run(env, pools=True, read_support=True, **kw)
    off = _run(env, **kw)
    return request.param, env, on, off


def test_support_equals_the_twin_on_the_steps_own_pools(pair):
    from gappadder_amd import read_support as RS
    name, env, (pipe, (res,)), _ = pair
    flanks = env[3]
    assert pipe.support.k == 31
    want, stats = RS.support_of_results(res, flanks, L, 31, pipe.min_count)
    bad = [g for g in range(len(want)) if res.support[g].tobytes() != want[g].tobytes()]
    assert not bad, [(g, res.support[g], want[g]) for g in bad[:4]]
    assert res.support_stats == dict(stats, k=31) and stats["mismatches"] == 0
    closed = res.best != 0
    nonzero = np.array([bool(r.tobytes().strip(b"\0")) for r in res.support])
    assert closed.any() and (nonzero == closed).all()
    print("%s: %d of %d gaps closed, windows %d, gaps with a zero-support window %d, zero_run max %d"
          % (name, int(closed.sum()), len(closed), stats["windows"], int((res.support["n_zero"] > 0).sum()), int(res.support["zero_run"].max())))
    if name == "merge_rescue":
        assert res.merge is not None and res.rescue is not None


def _records(res):
    """Every contig record with its bases, order-free: the workgroups of the assembly append to the list in the order they finish, so two
    runs of the SAME step list the same records in different orders (and a pick word names its contig by index)."""
    return sorted((int(c["gap"]), int(c["k"]), int(c["kv"]), int(c["n_nodes"]), int(c["length"]), int(c["cov_sum"]), s)
                  for c, (_, _, _, s) in zip(res.contigs, _contigs(res)))


def test_the_round_changes_nothing_else(pair):
    """`contigs`, `seq` and `best` of the step with the round on against the step with it off.  Byte equality of the three arrays holds
    only between two runs that list the contigs in the same order, which the step does not promise (_records); so the records with
    their bases and the picks by their bases are compared order-free, and the bytes wherever the two lists do come in one order."""
    _, _, (_, (res,)), (_, (ref,)) = pair
    assert ref.support is None and ref.support_stats is None
    assert _records(res) == _records(ref) and len(res.seq) == len(ref.seq)
    assert _picks(res) == _picks(ref) and (res.best != 0).tobytes() == (ref.best != 0).tobytes()
    assert res.merge == ref.merge and res.rescue == ref.rescue
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()


def test_constructor_refuses_what_the_round_excludes():
    from gappadder_amd.pipeline import Pipeline
    gf = _env(300, [(31, 29), (41, 39)])[0]
    with pytest.raises(ValueError, match="second_round"):
        Pipeline(gf, 24, L, [(31, 29)], read_support=True, second_round=True)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, [(31, 29)], read_support=True, world=2)
    with pytest.raises(ValueError, match="support_k"):
        Pipeline(gf, 24, L, [(31, 29)], read_support=True, support_k=65)
    with pytest.raises(ValueError, match="support_k"):
        Pipeline(gf, 24, L, [(71, 69)], read_support=True)
