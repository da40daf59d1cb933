"""The three after-pick rounds in ONE step (read_support, polish and pair_span together) on the shared synthetic step (step_util) in its
smallest layout — 24 gaps of 300 bases, kk = [(31, 29)], one library of 150-base reads: every round's records and statistics against
its host twin on that same Results, with exact anchors and in align mode (two prepared pipelines); a second step of the same pipeline
gives the same records and statistics (the statistics words are zeroed per launch); and one step with the three rounds off (exact
anchors) leaves the same contigs and picks."""
import pytest

from step_util import L, contigs as _contigs, picks as _picks, run as _run, setup as _setup

pytestmark = pytest.mark.gpu

KK = [(31, 29)]
ROUNDS = dict(read_support=True, polish=True, pair_span=True)
_ENV = []


def _env():
    if not _ENV:
        _ENV.append(_setup(300, KK))
    return _ENV[0]


_RUNS = {}


def _steps(mode):
    """The prepared pipeline of an anchor mode with the three rounds on, and the Results of two steps of it."""
    if mode not in _RUNS:
        _RUNS[mode] = _run(_env(), steps=2, pools=True, anchor_mode=mode, **ROUNDS)
    return _RUNS[mode]


@pytest.fixture(scope="module", params=["exact", "align"])
def steps(request):
    return (request.param,) + _steps(request.param)


def _polish_records(res):
    """Results.polish with `off` zeroed: where a polished contig lies in the base buffer is decided by the order of an atomic."""
    rec = res.polish.copy()
    rec["off"] = 0
    return rec


def test_every_round_equals_its_twin_on_the_same_results(steps):
    from gappadder_amd import pair_span as PS
    from gappadder_amd import polish as PL
    from gappadder_amd import read_support as RS
    name, pipe, (res, _) = steps
    flanks = _env()[3]
    closed = int((res.best != 0).sum())
    assert closed > 0 and (res.ctg_pick is not None) == (name == "align")
    sup, s_stats = RS.support_of_results(res, flanks, L, pipe.support.k, pipe.min_count)
    pol, texts, p_stats = PL.polish_of_results(res, flanks, L)
    prs, r_stats = PS.pair_span_of_results(res, flanks, L, [(lb.is_mean, lb.is_sd) for lb in pipe.libs])
    print("%s: %d of %d gaps closed; support %s; polish %s; pairs %s" % (name, closed, len(res.best), s_stats, p_stats, r_stats))
    assert res.support.tobytes() == sup.tobytes()
    assert _polish_records(res).tobytes() == pol.tobytes() and all(PL.polished_text(res, g) == t for g, t in texts.items())
    assert res.pairs.shape == (1, len(res.best)) and res.pairs.tobytes() == prs.tobytes()
    assert res.support_stats == dict(s_stats, k=pipe.support.k) and res.polish_stats == p_stats and res.pair_stats == r_stats
    assert s_stats["gaps"] == p_stats["gaps"] == r_stats[0]["gaps"] == closed and s_stats["mismatches"] == 0


def test_a_second_step_gives_the_same_records_and_statistics(steps):
    _, _, (first, second) = steps
    assert second.support.tobytes() == first.support.tobytes() and second.support_stats == first.support_stats
    assert _polish_records(second).tobytes() == _polish_records(first).tobytes() and second.polish_stats == first.polish_stats
    assert second.pairs.tobytes() == first.pairs.tobytes() and second.pair_stats == first.pair_stats


def test_the_rounds_change_neither_contigs_nor_picks():
    _, (res, _) = _steps("exact")
    pipe_off, (ref,) = _run(_env(), anchor_mode="exact")
    assert pipe_off.after_pick == [] and ref.support is None and ref.polish is None and ref.pairs is None
    assert sorted(_contigs(res)) == sorted(_contigs(ref)) and _picks(res) == _picks(ref)
