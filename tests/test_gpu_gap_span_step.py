"""Pipeline(gap_span=True) on the shared synthetic step (step_util, 300-base gaps) with a long-insert library of this test's own beside
the short one: 1 500 +/- 100, 30 000 pairs — pairs x (insert - gap - 2 L) / genome = 30 000 x 900 / 800 000 = 34 spanning pairs per gap
by arithmetic, and the twin on the CPU says so before the device is asked.  Results.gap_span and .gap_span_stats equal the twin on the
libraries' fetched records; a second step gives the same bytes; with tag_ahead (the tagger, and the span pass behind it, on a second
context) the bytes are the same; with the round off every other field of the Results is what it was and the new fields are None; what the
constructor refuses."""
import numpy as np
import pytest

import step_util as SU
from step_util import L, N_PAIRS, NSCF, SEED, SLEN, GPS

pytestmark = pytest.mark.gpu

LIB2 = (1500, 100, 30_000)
KK = [(31, 29)]
SPAN = dict(gap_span=True, span_z=3, span_shift=200, span_min_pairs=8)


@pytest.fixture(scope="module")
def env():
    import torch
    from gappadder_amd.hip_api import GapFill
    e = SU.setup(300, KK)
    gf = e[0]
    cfg2 = GapFill.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=300, read_len=L,
                             insert_mean=LIB2[0], insert_sd=LIB2[1], library=1)
    rb = (L + 3) // 4
    d_reads2 = torch.empty(2 * LIB2[2] * rb + 64, dtype=torch.uint8, device="cuda")
    d_recs2 = torch.empty(2 * LIB2[2] * 32, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg2, 0, LIB2[2], d_reads2.data_ptr(), d_recs2.data_ptr())
    gf.sync()
    return e, (d_reads2, d_recs2)


def _run(env, steps=1, tag_ahead=False, **kw):
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    (gf, cfg, gaps, flanks, d_reads, d_recs, kk), (d_reads2, d_recs2) = env
    ctxs = [None, None]
    if tag_ahead:
        for i in range(2):
            ctxs[i] = GapFill(0)
            ctxs[i].set_gaps(gaps, NSCF, None)
    pipe = Pipeline(gf, len(gaps), L, kk, **kw)
    pipe.tag_ahead = tag_ahead
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * N_PAIRS, d_reads, d_recs, tag_ctx=ctxs[0]))
    pipe.add_library(DeviceLibrary("y", LIB2[0], LIB2[1], 2 * LIB2[2], d_reads2, d_recs2, tag_ctx=ctxs[1]))
    pipe.prepare()
    out = []
    for _ in range(steps):
        pipe.step()
        out.append(pipe.fetch())
    return pipe, out


@pytest.fixture(scope="module")
def runs(env):
    return _run(env, steps=2, **SPAN), _run(env)


def _twin(pipe, gaps):
    from gappadder_amd import _lib as B
    from gappadder_amd import gap_span as GS
    recs = [np.frombuffer(lb.d_recs.cpu().numpy().tobytes(), dtype=B.ALNREC)[:lb.n_recs] for lb in pipe.libs]
    return GS.gap_span_of_results(recs, [(lb.is_mean, lb.is_sd) for lb in pipe.libs], gaps, NSCF, L, SPAN["span_z"], SPAN["span_shift"],
                                  pipe.anchor_mapq)


def test_records_equal_the_twin_on_the_fetched_records(env, runs):
    from gappadder_amd import gap_span as GS
    (pipe, (res, res2)), _ = runs
    gaps = env[0][2]
    want, stats = _twin(pipe, gaps)
    # from the twin alone, before the device is asked: the long-insert library spans every gap about 34 times, the short one never
    for l, st in enumerate(stats):
        print("library %d: %s" % (l, st))
    assert stats[0]["accepted"] == 0 and stats[1]["gaps_with_pairs"] == len(gaps) == 24
    assert 20 <= stats[1]["accepted"] / len(gaps) <= 50 and int(want[1]["n"].min()) >= SPAN["span_min_pairs"]
    assert res.gap_span.shape == (2, len(gaps)) and len(res.gap_span_stats) == 2
    bad = [(l, g) for l in range(2) for g in range(len(gaps)) if res.gap_span[l, g].tobytes() != want[l, g].tobytes()]
    assert not bad, [(l, g, res.gap_span[l, g], want[l, g]) for l, g in bad[:4]]
    assert res.gap_span_stats == stats
    # a second step: the same bytes
    assert res2.gap_span.tobytes() == res.gap_span.tobytes() and res2.gap_span_stats == res.gap_span_stats
    # the estimate of the 300-base gaps from about 34 pairs of sd 100: within four standard errors and 100 bases
    for g in range(len(gaps)):
        e = GS.estimate(res.gap_span[1, g], 300, L, LIB2[0], LIB2[1], SPAN["span_z"], SPAN["span_shift"], SPAN["span_min_pairs"])
        assert e is not None and abs(e.est - 300) <= max(4 * e.se, 1.0) and abs(e.est - 300) < 100, (g, e)
        assert GS.estimate(res.gap_span[0, g], 300, L, 300, 30, 3, 200, 8) is None


def _view(res):
    return (sorted(SU.contigs(res)), SU.picks(res), res.n_contigs, res.n_seq, res.n_closed, (res.best != 0).tobytes())


def test_the_option_changes_nothing_else(runs):
    (pipe, (res, _)), (pipe_off, (ref,)) = runs
    assert ref.gap_span is None and ref.gap_span_stats is None and pipe_off.gap_span is None
    assert _view(res) == _view(ref) and res.n_closed > 0
    assert [lb.counts for lb in pipe.libs] == [lb.counts for lb in pipe_off.libs]
    for name in ("merge", "rescue", "round2", "extended", "ext", "support", "polish", "pairs", "pair_anchors"):
        assert getattr(res, name) is None and getattr(ref, name) is None
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()


def test_tag_ahead_gives_the_same_bytes(env, runs):
    (_, (res, _)), _ = runs
    pipe, (a, b) = _run(env, steps=2, tag_ahead=True, **SPAN)
    assert all(lb.second_stream for lb in pipe.libs)
    assert a.gap_span.tobytes() == res.gap_span.tobytes() == b.gap_span.tobytes()
    assert a.gap_span_stats == res.gap_span_stats == b.gap_span_stats
    assert _view(a) == _view(res) and _view(b) == _view(res)


def test_with_the_other_rounds(env, runs):
    """Beside the merge round, the extended fill, the pair span and its anchored extension: the same records."""
    (_, (res, _)), _ = runs
    _, (r,) = _run(env, merge_in_step=True, extended_fill=True, pair_span=True, pair_anchors=True, **SPAN)
    assert r.gap_span.tobytes() == res.gap_span.tobytes() and r.gap_span_stats == res.gap_span_stats and r.pairs is not None


def test_constructor_refusals(env):
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    (gf, cfg, gaps, flanks, d_reads, d_recs, kk), _ = env
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, KK, gap_span=True, world=2)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, KK, gap_span=True, force_exchange=True)
    for kw in (dict(span_z=0), dict(span_z=1.5), dict(span_shift=-1), dict(span_min_pairs=0), dict(span_min_pairs="8")):
        with pytest.raises(ValueError, match="gap_span"):
            Pipeline(gf, 24, L, KK, gap_span=True, **kw)
    assert Pipeline(gf, 24, L, KK, span_z=0).gap_span is None                  # (off: the values are not looked at)
    pipe = Pipeline(gf, 24, L, KK, gap_span=True, span_shift=1 << 19)
    with pytest.raises(ValueError, match="2\\^20"):                            # before the library's buffers are touched
        pipe.add_library(DeviceLibrary("far", 1 << 19, 100, 2 * N_PAIRS, d_reads, d_recs))
    assert not pipe.libs
