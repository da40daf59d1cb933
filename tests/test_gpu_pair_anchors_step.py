"""Pipeline(pair_span=True, pair_anchors=True) on the environment of test_gpu_pair_span_step.py (300- and 550-base gaps, one and two
libraries, the second one long-insert): Results.pair_anchors and .pair_anchor_stats against the host twin on the same fetched step —
pools, read ids, tagger hits, and the libraries' records — with exact anchors beside the polish and read-support rounds, in align mode and
behind the merge round; a second step gives the same bytes; with the option off nothing changes and the new fields are None; what the
constructor refuses."""
import numpy as np
import pytest

import test_gpu_pair_span_step as S
from step_util import L, N_PAIRS

pytestmark = pytest.mark.gpu

# (a short-insert library anchors 2 to 11 in-range pairs per gap here: the default of 8 is gf_fill_pairs_anchored_dev's own test's)
MIN_PAIRS = {"exact": 2, "align": 4, "merge": 3}


def _run(envs, n_lib, steps=1, **kw):
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    (gf, cfg, gaps, flanks, d_reads, d_recs, kk), (d_reads2, d_recs2) = envs
    pipe = Pipeline(gf, len(gaps), L, kk, **kw)
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * N_PAIRS, d_reads, d_recs))
    if n_lib > 1:
        pipe.add_library(DeviceLibrary("y", S.LIB2[0], S.LIB2[1], 2 * S.LIB2[2], d_reads2, d_recs2))
    pipe.prepare()
    out = []
    for _ in range(steps):
        pipe.step()
        out.append(pipe.fetch(pools=True))
    return pipe, out


@pytest.fixture(scope="module", params=sorted(S.RUNS))
def anchored(request):
    gap_len, kk, n_lib, kw = S.RUNS[request.param]
    envs = S._env(gap_len, kk)
    on = _run(envs, n_lib, steps=2, pair_span=True, pair_anchors=True, pair_min_pairs=MIN_PAIRS[request.param], **kw)
    off = _run(envs, n_lib, pair_span=True, **kw)
    return request.param, envs, n_lib, on, off


def test_records_equal_the_twin_on_the_fetched_step(anchored):
    from gappadder_amd import _lib as B
    from gappadder_amd import pair_anchors as PA
    name, envs, n_lib, (pipe, (res, res2)), _ = anchored
    (gf, cfg, gaps, flanks, d_reads, d_recs, kk), (d_reads2, d_recs2) = envs
    assert pipe.anchored.min_pairs == MIN_PAIRS[name] and res.pair_anchors.shape == (n_lib, len(res.best)) and len(res.lib_taghits) == n_lib
    libs = [(lb.is_mean, lb.is_sd) for lb in pipe.libs]
    recs = [np.frombuffer(lb.d_recs.cpu().numpy().tobytes(), dtype=B.ALNREC)[:lb.n_recs] for lb in pipe.libs]
    for lb, hits in zip(pipe.libs, res.lib_taghits):
        assert len(hits) == lb.counts["tagger_hits"] > 0
    want, stats = PA.anchors_of_results(res, flanks, L, libs, gaps, recs, min_pairs=MIN_PAIRS[name])
    # the comparison is not vacuous, from the twin alone
    closed = np.nonzero(res.best)[0]
    assert len(closed) > 0 and ((want["n_in_range"] > 0) & (want["n_eval"] > 0)).any()
    for l in range(n_lib):
        print("%s, library %d: %d of %d gaps closed, %s" % (name, l, len(closed), len(res.best), stats[l]))
        assert stats[l]["mismatches"] == 0 and stats[l]["gaps"] == len(closed) and stats[l]["kept"] > 0 and stats[l]["anchored"] > 0
    assert stats[0]["placed"] > 0 and stats[0]["in_range"] > 0
    bad = [(l, g) for l in range(n_lib) for g in range(len(res.best)) if res.pair_anchors[l, g].tobytes() != want[l, g].tobytes()]
    assert not bad, [(l, g, res.pair_anchors[l, g], want[l, g]) for l, g in bad[:4]]
    assert res.pair_anchor_stats == stats
    assert not res.pair_anchors[:, res.best == 0].tobytes().strip(b"\0")
    # a second step: the same bytes
    assert res2.pair_anchors.tobytes() == res.pair_anchors.tobytes() and res2.pair_anchor_stats == res.pair_anchor_stats
    assert res2.pairs.tobytes() == res.pairs.tobytes()


def test_the_option_changes_nothing_else(anchored):
    name, _, _, (pipe, (res, _)), (pipe_off, (ref,)) = anchored
    assert ref.pair_anchors is None and ref.pair_anchor_stats is None and ref.lib_taghits is None and pipe_off.anchored is None
    assert S._records(res) == S._records(ref) and len(res.seq) == len(ref.seq)
    assert S._picks(res) == S._picks(ref) and (res.best != 0).tobytes() == (ref.best != 0).tobytes()
    assert res.pair_stats == ref.pair_stats and res.merge == ref.merge
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes() and res.pairs.tobytes() == ref.pairs.tobytes()
    else:                                                      # a record names no contig: order-free as it is
        assert res.pairs.tobytes() == ref.pairs.tobytes()


def test_constructor_refuses_what_the_round_excludes():
    from gappadder_amd.pipeline import Pipeline
    (gf, cfg, gaps, flanks, d_reads, d_recs, kk), _ = S._env(300, [(31, 29), (41, 39)])
    with pytest.raises(ValueError, match="pair_anchors needs pair_span"):
        Pipeline(gf, 24, L, [(31, 29)], pair_anchors=True)
    with pytest.raises(ValueError, match="second_round"):
        Pipeline(gf, 24, L, [(31, 29)], pair_span=True, pair_anchors=True, second_round=True)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, [(31, 29)], pair_span=True, pair_anchors=True, world=2)
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError, match="min_pairs"):
            Pipeline(gf, 24, L, [(31, 29)], pair_span=True, pair_anchors=True, pair_min_pairs=bad)
    assert Pipeline(gf, 24, L, [(31, 29)], pair_span=True).anchored is None
