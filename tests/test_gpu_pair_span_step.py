"""Pipeline(pair_span=True) on the shared synthetic step (step_util), with one library and with two of different insert sizes:
Results.pairs and .pair_stats against the host twin on the fetched per-library pools and read ids — exact anchors with the polish and
read-support rounds on as well, behind the merge round, and in align mode; nothing else of the step changes, the other rounds' results
included; what the constructor refuses."""
import numpy as np
import pytest

from step_util import L, N_PAIRS, NSCF, SEED, SLEN, GPS, contigs as _contigs, picks as _picks, setup as _setup

pytestmark = pytest.mark.gpu

# name -> (gap length, k pairs, libraries, Pipeline options)
RUNS = {"exact": (300, [(31, 29), (41, 39)], 1, {"anchor_mode": "exact", "polish": True, "read_support": True}),
        "align": (300, [(31, 29), (41, 39)], 2, {"anchor_mode": "align"}),
        "merge": (550, [(31, 29)], 2, {"merge_in_step": True})}
LIB2 = (700, 60, 30_000)       # the second library: insert mean, sd, pairs
_ENVS = {}


def _env(gap_len, kk):
    """step_util's environment and a second library on the same layout."""
    import torch
    from gappadder_amd.hip_api import GapFill
    key = (gap_len, tuple(kk))
    if key not in _ENVS:
        env = _setup(gap_len, kk)
        gf = env[0]
        cfg2 = GapFill.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=gap_len, read_len=L,
                                 insert_mean=LIB2[0], insert_sd=LIB2[1], library=1)
        rb = (L + 3) // 4
        d_reads2 = torch.empty(2 * LIB2[2] * rb + 64, dtype=torch.uint8, device="cuda")
        d_recs2 = torch.empty(2 * LIB2[2] * 32, dtype=torch.uint8, device="cuda")
        gf.synth_pairs_dev(cfg2, 0, LIB2[2], d_reads2.data_ptr(), d_recs2.data_ptr())
        gf.sync()
        _ENVS[key] = env, (d_reads2, d_recs2)
    return _ENVS[key]


def _run(envs, n_lib, pools=False, **kw):
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    (gf, cfg, gaps, flanks, d_reads, d_recs, kk), (d_reads2, d_recs2) = envs
    pipe = Pipeline(gf, len(gaps), L, kk, **kw)
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * N_PAIRS, d_reads, d_recs))
    if n_lib > 1:
        pipe.add_library(DeviceLibrary("y", LIB2[0], LIB2[1], 2 * LIB2[2], d_reads2, d_recs2))
    pipe.prepare()
    pipe.step()
    return pipe, pipe.fetch(pools=pools)


@pytest.fixture(scope="module", params=sorted(RUNS))
def pair(request):
    gap_len, kk, n_lib, kw = RUNS[request.param]
    envs = _env(gap_len, kk)
    on = _run(envs, n_lib, pools=True, pair_span=True, **kw)
    off = _run(envs, n_lib, **kw)
    return request.param, envs, n_lib, on, off


def test_pairs_equal_the_twin_on_the_libraries_own_pools(pair):
    from gappadder_amd import pair_span as PS
    name, envs, n_lib, (pipe, res), _ = pair
    flanks = envs[0][3]
    assert pipe.pairs.params == (16, 4, 48, 3) and pipe.keep_read_ids
    libs = [(lb.is_mean, lb.is_sd) for lb in pipe.libs]
    assert len(libs) == n_lib and res.pairs.shape == (n_lib, len(res.best)) and len(res.lib_pool_ids) == n_lib
    for off, rows, ids in zip(res.lib_pool_off, res.lib_pool_rows, res.lib_pool_ids):
        assert len(rows) == len(ids) == int(off[-1])
    want, stats = PS.pair_span_of_results(res, flanks, L, libs)
    closed = np.nonzero(res.best)[0]
    bad = [(l, g) for l in range(n_lib) for g in range(len(res.best)) if res.pairs[l, g].tobytes() != want[l, g].tobytes()]
    assert not bad, [(l, g, res.pairs[l, g], want[l, g]) for l, g in bad[:4]]
    assert res.pair_stats == stats
    for l in range(n_lib):
        print("%s, library %d: %d of %d gaps closed, %s" % (name, l, len(closed), len(res.best), stats[l]))
        assert stats[l]["mismatches"] == 0 and stats[l]["gaps"] == len(closed) > 0
        assert not res.pairs[l][res.best == 0].tobytes().strip(b"\0")
    assert stats[0]["placed"] > 0 and stats[0]["proper"] > 0 and stats[0]["in_range"] > 0
    if name == "merge":
        assert res.merge is not None


def test_a_librarys_masks_are_gathered_by_the_pools_read_ids():
    """Two libraries, the first with N masks over its reads (a run of 16 bases masked in 30 % of them, 3 % masked whole), the second
    without: the round gathers the first library's mask rows through its pool's read ids, and the records equal the twin given the same
    rows gathered on the host — and differ from the twin without masks."""
    import torch
    from gappadder_amd import pair_span as PS
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    (gf, cfg, gaps, flanks, d_reads, d_recs, kk), (d_reads2, d_recs2) = _env(300, [(31, 29), (41, 39)])
    gen = torch.Generator(device="cpu").manual_seed(5)
    nmw = (L + 31) // 32
    mask = torch.zeros(2 * N_PAIRS, nmw, dtype=torch.int32)
    u = torch.rand(2 * N_PAIRS, generator=gen)
    mask[u < 0.30, 1] = 0x00FFFF00                                # bases 40..55
    mask[u < 0.03] = -1
    d_mask = mask.cuda()
    pipe = Pipeline(gf, len(gaps), L, kk, pair_span=True)
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * N_PAIRS, d_reads, d_recs, d_nmask=d_mask))
    pipe.add_library(DeviceLibrary("y", LIB2[0], LIB2[1], 2 * LIB2[2], d_reads2, d_recs2))
    pipe.prepare()
    pipe.step()
    res = pipe.fetch(pools=True)
    libs = [(lb.is_mean, lb.is_sd) for lb in pipe.libs]
    host = mask.numpy().view(np.uint32)
    want, stats = PS.pair_span_of_results(res, flanks, L, libs, nmasks=[host[res.lib_pool_ids[0].astype(np.int64)], None])
    bad = [(l, g) for l in range(2) for g in range(len(res.best)) if res.pairs[l, g].tobytes() != want[l, g].tobytes()]
    assert not bad, [(l, g, res.pairs[l, g], want[l, g]) for l, g in bad[:4]]
    assert res.pair_stats == stats and stats[0]["gaps"] > 0 and stats[0]["placed"] > 0
    plain, _ = PS.pair_span_of_results(res, flanks, L, libs)
    assert plain[1].tobytes() == want[1].tobytes() and plain[0].tobytes() != want[0].tobytes()
    assert stats[0]["placed"] < int(plain[0]["pairs_placed"].sum())       # the reads masked whole place nowhere


def _records(res):
    """Every contig record with its bases, order-free: two runs of the SAME step list the same records in different orders."""
    return sorted((int(c["gap"]), int(c["k"]), int(c["kv"]), int(c["n_nodes"]), int(c["length"]), int(c["cov_sum"]), s)
                  for c, (_, _, _, s) in zip(res.contigs, _contigs(res)))


def test_the_round_changes_nothing_else(pair):
    """`contigs`, `seq`, `best` and the polish / support results of the step with the round on against the step with it off, order-free
    (the step lists its contigs in no fixed order, and a pick word names its contig by index), and the bytes wherever the two lists do
    come in one order."""
    from gappadder_amd import polish as PL
    name, _, _, (pipe, res), (pipe_off, ref) = pair
    assert ref.pairs is None and ref.pair_stats is None and ref.lib_pool_ids is None and pipe_off.pairs is None
    assert _records(res) == _records(ref) and len(res.seq) == len(ref.seq)
    assert _picks(res) == _picks(ref) and (res.best != 0).tobytes() == (ref.best != 0).tobytes()
    assert res.merge == ref.merge
    if name == "exact":
        assert res.support.tobytes() == ref.support.tobytes() and res.support_stats == ref.support_stats and res.polish_stats == ref.polish_stats
        strip = lambda r: [tuple(int(x[f]) for f in x.dtype.names if f != "off") for x in r.polish]
        assert strip(res) == strip(ref)
        assert all(PL.polished_text(res, g) == PL.polished_text(ref, g) for g in range(len(res.best)))
    else:
        assert res.polish is None and res.support is None
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()


def test_constructor_refuses_what_the_round_excludes():
    from gappadder_amd.pipeline import Pipeline
    gf = _env(300, [(31, 29), (41, 39)])[0][0]
    with pytest.raises(ValueError, match="second_round"):
        Pipeline(gf, 24, L, [(31, 29)], pair_span=True, second_round=True)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, [(31, 29)], pair_span=True, world=2)
    with pytest.raises(ValueError, match="pair_span"):
        Pipeline(gf, 24, L, [(31, 29)], pair_span=True, pair_seed=40)
    with pytest.raises(ValueError, match="pair_span"):
        Pipeline(gf, 24, L, [(31, 29)], pair_span=True, pair_z=0)
    with pytest.raises(ValueError, match="pair_span"):
        Pipeline(gf, 24, L, [(31, 29)], pair_span=True, pair_seed=32, pair_max_mismatch=4)
    assert not Pipeline(gf, 24, L, [(31, 29)]).keep_read_ids
