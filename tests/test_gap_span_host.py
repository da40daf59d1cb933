"""gappadder_amd/gap_span.py on the host: the twin (gap_span_host) on hand-built records — every inequality of the definition at its
boundary and one base on either side, every flag bit alone, the other drops, the order of the classification, the neighbour checks at
the ends of the table and between scaffolds (gap_span_util.hand_cases: the expectations are written by hand) —, the estimator on the
exact expected mean of its own model, and the three keys of the configuration."""
import json

import numpy as np
import pytest

import gap_span_util as U


def _twin(rows, shift, **kw):
    from gappadder_amd import gap_span as GS
    return GS.gap_span_host(U.records(rows), U.GAPS, U.N_SCAFFOLDS, U.L, U.MU, U.SD, U.Z, shift, U.Q, **kw)


@pytest.mark.parametrize("case", U.hand_cases(), ids=lambda c: c[0])
def test_one_record_lands_in_the_counter_the_definition_names(case):
    name, shift, row, want = case
    got, stats = _twin([row], shift)
    exp = U.expected([case], shift)
    assert got.tobytes() == exp.tobytes(), (name, got, exp)
    assert stats["candidates"] == len(want) and stats["accepted"] == sum(c == "n" for c in want.values())
    assert stats["gaps_with_pairs"] == sum(c == "n" for c in want.values())


@pytest.mark.parametrize("shift", [0, 200, 1000])
def test_all_records_of_a_shift_together(shift):
    from gappadder_amd import _lib as B
    cases = U.hand_cases()
    rows = [c[2] for c in cases if c[1] == shift]
    got, stats = _twin(rows, shift)
    exp = U.expected(cases, shift)
    assert got.tobytes() == exp.tobytes()
    assert stats["candidates"] == int(exp["n_cand"].sum()) > 0 and stats["accepted"] == int(exp["n"].sum()) > 0
    # ... in any record order
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(rows))
    assert _twin([rows[i] for i in perm], shift)[0].tobytes() == exp.tobytes()
    assert got.dtype == B.GAP_SPAN and B.GAP_SPAN.itemsize == 64


def test_every_counter_is_reached_by_the_hand_cases():
    seen = {cls for c in U.hand_cases() for cls in c[3].values()}
    assert seen == set(U.CLASSES)
    assert sum(not c[3] for c in U.hand_cases()) >= 20


def test_empty_inputs():
    from gappadder_amd import _lib as B
    from gappadder_amd import gap_span as GS
    got, stats = _twin([], 0)
    assert not got.tobytes().strip(b"\0") and all(v == 0 for v in stats.values())
    got, stats = GS.gap_span_host(U.records([U.rec(9500, 10900)]), np.zeros(0, dtype=B.GAP), 4, U.L, U.MU, U.SD)
    assert len(got) == 0 and stats["candidates"] == 0


def test_parameter_checks():
    from gappadder_amd import gap_span as GS
    assert GS.check_params() == (3, 1000, 8) and GS.check_params(1, 0, 1) == (1, 0, 1)
    for kw in (dict(z=0), dict(z=-1), dict(z=2.5), dict(z="3"), dict(shift=-1), dict(shift=0.5), dict(min_pairs=0), dict(min_pairs=True),
               dict(z=None)):
        with pytest.raises(ValueError, match="gap_span"):
            GS.check_params(**kw)
    assert GS.window(1500, 100, 3, 200) == (1800, 1000, 2000)
    assert GS.window(5000, 500, 3, 1000) == (6500, 2500, 7500)
    GS.window(1000000, 10000, 3, (1 << 20) - 1030001)           # hi = 2^20 - 1
    with pytest.raises(ValueError, match="2\\^20"):
        GS.window(1000000, 10000, 3, (1 << 20) - 1030000)
    with pytest.raises(ValueError, match="negative"):
        GS.window(1500, -1)
    # the round object refuses them before it looks at its pipeline
    for kw in (dict(z=0), dict(shift=-5), dict(min_pairs=0)):
        with pytest.raises(ValueError):
            GS.GapSpan(None, **kw)
    assert (GS.GapSpan(None).z, GS.GapSpan(None).shift, GS.GapSpan(None).min_pairs) == (GS.Z, GS.SHIFT, GS.MIN_PAIRS) == (3, 1000, 8)


# ---- the estimator ------------------------------------------------------------------------------------------------------------------
EST = dict(L=100, mu=1500, sigma=100, z=3, D=200)
G_GRID = (0, 100, 300, 700, 1000, 1100, 1200, 1300)       # (from 1000 on G + 2 L exceeds mu - 3 sigma: the truncation bites)


def _rec(n, mean, var=100.0 ** 2):
    from gappadder_amd import _lib as B
    r = np.zeros((), dtype=B.GAP_SPAN)
    r["n"], r["sum"], r["sum_sq"] = n, int(round(n * mean)), int(round(n * (mean * mean + var)))
    return r


@pytest.mark.parametrize("d", [0, 50, -200, 200])
def test_estimate_inverts_the_exact_expected_mean(d):
    from gappadder_amd import gap_span as GS
    n, off = 1_000_000, []
    for G in G_GRID:
        G0 = G + d
        if G0 < 0:
            continue
        m = GS.expected_mean(G, G0, **EST)
        e = GS.estimate(_rec(n, m), G0, EST["L"], EST["mu"], EST["sigma"], EST["z"], EST["D"], 8)
        assert e is not None and abs(e.est - G) <= 1.0, (G, G0, m, e)
        assert e.se > 0 and np.isfinite(e.se)
        assert abs(e.naive - (G0 + EST["mu"] - m)) < 1e-3
        off.append((G, e.naive - G))
    # where every insert of the library can span, the naive estimate is nearly right; where the truncation bites it is far off
    for G, err in off:
        if G + 2 * EST["L"] >= EST["mu"] - 3 * EST["sigma"] + 100:
            assert abs(err) > 1.0, (G, err)
    assert max(abs(err) for G, err in off if G >= 1100) > 20


def test_expected_mean_does_not_increase_with_the_gap():
    from gappadder_amd import gap_span as GS
    for G0 in (0, 300, 1000, 1400):
        ms = [GS.expected_mean(G, G0, **EST) for G in range(0, 1601, 20)]
        ms = [m for m in ms if m is not None]
        assert len(ms) > 40 and all(a >= b - 1e-9 for a, b in zip(ms, ms[1:])), G0
    big = dict(L=150, mu=5000, sigma=500, z=3, D=1000)
    ms = [GS.expected_mean(G, 2000, **big) for G in range(0, 6001, 100)]
    ms = [m for m in ms if m is not None]
    assert all(a >= b - 1e-9 for a, b in zip(ms, ms[1:]))
    # nothing of the support spans: undefined
    assert GS.expected_mean(1500 + 6 * 100, 300, **EST) is None


def test_estimate_is_none_below_min_pairs():
    from gappadder_amd import gap_span as GS
    m = GS.expected_mean(300, 300, **EST)
    assert GS.estimate(_rec(7, m), 300, 100, 1500, 100, 3, 200, 8) is None
    assert GS.estimate(_rec(8, m), 300, 100, 1500, 100, 3, 200, 8) is not None
    assert GS.estimate(_rec(0, 0.0), 300, 100, 1500, 100, 3, 200, 1) is None
    e = GS.estimate(_rec(1, m), 300, 100, 1500, 100, 3, 200, 1)
    assert e is not None and abs(e.est - 300) <= 1.0


def test_estimate_stays_inside_its_range():
    from gappadder_amd import gap_span as GS
    assert GS.estimate(_rec(100, 1999.0), 300, 100, 1500, 100, 3, 200, 8).est == 0.0            # a mean above m(0)
    assert GS.estimate(_rec(100, 1001.0), 300, 100, 1500, 100, 3, 200, 8).est <= 2000 - 200     # a mean below everything


# ---- the configuration --------------------------------------------------------------------------------------------------------------
def _config(tmp_path, **params):
    for fn in ("d.fa", "a.bam", "l.fq", "r.fq"):
        (tmp_path / fn).write_text("")
    wf = tmp_path / "wf"
    wf.mkdir(exist_ok=True)
    p = tmp_path / "c.json"
    p.write_text(json.dumps({"draft_genome": {"fa": str(tmp_path / "d.fa")},
                             "alignments": [{"bam": str(tmp_path / "a.bam"), "is": 300, "std": 30}],
                             "raw_reads": [{"left": str(tmp_path / "l.fq"), "right": str(tmp_path / "r.fq")}],
                             "parameters": dict(params, working_folder=str(wf))}))
    return str(p)


def test_configuration_keys(tmp_path):
    from gappadder_amd import gap_span as GS
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path))
    assert cfg["gap_span"] is False and cfg["gap_span_shift"] == GS.SHIFT == 1000 and cfg["gap_span_min_pairs"] == GS.MIN_PAIRS == 8
    cfg = parse_configuration(_config(tmp_path, gap_span=True, gap_span_shift=0, gap_span_min_pairs=1))
    assert cfg["gap_span"] is True and cfg["gap_span_shift"] == 0 and cfg["gap_span_min_pairs"] == 1
    cfg = parse_configuration(_config(tmp_path, gap_span_shift=250))
    assert cfg["gap_span"] is False and cfg["gap_span_shift"] == 250


@pytest.mark.parametrize("key,value", [("gap_span_shift", -1), ("gap_span_shift", "far"), ("gap_span_shift", 1.5), ("gap_span_min_pairs", 0),
                                       ("gap_span_min_pairs", -3), ("gap_span_min_pairs", "many"), ("gap_span_min_pairs", True)])
def test_a_value_out_of_range_makes_main_exit_with_a_message(tmp_path, key, value):
    from gappadder_amd import main as M
    cfgp = _config(tmp_path, gap_span=True, **{key: value})
    with pytest.raises(SystemExit) as e:
        M.parse_configuration(cfgp)
    assert key in str(e.value)
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert key in str(e.value)
