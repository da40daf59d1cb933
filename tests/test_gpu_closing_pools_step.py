"""Pipeline(second_round=True, recruit_rounds=4, closing_pools=True) on step_util's synthetic step (24 gaps of 1 400 bases, 80 000 pairs):
the closing pools against their definition built here from the step's pool, the recruits' read ids and the library's rows; every
after-pick round against its host twin evaluated on that host-built pool; that the rounds see what the step's pool alone does not show;
that nothing else of the step moves; two libraries; a capacity one row short."""
import copy

import numpy as np
import pytest

import step_util as SU
from step_util import L, N_PAIRS

pytestmark = pytest.mark.gpu

KK = [(31, 29)]
R_MAIN = 4
BASE = dict(second_round=True, recruit_rounds=R_MAIN, keep_read_ids=True)
ROUNDS = dict(read_support=True, polish=True, pileup=True, pair_span=True, alternatives=True, adjudicate=True)
RB = (L + 3) // 4


@pytest.fixture(scope="module")
def env():
    return SU.setup(1400, KK)


@pytest.fixture(scope="module")
def ref(env):
    """The step without the option (and without the rounds it lets in)."""
    pipe, (res,) = SU.run(env, pools=True, **BASE)
    return pipe, res


@pytest.fixture(scope="module")
def full(env):
    """Two steps with the closing pools and every round they let in."""
    pipe, (a, b) = SU.run(env, steps=2, pools=True, closing_pools=True, **BASE, **ROUNDS)
    return pipe, a, b


@pytest.fixture(scope="module")
def lib_rows(env):
    return env[4][:2 * N_PAIRS * RB].cpu().numpy().reshape(2 * N_PAIRS, RB)


def _unpack(rows):
    codes = np.stack([(rows >> s) & 3 for s in (6, 4, 2, 0)], axis=-1).reshape(len(rows), -1)[:, :L]
    return ["".join(r) for r in np.array(list("ACGT"))[codes]]


def _host_pool(res, src_off, src_rows, src_ids, libs_rows, library=None):
    """The definition, from the Results' own parts: per closed gap the source rows, then the recruits of round2_reads — (library, read id)
    in pool order — of the one library or of all.  -> (offsets, rows, ids, libraries)."""
    off, rows, ids, libs = [0], [], [], []
    for g in range(len(res.best)):
        if res.best[g]:
            a, z = int(src_off[g]), int(src_off[g + 1])
            rows.append(src_rows[a:z])
            ids += [int(x) for x in src_ids[a:z]] if src_ids is not None else [0xFFFFFFFF] * (z - a)
            libs += [library if library is not None else (0 if src_ids is not None else 0xFF)] * (z - a)
            rec = [(l, x) for l, x in res.round2_reads.get(g, []) if library is None or l == library]
            assert rec == sorted(set(rec))
            rows.append(np.stack([libs_rows[l][x] for l, x in rec]) if rec else np.zeros((0, RB), np.uint8))
            ids += [x for _, x in rec]
            libs += [l for l, _ in rec]
        off.append(sum(len(r) for r in rows))
    return (np.array(off, dtype=np.int64), np.concatenate(rows) if rows else np.zeros((0, RB), np.uint8), np.array(ids, dtype=np.uint32),
            np.array(libs, dtype=np.uint8))


def _on_pool(res, off, rows, ids=None):
    """A copy of the Results whose step pool (and library 0's) is the given one and that carries no closing pool: what a twin reads."""
    h = copy.copy(res)
    h.pool_off, h.pool_rows = off, rows
    h.closing_pool_off = h.closing_pool_rows = h.closing_lib_pool_off = None
    if ids is not None:
        h.lib_pool_off, h.lib_pool_rows, h.lib_pool_ids = [off], [rows], [ids]
    return h


def _late(res):
    """Gaps closed by a contig of round 2 or later."""
    from gappadder_amd.pipeline import decode_best
    first = res.recruit_rounds[1]["first"]
    return [g for g, w in enumerate(res.best.tolist()) if w and decode_best(w)[2] >= first]


@pytest.fixture(scope="module")
def host(full, lib_rows):
    """The host-built closing pool of the first step (one library: the step's pool is the library's own, its rows have ids)."""
    _, a, _ = full
    return _host_pool(a, a.pool_off, a.pool_rows, a.lib_pool_ids[0], [lib_rows])


# ---- a) the pool equals its definition ---------------------------------------------------------------------------------------------

def test_the_closing_pool_equals_its_definition(full, host):
    pipe, a, _ = full
    off, rows, ids, libs = host
    assert a.closing_pool_off.tolist() == off.tolist()
    assert a.closing_pool_rows.tobytes() == rows.tobytes() and a.closing_pool_nmask is None
    assert a.closing_pool_ids.tolist() == ids.tolist() and a.closing_pool_lib.tolist() == libs.tolist()
    # one library: its own closing pool is the merged one
    assert a.closing_lib_pool_off[0].tolist() == off.tolist() and a.closing_lib_pool_rows[0].tobytes() == rows.tobytes()
    assert a.closing_lib_pool_ids[0].tolist() == ids.tolist() and a.closing_lib_pool_nmask is None
    st = a.closing_pools
    n_rec = sum(len(v) for g, v in a.round2_reads.items() if a.best[g])
    assert (st["rows"], st["recruited_rows"], st["gaps"]) == (len(rows), n_rec, int((np.diff(off) > 0).sum())) and st["rows"] <= st["capacity"]
    assert st["per_library"] == [{"rows": len(rows), "gaps": st["gaps"], "recruited_rows": n_rec, "capacity": pipe.closing.lib_cap}]
    assert all(off[g] == off[g + 1] for g in np.nonzero(a.best == 0)[0])         # an open gap has no pool, whatever it recruited


def test_the_closing_pool_assembles_to_the_winning_contig(full):
    from gappadder_amd.pipeline import decode_best
    from oracle import c_oracle as CO
    _, a, _ = full
    late = _late(a)
    assert late
    rng = np.random.default_rng(5)
    for g in sorted(rng.choice(late, size=min(6, len(late)), replace=False).tolist()):
        pool = a.closing_pool_rows[int(a.closing_pool_off[g]):int(a.closing_pool_off[g + 1])]
        blob = "".join(_unpack(pool)).encode()
        texts = [c[0] for k, kv in KK for c in CO.assemble_pool(blob, L, k, kv)]
        assert SU.text(a, decode_best(a.best[g])[2]) in texts, g


# ---- b) every accepted round equals its twin on the host-built pool ----------------------------------------------------------------

def _records_equal(dev, want, texts_dev, texts):
    bad = []
    for g in range(len(want)):
        rec = dev[g].copy()
        o, n = int(rec["off"]), int(rec["len"])
        rec["off"] = 0
        if rec.tobytes() != want[g].tobytes() or (g in texts and not np.array_equal(texts_dev(g), texts[g])) or (g not in texts and (o or n)):
            bad.append(g)
    return bad


def test_support_equals_its_twin(env, full, host):
    from gappadder_amd import read_support as RS
    pipe, a, _ = full
    want, stats = RS.support_of_results(_on_pool(a, host[0], host[1]), env[3], L, 31, pipe.min_count)
    assert a.support.tobytes() == want.tobytes() and a.support_stats == dict(stats, k=31) and stats["gaps"] == int((a.best != 0).sum()) > 0


def test_polish_equals_its_twin(env, full, host):
    from gappadder_amd import polish as PL
    pipe, a, _ = full
    want, texts, stats = PL.polish_of_results(_on_pool(a, host[0], host[1]), env[3], L)
    assert not _records_equal(a.polish, want, lambda g: PL.polished_text(a, g), texts)
    assert a.polish_stats == stats and stats["placed"] > 0 and stats["mismatches"] == 0


def test_indel_polish_equals_its_twin(env, lib_rows):
    from gappadder_amd import polish as PL
    from gappadder_amd import polish_gapped as PG
    pipe, (res,) = SU.run(env, pools=True, closing_pools=True, polish=True, polish_indels=True, **BASE)
    off, rows, _, _ = _host_pool(res, res.pool_off, res.pool_rows, None, [lib_rows])
    assert res.closing_pool_off.tolist() == off.tolist() and res.closing_pool_rows.tobytes() == rows.tobytes()
    want, texts, stats = PG.polish_gapped_of_results(_on_pool(res, off, rows), env[3], L)
    assert not _records_equal(res.polish, want, lambda g: PL.polished_text(res, g), texts)
    assert res.polish_stats == stats and stats["placed"] > 0


def test_pileup_equals_its_twin(env, full, host):
    from gappadder_amd import pileup as PU
    pipe, a, _ = full
    want, tracks, stats = PU.pileup_of_results(_on_pool(a, host[0], host[1]), env[3], L)
    assert not _records_equal(a.pileup, want, lambda g: PU.track_of(a, g), tracks)
    assert a.pileup_stats == stats and stats["mismatches"] == 0


def test_pair_span_equals_its_twin(env, full, host):
    from gappadder_amd import pair_span as PS
    pipe, a, _ = full
    want, stats = PS.pair_span_of_results(_on_pool(a, host[0], host[1], host[2]), env[3], L, [(300, 30)])
    assert a.pairs.tobytes() == want.tobytes() and a.pair_stats == stats and stats[0]["placed"] > 0


def test_adjudication_equals_its_twin(full, host):
    from gappadder_amd import fill_adjudication as ADJ
    pipe, a, _ = full
    want, stats = ADJ.adjudication_of_results(pipe, _on_pool(a, host[0], host[1]))
    assert a.adjudication.tobytes() == want.tobytes() and a.adj_stats == stats and stats["mismatches"] == 0


# ---- c) not vacuous ----------------------------------------------------------------------------------------------------------------

def test_the_rounds_see_what_the_steps_pool_does_not_show(env, full, host):
    from gappadder_amd import pair_span as PS
    from gappadder_amd import read_support as RS
    pipe, a, _ = full
    late = _late(a)
    assert late, "no gap closed in round 2 or later"
    alone = _on_pool(a, a.pool_off, a.pool_rows, a.lib_pool_ids[0])             # P[g] alone
    sup_alone, _ = RS.support_of_results(alone, env[3], L, 31, pipe.min_count)
    print("gap: windows without support on the step's pool / on the closing pool",
          [(g, int(sup_alone[g]["n_zero"]), int(a.support[g]["n_zero"])) for g in late])
    assert all(sup_alone[g]["n_zero"] > 0 for g in late)                        # a long gap's middle has no read of the step's pool
    assert all(a.support[g]["n_zero"] < sup_alone[g]["n_zero"] for g in late)
    # a recruited pair has both mates unmapped: one that is placed lies on the fill with both mates
    pairs_alone, _ = PS.pair_span_of_results(alone, env[3], L, [(300, 30)])
    assert any(int(a.pairs[0, g]["pairs_placed"]) > int(pairs_alone[0, g]["pairs_placed"]) for g in late)
    g = max(late, key=lambda g: int(a.pairs[0, g]["pairs_placed"]) - int(pairs_alone[0, g]["pairs_placed"]))
    o0, o1 = int(host[0][g]), int(host[0][g + 1])
    recruited = set(x for _, x in a.round2_reads[g])
    assert recruited and recruited <= set(host[2][o0:o1].tolist())


# ---- d) nothing else moves ---------------------------------------------------------------------------------------------------------

def test_nothing_else_moves_and_two_steps_agree(ref, full):
    from test_gpu_recruit_rounds_step import _view
    pipe, a, b = full
    r = ref[1]
    assert _view(a) == _view(r) and _view(b) == _view(r)
    assert a.pool_off.tolist() == r.pool_off.tolist() and a.pool_rows.tobytes() == r.pool_rows.tobytes()
    assert r.closing_pools is None and r.closing_pool_off is None and r.support is None and ref[0].closing is None
    assert a.closing_pool_off.tolist() == b.closing_pool_off.tolist() and a.closing_pool_rows.tobytes() == b.closing_pool_rows.tobytes()
    assert a.closing_pool_ids.tobytes() == b.closing_pool_ids.tobytes() and a.closing_pools == b.closing_pools
    assert a.support_stats == b.support_stats and a.pair_stats == b.pair_stats and a.pileup_stats == b.pileup_stats
    if a.contigs.tobytes() == b.contigs.tobytes():          # the same list order: then every record is the same
        assert a.support.tobytes() == b.support.tobytes() and a.pairs.tobytes() == b.pairs.tobytes()


def test_gated_rounds_leave_the_closing_pool_of_the_rounds_that_ran(env, full):
    pipe6, (s,) = SU.run(env, pools=True, closing_pools=True, second_round=True, recruit_rounds=6, keep_read_ids=True)
    run = s.recruit_rounds_run
    assert run < 6 and all(d["gated"] for d in s.recruit_rounds[run:])
    want = full[1] if run == R_MAIN else SU.run(env, pools=True, closing_pools=True, second_round=True, recruit_rounds=run, keep_read_ids=True)[1][0]
    assert s.closing_pool_off.tolist() == want.closing_pool_off.tolist() and s.closing_pool_rows.tobytes() == want.closing_pool_rows.tobytes()
    assert s.closing_pool_ids.tobytes() == want.closing_pool_ids.tobytes() and s.closing_pools["rows"] == want.closing_pools["rows"] > 0


# ---- e) two libraries --------------------------------------------------------------------------------------------------------------

def test_two_libraries(env, lib_rows):
    import torch
    from gappadder_amd import pair_span as PS
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    half = N_PAIRS // 2
    d_reads2 = torch.empty(2 * half * RB + 64, dtype=torch.uint8, device="cuda")
    d_recs2 = torch.empty(2 * half * 32, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg, half, half, d_reads2.data_ptr(), d_recs2.data_ptr())      # (record read ids count from the batch's start)
    gf.sync()
    assert d_reads2[:2 * half * RB].cpu().numpy().tobytes() == lib_rows[2 * half:].tobytes()
    pipe = Pipeline(gf, len(gaps), L, kk, closing_pools=True, pair_span=True, **BASE)
    pipe.add_library(DeviceLibrary("a", 300, 30, 2 * half, d_reads, d_recs))
    pipe.add_library(DeviceLibrary("b", 300, 30, 2 * half, d_reads2, d_recs2))
    pipe.prepare()
    pipe.step()
    res = pipe.fetch(pools=True)
    libs_rows = [lib_rows[:2 * half], lib_rows[2 * half:]]
    assert _late(res) and {l for v in res.round2_reads.values() for l, _ in v} == {0, 1}
    off, rows, ids, libs = _host_pool(res, res.pool_off, res.pool_rows, None, libs_rows)
    assert res.closing_pool_off.tolist() == off.tolist() and res.closing_pool_rows.tobytes() == rows.tobytes()
    assert res.closing_pool_ids.tolist() == ids.tolist() and res.closing_pool_lib.tolist() == libs.tolist()
    per = []
    for l in (0, 1):
        o, r, i, _ = _host_pool(res, res.lib_pool_off[l], res.lib_pool_rows[l], res.lib_pool_ids[l], libs_rows, library=l)
        assert res.closing_lib_pool_off[l].tolist() == o.tolist() and res.closing_lib_pool_rows[l].tobytes() == r.tobytes()
        assert res.closing_lib_pool_ids[l].tolist() == i.tolist()
        assert res.closing_pools["per_library"][l]["rows"] == len(r) > 0
        per.append((o, r, i))
    assert sum(len(r) for _, r, _ in per) == len(rows)
    h = _on_pool(res, off, rows)
    h.lib_pool_off, h.lib_pool_rows, h.lib_pool_ids = [p[0] for p in per], [p[1] for p in per], [p[2] for p in per]
    want, stats = PS.pair_span_of_results(h, flanks, L, [(300, 30), (300, 30)])
    assert res.pairs.tobytes() == want.tobytes() and res.pair_stats == stats and all(s["placed"] > 0 for s in stats)


# ---- f) capacity -------------------------------------------------------------------------------------------------------------------

def test_a_step_beyond_the_capacity_raises_and_the_next_is_clean(env, full):
    """A pipeline of its own, prepared here: the assembly's pool bounds are options of the shared context, and the last prepare() sets them."""
    from test_gpu_recruit_rounds_step import _view
    a = full[1]
    pipe, (ref,) = SU.run(env, pools=True, closing_pools=True, **BASE, **ROUNDS)
    assert _view(ref) == _view(a) and ref.closing_pools == a.closing_pools and ref.closing_pool_rows.tobytes() == a.closing_pool_rows.tobytes()
    cap, lib_cap = pipe.closing.cap, pipe.closing.lib_cap
    for attr, keep in (("cap", cap), ("lib_cap", lib_cap)):
        setattr(pipe.closing, attr, ref.closing_pools["rows"] - 1)      # one row less than the pool needs
        pipe.step()
        with pytest.raises(RuntimeError, match="closing pools"):
            pipe.fetch()
        setattr(pipe.closing, attr, keep)
        pipe.step()
        c = pipe.fetch(pools=True)
        assert _view(c) == _view(ref) and c.closing_pools == ref.closing_pools
        assert c.closing_pool_off.tolist() == ref.closing_pool_off.tolist() and c.closing_pool_rows.tobytes() == ref.closing_pool_rows.tobytes()
        assert c.closing_lib_pool_rows[0].tobytes() == ref.closing_lib_pool_rows[0].tobytes()
        assert c.support_stats == ref.support_stats and c.pair_stats == ref.pair_stats and c.pileup_stats == ref.pileup_stats
