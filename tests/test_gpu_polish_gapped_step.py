"""Pipeline(polish=True, polish_indels=True) on the shared synthetic step (step_util): Results.polish and the polished bases against the
host twin on the step's own pools, contigs and picks — exact anchors, behind the merge round, and in align mode; with the option off the
Results are the plain polish's, compared here by running both settings; polished_sequences against picked_sequences, and on fills
whose length the device round changed: the step's winning contigs with an indel planted in each (tools/polish_fills.py's list), the entry
called on that list with the step's own pools."""
import numpy as np
import pytest

from step_util import L, contigs as _contigs, picks as _picks, run as _run, setup as _setup

pytestmark = pytest.mark.gpu

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
def trio(request):
    gap_len, kk, kw = RUNS[request.param]
    env = _env(gap_len, kk)
    on = _run(env, pools=True, polish=True, polish_indels=True, **kw)
    plain = _run(env, polish=True, **kw)
    explicit_off = _run(env, polish=True, polish_indels=False, polish_max_indel=3, **kw)
    return request.param, env, on, plain, explicit_off


def test_the_round_equals_the_twin_on_the_steps_own_pools(trio):
    from gappadder_amd import _lib as B
    from gappadder_amd import polish as PL
    from gappadder_amd import polish_gapped as PG
    name, env, (pipe, (res,)), _, _ = trio
    flanks = env[3]
    assert pipe.polish.params == (16, 4, 48, 2, 8) and res.polish.dtype == B.FILL_POLISH_GAPPED
    want, texts, stats = PG.polish_gapped_of_results(res, flanks, L)
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
    assert res.polish_stats == stats and set(PG.STAT_KEYS) == set(stats)
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == len(res.polish_bases) and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    print("%s: %d of %d gaps closed, rows placed %d (split %d), events %d, inserted %d, deleted %d, changed %d"
          % (name, len(closed), len(res.best), stats["placed"], stats["split"], stats["events"], stats["inserted"], stats["deleted"], stats["changed"]))
    assert stats["placed"] > 0 and pipe.polish.base_cap == pipe.seq_cap + 64 * len(res.best)


def test_with_the_option_off_the_results_are_the_plain_polishs(trio):
    from gappadder_amd import _lib as B
    _, _, (pipe, (res,)), (pipe_plain, (ref,)), (pipe_off, (off,)) = trio
    assert type(pipe_plain.polish).__name__ == type(pipe_off.polish).__name__ == "FillPolish" and pipe_off.polish.params == (16, 4, 48, 2)
    assert ref.polish.dtype == off.polish.dtype == B.FILL_POLISH and ref.polish_stats == off.polish_stats
    by_bases = lambda r: sorted((g, x.tobytes()[8:], r.polish_bases[int(x["off"]):int(x["off"]) + int(x["len"])]) for g, x in enumerate(r.polish))
    assert by_bases(ref) == by_bases(off) and len(ref.polish_bases) == len(off.polish_bases)
    # and the round, on or off or gapped, changes nothing else of the step
    recs = lambda r: sorted((int(c["gap"]), int(c["k"]), int(c["kv"]), int(c["n_nodes"]), int(c["length"]), int(c["cov_sum"]), s)
                            for c, (_, _, _, s) in zip(r.contigs, _contigs(r)))
    assert recs(res) == recs(ref) == recs(off) and _picks(res) == _picks(ref) == _picks(off) and res.merge == ref.merge


def test_polished_sequences_follow_the_length_of_the_polished_contig(trio):
    from gappadder_amd import polish as PL
    from gappadder_amd.pipeline import contig_text
    _, _, (pipe, (res,)), (pipe_plain, (ref,)), _ = trio
    picked, polished, plain = pipe.picked_sequences(res), pipe.polished_sequences(res), pipe_plain.polished_sequences(ref)
    assert sorted(picked) == sorted(polished) == np.nonzero(res.best)[0].tolist()
    for g, (ci, body, rev) in picked.items():
        rec = res.polish[g]
        assert polished[g][0] == ci and polished[g][2] == rev
        assert len(polished[g][1]) - len(body) == int(rec["len"]) - int(res.contigs[ci]["length"]) == int(rec["n_inserted"]) - int(rec["n_deleted"])
        if int(rec["n_changed"]) == 0 and int(rec["n_events"]) == 0:
            assert polished[g][1] == body and PL.polished_text(res, g) == contig_text(res, ci)
        if int(rec["reads_split"]) == 0:                      # no row placed split: the plain polish's answer
            assert polished[g][1] == plain[g][1]


def test_polished_sequences_on_fills_whose_length_the_round_changed():
    """An indel of 1..8 bases planted in the body of every winning contig of the exact step; the round, on the step's pools, has to take
    it out again, and polished_sequences has to cut the step's own gap sequence from the polished contig."""
    import types
    import polish_fills as PF
    from gappadder_amd import _lib as B
    from gappadder_amd import polish_gapped as PG
    gap_len, kk, kw = RUNS["exact"]
    env = _env(gap_len, kk)
    pipe, (res,) = _run(env, polish=True, polish_indels=True, **kw)
    before = pipe.picked_sequences(res)
    recs, seq, words, planted = PF.planted_list(res, before, sorted(before), env[3], 8, np.random.default_rng(5))
    assert len(planted) == len(before) == 24 and all(len(a) != len(b) for a, b in planted.values())
    rec, bases, st = PF.run_entry(pipe, pipe.lib.gf_fill_polish_gapped_dev, B.FILL_POLISH_GAPPED, pipe.polish.params, B.PLG_WORDS, recs, seq, words)
    stats = PG.stats_of(st)
    edited = types.SimpleNamespace(best=words, contigs=recs, seq=seq, ctg_pick=None, polish=rec, polish_bases=bases)
    cut, polished = pipe.picked_sequences(edited), pipe.polished_sequences(edited)
    assert sorted(polished) == sorted(planted) and stats["mismatches"] == 0 and stats["gaps"] == 24
    restored = 0
    for g in planted:
        assert len(polished[g][1]) - len(cut[g][1]) == int(rec[g]["n_inserted"]) - int(rec[g]["n_deleted"]) == int(rec[g]["len"]) - int(recs[polished[g][0]]["length"])
        if int(rec[g]["n_events"]) == 1 and int(rec[g]["n_changed"]) == 0:
            restored += polished[g][1] == before[g][1] and len(polished[g][1]) != len(cut[g][1])
    print("planted %d, events %d, inserted %d, deleted %d, restored %d" % (len(planted), stats["events"], stats["inserted"], stats["deleted"], restored))
    # a pool of ~200 rows of 150 bases over a 300-base fill crosses every column some fifty times: most indels must come out again
    assert stats["events"] >= restored > len(planted) // 2
