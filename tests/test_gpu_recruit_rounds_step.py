"""Pipeline(second_round=True, recruit_rounds=R): the second round repeated inside the device step, chained round by round against its
definition on step_util's synthetic step (24 gaps, 80 000 pairs): the recruits of round r against the CLI's predicate on the device's own
contigs of round r - 1, the pools' assembly against the oracle's, the picks against the oracle's picker; the default, the gated rounds,
the 128-bit path, the other optional rounds, and a contig list too small for a later round."""
import numpy as np
import pytest

import sample_check as SC
import step_util as SU
from step_util import L, N_PAIRS

pytestmark = pytest.mark.gpu

KK = [(31, 29)]
R_MAIN = 4


@pytest.fixture(scope="module")
def env():
    return SU.setup(1400, KK)


@pytest.fixture(scope="module")
def main(env):
    pipe, (res,) = SU.run(env, pools=True, second_round=True, recruit_rounds=R_MAIN, keep_read_ids=True)
    return pipe, res


@pytest.fixture(scope="module")
def one(env):
    """R = 1 spelled out, and the same step without the argument."""
    return SU.run(env, pools=True, second_round=True, recruit_rounds=1, keep_read_ids=True), \
        SU.run(env, pools=True, second_round=True, keep_read_ids=True)


def _unpack(rows):
    codes = np.stack([(rows >> s) & 3 for s in (6, 4, 2, 0)], axis=-1).reshape(len(rows), -1)[:, :L]
    return ["".join(r) for r in np.array(list("ACGT"))[codes]]


def _read_rows(d_reads):
    return d_reads[:2 * N_PAIRS * ((L + 3) // 4)].cpu().numpy().reshape(2 * N_PAIRS, -1)


def _candidates(d_recs):
    from gappadder_amd import _lib as B
    recs = np.frombuffer(d_recs.cpu().numpy().tobytes(), dtype=B.ALNREC)
    return sorted(set(int(r) >> 1 for r in recs["read"][(recs["flag"] & 12) == 12]))


def _firsts(res):
    """F_1 .. F_R and the end of the list: round r's contigs are [F[r - 1], F[r])."""
    return [d["first"] for d in res.recruit_rounds] + [len(res.contigs)]


def _open_at(res, first):
    """Gaps open when the round whose contigs start at `first` begins: still open, or closed by a contig at or beyond it."""
    from gappadder_amd.pipeline import decode_best
    return [g for g, w in enumerate(res.best.tolist()) if not w or decode_best(w)[2] >= first]


def _view(res):
    return (sorted(SU.contigs(res)), SU.picks(res), res.n_contigs, res.n_seq, res.n_closed, res.round2, res.round2_reads, res.recruit_rounds,
            res.recruit_rounds_run, res.recruit_reads)


def test_every_round_equals_its_definition(env, main):
    """Round by round: H_r by the CLI's predicate on the contigs round r - 1 appended, of the gaps then open; new pairs, grown gaps and
    counters; the contigs of six grown gaps against the oracle's assembly of round-1 rows + all recruits so far; every tried gap's pick."""
    from gappadder_amd.collect_both_unmapped_reads import kmer_recruit_unmapped
    from gappadder_amd.hip_api import GapFill
    from oracle import c_oracle as CO
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    pipe, res = main
    n_gaps = len(gaps)
    rounds, F = res.recruit_rounds, _firsts(res)
    assert len(rounds) == R_MAIN == len(res.recruit_reads) and res.round2_first == F[0]
    assert all(d["dropped"] == 0 for d in rounds) and res.round2["dropped"] == 0
    pairs = _candidates(d_recs)
    assert 2 * len(pairs) == rounds[0]["candidates"] > 0
    rows = _read_rows(d_reads)
    ids = [r for p in pairs for r in (2 * p, 2 * p + 1)]
    seqs = _unpack(rows[ids])
    names = ["%d_%d" % (r >> 1, (r & 1) + 1) for r in ids]
    seen = {g: set() for g in range(n_gaps)}                   # S: reads recruited so far
    expected_best = {g: 0 for g in _open_at(res, F[0])}
    rng = np.random.default_rng(3)
    grew_later = False
    for r in range(R_MAIN):
        d = rounds[r]
        lo, hi = (0, F[0]) if r == 0 else (F[r - 1], F[r])
        open_now = _open_at(res, F[r])
        if d["gated"]:
            assert r >= res.recruit_rounds_run and d["contigs"] == 0 and F[r + 1] == F[r] and res.recruit_reads[r] == {}
            continue
        assert d["gaps_tried"] == len(open_now) and d["first"] == F[r] and d["contigs"] == F[r + 1] - F[r]
        contigs = [[SU.text(res, i) for i in range(lo, hi) if int(res.contigs[i]["gap"]) == g] for g in open_now]
        host = kmer_recruit_unmapped(GapFill(0), contigs, names, seqs, 31)
        grown = []
        for g, idx in zip(open_now, host):
            new = sorted(set(ids[i] for i in idx) - seen[g])
            got = [x for _, x in res.recruit_reads[r].get(g, [])]
            assert got == new, (r, g, len(got), len(new))
            seen[g].update(new)
            if new:
                grown.append(g)
        assert set(res.recruit_reads[r]) == set(grown)           # nothing for a closed gap, nothing for an open gap that met no new pair
        assert d["gaps_grown"] == len(grown) and 2 * d["new_pairs"] == sum(len(v) for v in res.recruit_reads[r].values())
        assert d["reads_recruited"] == sum(len(v) for v in seen.values())
        grew_later |= r >= 1 and bool(grown)
        ctg = res.contigs[F[r]:F[r + 1]]
        assert set(int(x) for x in ctg["gap"]) <= set(grown)     # an open gap that did not grow is not assembled again
        sample = sorted(rng.choice(grown, size=min(6, len(grown)), replace=False).tolist()) if grown else []
        expected = []
        for g in sample:
            pool = list(res.pool_rows[int(res.pool_off[g]):int(res.pool_off[g + 1])]) + [rows[x] for x in sorted(seen[g])]
            blob = "".join(_unpack(np.stack(pool))).encode()
            expected.append([CO.assemble_pool(blob, L, k, kv) for k, kv in kk])
        assert SC.contigs_equal(ctg, res.seq, expected, kk, sample), (r, sample)
        for g in open_now:
            w = SC.expected_pick_word(ctg, res.seq, g, flanks, kk)
            if w and not expected_best[g]:
                expected_best[g] = w - (F[r] << 1)
        assert d["gaps_closed"] == len([g for g in open_now if g not in _open_at(res, F[r + 1])]), r
    for g, w in expected_best.items():
        assert int(res.best[g]) == w, g
    # the cumulative list is what the rounds' new reads add up to
    assert {g: [x for _, x in v] for g, v in res.round2_reads.items()} == {g: sorted(s) for g, s in seen.items() if s}
    # not vacuous: a gap grew in a later round, and a pick names a contig of round 2 or later
    from gappadder_amd.pipeline import decode_best
    assert grew_later
    assert any(w and decode_best(w)[2] >= F[1] for w in res.best.tolist())
    run = res.recruit_rounds_run
    assert 1 <= run <= R_MAIN and (run == R_MAIN or rounds[run - 1]["gaps_grown"] == 0)
    assert all(rounds[j]["gaps_grown"] > 0 for j in range(run - 1))


def test_more_rounds_close_more_gaps_mostly_with_the_truth(env, main, one):
    from gappadder_amd.hip_api import GapFill
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    pipe, res = main
    (p1, (res1,)), _ = one
    s4, s1 = pipe.picked_sequences(res), p1.picked_sequences(res1)
    assert len(s4) > len(s1), (len(s4), len(s1))
    assert all(s4[g][1:] == s1[g][1:] for g in s1), "a gap closed by round 1 changed its fill"
    later = [g for g in s4 if g not in s1]
    truth = 0
    for g in later:
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        truth += s4[g][1] in (GapFill.synth_truth(cfg, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg, sc, st - 6, en - st + 11))
    print("rounds 2..%d: %d gaps closed, %d equal the truth; per round %s" % (R_MAIN, len(later), truth, [d["gaps_closed"] for d in res.recruit_rounds]))
    assert truth >= 0.9 * len(later)
    assert sum(d["gaps_closed"] for d in res.recruit_rounds[1:]) == len(later) > 0


def test_one_round_is_the_step_without_the_argument(one):
    (_, (a,)), (_, (b,)) = one
    assert a.round2 == b.round2 and a.round2_reads == b.round2_reads and a.round2_first == b.round2_first
    assert sorted(SU.contigs(a)) == sorted(SU.contigs(b)) and SU.picks(a) == SU.picks(b)
    assert (a.n_contigs, a.n_seq, a.n_closed) == (b.n_contigs, b.n_seq, b.n_closed)
    assert a.recruit_rounds_run == 1 and len(a.recruit_rounds) == 1 and not a.recruit_rounds[0]["gated"]
    assert a.recruit_rounds[0]["gaps_grown"] == a.round2["gaps_with_recruits"] and 2 * a.recruit_rounds[0]["new_pairs"] == a.round2["reads_recruited"]
    assert a.recruit_reads == [a.round2_reads]


def test_rounds_behind_the_last_are_gated_and_steps_repeat(env, main):
    pipe6, (a, b) = SU.run(env, steps=2, second_round=True, recruit_rounds=6, keep_read_ids=True)
    run = a.recruit_rounds_run
    assert run < 6, "six rounds and every one grew a gap: nothing gated to look at"
    for d in a.recruit_rounds[run:]:
        assert d["gated"] and d["contigs"] == 0 and d["first"] == a.n_contigs and d["new_pairs"] == 0 and d["gaps_grown"] == 0
    assert not any(d["gated"] for d in a.recruit_rounds[:run])
    assert _view(a) == _view(b)
    ref = main[1] if run == R_MAIN else SU.run(env, second_round=True, recruit_rounds=run, keep_read_ids=True)[1][0]
    va, vr = _view(a), _view(ref)
    assert va[:7] == vr[:7] and a.recruit_rounds[:run] == ref.recruit_rounds and a.recruit_rounds_run == ref.recruit_rounds_run
    assert a.recruit_reads[:run] == ref.recruit_reads and all(x == {} for x in a.recruit_reads[run:])


def test_two_pairs_beyond_32_bases(env):
    """450 bp at (51, 49) + (61, 59): the 128-bit k-mers.  Round 1 closes what is open there, so rounds 2 and 3 have little or nothing to
    do: each is gated, or consistent with the definition."""
    from gappadder_amd.collect_both_unmapped_reads import kmer_recruit_unmapped
    from gappadder_amd.hip_api import GapFill
    kk = [(51, 49), (61, 59)]
    e = SU.setup(450, kk)
    gf, cfg, gaps, flanks, d_reads, d_recs, _ = e
    pipe, (res,) = SU.run(e, second_round=True, recruit_rounds=3, keep_read_ids=True)
    F = _firsts(res)
    pairs = _candidates(d_recs)
    rows = _read_rows(d_reads)
    ids = [r for p in pairs for r in (2 * p, 2 * p + 1)]
    seqs, names = _unpack(rows[ids]), ["%d_%d" % (r >> 1, (r & 1) + 1) for r in ids]
    seen = {g: set() for g in range(len(gaps))}
    for r, d in enumerate(res.recruit_rounds):
        if d["gated"]:
            assert r >= res.recruit_rounds_run and d["contigs"] == 0 and res.recruit_reads[r] == {}
            continue
        lo, hi = (0, F[0]) if r == 0 else (F[r - 1], F[r])
        open_now = _open_at(res, F[r])
        contigs = [[SU.text(res, i) for i in range(lo, hi) if int(res.contigs[i]["gap"]) == g] for g in open_now]
        host = kmer_recruit_unmapped(GapFill(0), contigs, names, seqs, 51) if open_now else []
        grown = 0
        for g, idx in zip(open_now, host):
            new = sorted(set(ids[i] for i in idx) - seen[g])
            assert [x for _, x in res.recruit_reads[r].get(g, [])] == new, (r, g)
            seen[g].update(new)
            grown += bool(new)
        assert d["gaps_grown"] == grown and set(int(x) for x in res.contigs[F[r]:F[r + 1]]["gap"]) <= set(open_now)
        for g in open_now:
            if g in _open_at(res, F[r + 1]):
                continue            # (open behind this round, or closed by a later one)
            w = SC.expected_pick_word(res.contigs[F[r]:F[r + 1]], res.seq, g, flanks, kk)
            assert int(res.best[g]) == w - (F[r] << 1), (r, g)
    assert not res.recruit_rounds[0]["gated"] and res.round2["gaps_closed"] > 0


def test_with_the_other_rounds(env, main):
    """Extended fill, flank joins and alternatives behind four recruitment rounds: each equals its own host twin on this run's Results,
    and the recruitment is what it is without them."""
    from gappadder_amd import fill_alternatives as FA
    from gappadder_amd import flank_joins as FJ
    from test_gpu_extended_fill import twin_expect
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    pipe, (res,) = SU.run(env, second_round=True, recruit_rounds=R_MAIN, keep_read_ids=True, extended_fill=True, flank_joins=True,
                          alternatives=True)
    ref = main[1]
    assert _view(res) == _view(ref)
    want, stats = FJ.joins_of_results(pipe, res)
    assert res.joins.tobytes() == want.tobytes() and res.join_stats == stats
    want, per, stats = FA.alts_of_results(pipe, res)
    assert res.alts.tobytes() == want.tobytes() and res.alt_contigs.tobytes() == per.tobytes() and res.alt_stats == stats
    assert stats["closed_gaps"] == res.n_closed > res.round2["gaps_closed"]
    # the extended fill goes over every recruitment round's contigs: from round 1's FIRST on
    open_gaps = [g for g in range(len(flanks)) if not res.best[g]]
    assert pipe.extended_sequences(res) == twin_expect(flanks, SU.contigs(res), pipe.kk, "exact", open_gaps, res.round2_first)


def test_a_later_round_beyond_the_contig_list_raises_and_the_next_step_is_clean(env, main):
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    ref = main[1]
    F = _firsts(ref)
    j = max(r for r in range(R_MAIN) if ref.recruit_rounds[r]["contigs"])       # the last round that appends contigs: a later one
    assert j >= 1 and F[j + 1] == len(ref.contigs) > F[j] > F[0]
    pipe = Pipeline(gf, len(gaps), L, kk, second_round=True, recruit_rounds=R_MAIN, keep_read_ids=True)
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * N_PAIRS, d_reads, d_recs))
    pipe.prepare()
    caps = (pipe.contig_cap, pipe.seq_cap)
    pipe.step()
    want = _view(pipe.fetch())
    assert want == _view(ref)
    # room for the rounds before, one record or one base short of that round's contigs; and room for round 1's contigs alone, less one
    # (the device's contig order may differ between steps: the counts do not)
    for cc, sc, what in ((F[j + 1] - 1, caps[1], "records"), (caps[0], ref.n_seq - 1, "bases"), (F[j] + 1, caps[1], "all but one record"),
                         (F[1] - 1, caps[1], "records of round 1")):
        pipe.contig_cap, pipe.seq_cap = cc, sc
        pipe.step()
        with pytest.raises(RuntimeError):
            pipe.fetch()
        pipe.contig_cap, pipe.seq_cap = caps
        pipe.step()
        assert _view(pipe.fetch()) == want, what
