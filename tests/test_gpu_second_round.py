"""Pipeline(second_round=True): the reference's second assembly round (assemble_gaps.py:344-351) inside the device step, against the
CLI's definition (collect_both_unmapped_reads.kmer_recruit_unmapped) and the oracle's assembly and picker, on synthetic steps: one whose
gaps are long enough that the first round closes none of them, and two where the first round closes some gaps and leaves the others
open (gap lengths measured on the GPU), one of them at k > 32 with two (k, kv) pairs."""
import numpy as np
import pytest

import sample_check as SC
from step_util import L, N_PAIRS, picks as _picks, run as _run, setup as _setup, text as _text

pytestmark = pytest.mark.gpu

# name -> (gap length, k pairs, does the first round close some of the 24 gaps?).  Round 1 reaches about one insert (300 bp) past each
# flank; measured on the GPU: 900 bp / k 31 closes 0 of 24 in round 1 (24 with round 2), 550 bp / k 31 closes 3 (24 with round 2),
# 450 bp / k 51 + 61 closes 15 (24 with round 2)
CONFIGS = {"open900_k31": (900, [(31, 29)], False), "mixed550_k31": (550, [(31, 29)], True),
           "mixed450_k51_61": (450, [(51, 49), (61, 59)], True)}


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def config(request):
    return CONFIGS[request.param]


@pytest.fixture(scope="module")
def env(config):
    return _setup(*config[:2])


@pytest.fixture(scope="module")
def on(env):
    pipe, (r1, r2) = _run(env, steps=2, pools=True, second_round=True, keep_read_ids=True)
    return pipe, r1, r2


@pytest.fixture(scope="module")
def off(env):
    return _run(env)


def _contig_set(res, lo=0, hi=None):
    hi = len(res.contigs) if hi is None else hi
    return sorted((int(res.contigs[i]["gap"]), int(res.contigs[i]["k"]), _text(res, i)) for i in range(lo, hi))


def _tried(res):
    """Gaps open after the first pick: still open, or closed by a round-2 contig."""
    from gappadder_amd.pipeline import decode_best
    return [g for g, w in enumerate(res.best.tolist()) if not w or decode_best(w)[2] >= res.round2_first]


def r2_gaps(res):
    """Gaps whose pick word names a round-2 contig."""
    from gappadder_amd.pipeline import decode_best
    return {g for g, w in enumerate(res.best.tolist()) if w and decode_best(w)[2] >= res.round2_first}


def _unpack(rows):
    codes = np.stack([(rows >> s) & 3 for s in (6, 4, 2, 0)], axis=-1).reshape(len(rows), -1)[:, :L]
    return ["".join(r) for r in np.array(list("ACGT"))[codes]]


def _candidates(d_recs):
    from gappadder_amd import _lib as B
    recs = np.frombuffer(d_recs.cpu().numpy().tobytes(), dtype=B.ALNREC)
    return sorted(set(int(r) >> 1 for r in recs["read"][(recs["flag"] & 12) == 12]))


def test_only_the_gaps_round_one_leaves_open_are_tried(env, config, on, off):
    """Gaps tried = the gaps the first pick leaves open (the run without the round): the others get no recruits, no round-2 contigs and
    keep their pick words; the mixed configurations have gaps of both kinds."""
    gaps = env[2]
    _, res, _ = on
    _, (res_off,) = off
    closed1 = set(np.nonzero(res_off.best)[0].tolist())
    if config[2]:
        assert 0 < len(closed1) < len(gaps), len(closed1)
    else:
        assert not closed1
    assert set(_tried(res)) == set(range(len(gaps))) - closed1
    assert res.round2["gaps_tried"] == len(gaps) - len(closed1)
    assert not closed1 & set(res.round2_reads)
    assert not closed1 & set(int(x) for x in res.contigs[res.round2_first:]["gap"])
    pk, pk_off = _picks(res), _picks(res_off)
    assert all(pk[g] == pk_off[g] for g in closed1)


def test_recruits_equal_the_cli_predicate(env, on):
    from gappadder_amd.collect_both_unmapped_reads import kmer_recruit_unmapped
    from gappadder_amd.hip_api import GapFill
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    _, res, _ = on
    r2 = res.round2
    assert r2["dropped"] == 0 and r2["gaps_tried"] == len(_tried(res)) > 0, r2
    pairs = _candidates(d_recs)
    assert 2 * len(pairs) == r2["candidates"] > 0
    rows = d_reads[:2 * N_PAIRS * ((L + 3) // 4)].cpu().numpy().reshape(2 * N_PAIRS, -1)
    ids = [r for p in pairs for r in (2 * p, 2 * p + 1)]
    seqs = _unpack(rows[ids])
    names = ["%d_%d" % (r >> 1, (r & 1) + 1) for r in ids]
    tried = _tried(res)
    contigs = [[_text(res, i) for i in range(res.round2_first) if int(res.contigs[i]["gap"]) == g] for g in tried]
    host = kmer_recruit_unmapped(GapFill(0), contigs, names, seqs, min(k for k, _ in kk))
    n_with = 0
    for g, idx in zip(tried, host):
        want = sorted(ids[i] for i in idx)
        got = [r for _, r in res.round2_reads.get(g, [])]
        assert got == want, (g, len(got), len(want))
        n_with += bool(want)
    assert set(res.round2_reads) <= set(tried)
    assert n_with == r2["gaps_with_recruits"] > 0 and r2["reads_recruited"] == sum(len(v) for v in res.round2_reads.values())


def test_round2_contigs_and_picks_equal_the_oracle(env, on):
    from oracle import c_oracle as CO
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    _, res, _ = on
    first = res.round2_first
    rows = d_reads[:2 * N_PAIRS * ((L + 3) // 4)].cpu().numpy().reshape(2 * N_PAIRS, -1)
    with_recruits = sorted(res.round2_reads)
    rng = np.random.default_rng(3)
    sample = sorted(rng.choice(with_recruits, size=min(6, len(with_recruits)), replace=False).tolist())
    assert sample
    expected = []
    for g in sample:
        pool = list(res.pool_rows[int(res.pool_off[g]):int(res.pool_off[g + 1])]) + [rows[r] for _, r in res.round2_reads[g]]
        blob = "".join(_unpack(np.stack(pool))).encode()
        expected.append([CO.assemble_pool(blob, L, k, kv) for k, kv in kk])
    ctg2 = res.contigs[first:]
    assert SC.contigs_equal(ctg2, res.seq, expected, kk, sample)
    # round-2 pick words of every tried gap: the oracle's picker over the gap's round-2 contigs (indices shifted by `first`)
    for g in _tried(res):
        w = SC.expected_pick_word(ctg2, res.seq, g, flanks, kk)
        assert int(res.best[g]) == (w - (first << 1) if w else 0), g
    # gaps without recruits keep no round-2 contigs
    assert set(int(x) for x in ctg2["gap"]) <= set(with_recruits)


def test_align_mode_round2_picks_equal_the_host_twin(env):
    from gappadder_amd.pick_contigs import pick_gap_sequence
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    pipe, (res,) = _run(env, second_round=True, anchor_mode="align")
    first = res.round2_first
    seqs = pipe.picked_sequences(res)
    n2 = 0
    for g in _tried(res):
        own = [("c%d" % i, _text(res, i)) for i in range(first, len(res.contigs)) if int(res.contigs[i]["gap"]) == g]
        want = None
        for t in (30, 15):
            want = pick_gap_sequence(own, flanks[g][0], flanks[g][1], t, mode="align") if own else None
            if want:
                break
        if want is None:
            assert g not in seqs, g
        else:
            assert g in seqs and seqs[g][1] == want[1], g
            n2 += 1
    assert n2 == res.round2["gaps_closed"]


def test_second_round_closes_more_gaps_mostly_with_the_truth(env, config, on, off):
    from gappadder_amd.hip_api import GapFill
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    p_on, res_on, _ = on
    p_off, (res_off,) = off
    s_on, s_off = p_on.picked_sequences(res_on), p_off.picked_sequences(res_off)
    assert len(s_on) > len(s_off) and (len(s_off) > 0) == config[2]
    pk_on, pk_off = _picks(res_on), _picks(res_off)
    assert all(pk_on[g] == pk_off[g] for g in pk_off), "a gap closed in round 1 changed its pick"
    assert set(pk_off) == set(g for g in pk_on if g not in r2_gaps(res_on))
    r2 = [g for g in s_on if g not in s_off]
    assert len(r2) == res_on.round2["gaps_closed"]
    truth = 0
    for g in r2:
        st, en, sc = int(gaps[g]["start"]), int(gaps[g]["end"]), int(gaps[g]["scaffold"])
        truth += s_on[g][1] in (GapFill.synth_truth(cfg, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg, sc, st - 6, en - st + 11))
    print("round 2: %d of %d closed gaps equal the truth" % (truth, len(r2)))
    assert truth >= 0.9 * len(r2)


def test_off_is_the_default_and_steps_repeat(env, on, off):
    _, (res_off,) = off
    _, (res_def,) = _run(env, second_round=False)
    assert res_off.round2 is None and res_def.round2 is None
    assert _picks(res_off) == _picks(res_def) and _contig_set(res_off) == _contig_set(res_def)
    assert (res_off.best != 0).tolist() == (res_def.best != 0).tolist()
    _, a, b = on
    assert a.round2 == b.round2 and a.round2_reads == b.round2_reads
    assert _picks(a) == _picks(b) and _contig_set(a) == _contig_set(b)
    # round 1's contigs are those of the run without the round
    assert _contig_set(a, 0, a.round2_first) == _contig_set(res_off)


def test_refused_combinations(env):
    from gappadder_amd.pipeline import Pipeline
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    with pytest.raises(ValueError):
        Pipeline(gf, len(gaps), L, kk, second_round=True, world=2)
    with pytest.raises(ValueError):
        Pipeline(gf, len(gaps), L, kk, second_round=True, merge_in_step=True)


def test_assembly_does_not_depend_on_the_pool_row_order(env, on):
    """The round-2 pool order (round-1 rows, then recruits by library and read id) is a convention: the same rows in another order
    give the same contigs (sequence, nodes, coverage)."""
    from gappadder_amd.hip_api import GapFill
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = env
    _, res, _ = on
    rows = d_reads[:2 * N_PAIRS * ((L + 3) // 4)].cpu().numpy().reshape(2 * N_PAIRS, -1)
    rng = np.random.default_rng(11)
    for g in sorted(res.round2_reads)[:4]:
        pool = np.stack(list(res.pool_rows[int(res.pool_off[g]):int(res.pool_off[g + 1])]) + [rows[r] for _, r in res.round2_reads[g]])
        got = []
        for perm in (np.arange(len(pool)), rng.permutation(len(pool)), np.arange(len(pool))[::-1]):
            ctg, seq = gf.assemble(np.ascontiguousarray(pool[perm]), np.array([0, len(pool)], dtype=np.uint64), L, kk)
            got.append(sorted((seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])], int(c["n_nodes"]), int(c["cov_sum"])) for c in ctg))
        assert got[0] and got[0] == got[1] == got[2], g
