"""Pipeline(alternatives=True) on the shared synthetic step (step_util: 24 gaps of 300 bases, 80 000 pairs) with two (k, kv) pairs, so
that a closed gap has a contig of either.  Before the device is asked, the reference pipeline on the CPU (the oracle's layout, reads,
k-mer screen, mates and assembly at both pairs, the exact host picker, then the twin) must give at least half of the gaps it closes a
second candidate.  On the device: records, per-contig records and statistics equal the twin on the fetched contigs; no gap is lost or
outranked; a second step gives the same records up to the contig indices; everything else equals the run with the option off; the round
goes with second_round + extended_fill and with merge_in_step + flank_joins and leaves their results alone; the constructor refusals."""
import numpy as np
import pytest

import step_util as SU
from step_util import GPS, L, N_PAIRS, NSCF, SEED, SLEN

KK = [(31, 29), (41, 39)]
GAP_LEN = 300
INDEX_FREE = ("fill_len", "rival_len", "lcp", "lcs", "len_min", "len_max", "n_candidates", "n_lower", "n_identical", "n_near", "n_far", "dist", "level", "flags")


def test_the_reference_pipeline_gives_the_closed_gaps_a_second_candidate_on_the_cpu():
    """The floor, from the CPU alone: the oracle's reads of the same seed, screened at k = 31 against the flanks, with their mates,
    assembled by the oracle at both pairs, picked by the exact host picker at 30 then 15, through the twin."""
    from gappadder_amd import fill_alternatives as FA
    from gappadder_amd.pick_contigs import select_full, stand_in_hits
    from oracle import c_oracle as CO
    text = lambda s: s if isinstance(s, str) else bytes(s).decode()
    ocfg = CO.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=GAP_LEN, read_len=L)
    _, flanks = CO.synth_layout(ocfg)
    flanks = [(text(l), text(r)) for l, r in flanks]
    packed, _ = CO.synth_pairs(ocfg, 0, N_PAIRS, with_records=False)
    blob = CO.unpack_reads(packed, L)
    blob = blob.tobytes() if hasattr(blob, "tobytes") else bytes(blob)
    hits = CO.screen_reads(blob, L, flanks, 31)
    closed = several = 0
    for g, (lf, rf) in enumerate(flanks):
        ids = sorted(set(int(x["read"]) for x in hits if x["gap"] == g) | set(int(x["read"]) ^ 1 for x in hits if x["gap"] == g))
        pool = b"".join(blob[i * L:(i + 1) * L] for i in ids)
        contigs = [text(s) for k, kv in KK for s, _, _ in CO.assemble_pool(pool, L, k, kv)]
        sel = None
        for a in (30, 15):
            sel = select_full(stand_in_hits("exact", [("c%d" % i, s) for i, s in enumerate(contigs)], lf, rf, a))
            if sel is not None:
                break
        if sel is None:
            continue
        ci, _, _, _, _, rev = sel
        k = FA.candidate(contigs[ci].encode(), lf.encode(), rf.encode(), 30, 15)
        assert k is not None and (k[0], k[2]) == (a, int(rev)), (g, k[:3], a, rev)      # the twin's word is the host picker's selection
        rec, _, st = FA.alts_host([(0, s) for s in contigs], [(lf, rf)], [FA.pick_word(k[0], k[1], ci, k[2])])
        print("gap %d: %d reads, %d contigs, %s" % (g, len(ids), len(contigs), rec[0]))
        assert not st["lost"] and not st["outranked"]
        closed += 1
        several += int(rec[0]["n_candidates"]) >= 2
    assert closed >= 12 and 2 * several >= closed, (closed, several)


@pytest.fixture(scope="module")
def env():
    return SU.setup(GAP_LEN, KK)


@pytest.fixture(scope="module")
def runs(env):
    return SU.run(env, steps=2, alternatives=True), SU.run(env)


def _view(res):
    return (sorted(SU.contigs(res)), SU.picks(res), res.n_contigs, res.n_seq, res.n_closed, (res.best != 0).tobytes())


def _check_against_the_twin(pipe, res):
    from gappadder_amd import fill_alternatives as FA
    want, per, stats = FA.alts_of_results(pipe, res)
    print(stats)
    bad = [g for g in range(len(want)) if res.alts[g].tobytes() != want[g].tobytes()]
    assert not bad, [(g, res.alts[g], want[g]) for g in bad[:4]]
    assert res.alt_contigs.tobytes() == per.tobytes() and len(res.alt_contigs) == len(res.contigs)
    assert res.alt_stats == stats
    assert stats["lost"] == 0 and stats["outranked"] == 0 and stats["closed_gaps"] == int((res.best != 0).sum()) == res.n_closed
    for g in np.nonzero(res.best == 0)[0]:
        assert res.alts[g].tobytes() == bytes(48)
    return want


@pytest.mark.gpu
def test_records_equal_the_twin_and_nothing_else_changes(runs):
    from gappadder_amd import _lib as B
    from gappadder_amd.pipeline import decode_best
    (pipe, (res, res2)), (pipe_off, (ref,)) = runs
    assert res.alts.dtype.itemsize == 48 and len(res.alts) == 24 and res.alt_contigs.dtype.itemsize == 8
    want = _check_against_the_twin(pipe, res)
    closed = np.nonzero(res.best)[0]
    assert len(closed) >= 12 and 2 * int((want["n_candidates"][closed] >= 2).sum()) >= len(closed)       # the CPU's floor, on the device
    for g in closed:
        assert int(want[g]["contig"]) == decode_best(res.best[g])[2] and int(res.alt_contigs[int(want[g]["contig"])]["cls"]) == B.FA_C_WINNER
    seqs, picked = pipe.alternative_sequences(res), pipe.picked_sequences(res)
    assert sorted(seqs) == [int(g) for g in closed if int(want[g]["flags"]) & B.FA_F_HAS_RIVAL]
    for g, (ci, s, rev) in seqs.items():
        assert ci == int(want[g]["rival"]) != picked[g][0] and s != picked[g][1] and rev == bool(int(want[g]["flags"]) & B.FA_F_RIVAL_REVERSE)
    # a second step: the same records up to the contig indices (the list's order may differ)
    want2 = _check_against_the_twin(pipe, res2)
    assert [tuple(int(r[f]) for f in INDEX_FREE) for r in want2] == [tuple(int(r[f]) for f in INDEX_FREE) for r in want]
    # the option off: no records, everything else the same
    assert ref.alts is None and ref.alt_contigs is None and ref.alt_stats is None and pipe_off.alts is None
    with pytest.raises(ValueError):
        pipe_off.alternative_sequences(ref)
    assert _view(res) == _view(ref) and res.n_closed > 0
    assert [lb.counts for lb in pipe.libs] == [lb.counts for lb in pipe_off.libs]
    for name in ("merge", "rescue", "round2", "extended", "ext", "support", "polish", "pairs", "pair_anchors", "gap_span", "pileup", "joins"):
        assert getattr(res, name) is None and getattr(ref, name) is None
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("other", [dict(second_round=True, extended_fill=True), dict(merge_in_step=True, flank_joins=True)],
                         ids=["second_round_and_extended_fill", "merge_in_step_and_flank_joins"])
def test_with_the_other_rounds(env, other):
    """The round is accepted beside them, its records equal the twin on that run's contigs, and their results are what they are without it."""
    pipe, (res,) = SU.run(env, alternatives=True, **other)
    _, (ref,) = SU.run(env, **other)
    _check_against_the_twin(pipe, res)
    assert _view(res) == _view(ref)
    assert res.round2 == ref.round2 and res.extended == ref.extended and res.rescue == ref.rescue and res.merge == ref.merge
    assert res.join_stats == ref.join_stats
    if "flank_joins" in other and res.contigs.tobytes() == ref.contigs.tobytes():
        assert res.joins.tobytes() == ref.joins.tobytes()
    if "extended_fill" in other:
        ext = lambda p, r: {g: v[2:] for g, v in p.extended_sequences(r).items()}
        assert ext(pipe, res) == ext(pipe, ref) and res.extended["gaps_extended"] >= 0
        if res.contigs.tobytes() == ref.contigs.tobytes():
            assert res.ext.tobytes() == ref.ext.tobytes() and res.ext_bases == ref.ext_bases


@pytest.mark.gpu
def test_constructor_refusals(env):
    from gappadder_amd.pipeline import Pipeline
    gf = env[0]
    for mode in ("align", "gapped"):
        with pytest.raises(ValueError, match="exact"):
            Pipeline(gf, 24, L, KK, alternatives=True, anchor_mode=mode)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, KK, alternatives=True, world=2)
    for v in (0, 32, "16", 2.5, True):
        with pytest.raises(ValueError, match="alt_max_dist"):
            Pipeline(gf, 24, L, KK, alternatives=True, alt_max_dist=v)
    assert Pipeline(gf, 24, L, KK, alt_max_dist=0).alts is None                  # (off: the value is not looked at)
    assert Pipeline(gf, 24, L, KK, alternatives=True, alt_max_dist=31).alts.max_dist == 31
