"""Pipeline(flank_joins=True) on the shared synthetic step (step_util: 24 gaps of 300 bases, 80 000 pairs).  Six gaps get a doctored left
flank: truth text of the same length that ends o bases PAST the right flank's first base, o in {12, 29, 30, 31, 90, 200} — the flanks
overlap, the reads still come from the generator's truth, so the assembled contigs run through the junction with the two anchors out of
order.  Before the device is asked, the reference pipeline on the CPU (the oracle's reads, k-mer screen, mates and assembly, then the
twin) must join at least 4 of the 6 with exactly their o.  On the device: records and statistics equal the twin on the fetched contigs;
everything else equals the run with the option off; the planted gaps are open in both; no unplanted gap has a record; the round goes
with second_round and extended_fill and leaves their results alone; anchor_mode "align" is refused."""
import numpy as np
import pytest

import step_util as SU
from step_util import GPS, L, N_PAIRS, NSCF, SEED, SLEN

pytestmark = pytest.mark.gpu

KK = [(31, 29)]
GAP_LEN = 300
PLANTED = {1: 12, 5: 29, 9: 30, 13: 31, 17: 90, 21: 200}        # gap: o


def _doctored(cfg, gaps, flanks):
    from gappadder_amd.hip_api import GapFill
    out = list(flanks)
    for g, o in PLANTED.items():
        lf, rf = flanks[g]
        at = int(gaps[g]["end"]) + 5                # the right flank's first base (gnrt_pos_true_seqs.flanks)
        assert GapFill.synth_truth(cfg, int(gaps[g]["scaffold"]), at, 40) == rf[:40]
        new = GapFill.synth_truth(cfg, int(gaps[g]["scaffold"]), at + o - len(lf), len(lf))
        assert len(new) == len(lf) and new[-o:] == rf[:o]
        out[g] = (new, rf)
    return out


@pytest.fixture(scope="module")
def env():
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = SU.setup(GAP_LEN, KK)
    flanks = _doctored(cfg, gaps, flanks)
    gf.set_gaps(gaps, NSCF, flanks)
    return gf, cfg, gaps, flanks, d_reads, d_recs, kk


def test_the_reference_pipeline_joins_the_planted_gaps_on_the_cpu(env):
    """The floor, from the CPU alone: the oracle's reads of the same seed, screened at k = 31 against the planted gaps' flanks, with
    their mates, assembled by the oracle, through the twin."""
    from gappadder_amd import flank_joins as FJ
    from oracle import c_oracle as CO
    _, _, gaps, flanks, _, _, _ = env
    ocfg = CO.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=GAP_LEN, read_len=L)
    packed, _ = CO.synth_pairs(ocfg, 0, N_PAIRS, with_records=False)
    blob = CO.unpack_reads(packed, L)
    blob = blob.tobytes() if hasattr(blob, "tobytes") else bytes(blob)
    order = sorted(PLANTED)
    hits = CO.screen_reads(blob, L, [flanks[g] for g in order], 31)
    joined = 0
    for n, g in enumerate(order):
        ids = sorted(set(int(x["read"]) for x in hits if x["gap"] == n) | set(int(x["read"]) ^ 1 for x in hits if x["gap"] == n))
        pool = b"".join(blob[i * L:(i + 1) * L] for i in ids)
        contigs = [(0, s) for s, _, _ in CO.assemble_pool(pool, L, *KK[0])]
        rec, st = FJ.joins_host(contigs, [flanks[g]], [0])
        print("gap %d o=%d: %d reads, %d contigs, %s %s" % (g, PLANTED[g], len(ids), len(contigs), rec[0], st))
        joined += int(rec[0]["overlap"]) == PLANTED[g] and FJ.usable(rec[0])
    assert joined >= 4


@pytest.fixture(scope="module")
def runs(env):
    return SU.run(env, steps=2, flank_joins=True), SU.run(env)


def _view(res):
    return (sorted(SU.contigs(res)), SU.picks(res), res.n_contigs, res.n_seq, res.n_closed, (res.best != 0).tobytes())


def _check_against_the_twin(pipe, res):
    from gappadder_amd import flank_joins as FJ
    want, stats = FJ.joins_of_results(pipe, res)
    print(stats, {g: int(want[g]["overlap"]) for g in np.nonzero(want["overlap"])[0]})
    bad = [g for g in range(len(want)) if res.joins[g].tobytes() != want[g].tobytes()]
    assert not bad, [(g, res.joins[g], want[g]) for g in bad[:4]]
    assert res.join_stats == stats
    for g, o in PLANTED.items():
        assert int(res.best[g]) == 0, g                       # open: its anchors are out of order on every contig
        if int(want[g]["overlap"]):
            assert int(res.joins[g]["overlap"]) == o, (g, res.joins[g])
    unplanted = [g for g in range(len(want)) if g not in PLANTED]
    assert res.joins[unplanted].tobytes() == bytes(32 * len(unplanted))
    return want


def test_records_equal_the_twin_and_nothing_else_changes(runs):
    from gappadder_amd import flank_joins as FJ
    (pipe, (res, res2)), (pipe_off, (ref,)) = runs
    assert res.joins.dtype.itemsize == 32 and len(res.joins) == 24
    want = _check_against_the_twin(pipe, res)
    assert res.join_stats["open_gaps"] == int((res.best == 0).sum()) >= len(PLANTED)
    assert pipe.joined_gaps(res) == {g: int(want[g]["overlap"]) for g in range(24) if FJ.usable(want[g])}
    # a second step: the same records (the contig order may differ: the index is the list's)
    _check_against_the_twin(pipe, res2)
    assert [(int(r["overlap"]), int(r["flags"]), int(r["level"])) for r in res2.joins] == [(int(r["overlap"]), int(r["flags"]), int(r["level"])) for r in res.joins]
    # the option off: no records, everything else the same, the planted gaps open there too
    assert ref.joins is None and ref.join_stats is None and pipe_off.joins is None
    with pytest.raises(ValueError):
        pipe_off.joined_gaps(ref)
    assert _view(res) == _view(ref) and res.n_closed > 0
    assert all(int(ref.best[g]) == 0 for g in PLANTED)
    assert [lb.counts for lb in pipe.libs] == [lb.counts for lb in pipe_off.libs]
    for name in ("merge", "rescue", "round2", "extended", "ext", "support", "polish", "pairs", "pair_anchors", "gap_span", "pileup"):
        assert getattr(res, name) is None and getattr(ref, name) is None
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()


@pytest.mark.parametrize("other", [dict(second_round=True, extended_fill=True), dict(merge_in_step=True, extended_fill=True)],
                         ids=["second_round_and_extended_fill", "merge_in_step_and_extended_fill"])
def test_with_the_other_rounds(env, other):
    """The round is accepted beside them, its records equal the twin on that run's contigs, and their results are what they are without it."""
    pipe, (res,) = SU.run(env, flank_joins=True, **other)
    _, (ref,) = SU.run(env, **other)
    _check_against_the_twin(pipe, res)
    assert _view(res) == _view(ref)
    assert res.round2 == ref.round2 and res.extended == ref.extended and res.rescue == ref.rescue and res.merge == ref.merge
    if "extended_fill" in other:
        ext = lambda p, r: {g: v[2:] for g, v in p.extended_sequences(r).items()}
        assert ext(pipe, res) == ext(pipe, ref) and res.extended["gaps_extended"] >= 0
        if res.contigs.tobytes() == ref.contigs.tobytes():
            assert res.ext.tobytes() == ref.ext.tobytes() and res.ext_bases == ref.ext_bases


def test_constructor_refusals(env):
    from gappadder_amd.pipeline import Pipeline
    gf = env[0]
    for mode in ("align", "gapped"):
        with pytest.raises(ValueError, match="exact"):
            Pipeline(gf, 24, L, KK, flank_joins=True, anchor_mode=mode)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(gf, 24, L, KK, flank_joins=True, world=2)
    for kw in (dict(join_max_overlap=0), dict(join_max_overlap=1025), dict(join_min_context=256), dict(join_max_mismatch=16), dict(join_max_mismatch="2")):
        with pytest.raises(ValueError, match="flank_joins"):
            Pipeline(gf, 24, L, KK, flank_joins=True, **kw)
    assert Pipeline(gf, 24, L, KK, join_max_overlap=0).joins is None                  # (off: the values are not looked at)
