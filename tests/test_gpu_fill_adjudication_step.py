"""Pipeline(alternatives=True, adjudicate=True) on the shared synthetic step (step_util: 24 gaps of 300 bases, 80 000 pairs) with two
(k, kv) pairs.  On that draft the two assemblies agree, so nothing is contested; the test PLANTS a heterozygous site in every gap: of the
reads that carry the 25 true bases around the middle of the gap (either strand), every second one gets the middle base substituted.
With the two alleles at equal depth the assemblies at k = 31 and k = 41 often resolve the bubble differently, and the gap is contested.
Before the device is asked, the reference pipeline on the CPU (the oracle's reads with the same plant, k-mer screen, mates, the oracle's
assembly at both pairs, the exact host picker, alts_host, then the twin) must give at least one contested gap with at least min_votes
votes.  On the device: records and statistics equal the twin on the fetched Results; a second step gives the same bytes up to the contig
indices; with adjudicate=False the step's contigs, picks, alts and alt_contigs are byte-identical; adjudicated_sequences equals
picked_sequences except at the SWITCH gaps."""
import numpy as np
import pytest

import step_util as SU
from step_util import GPS, L, N_PAIRS, NSCF, SEED, SLEN

KK = [(31, 29), (41, 39)]
GAP_LEN = 300
INDEX_FREE = ("locus_w", "locus_r", "votes_w", "votes_r", "votes_w_s0", "votes_r_s0", "ties", "unplaced", "only", "verdict", "flags")


def plant(blob, gaps, cfg, every=2, at=GAP_LEN // 2):
    """The reads (ASCII, L bytes each) with the site planted in every gap; returns (reads, reads changed per gap)."""
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pick_contigs import revcomp
    blob, changed = bytearray(blob), []
    for gap in gaps:
        T = GapFill.synth_truth(cfg, int(gap["scaffold"]), int(gap["start"]) + at - 12, 25)
        alt = "ACGT"[("ACGT".index(T[12]) + 1) % 4]
        n = 0
        for pat, sub in ((T.encode(), alt), (revcomp(T).encode(), revcomp(alt))):
            i = blob.find(pat)
            while i >= 0:
                if i // L == (i + 24) // L:                           # (inside one read)
                    if n % every == 0:
                        blob[i + 12] = ord(sub)
                    n += 1
                i = blob.find(pat, i + 1)
        changed.append((n + every - 1) // every)
    return bytes(blob), changed


def test_the_reference_pipeline_gives_a_contested_gap_with_votes_on_the_cpu():
    """The floor, from the CPU alone."""
    from gappadder_amd import fill_adjudication as ADJ
    from gappadder_amd import fill_alternatives as FA
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pick_contigs import select_full, stand_in_hits
    from oracle import c_oracle as CO
    text = lambda s: s if isinstance(s, str) else bytes(s).decode()
    ocfg = CO.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=GAP_LEN, read_len=L)
    gaps, flanks = CO.synth_layout(ocfg)
    flanks = [(text(l), text(r)) for l, r in flanks]
    packed, _ = CO.synth_pairs(ocfg, 0, N_PAIRS, with_records=False)
    blob = CO.unpack_reads(packed, L)
    cfg = GapFill.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=GAP_LEN, read_len=L)
    blob, changed = plant(blob.tobytes() if hasattr(blob, "tobytes") else bytes(blob), gaps, cfg)
    assert min(changed) >= 2, changed
    hits = CO.screen_reads(blob, L, flanks, 31)
    contested, with_votes, verdicts = 0, 0, []
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
        k = FA.candidate(contigs[sel[0]].encode(), lf.encode(), rf.encode(), 30, 15)
        best = [FA.pick_word(k[0], k[1], sel[0], k[2])]
        listed = [(0, s) for s in contigs]
        alts, _, st = FA.alts_host(listed, [(lf, rf)], best)
        reads = [pool[i * L:(i + 1) * L].decode() for i in range(len(ids))]
        rec, ast = ADJ.adjudicate_gaps(alts, listed, [(lf, rf)], best, lambda _: reads, L)
        print("gap %d: %d reads, %d contigs, %s" % (g, len(ids), len(contigs), rec[0]))
        assert not st["lost"] and not ast["mismatches"]
        contested += ast["contested"]
        with_votes += int(rec[0]["votes_w"]) + int(rec[0]["votes_r"]) >= ADJ.MIN_VOTES
        verdicts.append(int(rec[0]["verdict"]))
    assert contested >= 1 and with_votes >= 1, (contested, with_votes, verdicts)


@pytest.fixture(scope="module")
def env():
    """step_util's environment with the site planted in the device's reads."""
    import torch
    from gappadder_amd import read_support as RS
    from gappadder_amd.hip_api import GapFill
    e = SU.setup(GAP_LEN, KK)
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = e
    rb = (L + 3) // 4
    codes, _ = RS.codes_of_rows(d_reads[:2 * N_PAIRS * rb].cpu().numpy().reshape(-1, rb), L)
    blob, changed = plant(np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes(), gaps, cfg)
    assert min(changed) >= 2, changed
    packed, _ = GapFill.pack_reads(blob, L)
    d_reads[:2 * N_PAIRS * rb] = torch.from_numpy(np.ascontiguousarray(packed).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return e


@pytest.fixture(scope="module")
def runs(env):
    return SU.run(env, steps=2, pools=True, alternatives=True, adjudicate=True), SU.run(env, alternatives=True)


def _check_against_the_twin(pipe, res):
    from gappadder_amd import fill_adjudication as ADJ
    want, stats = ADJ.adjudication_of_results(pipe, res)
    print(stats)
    bad = [g for g in range(len(want)) if res.adjudication[g].tobytes() != want[g].tobytes()]
    assert not bad, [(g, res.adjudication[g], want[g]) for g in bad[:4]]
    assert res.adj_stats == stats and stats["mismatches"] == 0 and stats["contested"] == res.alt_stats["contested"]
    return want, stats


@pytest.mark.gpu
def test_records_equal_the_twin_and_nothing_else_changes(runs):
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_adjudication as ADJ
    (pipe, (res, res2)), (pipe_off, (ref,)) = runs
    assert res.adjudication.dtype.itemsize == 48 and len(res.adjudication) == 24
    want, stats = _check_against_the_twin(pipe, res)
    # the CPU's floor, on the device
    votes = want["votes_w"].astype(np.int64) + want["votes_r"]
    assert stats["contested"] >= 1 and stats["adjudicated"] == stats["contested"] and int((votes >= ADJ.MIN_VOTES).sum()) >= 1
    for g in range(24):
        if not int(res.alts[g]["flags"]) & B.FA_F_HAS_RIVAL:
            assert res.adjudication[g].tobytes() == bytes(48)
        else:
            assert int(want[g]["verdict"]) in (1, 2, 3) and (int(want[g]["contig"]), int(want[g]["rival"])) == (int(res.alts[g]["contig"]), int(res.alts[g]["rival"]))
    # a second step: the same records up to the contig indices (the list's order may differ)
    want2, stats2 = _check_against_the_twin(pipe, res2)
    assert [tuple(int(r[f]) for f in INDEX_FREE) for r in want2] == [tuple(int(r[f]) for f in INDEX_FREE) for r in want] and stats2 == stats
    if res2.contigs.tobytes() == res.contigs.tobytes():
        assert res2.adjudication.tobytes() == res.adjudication.tobytes()
    # adjudicated_sequences: the picked text, the rival's at the SWITCH gaps
    picked, rivals, seqs = pipe.picked_sequences(res), pipe.alternative_sequences(res), pipe.adjudicated_sequences(res)
    switch = {int(g) for g in np.nonzero(want["verdict"] == B.AJ_SWITCH)[0]}
    assert sorted(seqs) == sorted(picked)
    for g, (s, which) in seqs.items():
        assert (s, which) == ((rivals[g][1], "rival") if g in switch else (picked[g][1], "picked"))
        assert g not in switch or s != picked[g][1]
    # the option off: no records; contigs, picks, alts and alt_contigs byte-identical
    assert ref.adjudication is None and ref.adj_stats is None and pipe_off.adj is None
    with pytest.raises(ValueError):
        pipe_off.adjudicated_sequences(ref)
    assert (sorted(SU.contigs(res)), SU.picks(res), res.n_contigs, res.n_seq, res.n_closed) == (sorted(SU.contigs(ref)), SU.picks(ref), ref.n_contigs, ref.n_seq, ref.n_closed)
    assert res.alt_stats == ref.alt_stats and [lb.counts for lb in pipe.libs] == [lb.counts for lb in pipe_off.libs]
    assert pipe.picked_sequences(res) == pipe_off.picked_sequences(ref) or res.contigs.tobytes() != ref.contigs.tobytes()
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()
        assert res.alts.tobytes() == ref.alts.tobytes() and res.alt_contigs.tobytes() == ref.alt_contigs.tobytes()
    else:
        free = ("fill_len", "rival_len", "lcp", "lcs", "len_min", "len_max", "n_candidates", "n_lower", "n_identical", "n_near", "n_far", "dist", "level", "flags")
        assert [tuple(int(r[f]) for f in free) for r in res.alts] == [tuple(int(r[f]) for f in free) for r in ref.alts]


@pytest.mark.gpu
def test_with_the_other_after_pick_rounds_and_the_refusals(env):
    """Beside the polish and merge_in_step the records still equal the twin; the constructor's refusals."""
    from gappadder_amd.pipeline import Pipeline
    pipe, (res,) = SU.run(env, pools=True, alternatives=True, adjudicate=True, polish=True, merge_in_step=True, adj_context=60, adj_min_votes=1, adj_ratio=4)
    assert pipe.adj.params == (16, 4, 48, 60, 1, 4)
    _check_against_the_twin(pipe, res)
    gf = env[0]
    with pytest.raises(ValueError, match="adjudicate needs alternatives"):
        Pipeline(gf, 24, L, KK, adjudicate=True)
    with pytest.raises(ValueError, match="second_round"):
        Pipeline(gf, 24, L, KK, alternatives=True, adjudicate=True, second_round=True)
    for kw in (dict(adj_seed=11), dict(adj_context=47), dict(adj_context=1001), dict(adj_min_votes=0), dict(adj_ratio=17), dict(adj_max_mismatch=16)):
        with pytest.raises(ValueError, match="^adjudicate "):
            Pipeline(gf, 24, L, KK, alternatives=True, adjudicate=True, **kw)
    assert Pipeline(gf, 24, L, KK, alternatives=True, adj_ratio=99).adj is None                  # (off: the values are not looked at)
