"""The host side of the flank-overlap joins: the twin flank_joins.joins_host on hand-derived cases
(tests/flank_join_cases.py), check_params, the CLI keys in main.parse_configuration, and the write-back's optional fifth argument."""
import json
import os

import numpy as np
import pytest

import flank_join_cases as FC
from test_pair_span_config_host import _config

CASES = FC.cases()


def _check(recs, stats, cs, index):
    from gappadder_amd import flank_joins as FJ
    want, want_stats = FC.expected(cs, index)
    for g, (c, w) in enumerate(zip(cs, want)):
        if w is None:
            assert recs[g].tobytes() == bytes(32), c["name"]
            assert not FJ.usable(recs[g])
        else:
            got = {k: int(recs[g][k]) for k in w}
            assert got == w, (c["name"], got, w)
            assert FJ.usable(recs[g]) == (not w["flags"] & (FC.AMBIGUOUS | FC.MULTI)), c["name"]
    assert stats == want_stats


@pytest.mark.parametrize("interleave", [False, True])
def test_twin_gives_the_hand_derived_records_and_statistics(interleave):
    from gappadder_amd import flank_joins as FJ
    contigs, flanks, best, index = FC.assemble(CASES, interleave)
    recs, stats = FJ.joins_host(contigs, flanks, best, FC.ANCHORS, FC.X, FC.C, FC.M)
    assert recs.dtype.itemsize == 32 and len(recs) == len(CASES) >= 25
    _check(recs, stats, CASES, index)
    # the defaults are the cases' parameters
    again, stats2 = FJ.joins_host(contigs, flanks, best)
    assert again.tobytes() == recs.tobytes() and stats2 == stats


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_alone(case):
    from gappadder_amd import flank_joins as FJ
    contigs, flanks, best, index = FC.assemble([case])
    _check(*FJ.joins_host(contigs, flanks, best, FC.ANCHORS, FC.X, FC.C, FC.M), [case], index)


def test_first_skips_the_contigs_before_it_and_keeps_the_indices():
    from gappadder_amd import flank_joins as FJ
    case = next(c for c in CASES if c["name"] == "the earlier contig wins ties")
    contigs, flanks, best, index = FC.assemble([case])
    recs, stats = FJ.joins_host(contigs, flanks, best, first=1)
    assert int(recs[0]["contig"]) == 1 and int(recs[0]["n_accepted"]) == 1 and stats["candidates"] == 1
    recs, stats = FJ.joins_host(contigs, flanks, best, first=2)
    assert recs.tobytes() == bytes(32) and stats == dict(dict.fromkeys(FJ.STAT_KEYS, 0), open_gaps=1)


def test_a_single_anchor_length_and_other_parameters():
    """One anchor length: the long level alone.  X below the overlap: far; M = 0 refuses the one difference; C = 0 needs no context."""
    from gappadder_amd import flank_joins as FJ
    by = {c["name"]: c for c in CASES}
    contigs, flanks, best, _ = FC.assemble([by["short level only"]])
    assert FJ.joins_host(contigs, flanks, best, (30,))[0].tobytes() == bytes(32)
    assert int(FJ.joins_host(contigs, flanks, best, (15,))[0][0]["level"]) == 15
    contigs, flanks, best, _ = FC.assemble([by["o=100"]])
    assert FJ.joins_host(contigs, flanks, best, X=99)[1]["far"] == 1 and int(FJ.joins_host(contigs, flanks, best, X=100)[0][0]["overlap"]) == 100
    contigs, flanks, best, _ = FC.assemble([by["m_l = M"]])
    assert FJ.joins_host(contigs, flanks, best, M=1)[1]["mismatch"] == 1
    contigs, flanks, best, _ = FC.assemble([by["left context C-1"]])
    assert int(FJ.joins_host(contigs, flanks, best, C=29)[0][0]["overlap"]) == 40
    assert int(FJ.joins_host(contigs, flanks, best, C=0)[0][0]["overlap"]) == 40


@pytest.mark.parametrize("params", [dict(max_overlap=0), dict(max_overlap=1025), dict(min_context=-1), dict(min_context=256), dict(max_mismatch=-1),
                                    dict(max_mismatch=16), dict(max_overlap=2.5), dict(min_context="x"), dict(max_mismatch=True)])
def test_check_params_refuses_every_bound(params):
    from gappadder_amd import flank_joins as FJ
    with pytest.raises(ValueError):
        FJ.check_params(**params)


def test_check_params_takes_the_edges_and_the_anchor_limits_hold():
    from gappadder_amd import flank_joins as FJ
    assert FJ.check_params() == (256, 30, 2)
    assert FJ.check_params(1, 0, 0) == (1, 0, 0) and FJ.check_params(1024, 255, 15) == (1024, 255, 15)
    assert FJ.check_anchors((30, 15)) == (30, 15) and FJ.check_anchors((32, 8)) == (32, 8) and FJ.check_anchors((20,)) == (20, 0)
    for bad in ((33, 15), (30, 7), (15, 30), (15, 15), (7,)):
        with pytest.raises(ValueError):
            FJ.check_anchors(bad)
    with pytest.raises(ValueError):          # a flank of 65 536 bases
        FJ.joins_host([], [("A" * 65536, "ACGT")], [0])


# ---- the CLI keys -------------------------------------------------------------------------------------------------------------------

KEYS = ("flank_joins_max_overlap", "flank_joins_min_context", "flank_joins_max_mismatch")


def test_flank_joins_is_off_by_default_with_the_twins_defaults(tmp_path):
    from gappadder_amd import flank_joins as FJ
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path))
    assert cfg["flank_joins"] is False
    assert tuple(cfg[k] for k in KEYS) == (FJ.MAX_OVERLAP, FJ.MIN_CONTEXT, FJ.MAX_MISMATCH) == (256, 30, 2)


def test_flank_joins_and_its_parameters_are_read(tmp_path):
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path, flank_joins=True, flank_joins_max_overlap=100, flank_joins_min_context=20, flank_joins_max_mismatch=0))
    assert cfg["flank_joins"] is True and tuple(cfg[k] for k in KEYS) == (100, 20, 0)
    assert tuple(parse_configuration(_config(tmp_path, flank_joins_max_overlap=1, flank_joins_min_context=0))[k] for k in KEYS) == (1, 0, 2)
    assert tuple(parse_configuration(_config(tmp_path, flank_joins_max_overlap=1024, flank_joins_min_context=255, flank_joins_max_mismatch=15))[k]
                 for k in KEYS) == (1024, 255, 15)


@pytest.mark.parametrize("params, name", [(dict(flank_joins_max_overlap=0), "flank_joins_max_overlap"), (dict(flank_joins_max_overlap=1025), "flank_joins_max_overlap"),
                                          (dict(flank_joins_min_context=-1), "flank_joins_min_context"), (dict(flank_joins_min_context=256), "flank_joins_min_context"),
                                          (dict(flank_joins_max_mismatch=16), "flank_joins_max_mismatch"), (dict(flank_joins_max_mismatch="2"), "flank_joins_max_mismatch"),
                                          (dict(flank_joins_max_overlap=True), "flank_joins_max_overlap")])
def test_a_value_out_of_range_makes_main_exit_with_a_message(tmp_path, params, name):
    from gappadder_amd import main as M
    cfgp = _config(tmp_path, flank_joins=True, **params)
    with pytest.raises(SystemExit) as e:
        M.parse_configuration(cfgp)
    assert name in str(e.value)
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert name in str(e.value)


# ---- the write-back -----------------------------------------------------------------------------------------------------------------

def _draft(tmp_path, o=17):
    """One scaffold with three gaps of 100 N (and a second scaffold with one), built from a truth: around gap 2 of scf0 and the gap of
    scf1 the draft's flanks overlap by o bases — the text behind the run repeats the o + 5 + 5 bases before it (the flanks stop 5 bases
    short of the run on either side).  Returns (paths, truth per scaffold, gaps per scaffold [(start, end)])."""
    import random
    rng = random.Random(11)
    t0, t1 = FC.rnd(rng, 3000), FC.rnd(rng, 1500)
    n = "N" * 100
    # scf0: gap 1 a true gap of 40 missing bases at 500; gap 2 an overlap at 1500; gap 3 a true gap of 30 missing bases at 2500
    s0 = t0[:500] + n + t0[540:1500] + n + t0[1500 - o - 10:2500] + n + t0[2530:]
    s1 = t1[:700] + n + t1[700 - o - 10:]
    d = str(tmp_path)
    with open(d + "/draft.fa", "w") as f:
        f.write(">scf0 first\n" + "".join(s0[i:i + 70] + "\n" for i in range(0, len(s0), 70)))
        f.write(">scf1\n" + "".join(s1[i:i + 70] + "\n" for i in range(0, len(s1), 70)))
    from gappadder_amd.gnrt_pos_true_seqs import scan_gaps
    gaps = [scan_gaps(s0, 100), scan_gaps(s1, 100)]
    assert [len(g) for g in gaps] == [3, 1] and all(e - s == 100 for gs in gaps for s, e in gs)
    with open(d + "/draft.fa.fai", "w") as f:
        f.write("scf0\t%d\t12\t70\t71\nscf1\t%d\t0\t70\t71\n" % (len(s0), len(s1)))
    with open(d + "/gaps.txt", "w") as f:
        for name, gs in zip(("scf0", "scf1"), gaps):
            for s, e in gs:
                f.write("%d %d %d %s\n" % (s, e, e - s, name))
    return d, (s0, s1), (t0, t1), gaps


def _joins_tsv(path, rows):
    """rows: (key, overlap, usable, cut_from, resume_at); the columns the write-back reads, among others it must not care about."""
    with open(path, "w") as f:
        f.write("gap\tG0\toverlap\tusable\tname\tcut_from\tresume_at\n")
        for key, o, ok, a, b in rows:
            f.write("%s\t100\t%d\t%d\t%s_31_29_NODE_1_length_9_cov_3.000000\t%d\t%d\n" % (key, o, ok, key, a, b))


def _fasta(path):
    from gappadder_amd.put_gap_seq_back_to_scaffold import _records
    return {name: (desc, seq) for name, desc, seq in _records(path)}


def _row(key, gap, o, ok=1):
    return (key, o, ok, gap[0] - 5, gap[1] + 5 + o)


def test_write_back_joins_alone(tmp_path):
    from gappadder_amd.put_gap_seq_back_to_scaffold import put_gap_seq_back_to_scaffold
    d, (s0, s1), (t0, t1), gaps = _draft(tmp_path)
    open(d + "/picked.fa", "w").write("")
    _joins_tsv(d + "/joins.tsv", [_row("0_2", gaps[0][1], 17), _row("1_1", gaps[1][0], 17)])
    put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gaps.txt", d + "/picked.fa", d + "/new.fa", d + "/joins.tsv")
    new = _fasta(d + "/new.fa")
    # scf1: the truth itself, under the bare id; scf0: its overlap gone, the two true gaps as they were
    assert new["scf1"] == ("scf1", t1)
    n = "N" * 100
    assert new["scf0"] == ("scf0", t0[:500] + n + t0[540:2500] + n + t0[2530:])
    # without the fifth argument nothing is filled: the draft as it is, descriptions kept
    put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gaps.txt", d + "/picked.fa", d + "/plain.fa")
    assert _fasta(d + "/plain.fa") == {"scf0": ("scf0 first", s0), "scf1": ("scf1", s1)}


def test_write_back_joins_beside_fills_and_against_an_extended_record(tmp_path, capsys):
    from gappadder_amd.put_gap_seq_back_to_scaffold import put_gap_seq_back_to_scaffold
    d, (s0, s1), (t0, t1), gaps = _draft(tmp_path)
    # gap 1 filled by a full pick (the missing 40 bases + the base at `end`, which the write-back drops from the draft), gap 2 with a
    # partial fill only: the join replaces it; gap 3 open
    open(d + "/picked.fa", "w").write(">0_1_31_29_NODE_1_length_99_cov_7.000000\n%s\n>0_2_NODE_1_NODE_2_extended\nACGTNNACGT\n" % t0[500:541])
    _joins_tsv(d + "/joins.tsv", [_row("0_2", gaps[0][1], 17)])
    put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gaps.txt", d + "/picked.fa", d + "/new.fa", d + "/joins.tsv")
    new = _fasta(d + "/new.fa")
    assert new["scf0"] == ("scf0", t0[:2500] + "N" * 100 + t0[2530:]) and new["scf1"] == ("scf1", s1)
    assert "Gap  3 of Scaffold  0 does not exist!!!" in capsys.readouterr().out
    # the same without the table: the partial fill goes in, as today
    put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gaps.txt", d + "/picked.fa", d + "/plain.fa")
    s, e = gaps[0][1]
    assert _fasta(d + "/plain.fa")["scf0"][1] == t0[:1500] + "ACGTNNACGT" + s0[e + 1:]
    # a full pick of the joined gap outranks the join
    open(d + "/picked.fa", "w").write(">0_2_31_29_NODE_1_length_99_cov_7.000000\nTTTT\n")
    put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gaps.txt", d + "/picked.fa", d + "/full.fa", d + "/joins.tsv")
    assert _fasta(d + "/full.fa")["scf0"][1] == s0[:s] + "TTTT" + s0[e + 1:]


def test_write_back_ignores_unusable_rows_and_skips_a_join_that_reaches_back(tmp_path, capsys):
    from gappadder_amd.put_gap_seq_back_to_scaffold import put_gap_seq_back_to_scaffold
    d, (s0, s1), (t0, t1), gaps = _draft(tmp_path)
    open(d + "/picked.fa", "w").write("")
    _joins_tsv(d + "/joins.tsv", [_row("0_2", gaps[0][1], 17, ok=0), _row("1_1", gaps[1][0], 17, ok=0)])
    put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gaps.txt", d + "/picked.fa", d + "/new.fa", d + "/joins.tsv")
    assert _fasta(d + "/new.fa") == {"scf0": ("scf0 first", s0), "scf1": ("scf1", s1)}
    # gap 1 joined with a resume point beyond gap 2's cut: gap 2's join would copy backwards, and is skipped
    g1, g2 = gaps[0][0], gaps[0][1]
    _joins_tsv(d + "/joins.tsv", [("0_1", 17, 1, g1[0] - 5, g2[0]), _row("0_2", g2, 17)])
    capsys.readouterr()
    put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gaps.txt", d + "/picked.fa", d + "/new.fa", d + "/joins.tsv")
    out = capsys.readouterr().out
    assert "Join of Gap  2 of Scaffold  0 reaches before the previous gap!!!" in out
    assert _fasta(d + "/new.fa")["scf0"] == ("scf0", s0[:g1[0] - 5] + s0[g2[0]:])


def test_write_back_without_the_fifth_argument_gives_todays_bytes_on_the_reference_fixture(tmp_path):
    import gzip
    from golden_util import Case
    from gappadder_amd import put_gap_seq_back_to_scaffold as PB
    case = Case("twolib")
    wb = json.loads(gzip.open(os.path.join(case.dir, "writeback.json.gz")).read())
    d = str(tmp_path)
    open(d + "/draft.fa", "w").write(case.draft_fa)
    open(d + "/draft.fa.fai", "w").write(case.fai)
    open(d + "/gap_positions.txt", "w").write(case.expected["gap_positions.txt"])
    open(d + "/picked.fa", "w").write(wb["picked_fa"])
    PB.put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gap_positions.txt", d + "/picked.fa", d + "/new.fa")
    assert open(d + "/new.fa").read() == wb["new_scaffolds_fa"]
    PB.put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gap_positions.txt", d + "/picked.fa", d + "/none.fa", None)
    assert open(d + "/none.fa").read() == wb["new_scaffolds_fa"]
    # a table without a usable row changes nothing either
    _joins_tsv(d + "/joins.tsv", [("0_2", 17, 0, 10, 200)])
    PB.put_gap_seq_back_to_scaffold(d + "/draft.fa", d + "/gap_positions.txt", d + "/picked.fa", d + "/empty.fa", d + "/joins.tsv")
    assert open(d + "/empty.fa").read() == wb["new_scaffolds_fa"]
