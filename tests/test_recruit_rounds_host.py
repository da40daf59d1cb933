"""Recruitment rounds of the CLI (parameters.recruit_rounds) without a GPU: the key's validation, the assembly stage's round
bookkeeping, the collector's appending of new records only, and the host restatement of the rounds (tests/recruit_floor.py) on the
synthetic step with 1 400 bp gaps: what repeating the round is worth where one round closes nothing."""
import os

import pytest

from test_pair_span_config_host import _config


def test_cli_key_default_range_and_error_text(tmp_path):
    from gappadder_amd import main as M
    assert M.parse_configuration(_config(tmp_path))["recruit_rounds"] == 1
    for v in (1, 4, 16):
        assert M.parse_configuration(_config(tmp_path, recruit_rounds=v))["recruit_rounds"] == v
    for v in (0, 17, "2", 2.5, True):
        cfgp = _config(tmp_path, recruit_rounds=v)
        with pytest.raises(SystemExit) as e:
            M.parse_configuration(cfgp)
        assert str(e.value) == "parameters.recruit_rounds must be an integer in 1..16, not %r" % (v,)
        with pytest.raises(SystemExit) as e:
            M.main(["-c", "Collect", "-g", cfgp])
        assert "recruit_rounds" in str(e.value)


def test_cli_rounds_stop_at_the_first_that_appends_nothing(tmp_path, monkeypatch):
    """recruit_rounds_run counts the rounds up to and including the first that appended no read to any gap; a further round assembles
    only the gaps that got reads (the recruitment, the assembly and the picks are stand-ins here)."""
    from gappadder_amd import assemble_gaps as AG
    from gappadder_amd import collect_both_unmapped_reads as CB
    from gappadder_amd import pick_contigs as PC
    script = [{"a": ["r1_1"]}, {"a": ["r2_1"]}, {}, {"a": ["never"]}]
    calls, assembled = [], []

    class Burc:
        def __init__(self, *a, **kw):
            pass

        def collect_both_unmapped_reads(self, bams, ids):
            calls.append(list(ids))
            return script[len(calls) - 1]

        def align_unmapped_to_contigs(self, ids):
            calls.append(list(ids))
            return script[len(calls) - 1]

    class CS:
        def __init__(self, *a, **kw):
            pass

        def pick_full_constructed_contigs(self, *a):
            return 0

        def pick_extended_contigs(self, *a):
            return 0

        def get_already_picked(self, sf):
            return set()
    monkeypatch.setattr(CB, "BothUnmappedReadsCollector", Burc)
    monkeypatch.setattr(PC, "ContigsSelection", CS)
    for name in ("_gf", "working_folder", "kmer_len_list"):      # (the constructor sets the module's globals: put back afterwards)
        monkeypatch.setattr(AG, name, getattr(AG, name))
    for n, want in ((1, 1), (2, 2), (4, 3), (16, 3)):
        del calls[:], assembled[:]
        ga = AG.GapAssembler("x.fai", "x.pos", 1, str(tmp_path) + "/", [(31, 29)], gf=object(), bam_list=["x.bam"], samtools_path="builtin",
                             recruit_rounds=n)
        monkeypatch.setattr(ga, "prepare_list", lambda: ["a", "b"])
        monkeypatch.setattr(ga, "assembly", lambda ids: assembled.append(list(ids)))
        monkeypatch.setattr(ga, "assembly_given_list", lambda ids: assembled.append(list(ids)))
        monkeypatch.setattr(ga, "run_contigs_merge", lambda ids: {})
        monkeypatch.setattr(ga, "collect_high_quality_unmap_to_contigs_reads", lambda ids: 0)
        res = ga.assemble_pipeline()
        assert res["recruit_rounds_run"] == want == len(calls), (n, res, calls)
        assert assembled == [["a", "b"], ["a", "b"]] + [["a"]] * (min(n, 2) - 1), (n, assembled)


def test_collector_appends_only_new_records_and_lists_all(tmp_path, monkeypatch):
    from gappadder_amd import collect_both_unmapped_reads as CB
    wf = str(tmp_path) + "/"
    os.makedirs(wf + "gap_reads")
    os.makedirs(wf + "velvet_temp/g1")
    open(wf + "velvet_temp/g1/contigs.fa", "w").write(">c1\nACGT\n")
    open(wf + "gap_reads/g1.fastq", "w").write("@x\nA\n+\nI\n")
    b = CB.BothUnmappedReadsCollector(wf, "builtin", gf=object(), k=31)
    b.reads = {"p%d_%d" % (p, m): "ACGT\n+\nIIII\n" for p in range(4) for m in (1, 2)}
    names = list(b.reads)
    answers = [[[2, 3]], [[0, 1, 2, 3]], [[0, 1, 2, 3]]]
    monkeypatch.setattr(CB, "kmer_recruit_unmapped", lambda *a, **kw: answers.pop(0))
    rec = lambda ids: "".join("@" + names[i] + "\nACGT\n+\nIIII\n" for i in ids)
    assert b.align_unmapped_to_contigs(["g1"]) == {"g1": [names[2], names[3]]}
    assert open(wf + "unmapped_reads/g1.fastq").read() == rec([2, 3])
    assert b.align_unmapped_to_contigs(["g1"]) == {"g1": [names[0], names[1]]}
    assert open(wf + "unmapped_reads/g1.fastq").read() == rec([0, 1, 2, 3])
    assert open(wf + "gap_reads/g1.fastq").read() == "@x\nA\n+\nI\n" + rec([2, 3]) + rec([0, 1])
    assert b.align_unmapped_to_contigs(["g1"]) == {}
    assert open(wf + "gap_reads/g1.fastq").read() == "@x\nA\n+\nI\n" + rec([2, 3]) + rec([0, 1])


def test_cpu_floor_1400_k31():
    """The host restatement on 24 gaps of 1 400 bp at (31, 29).  Measured here: closed 0 after the first pick, then 0 / 22 / 24 after
    recruitment rounds 1 / 2 / 3, and round 4 recruits nothing."""
    import __graft_entry__ as G
    G.build()
    import recruit_floor as RF
    closed, fresh = RF.rounds(1400, [(31, 29)], 6)
    print("closed after the first pick and every round:", closed, "pairs new per round:", fresh)
    assert closed[0] == 0, "the first pick closes none"
    assert closed[1] == 0, "one recruitment round (today's second round) closes none"
    assert 24 in closed[:5], "all 24 closed after at most 4 rounds"
    done = closed.index(24)
    assert done <= 4 and fresh[done] == 0 and len(fresh) == done + 1, "the first round after that recruits nothing"
