"""The CLI's `parameters.recruit_rounds`: the assembly stage repeats the second round's recruitment of both-unmapped pairs on the gaps
still open, each round with the contigs the round before built, appending only the pairs a gap does not have yet.  A small file set with
1 400 bp gaps, which one library of 300 bp inserts cannot close in one recruitment round: recruit_rounds 1 leaves the working folder
byte-identical to a run without the key; recruit_rounds 4 closes more gaps.  Measured on the GPU: 0 of 12 gaps closed with one round (all
twelve get partial fills), 12 of 12 with up to four, of which three ran (the third appended nothing)."""
import json
import os

import pytest

import synth_files_util as SF
from test_gpu_cli_pair_span import _tree

pytestmark = pytest.mark.gpu


def _heads(wf):
    """Headers of the full fills of picked_seqs.fa (the partial, 'NN'-joined ones carry _extended)."""
    heads = [blk.split("\n", 1)[0].split()[0] for blk in open(wf + "picked_seqs.fa").read().split(">")[1:]]
    return [h for h in heads if not h.endswith("_extended")]


def _names(path):
    return [ln[1:].strip() for ln in open(path).read().split("\n")[0::4] if ln]


def test_recruit_rounds_in_the_cli(tmp_path, capfd, monkeypatch):
    from gappadder_amd import collect_both_unmapped_reads as CB
    from gappadder_amd import main as M
    rounds = []                  # what every recruitment round of a run appended: {gap: names}
    orig = CB.BothUnmappedReadsCollector.align_unmapped_to_contigs

    def align(self, fa_list):
        out = orig(self, fa_list)
        rounds.append(out)
        return out
    monkeypatch.setattr(CB.BothUnmappedReadsCollector, "align_unmapped_to_contigs", align)
    seed, slen, nscf, gps, glen = 20260021, 200_000, 3, 4, 1400
    cfgp, wf = SF.write_case(str(tmp_path), seed, slen, nscf, gps, glen, [(300, 30, 60_000)], [(31, 29)], kmer_screen=31)
    c = json.load(open(cfgp))
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert " (1 recruitment rounds run)" in capfd.readouterr().out
    c["parameters"]["recruit_rounds"] = 1
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    one = _tree(wf)
    assert sorted(one) == sorted(off) and not [q for q in one if one[q] != off[q]]
    closed1 = _heads(wf)
    first = {fn: _names(wf + "merged/unmapped_reads/" + fn) for fn in os.listdir(wf + "merged/unmapped_reads")}
    assert first
    capfd.readouterr()
    assert len(rounds) == 2 and all(rounds), "one recruitment round per run so far, and it recruits"
    del rounds[:]
    c["parameters"]["recruit_rounds"] = 4
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])
    out = capfd.readouterr().out
    closed4 = _heads(wf)
    print("closed with 1 round: %d, with up to 4: %d of %d" % (len(closed1), len(closed4), nscf * gps))
    assert len(closed4) > len(closed1)
    # the gaps' recruits: they hold what the first round alone recruited, some gap got more; every recruit of every round went into the
    # gap's read file — which the rounds append to — exactly once
    more = 0
    for fn in os.listdir(wf + "merged/unmapped_reads"):
        names = _names(wf + "merged/unmapped_reads/" + fn)
        assert len(names) == len(set(names)), fn
        assert set(first.get(fn, ())) <= set(names), fn
        more += len(names) > len(first.get(fn, ()))
        key = fn[:-len(".fastq")]
        assert sorted(names) == sorted(n for r in rounds for n in r.get(key, ())), fn
        pool = _names(wf + "merged/gap_reads/" + fn)
        count = {}
        for n in pool:
            count[n] = count.get(n, 0) + 1
        assert all(count.get(n, 0) == 1 for n in names), (fn, [n for n in names if count.get(n, 0) != 1][:5])
    assert more > 0
    # the rounds end behind the first that appended nothing: the third here, below the cap of four
    run = int(out.split(" recruitment rounds run)")[0].rsplit("(", 1)[1])
    print("recruitment rounds run:", run, "gaps that got reads per round:", [len(r) for r in rounds])
    assert run == len(rounds) == [bool(r) for r in rounds].index(False) + 1
    assert run == 3 < 4
