"""The CLI's `parameters.fill_adjudication` (+ _seed, _max_mismatch, _min_overlap, _context, _min_votes, _ratio; only with
fill_alternatives): the device-resident Collect of `-c All` writes {working_folder}fill_adjudication.tsv — one row per contested gap —
and {working_folder}adjudicated_seqs.fa — every closed gap's sequence under its picked name, the rival's where the verdict is switch —,
both consistent with the step's records, and every other file of the working folder is byte-identical to the run with
fill_alternatives alone, which writes neither; on the per-scaffold path one line on stderr and no file.  The small file set of the
other CLI tests, at two (k, kv) pairs."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF
from test_gpu_cli_pair_span import _tree

pytestmark = pytest.mark.gpu


def test_fill_adjudication_files_and_nothing_else(tmp_path, monkeypatch, capfd):
    from gappadder_amd import _lib as B
    from gappadder_amd import device_collect as DC
    from gappadder_amd import fill_adjudication as ADJ
    from gappadder_amd import fill_alternatives as FA
    from gappadder_amd import main as M
    seed, slen, nscf, gps, glen = 20260013, 200_000, 3, 4, 120
    libs = [(300, 30, 40_000), (600, 50, 15_000)]
    kmers = [(31, 29), (41, 39)]
    cfgp, wf = SF.write_case(str(tmp_path), seed, slen, nscf, gps, glen, libs, kmers, kmer_screen=31)
    c = json.load(open(cfgp))
    seen = []
    orig = DC.DeviceCollector.run

    def run(self, *a, **kw):
        res = orig(self, *a, **kw)
        seen.append((res, self))
        return res
    monkeypatch.setattr(DC.DeviceCollector, "run", run)
    c["parameters"].update(fill_alternatives=True)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert "fill_adjudication.tsv" not in off and "adjudicated_seqs.fa" not in off and seen[-1][0].adjudication is None
    c["parameters"].update(fill_adjudication=True, fill_adjudication_min_votes=1, fill_adjudication_context=120)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv = on.pop("fill_adjudication.tsv").decode().splitlines()
    fa = on.pop("adjudicated_seqs.fa").decode()
    assert sorted(on) == sorted(off)
    if seen[-1][0].contigs.tobytes() != seen[-2][0].contigs.tobytes():
        # The device lists its contigs in another order from run to run.  fill_alternatives.tsv's `contig` and `rival` columns are indices
        # into that list, and among differing peers of one span the earlier contig is the rival, so the rival's columns follow the order
        # too (two runs with fill_alternatives alone differ the same way).  What does not depend on the order must be equal cell for cell;
        # and the table must be exactly what the alternatives' twin gives on THIS run's list: the adjudication changed nothing of it.
        keep = ("gap", "fill_len", "len_min", "len_max", "n_candidates", "n_lower", "n_identical", "n_near", "n_far", "level", "contested", "name")

        def order_free(raw):
            rows = [l.split("\t") for l in raw.decode().splitlines()]
            return [[r[rows[0].index(k)] for k in keep] for r in rows]
        a, b = order_free(on["fill_alternatives.tsv"]), order_free(off["fill_alternatives.tsv"])
        print("contig lists differ between the runs; fill_alternatives.tsv equal:", on["fill_alternatives.tsv"] == off["fill_alternatives.tsv"])
        assert a == b, [(x, y) for x, y in zip(a, b) if x != y][:3]
        res_on, pipe_on = seen[-1][0], seen[-1][1].pipe
        want = FA.alts_of_results(pipe_on, res_on)
        assert want[0].tobytes() == res_on.alts.tobytes() and want[1].tobytes() == res_on.alt_contigs.tobytes() and want[2] == res_on.alt_stats
        assert DC.fill_alternatives_files(pipe_on, res_on, kmers)[0].encode() == on["fill_alternatives.tsv"]
        on["fill_alternatives.tsv"] = off["fill_alternatives.tsv"]           # (alt_seqs.fa, like every other file, stays byte for byte)
    diff = [q for q in on if on[q] != off[q]]
    assert not diff, diff[:5]
    res, coll = seen[-1]
    pipe = coll.pipe
    assert pipe.adj.params == (16, 4, 48, 120, 1, 2) and len(res.adjudication) == len(res.best) == nscf * gps
    print(res.adj_stats)
    assert res.adj_stats["mismatches"] == 0 and res.adj_stats["contested"] == res.alt_stats["contested"]
    # the rows: in gap order, the contested gaps, the record's fields and the verdict as a word
    assert tsv[0].split("\t") == ["name"] + list(DC.ADJ_FIELDS) + ["verdict_word"]
    rows = [r.split("\t") for r in tsv[1:]]
    listed = [g for g in range(len(res.alts)) if FA.contested(res.alts[g])]
    picked = DC.picked_names(res, kmers)
    assert [r[0] for r in rows] == [picked[g] for g in listed]
    for row, g in zip(rows, listed):
        rec = res.adjudication[g]
        assert [int(x) for x in row[1:-1]] == [int(rec[f]) for f in DC.ADJ_FIELDS] and row[-1] == ADJ.VERDICTS[int(rec["verdict"])]
    # the sequences: picked_seqs' records of the step, the rival's text at the SWITCH gaps
    seqs, first, rivals = pipe.adjudicated_sequences(res), pipe.picked_sequences(res), pipe.alternative_sequences(res)
    recs = [r.split("\n") for r in fa.split(">")[1:]]
    closed = [int(g) for g in np.nonzero(res.best)[0]]
    assert [r[0] for r in recs] == [picked[g] for g in closed] and ["".join(r[1:]) for r in recs] == [seqs[g][0] for g in closed]
    for g in closed:
        switch = int(res.adjudication[g]["verdict"]) == B.AJ_SWITCH
        assert seqs[g] == ((rivals[g][1], "rival") if switch else (first[g][1], "picked"))
    capfd.readouterr()
    # no device step, no file: one line on stderr
    os.remove(wf + "fill_adjudication.tsv")
    os.remove(wf + "adjudicated_seqs.fa")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("fill_adjudication:") == 1 and not os.path.exists(wf + "fill_adjudication.tsv") and not os.path.exists(wf + "adjudicated_seqs.fa")
