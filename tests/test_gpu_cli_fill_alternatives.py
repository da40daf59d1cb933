"""The CLI's `parameters.fill_alternatives` (+ fill_alternatives_max_dist): the device-resident Collect of `-c All` writes
{working_folder}fill_alternatives.tsv — one row per closed gap with more than one candidate — and {working_folder}alt_seqs.fa — the
rival's gap sequence of every contested gap —, both consistent with the step's records, and every other file of the working folder is
byte-identical to a run without the key, which writes neither; on the per-scaffold path one line on stderr and no file.  The small file
set of the other CLI tests, at two (k, kv) pairs so that the closed gaps have more than one candidate."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF
from test_gpu_cli_pair_span import _tree

pytestmark = pytest.mark.gpu


def test_fill_alternatives_files_and_nothing_else(tmp_path, monkeypatch, capfd):
    from gappadder_amd import device_collect as DC
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
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert "fill_alternatives.tsv" not in off and "alt_seqs.fa" not in off and seen[-1][0].alts is None
    c["parameters"].update(fill_alternatives=True, fill_alternatives_max_dist=12)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv = on.pop("fill_alternatives.tsv").decode().splitlines()
    fa = on.pop("alt_seqs.fa").decode()
    assert sorted(on) == sorted(off)
    diff = [q for q in on if on[q] != off[q]]
    assert not diff, diff[:5]
    # the records of the run equal the twin
    res, coll = seen[-1]
    pipe = coll.pipe
    assert pipe.alts.max_dist == 12 and len(res.alts) == len(res.best) == nscf * gps
    want, per, stats = FA.alts_of_results(pipe, res)
    print(stats)
    assert want.tobytes() == res.alts.tobytes() and per.tobytes() == res.alt_contigs.tobytes() and stats == res.alt_stats and not stats["lost"]
    # the rows: in gap order, the closed gaps with more than one candidate
    assert tsv[0].split("\t") == ["gap"] + list(DC.ALT_FIELDS) + ["contested", "name", "rival_name"]
    rows = [r.split("\t") for r in tsv[1:]]
    listed = [int(g) for g in np.nonzero(res.alts["n_candidates"] > 1)[0]]
    assert len(listed) >= 1 and [r[0] for r in rows] == [res.keys[g] for g in listed]
    picked = DC.picked_names(res, kmers)
    heads = set(blk.split("\n", 1)[0].split()[0] for blk in open(wf + "picked_seqs.fa").read().split(">")[1:])
    for row, g in zip(rows, listed):
        rec = res.alts[g]
        assert [int(x) for x in row[1:1 + len(DC.ALT_FIELDS)]] == [int(rec[f]) for f in DC.ALT_FIELDS]
        assert int(row[-3]) == int(FA.contested(rec)) and row[-2] == picked[g]
        assert (row[-1] != "") == FA.contested(rec) and (not row[-1] or row[-1].startswith(res.keys[g] + "_"))
    # (the merge round of the assembly stage may pick another contig for a gap: some of the names are headers of picked_seqs.fa as they stand)
    assert sum(1 for row in rows if row[-2] in heads) > 0
    # the sequences: one record per contested gap, the step's rival sequence under the picked name + _alt
    seqs = pipe.alternative_sequences(res)
    recs = [r.split("\n") for r in fa.split(">")[1:]]
    assert [r[0] for r in recs] == [picked[g] + "_alt" for g in sorted(seqs)] and len(recs) == stats["contested"]
    assert ["".join(r[1:]) for r in recs] == [seqs[g][1] for g in sorted(seqs)]
    capfd.readouterr()
    # no device step, no file: one line on stderr
    os.remove(wf + "fill_alternatives.tsv")
    os.remove(wf + "alt_seqs.fa")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("fill_alternatives:") == 1 and not os.path.exists(wf + "fill_alternatives.tsv") and not os.path.exists(wf + "alt_seqs.fa")
