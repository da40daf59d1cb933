"""The CLI's `parameters.fill_pairs`: the first assembly round of the device-resident Collect runs with the pair-span round on and
writes {working_folder}fill_pairs.tsv — one row per gap the device step closed and library, named as in picked_seqs.fa — and nothing
else of the working folder changes; on the per-scaffold path one line on stderr and no file."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF

pytestmark = pytest.mark.gpu


def _tree(wf):
    out = {}
    for d, _, files in os.walk(wf):
        for fn in files:
            p = os.path.join(d, fn)
            out[os.path.relpath(p, wf)] = open(p, "rb").read()
    return out


def test_fill_pairs_tsv_and_nothing_else(tmp_path, monkeypatch, capfd):
    from gappadder_amd import _lib as B
    from gappadder_amd import device_collect as DC
    from gappadder_amd import main as M
    seed, slen, nscf, gps, glen, L = 20260013, 200_000, 3, 4, 120, 150
    libs = [(300, 30, 40_000), (600, 50, 15_000)]
    cfgp, wf = SF.write_case(str(tmp_path), seed, slen, nscf, gps, glen, libs, [(31, 29)], kmer_screen=31)
    seen = []
    orig = DC.DeviceCollector.run

    def run(self, *a, **kw):
        res = orig(self, *a, **kw)
        seen.append((res, self))
        return res
    monkeypatch.setattr(DC.DeviceCollector, "run", run)
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert "fill_pairs.tsv" not in off and seen[-1][0].pairs is None
    c = json.load(open(cfgp))
    c["parameters"].update(fill_pairs=True, fill_pairs_z=2)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv = on.pop("fill_pairs.tsv").decode().splitlines()
    assert sorted(on) == sorted(off)
    diff = [p for p in on if on[p] != off[p]]
    assert not diff, diff[:5]
    # the rows are the records of the collector's own Results: per gap the device step closed, in gap order, one per library
    res, coll = seen[-1]
    fields = B.FILL_PAIRS.names
    assert coll.pipe.pairs.params == (16, 4, 48, 2) and res.pairs.shape == (len(libs), len(res.best))
    assert tsv[0].split("\t") == ["library", "name"] + list(fields) + ["span_mean_minus_is"]
    rows = [r.split("\t") for r in tsv[1:]]
    closed = np.nonzero(res.best)[0]
    assert len(rows) == len(libs) * len(closed) > 0 and all(len(r) == len(fields) + 3 for r in rows)
    assert all(s["gaps"] == len(closed) for s in res.pair_stats) and res.pair_stats[0]["placed"] > 0
    for i, row in enumerate(rows):
        g, l = int(closed[i // len(libs)]), i % len(libs)
        rec = res.pairs[l, g]
        assert int(row[0]) == l and row[1].startswith(res.keys[g] + "_31_29_NODE_")
        assert [int(x) for x in row[2:-1]] == [int(rec[f]) for f in fields]
        want = "" if not int(rec["n_span"]) else str(int(rec["span_insert_sum"]) // int(rec["n_span"]) - libs[l][0])
        assert row[-1] == want
    assert any(r[-1] != "" for r in rows) and sum(int(r[2 + fields.index("pairs_placed")]) for r in rows) > 0
    capfd.readouterr()
    # no device step, no file: one line on stderr
    os.remove(wf + "fill_pairs.tsv")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("fill_pairs:") == 1 and not os.path.exists(wf + "fill_pairs.tsv")


def test_parameters_the_read_length_excludes_make_main_exit_with_a_message(tmp_path):
    from gappadder_amd import main as M
    cfgp, wf = SF.write_case(str(tmp_path), 20260014, 100_000, 1, 2, 120, [(300, 30, 4_000)], [(31, 29)], kmer_screen=31)
    c = json.load(open(cfgp))
    c["parameters"].update(fill_pairs=True, fill_pairs_seed=32, fill_pairs_max_mismatch=4)      # reads of 150 bases have four seeds of 32
    json.dump(c, open(cfgp, "w"))
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "All", "-g", cfgp])
    assert "fill_pairs" in str(e.value)
