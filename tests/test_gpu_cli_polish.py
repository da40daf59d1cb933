"""The CLI's `parameters.fill_polish`: the first assembly round of the device-resident Collect runs with the polish round on and writes
{working_folder}polished_seqs.fa and {working_folder}fill_polish.tsv — one record / row per gap the device step closed, named as in
picked_seqs.fa — and nothing else of the working folder changes."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF

pytestmark = pytest.mark.gpu

FIELDS = ("len", "flags", "n_cols", "n_changed", "n_uncovered", "reads_placed", "reads_ambiguous")


def _tree(wf):
    out = {}
    for d, _, files in os.walk(wf):
        for fn in files:
            p = os.path.join(d, fn)
            out[os.path.relpath(p, wf)] = open(p, "rb").read()
    return out


def test_polished_seqs_fill_polish_tsv_and_nothing_else(tmp_path, monkeypatch, capfd):
    from gappadder_amd import device_collect as DC
    from gappadder_amd import main as M
    seed, slen, nscf, gps, glen, L = 20260013, 200_000, 3, 4, 120, 150
    cfgp, wf = SF.write_case(str(tmp_path), seed, slen, nscf, gps, glen, [(300, 30, 40_000)], [(31, 29)], kmer_screen=31)
    seen = []
    orig = DC.DeviceCollector.run

    def run(self, *a, **kw):
        res = orig(self, *a, **kw)
        seen.append((res, self))
        return res
    monkeypatch.setattr(DC.DeviceCollector, "run", run)
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert "polished_seqs.fa" not in off and "fill_polish.tsv" not in off and seen[-1][0].polish is None
    c = json.load(open(cfgp))
    c["parameters"].update(fill_polish=True, fill_polish_min_votes=3)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    fa, tsv = on.pop("polished_seqs.fa").decode(), on.pop("fill_polish.tsv").decode().splitlines()
    assert sorted(on) == sorted(off)
    diff = [p for p in on if on[p] != off[p]]
    assert not diff, diff[:5]
    # the rows are the records of the collector's own Results, one per gap the device step closed, in gap order
    res = seen[-1][0]
    assert tsv[0].split("\t") == ["name"] + list(FIELDS)
    rows = [r.split("\t") for r in tsv[1:]]
    closed = np.nonzero(res.best)[0]
    assert len(rows) == len(closed) > 0 and res.polish_stats["gaps"] == len(closed) and res.polish_stats["placed"] > 0
    for row, g in zip(rows, closed.tolist()):
        assert row[0].startswith(res.keys[g] + "_31_29_NODE_")
        assert [int(x) for x in row[1:]] == [int(res.polish[g][f]) for f in FIELDS]
        assert int(row[1]) > 0 and int(row[3]) > 0
    # polished_seqs.fa: the same names in the same order, lines of 60, the polished cut of every gap
    blocks = fa.split(">")[1:]
    assert [b.split("\n", 1)[0] for b in blocks] == [r[0] for r in rows]
    picked = {}
    for blk in open(wf + "picked_seqs.fa").read().split(">")[1:]:
        h, s = blk.split("\n", 1)
        picked[h.split()[0]] = s.replace("\n", "")
    same = 0
    for blk, row, g in zip(blocks, rows, closed.tolist()):
        lines = blk.split("\n")[1:]
        assert lines[-1] == "" and all(len(x) == 60 for x in lines[:-2]) and 0 < len(lines[-2]) <= 60
        seq = "".join(lines)
        assert set(seq) <= set("ACGT")
        if row[0] in picked and int(row[4]) == 0:                  # an unchanged fill is the sequence picked_seqs.fa has under that name
            assert seq == picked[row[0]]
            same += 1
    assert same > 0
    capfd.readouterr()
    # no device step, no files: one line on stderr
    os.remove(wf + "polished_seqs.fa")
    os.remove(wf + "fill_polish.tsv")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("fill_polish:") == 1 and not os.path.exists(wf + "polished_seqs.fa") and not os.path.exists(wf + "fill_polish.tsv")


def test_parameters_the_read_length_excludes_make_main_exit_with_a_message(tmp_path):
    from gappadder_amd import main as M
    cfgp, wf = SF.write_case(str(tmp_path), 20260014, 100_000, 1, 2, 120, [(300, 30, 4_000)], [(31, 29)], kmer_screen=31)
    c = json.load(open(cfgp))
    c["parameters"].update(fill_polish=True, fill_polish_seed=32, fill_polish_max_mismatch=4)      # reads of 150 bases have four seeds of 32
    json.dump(c, open(cfgp, "w"))
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "All", "-g", cfgp])
    assert "fill_polish" in str(e.value)
