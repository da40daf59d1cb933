"""The CLI's `parameters.fill_polish_indels`: with it on, fill_polish.tsv has the six event columns and polished_seqs.fa carries the
indel-aware result; with it off — absent or false — both files are what `fill_polish` alone writes, compared here by running the
settings one after the other; nothing else of the working folder changes either way."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF

pytestmark = pytest.mark.gpu

FIELDS = ("len", "flags", "n_cols", "n_changed", "n_uncovered", "reads_placed", "reads_ambiguous")
MORE = ("n_events", "n_inserted", "n_deleted", "reads_split", "events_seen", "events_outside")


def _tree(wf):
    out = {}
    for d, _, files in os.walk(wf):
        for fn in files:
            p = os.path.join(d, fn)
            out[os.path.relpath(p, wf)] = open(p, "rb").read()
    return out


def test_the_extended_tsv_the_fasta_and_the_option_off(tmp_path, monkeypatch):
    from gappadder_amd import _lib as B
    from gappadder_amd import device_collect as DC
    from gappadder_amd import main as M
    cfgp, wf = SF.write_case(str(tmp_path), 20260013, 200_000, 3, 4, 120, [(300, 30, 40_000)], [(31, 29)], kmer_screen=31)
    seen = []
    orig = DC.DeviceCollector.run

    def run(self, *a, **kw):
        res = orig(self, *a, **kw)
        seen.append((res, self))
        return res
    monkeypatch.setattr(DC.DeviceCollector, "run", run)
    trees = {}
    for name, params in (("plain", dict(fill_polish=True)), ("off", dict(fill_polish=True, fill_polish_indels=False, fill_polish_max_indel=3)),
                         ("on", dict(fill_polish=True, fill_polish_indels=True))):
        c = json.load(open(cfgp))
        c["parameters"] = dict({k: v for k, v in c["parameters"].items() if not k.startswith("fill_polish")}, **params)
        json.dump(c, open(cfgp, "w"))
        M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
        trees[name] = _tree(wf)
    assert trees["plain"] == trees["off"]               # every file, byte for byte
    on, plain = dict(trees["on"]), dict(trees["plain"])
    fa, tsv = on.pop("polished_seqs.fa").decode(), on.pop("fill_polish.tsv").decode().splitlines()
    plain_fa, plain_tsv = plain.pop("polished_seqs.fa").decode(), plain.pop("fill_polish.tsv").decode().splitlines()
    assert on == plain
    res = seen[-1][0]
    assert res.polish.dtype == B.FILL_POLISH_GAPPED and seen[0][0].polish.dtype == seen[1][0].polish.dtype == B.FILL_POLISH
    assert tsv[0].split("\t") == ["name"] + list(FIELDS + MORE) and plain_tsv[0].split("\t") == ["name"] + list(FIELDS)
    rows = [r.split("\t") for r in tsv[1:]]
    closed = np.nonzero(res.best)[0]
    assert len(rows) == len(closed) > 0 and res.polish_stats["gaps"] == len(closed) and res.polish_stats["placed"] > 0
    for row, g in zip(rows, closed.tolist()):
        assert row[0].startswith(res.keys[g] + "_31_29_NODE_")
        assert [int(x) for x in row[1:]] == [int(res.polish[g][f]) for f in FIELDS + MORE]
    # polished_seqs.fa: the same names in the same order, lines of 60; a gap without a split row has the plain polish's sequence, and a
    # sequence differs in length from the plain one by what the gap's events insert and delete
    blocks, plain_blocks = fa.split(">")[1:], plain_fa.split(">")[1:]
    assert [b.split("\n", 1)[0] for b in blocks] == [r[0] for r in rows] == [b.split("\n", 1)[0] for b in plain_blocks]
    for blk, pblk, row, g in zip(blocks, plain_blocks, rows, closed.tolist()):
        lines = blk.split("\n")[1:]
        assert lines[-1] == "" and all(len(x) == 60 for x in lines[:-2]) and 0 < len(lines[-2]) <= 60
        seq, pseq = "".join(lines), "".join(pblk.split("\n")[1:])
        assert set(seq) <= set("ACGT") and len(seq) - len(pseq) == int(res.polish[g]["n_inserted"]) - int(res.polish[g]["n_deleted"])
        if int(res.polish[g]["reads_split"]) == 0:
            assert seq == pseq
