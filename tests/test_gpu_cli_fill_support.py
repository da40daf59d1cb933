"""The CLI's `parameters.fill_support`: the first assembly round of the device-resident Collect runs with the read-support round on and
writes {working_folder}fill_support.tsv — one row per gap the device step closed, named as in picked_seqs.fa — and nothing else of the
working folder changes."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF

pytestmark = pytest.mark.gpu

FIELDS = ("n_windows", "n_zero", "n_below", "min", "max", "zero_run", "sum")


def _tree(wf):
    out = {}
    for d, _, files in os.walk(wf):
        for fn in files:
            p = os.path.join(d, fn)
            out[os.path.relpath(p, wf)] = open(p, "rb").read()
    return out


def _fasta(path):
    out = {}
    for blk in open(path).read().split(">")[1:]:
        h, s = blk.split("\n", 1)
        out[h.split()[0]] = s.replace("\n", "")
    return out


def test_fill_support_tsv_and_nothing_else(tmp_path, monkeypatch, capfd):
    from gappadder_amd import device_collect as DC
    from gappadder_amd import main as M
    from gappadder_amd import read_support as RS
    from gappadder_amd.pick_contigs import revcomp
    seed, slen, nscf, gps, glen, L = 20260013, 200_000, 3, 4, 120, 150
    cfgp, wf = SF.write_case(str(tmp_path), seed, slen, nscf, gps, glen, [(300, 30, 40_000)], [(31, 29)], kmer_screen=31)
    seen = []
    orig = DC.DeviceCollector.run

    def run(self, *a, **kw):
        res = orig(self, *a, **kw)
        seen.append(res)
        return res
    monkeypatch.setattr(DC.DeviceCollector, "run", run)
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert "fill_support.tsv" not in off and seen[-1].support is None
    c = json.load(open(cfgp))
    c["parameters"]["fill_support"] = True
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv = on.pop("fill_support.tsv").decode().splitlines()
    assert sorted(on) == sorted(off)
    diff = [p for p in on if on[p] != off[p]]
    assert not diff, diff[:5]
    # the rows are the records of the collector's own Results, one per gap the device step closed
    res = seen[-1]
    assert tsv[0].split("\t") == ["name"] + list(FIELDS)
    rows = [r.split("\t") for r in tsv[1:]]
    closed = np.nonzero(res.best)[0]
    assert len(rows) == len(closed) > 0 and res.support_stats["gaps"] == len(closed) and res.support_stats["k"] == 31
    for row, g in zip(rows, closed.tolist()):
        assert row[0].startswith(res.keys[g] + "_31_29_NODE_")
        assert [int(x) for x in row[1:]] == [int(res.support[g][f]) for f in FIELDS]
        assert int(row[1]) > 0
    # every row's name, whole: the record of that name in the gap's own contigs file (as the assembly stage wrote it from the step's
    # contigs) holds the bases of the contig the step's pick word names; some of the rows are headers of picked_seqs.fa as they stand
    from gappadder_amd import pipeline as P
    picked = _fasta(wf + "picked_seqs.fa")
    for row, g in zip(rows, closed.tolist()):
        key, written = res.keys[g], {}
        for fn in ("contigs.fa", "original_contigs_before_merging.fa"):      # (the merge round rewrites contigs.fa and keeps the assembly's
            if os.path.exists(wf + "merged/velvet_temp/%s/%s" % (key, fn)):   # own records beside it)
                written.update(_fasta(wf + "merged/velvet_temp/%s/%s" % (key, fn)))
        assert written.get(row[0][len(key) + 1:]) == P.contig_text(res, P.decode_best(res.best[g])[2]), row[0]
    in_picked = sum(row[0] in picked for row in rows)
    assert in_picked > 0
    # one gap against the twin, from the files alone: its per-gap FASTQ, the contig of contigs.fa that the row names, its flanks
    checked = 0
    for row, g in zip(rows, closed.tolist()):
        key = res.keys[g]
        if row[0] not in picked:
            continue
        # (the merge round rewrites contigs.fa and keeps the assembly's own records beside it)
        d, contig = wf + "merged/velvet_temp/%s/" % key, None
        for fn in ("original_contigs_before_merging.fa", "contigs.fa"):
            if contig is None and os.path.exists(d + fn):
                contig = _fasta(d + fn).get(row[0][len(key) + 1:])
        if contig is None:
            continue
        fl = _fasta(wf + "flank_regions/%s.fa" % key)
        body = None
        for a in (30, 15):
            for rev in (False, True):
                body = body or RS.locate_exact(contig, fl[key + "_left"], fl[key + "_right"], a, rev)
        assert body is not None
        fill = contig[body[0]:body[1]]
        assert fill in picked[row[0]] or revcomp(fill) in picked[row[0]]
        lines = open(wf + "merged/gap_reads/%s.fastq" % key).read().splitlines()
        reads = [s for s in lines[1::4]]
        assert reads and all(len(s) == L for s in reads)
        want = RS.support_host(reads, contig, body[0], body[1], 31, 2)
        assert [int(x) for x in row[1:]] == [int(want[f]) for f in FIELDS], (key, row, want)
        checked += 1
        break
    assert checked == 1
    capfd.readouterr()
    # no device step, no file: one line on stderr
    os.remove(wf + "fill_support.tsv")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("fill_support:") == 1 and not os.path.exists(wf + "fill_support.tsv")
