"""The CLI's `parameters.flank_joins` (+ flank_joins_max_overlap, flank_joins_min_context, flank_joins_max_mismatch): the device-resident
Collect of `-c All` writes {working_folder}flank_joins.tsv — one row per gap the step leaves open and joins — and every other file of the
working folder is byte-identical to a run without the key, which writes no such file; put_gap_seq_back_to_scaffold takes the table as its
fifth argument; on the per-scaffold path one line on stderr and no file.

The case: the synthetic files with the draft FASTA doctored in place (same length, same line width).  In a gap-free stretch of scaffold 0,
at p, an N-run of R bases is written over D[p : p + R), and the 400 bases before it are overwritten by the draft's own text shifted
forward by R + 10 + o: D'[p - 400 : p) = D[p - 400 + R + 10 + o : p + R + 10 + o).  The flanks of the new gap stop 5 bases short of the
run, so the left one ends o bases past the right one's first base: the flanks overlap by exactly o, and the truth the reads come from is
the undoctored draft."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF
from test_gpu_cli_pair_span import _tree

pytestmark = pytest.mark.gpu

R, O = 120, 40


def _read(path):
    """([header line], [sequence], line width) of a FASTA file."""
    heads, seqs, width = [], [], 0
    for line in open(path).read().split("\n"):
        if line.startswith(">"):
            heads.append(line)
            seqs.append([])
        elif line:
            seqs[-1].append(line)
            width = max(width, len(line))
    return heads, ["".join(s) for s in seqs], width


def _write(path, heads, seqs, width):
    with open(path, "w") as f:
        for h, s in zip(heads, seqs):
            f.write(h + "\n" + "".join(s[i:i + width] + "\n" for i in range(0, len(s), width)))


def _doctor(path):
    """Plants the overlap in scaffold 0; returns (the undoctored scaffold 0, p)."""
    from gappadder_amd.gnrt_pos_true_seqs import scan_gaps
    before = open(path, "rb").read()
    heads, seqs, width = _read(path)
    _write(path, heads, seqs, width)
    assert open(path, "rb").read() == before              # the writer reproduces the file: only the planted bases will differ
    D = seqs[0]
    gaps = scan_gaps(D, 100)
    p = (gaps[0][1] + gaps[1][0]) // 2
    assert gaps[0][1] + 2000 < p - 400 and p + R + 10 + O + 2000 < gaps[1][0] and "N" not in D[p - 1000:p + 1000]
    seqs[0] = D[:p - 400] + D[p - 400 + R + 10 + O:p + R + 10 + O] + "N" * R + D[p + R:]
    assert len(seqs[0]) == len(D)
    _write(path, heads, seqs, width)
    assert len(open(path, "rb").read()) == len(before)
    return D, p


def test_flank_joins_tsv_the_write_back_and_nothing_else(tmp_path, monkeypatch, capfd):
    from gappadder_amd import _lib as B
    from gappadder_amd import device_collect as DC
    from gappadder_amd import flank_joins as FJ
    from gappadder_amd import main as M
    from gappadder_amd import sam_io
    from gappadder_amd.put_gap_seq_back_to_scaffold import _records, put_gap_seq_back_to_scaffold
    seed, slen, nscf, gps, glen, L = 20260013, 200_000, 3, 4, 120, 150
    libs = [(300, 30, 40_000), (600, 50, 15_000)]
    cfgp, wf = SF.write_case(str(tmp_path), seed, slen, nscf, gps, glen, libs, [(31, 29)], kmer_screen=31)
    c = json.load(open(cfgp))
    draft = c["draft_genome"]["fa"]
    D, p = _doctor(draft)
    seen = []
    orig = DC.DeviceCollector.run

    def run(self, *a, **kw):
        res = orig(self, *a, **kw)
        seen.append((res, self))
        return res
    monkeypatch.setattr(DC.DeviceCollector, "run", run)
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert "flank_joins.tsv" not in off and seen[-1][0].joins is None
    c["parameters"].update(flank_joins=True, flank_joins_max_overlap=200, flank_joins_min_context=25, flank_joins_max_mismatch=1)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv = on.pop("flank_joins.tsv").decode().splitlines()
    assert sorted(on) == sorted(off)
    diff = [q for q in on if on[q] != off[q]]
    assert not diff, diff[:5]
    # the rows: the records of the run, in gap order, for the gaps with a join
    res, coll = seen[-1]
    pipe = coll.pipe
    assert pipe.joins.params == (200, 25, 1) and len(res.joins) == len(res.best) == nscf * gps + 1
    names = sam_io.read_fai(draft + ".fai")
    gaps, keys = sam_io.read_gap_positions(wf + "gap_positions.txt", {n: i for i, n in enumerate(names)})
    assert list(keys) == list(res.keys)
    planted = [g for g in range(len(gaps)) if int(gaps[g]["scaffold"]) == 0 and int(gaps[g]["start"]) == p]
    assert len(planted) == 1 and int(gaps[planted[0]]["end"]) == p + R and keys[planted[0]] == "0_2"
    want, stats = FJ.joins_of_results(pipe, res)
    print(stats, res.joins[planted[0]])
    assert want.tobytes() == res.joins.tobytes() and stats == res.join_stats
    fields = B.FLANK_JOIN.names[:-1]
    assert tsv[0].split("\t") == ["gap", "G0"] + list(fields) + ["usable", "name", "cut_from", "resume_at"]
    rows = [r.split("\t") for r in tsv[1:]]
    joined = [int(g) for g in np.nonzero(res.joins["overlap"])[0]]
    assert [r[0] for r in rows] == [keys[g] for g in joined]
    for row, g in zip(rows, joined):
        rec, start, end = res.joins[g], int(gaps[g]["start"]), int(gaps[g]["end"])
        assert int(row[1]) == end - start and [int(x) for x in row[2:2 + len(fields)]] == [int(rec[f]) for f in fields]
        assert int(row[-4]) == int(FJ.usable(rec) and start >= 5)
        assert row[-3].startswith(keys[g] + "_31_29_NODE_") and int(res.contigs[int(rec["contig"])]["gap"]) == g
        assert (int(row[-2]), int(row[-1])) == (start - 5, end + 5 + int(rec["overlap"]))
    # the planted gap: open, joined with exactly o, usable; no other gap has a row
    g = planted[0]
    assert int(res.best[g]) == 0 and joined == [g] and int(res.joins[g]["overlap"]) == O and FJ.usable(res.joins[g])
    assert (int(rows[0][-2]), int(rows[0][-1])) == (p - 5, p + R + 5 + O)
    # the write-back with the table: around the join the new scaffold is the undoctored draft (300 bases before it — the planted text is
    # 395 bases of the draft — and 200 behind), and the N-run is gone
    new = str(tmp_path / "new.fa")
    put_gap_seq_back_to_scaffold(draft, wf + "gap_positions.txt", wf + "picked_seqs.fa", new, wf + "flank_joins.tsv")
    plain = str(tmp_path / "plain.fa")
    put_gap_seq_back_to_scaffold(draft, wf + "gap_positions.txt", wf + "picked_seqs.fa", plain)
    s_new = {n: s for n, _, s in _records(new)}[names[0]]
    s_plain = {n: s for n, _, s in _records(plain)}[names[0]]
    at = s_new.find(D[p + R + 5 + O:p + R + 5 + O + 200])                    # the text behind the join, as the undoctored draft has it
    assert at >= 300 and s_new[at - 300:at + 200] == D[p + R + 5 + O - 300:p + R + 5 + O + 200]
    assert D[p + R + 5 + O - 300:p + R + 5 + O + 200] not in s_plain
    assert {n: s for n, _, s in _records(new) if n != names[0]} == {n: s for n, _, s in _records(plain) if n != names[0]}
    capfd.readouterr()
    # no device step, no file: one line on stderr
    os.remove(wf + "flank_joins.tsv")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("flank_joins:") == 1 and not os.path.exists(wf + "flank_joins.tsv")
