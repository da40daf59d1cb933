"""The CLI's `parameters.gap_span` (+ gap_span_shift, gap_span_min_pairs): the device-resident Collect of `-c All` measures every gap,
open or closed, from the pairs that span it and writes {working_folder}gap_span.tsv — one row per gap and library, in gap order then
library order, equal to the host twin on the BAM files decoded again — and every other file of the working folder is byte-identical to a
run without the key, which writes no such file; on the per-scaffold path one line on stderr and no file."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF
from test_gpu_cli_pair_span import _tree

pytestmark = pytest.mark.gpu


def test_gap_span_tsv_equals_the_twin_and_nothing_else_changes(tmp_path, monkeypatch, capfd):
    from gappadder_amd import _lib as B
    from gappadder_amd import bam_io
    from gappadder_amd import device_collect as DC
    from gappadder_amd import gap_span as GS
    from gappadder_amd import main as M
    from gappadder_amd import sam_io
    from gappadder_amd.hip_api import GapFill
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
    assert "gap_span.tsv" not in off and seen[-1][0].gap_span is None
    c = json.load(open(cfgp))
    # (15 000 pairs of 600 +/- 50 over 600 kb: pairs x (insert - gap - 2 L) / genome = 4.5 spanning pairs per 120-base gap)
    c["parameters"].update(gap_span=True, gap_span_shift=100, gap_span_min_pairs=3)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv = on.pop("gap_span.tsv").decode().splitlines()
    assert sorted(on) == sorted(off)
    diff = [p for p in on if on[p] != off[p]]
    assert not diff, diff[:5]
    # the twin on the BAM files decoded again, on a context of its own
    res, coll = seen[-1]
    pipe = coll.pipe
    assert (pipe.gap_span.z, pipe.gap_span.shift, pipe.gap_span.min_pairs) == (3, 100, 3) and res.gap_span.shape == (len(libs), len(res.best))
    names = sam_io.read_fai(c["draft_genome"]["fa"] + ".fai")
    gaps, keys = sam_io.read_gap_positions(wf + "gap_positions.txt", {n: i for i, n in enumerate(names)})
    assert list(keys) == list(res.keys) and len(gaps) == nscf * gps
    gf2 = GapFill(0)
    recs = [np.concatenate([r for r, _ in bam_io.decode_file(gf2, a["bam"], names)]) for a in c["alignments"]]
    assert [len(r) for r in recs] == [lb.n_recs for lb in pipe.libs]
    want, stats = GS.gap_span_of_results(recs, [(mu, sd) for mu, sd, _ in libs], gaps, len(names), res.read_len, 3, 100, pipe.anchor_mapq)
    print(stats)
    assert stats[1]["accepted"] > 20 and int((want[1]["n"] >= 3).sum()) >= 4
    assert want.tobytes() == res.gap_span.tobytes() and stats == res.gap_span_stats
    # the rows: per gap, in gap order, one per library
    fields = B.GAP_SPAN.names[:-1]
    assert tsv[0].split("\t") == ["library", "name", "G0"] + list(fields) + ["naive", "est", "se", "fill_len", "fill_len_minus_est"]
    rows = [r.split("\t") for r in tsv[1:]]
    assert len(rows) == len(libs) * len(gaps) and all(len(r) == len(fields) + 8 for r in rows)
    closed = set(int(g) for g in np.nonzero(res.best)[0])
    fills = pipe.picked_sequences(res)
    assert closed
    n_est = 0
    for i, row in enumerate(rows):
        g, l = i // len(libs), i % len(libs)
        rec = want[l, g]
        assert int(row[0]) == l and int(row[2]) == int(gaps[g]["end"]) - int(gaps[g]["start"]) == glen
        assert row[1].startswith(res.keys[g] + "_31_29_NODE_") if g in closed else row[1] == res.keys[g]
        assert [int(x) for x in row[3:3 + len(fields)]] == [int(rec[f]) for f in fields]
        e = GS.estimate(rec, glen, res.read_len, libs[l][0], libs[l][1], 3, 100, 3)
        if e is None:
            assert row[-5:-2] == ["", "", ""] and row[-1] == "" and int(rec["n"]) < 3
        else:
            n_est += 1
            assert row[-5:-2] == ["%.2f" % e.naive, "%.2f" % e.est, "%.2f" % e.se]
        if g in closed:
            assert int(row[-2]) == len(fills[g][1])
            assert row[-1] == ("" if e is None else "%.2f" % (len(fills[g][1]) - e.est))
        else:
            assert row[-2:] == ["", ""]
    assert n_est >= 4
    capfd.readouterr()
    # no device step, no file: one line on stderr
    os.remove(wf + "gap_span.tsv")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("gap_span:") == 1 and not os.path.exists(wf + "gap_span.tsv")
