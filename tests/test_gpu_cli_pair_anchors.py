"""The CLI's `parameters.fill_pairs_anchored`: the first assembly round of the device-resident Collect runs the anchored pair span behind
the pair-span round and writes {working_folder}fill_pairs_anchored.tsv — one row per gap the device step closed and library, named as in
picked_seqs.fa, equal to the host twin on the step the collector left on the device — and every other file of the working folder,
fill_pairs.tsv included, is byte-identical to a run without the option; on the per-scaffold path one line on stderr and no file."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF
from test_gpu_cli_pair_span import _tree

pytestmark = pytest.mark.gpu


def test_fill_pairs_anchored_tsv_equals_the_twin_and_nothing_else_changes(tmp_path, monkeypatch, capfd):
    from gappadder_amd import _lib as B
    from gappadder_amd import device_collect as DC
    from gappadder_amd import main as M
    from gappadder_amd import pair_anchors as PA
    from gappadder_amd import sam_io
    from gappadder_amd.kmer_recruit import flank_table
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
    c = json.load(open(cfgp))
    c["parameters"].update(fill_pairs=True, fill_pairs_z=2)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    assert "fill_pairs.tsv" in off and "fill_pairs_anchored.tsv" not in off and seen[-1][0].pair_anchors is None
    c["parameters"].update(fill_pairs_anchored=True, fill_pairs_min_pairs=1)       # (a 120-base gap anchors one or two in-range pairs here)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv = on.pop("fill_pairs_anchored.tsv").decode().splitlines()
    assert sorted(on) == sorted(off)
    diff = [p for p in on if on[p] != off[p]]
    assert not diff, diff[:5]
    # the twin on the step the collector left on the device
    res, coll = seen[-1]
    pipe = coll.pipe
    assert pipe.anchored.min_pairs == 1 and pipe.pairs.params == (16, 4, 48, 2) and res.pair_anchors.shape == (len(libs), len(res.best))
    full = pipe.fetch(pools=True)
    assert full.pair_anchors.tobytes() == res.pair_anchors.tobytes()
    names = sam_io.read_fai(c["draft_genome"]["fa"] + ".fai")
    gaps, keys = sam_io.read_gap_positions(wf + "gap_positions.txt", {n: i for i, n in enumerate(names)})
    assert list(keys) == list(res.keys)
    nmw = (res.read_len + 31) // 32
    recs = [np.frombuffer(lb.d_recs.cpu().numpy().tobytes(), dtype=B.ALNREC)[:lb.n_recs] for lb in pipe.libs]
    masks = [None if lb.d_nmask is None else lb.d_nmask.cpu().numpy().view(np.uint32).reshape(-1, nmw)[ids.astype(np.int64)]
             for lb, ids in zip(pipe.libs, full.lib_pool_ids)]
    want, stats = PA.anchors_of_results(full, flank_table(wf, keys), res.read_len, [(lb.is_mean, lb.is_sd) for lb in pipe.libs], gaps, recs,
                                        z=2, min_pairs=1, nmasks=masks)
    assert ((want["n_in_range"] > 0) & (want["n_eval"] > 0)).any() and stats[0]["kept"] > 0
    assert want.tobytes() == res.pair_anchors.tobytes() and stats == res.pair_anchor_stats
    # the rows: per gap the device step closed, in gap order, one per library
    fields = B.FILL_ANCHORS.names
    assert tsv[0].split("\t") == ["library", "name"] + list(fields) + ["dev_min_mean", "dev_max_mean"]
    rows = [r.split("\t") for r in tsv[1:]]
    closed = np.nonzero(res.best)[0]
    assert len(rows) == len(libs) * len(closed) > 0 and all(len(r) == len(fields) + 4 for r in rows)
    for i, row in enumerate(rows):
        g, l = int(closed[i // len(libs)]), i % len(libs)
        rec = want[l, g]
        assert int(row[0]) == l and row[1].startswith(res.keys[g] + "_31_29_NODE_")
        assert [int(x) for x in row[2:-2]] == [int(rec[f]) for f in fields]
        if int(rec["n_eval"]):
            assert [int(x) for x in row[-2:]] == [int(rec["dev_min_sum"]) // int(rec["dev_min_n"]), int(rec["dev_max_sum"]) // int(rec["dev_max_n"])]
        else:
            assert row[-2:] == ["", ""]
    assert any(r[-1] != "" for r in rows)
    capfd.readouterr()
    # no device step, no file: one line on stderr
    os.remove(wf + "fill_pairs_anchored.tsv")
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("fill_pairs_anchored:") == 1 and not os.path.exists(wf + "fill_pairs_anchored.tsv")
