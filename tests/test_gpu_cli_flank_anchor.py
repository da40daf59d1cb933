"""The CLI's `parameters.flank_anchor`: with "align" the picker aligns the whole flanks, so gaps whose draft carries one wrong base
6-15 bases from the gap edge are closed with their true sequences; without the key (exact anchors) those gaps stay open."""
import json
import os

import numpy as np
import pytest

import synth_files_util as SF

pytestmark = pytest.mark.gpu


def _full_picks(path):
    out = {}
    for blk in open(path).read().split(">")[1:]:
        h, s = blk.split("\n", 1)
        if not h.endswith("_extended"):
            out["_".join(h.split("_")[:2])] = s.replace("\n", "")
    return out


def _run(tmp, mode):
    from gappadder_amd import main as M
    from gappadder_amd.hip_api import GapFill
    seed, slen, nscf, gps, glen, L = 20260013, 200_000, 3, 4, 120, 150
    cfgp, wf = SF.write_case(str(tmp), seed, slen, nscf, gps, glen, [(300, 30, 40_000)], [(31, 29)], kmer_screen=31)
    cfg0 = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L)
    gaps, _ = GapFill.synth_layout(cfg0)
    # one wrong draft base 6-15 bases from the edge of every other gap (left edge, then right edge)
    draft = json.load(open(cfgp))["draft_genome"]["fa"]
    recs, name = [], None
    for line in open(draft).read().splitlines():
        if line.startswith(">"):
            recs.append([line, []])
        elif line:
            recs[-1][1].append(line)
    seqs = [list("".join(r[1])) for r in recs]
    mutated = []
    for s, seq in enumerate(seqs):
        txt = "".join(seq)
        starts = [i for i in range(1, len(txt)) if txt[i] == "N" and txt[i - 1] != "N"]
        ends = [i for i in range(1, len(txt)) if txt[i] != "N" and txt[i - 1] == "N"]
        for j, (a, b) in enumerate(zip(starts, ends)):
            if j % 2:
                continue
            p = a - (6 + (s + j) % 10) if (s + j // 2) % 2 == 0 else b - 1 + (6 + (s + j) % 10)
            seq[p] = "A" if seq[p] != "A" else "C"
            mutated.append((s, a, b))
    with open(draft, "w") as f:
        for (hdr, _), seq in zip(recs, seqs):
            f.write(hdr + "\n" + "".join(seq) + "\n")
    if os.path.exists(draft + ".fai"):
        os.remove(draft + ".fai")
    if mode is not None:
        c = json.load(open(cfgp))
        c["parameters"]["flank_anchor"] = mode
        json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])
    keys = {}
    for g in gaps:
        keys[(int(g["scaffold"]), int(g["start"]))] = ("%d_%d" % (int(g["scaffold"]), int(g["idx_in_scaffold"])), g)
    return _full_picks(wf + "picked_seqs.fa"), keys, mutated, cfg0, gaps


def test_flank_anchor_align_closes_gaps_with_a_draft_error_next_to_the_gap(tmp_path):
    from gappadder_amd.hip_api import GapFill
    picked_ex, _, mutated, cfg0, gaps = _run(tmp_path / "exact", None)
    picked_al, _, _, _, _ = _run(tmp_path / "align", "align")
    mut_keys = []
    for g in gaps:
        sc, st = int(g["scaffold"]), int(g["start"])
        if any(s == sc and abs(a - st) <= 1 for s, a, _ in mutated):
            mut_keys.append(("%d_%d" % (sc, int(g["idx_in_scaffold"])), g))
    assert len(mut_keys) >= 5, (mutated, [(int(g["scaffold"]), int(g["start"])) for g in gaps])
    n_true = 0
    for key, g in mut_keys:
        assert key not in picked_ex, key
        assert key in picked_al, key
        st, en, sc = int(g["start"]), int(g["end"]), int(g["scaffold"])
        t = (GapFill.synth_truth(cfg0, sc, st - 5, en - st + 11), GapFill.synth_truth(cfg0, sc, st - 6, en - st + 11))
        n_true += picked_al[key] in t
    assert n_true >= len(mut_keys) - 1
    # the gaps with an error-free draft are picked alike
    for key in picked_ex:
        assert picked_al.get(key) == picked_ex[key], key
