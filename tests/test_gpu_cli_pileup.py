"""The CLI's `parameters.fill_pileup`: the first assembly round of the device-resident Collect runs with the pile-up round on and writes
{working_folder}fill_pileup.tsv, picked_seqs.fq, picked_seqs.masked.fa and — with the plain fill_polish — polished_seqs.fq, one record /
row per gap the device step closed, named as in picked_seqs.fa; nothing else of the working folder changes, and with the parameter off
the folder is what it was."""
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


def _fastq(text):
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) % 4 == 1
    recs = [lines[i:i + 4] for i in range(0, len(lines) - 1, 4)]
    assert all(r[0][0] == "@" and r[2] == "+" and len(r[1]) == len(r[3]) > 0 for r in recs)
    return [(r[0][1:], r[1], r[3]) for r in recs]


def test_the_four_files_and_nothing_else(tmp_path, monkeypatch, capfd):
    from gappadder_amd import _lib as B
    from gappadder_amd import device_collect as DC
    from gappadder_amd import main as M
    from gappadder_amd import pileup as PU
    seed, slen, nscf, gps, glen, L = 20260013, 200_000, 3, 4, 120, 150
    cfgp, wf = SF.write_case(str(tmp_path), seed, slen, nscf, gps, glen, [(300, 30, 40_000)], [(31, 29)], kmer_screen=31)
    seen = []
    orig = DC.DeviceCollector.run

    def run(self, *a, **kw):
        res = orig(self, *a, **kw)
        seen.append((res, self))
        return res
    monkeypatch.setattr(DC.DeviceCollector, "run", run)
    c = json.load(open(cfgp))
    c["parameters"].update(fill_polish=True)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])
    off = _tree(wf)
    new = ("fill_pileup.tsv", "picked_seqs.fq", "picked_seqs.masked.fa", "polished_seqs.fq")
    assert not any(n in off for n in new) and seen[-1][0].pileup is None and "polished_seqs.fa" in off
    c["parameters"].update(fill_pileup=True, fill_pileup_min_depth=4, fill_pileup_min_agree=90)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])               # (`All` cleans the working folder first)
    on = _tree(wf)
    tsv, fq, fa, pq = (on.pop(n).decode() for n in new)
    assert sorted(on) == sorted(off)
    diff = [p for p in on if on[p] != off[p]]
    assert not diff, diff[:5]
    res, dc = seen[-1]
    assert dc.pipe.pileup.params == (16, 4, 48, 4, 90)
    conf, closed = dc.pipe.fill_confidence(res), np.nonzero(res.best)[0].tolist()
    # fill_pileup.tsv: the records of the collector's own Results, one per gap the device step closed, in gap order
    fields = [f for f in B.FILL_PILEUP.names if f != "off"]
    rows = [r.split("\t") for r in tsv.splitlines()]
    assert rows[0] == ["name"] + fields and len(rows) - 1 == len(closed) > 0 and res.pileup_stats["gaps"] == len(closed)
    for row, g in zip(rows[1:], closed):
        assert row[0].startswith(res.keys[g] + "_31_29_NODE_") and [int(x) for x in row[1:]] == [int(res.pileup[g][f]) for f in fields]
        assert int(row[1]) > 0 and int(res.pileup[g]["reads_placed"]) > 0
    names = [r[0] for r in rows[1:]]
    picked = {}
    for blk in open(wf + "picked_seqs.fa").read().split(">")[1:]:
        h, s = blk.split("\n", 1)
        picked[h.split()[0]] = s.replace("\n", "")
    # picked_seqs.fq: picked_seqs.fa's sequences, phred of the fetched track per base
    recs = _fastq(fq)
    assert [r[0] for r in recs] == names
    scored = same = 0
    for (name, seq, qual), g in zip(recs, closed):
        _, text, entries, _ = conf[g]
        assert seq == text
        if name in picked:                          # (a later round may have replaced the fill of a gap under another name)
            assert seq == picked[name]
            same += 1
        assert [ord(q) - 33 for q in qual] == [PU.phred(e, b) for e, b in zip(entries, seq)]
        scored += sum(q == "I" for q in qual)       # chr(33 + 40)
    assert scored > 0 and same > 0
    # picked_seqs.masked.fa: the same sequences in lines of 60, is_low at the configured thresholds in lower case
    blocks = fa.split(">")[1:]
    assert [b.split("\n", 1)[0] for b in blocks] == names
    lower = 0
    for blk, g in zip(blocks, closed):
        lines = blk.split("\n")[1:]
        assert lines[-1] == "" and all(len(x) == 60 for x in lines[:-2]) and 0 < len(lines[-2]) <= 60
        masked, (_, text, entries, _) = "".join(lines), conf[g]
        assert masked.upper() == text
        assert [ch.islower() for ch in masked] == [PU.is_low(e, b, 4, 90) for e, b in zip(entries, text)]
        lower += sum(ch.islower() for ch in masked)
    print("%d closed gaps, %d bases at the top score, %d low" % (len(closed), scored, lower))
    # polished_seqs.fq: polished_seqs.fa's sequences, the polished base's score from the same counters
    polished = {}
    for blk in on["polished_seqs.fa"].decode().split(">")[1:]:
        h, s = blk.split("\n", 1)
        polished[h.split()[0]] = s.replace("\n", "")
    precs = _fastq(pq)
    assert [r[0] for r in precs] == names
    for (name, seq, qual), g in zip(precs, closed):
        assert seq == polished[name] and [ord(q) - 33 for q in qual] == [PU.phred(e, b) for e, b in zip(conf[g][2], seq)]
    # with fill_polish_indels no polished FASTQ is written, the other three are
    c["parameters"].update(fill_polish_indels=True)
    json.dump(c, open(cfgp, "w"))
    M.main(["-c", "All", "-g", cfgp])
    assert not os.path.exists(wf + "polished_seqs.fq") and open(wf + "picked_seqs.fq").read() == fq and open(wf + "picked_seqs.masked.fa").read() == fa
    capfd.readouterr()
    # no device step, no files: one line on stderr that names them
    for n in new[:3]:
        os.remove(wf + n)
    monkeypatch.setenv("GF_DEVICE_COLLECT", "0")
    monkeypatch.setattr(M, "collect_per_scaffold", lambda *a, **kw: None)      # (the per-scaffold path itself is not what this is about)
    M.main(["-c", "Collect", "-g", cfgp])
    err = capfd.readouterr().err
    assert err.count("fill_pileup:") == 1 and all(n in err for n in new[:3]) and not any(os.path.exists(wf + n) for n in new)
    assert new[3] not in err                        # (fill_polish_indels is on: that file would never be written)


def test_parameters_out_of_range_make_main_exit_with_a_message(tmp_path):
    from gappadder_amd import main as M
    cfgp, wf = SF.write_case(str(tmp_path), 20260014, 100_000, 1, 2, 120, [(300, 30, 4_000)], [(31, 29)], kmer_screen=31)
    for kw in (dict(fill_pileup_min_agree=101), dict(fill_pileup_min_depth=0), dict(fill_pileup_seed=32, fill_pileup_max_mismatch=4)):
        c = json.load(open(cfgp))
        c["parameters"].update(fill_pileup=True, **kw)
        json.dump(c, open(cfgp + ".bad", "w"))
        with pytest.raises(SystemExit) as e:
            M.main(["-c", "All", "-g", cfgp + ".bad"])
        assert "fill_pileup" in str(e.value)
