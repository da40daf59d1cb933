"""The contig merger as one device call with its graph exported (gf_merge_sets, GapFill.merge_sets_device) and the CLI's
MergeContigs.merge_contigs(engine="device") on top of it: every set's first dedup, nodes, edges (in merge_edges.txt's order), paths,
merged strings and second dedup equal the host twin (MergeContigs.drop_contained / merge_sets) and, where no contig is contained, the
reference binary's own answers (tests/golden/merger_kat.json.gz); both engines leave byte-identical working folders."""
import filecmp
import gzip
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN

pytestmark = pytest.mark.gpu

LUT = np.frombuffer(b"ACGT", np.uint8)


def rc(x):
    return x[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def rnd(rng, n):
    return LUT[rng.integers(0, 4, n)].tobytes().decode()


def recs_of(seqs):
    return [("c%d" % i, s) for i, s in enumerate(seqs)]


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def kat():
    cases = json.loads(gzip.open(os.path.join(GOLDEN, "merger_kat.json.gz")).read())
    return cases, [recs_of(c["contigs"]) for c in cases]


@pytest.fixture(scope="module")
def kat_device(gf, kat):
    return gf.merge_sets_device(kat[1]), dict(gf.last_merge_sets_stats)


def host_twin(gf, rec_sets):
    """Per set what the host engine computes: (nodup, merge_sets' dict of it, final)."""
    from gappadder_amd import MergeContigs as MC
    nodups = [MC.drop_contained(r) for r in rec_sets]
    out = []
    for nodup, m in zip(nodups, MC.merge_sets(gf, nodups)):
        out.append((nodup, m, MC.drop_contained([(n, s) for n, s, _ in m["new"]] + nodup)))
    return out


def assert_equals_twin(d, twin, what):
    nodup, m, final = twin
    assert d["nodup"] == nodup, what
    assert d["nodes"] == m["nodes"], what
    assert isinstance(d["edges"], list) and d["edges"] == m["edges"], what
    assert d["new"] == m["new"], what
    assert d["final"] == final, what


def truncation_set(rng):
    """Four 4 000-base contigs, neighbours overlapping by 100 bases: the running string is 7 900, then 11 800 bases, and the path ends there."""
    g = rnd(rng, 4 * 4000 - 3 * 100)
    return [g[i * 3900:i * 3900 + 4000] for i in range(4)]


def limit_sets(rng):
    g = rnd(rng, 900)
    three = [g[0:400], g[330:800], g[700:900]]
    h = rnd(rng, 700)
    both = [h[0:400], rc(h[0:400]), h[300:700]]
    return {"big": [rnd(rng, 90) for _ in range(140)],
            "three": list(three),
            "pass_through": [rnd(rng, 20)] + three + [rnd(rng, 9000)],
            "lower": [s.lower() for s in three],
            "both_strands": both}


def test_kat_sets_equal_the_host_twin_and_the_reference_binary(gf, kat, kat_device):
    cases, rec_sets = kat
    got, stats = kat_device
    assert len(cases) == 41 and len(got) == 41
    twins = host_twin(gf, rec_sets)
    n_direct = 0
    for ci, (c, d, tw) in enumerate(zip(cases, got, twins)):
        assert d["status"] in ("merged", "nothing"), ci
        assert_equals_twin(d, tw, ci)
        if len(tw[0]) == len(c["contigs"]):          # no contained contig: the reference binary's own answer, sequence and path
            names = [n for n, _ in d["nodes"]]
            assert [s for _, s, _ in d["new"]] == [x["seq"] for x in c["new"]], ci
            assert [[names[v >> 1] + ("_R" if v & 1 else "") for v in p] for _, _, p in d["new"]] == [x["path"] for x in c["new"]], ci
            n_direct += 1
    assert n_direct >= 30
    assert stats["paths"] == sum(len(d["new"]) for d in got) and stats["edges"] == sum(len(d["edges"]) for d in got)
    assert stats["flags"] == 0 and stats["truncated_paths"] == 0


def random_sets(seed):
    """The generator of test_gpu_merge.py::test_device_merge_round_on_random_contig_sets, with another seed."""
    rng = np.random.default_rng(seed)
    sets = []
    for s in range(120):
        g = rnd(rng, int(rng.integers(600, 4000)))
        if s % 7 == 0:
            rep = rnd(rng, 120)
            g = g[:200] + rep + g[200:len(g) // 2] + rep + g[len(g) // 2:]
        cs, at = [], 0
        while at < len(g) - 80:
            ln = int(rng.integers(80, 700))
            c = g[at:at + ln]
            if rng.integers(0, 50) == 0:
                q = int(rng.integers(0, len(c)))
                c = c[:q] + "ACGT"[("ACGT".index(c[q]) + 1) % 4] + c[q + 1:]
            cs.append(rc(c) if rng.integers(0, 2) else c)
            at += max(20, ln - int(rng.integers(15, 120)))
        if rng.integers(0, 3) == 0:
            cs.append(cs[0])
        if rng.integers(0, 3) == 0:
            cs.append(g[100:160])
        if rng.integers(0, 4) == 0:
            cs.append(rnd(rng, 200))
        order = rng.permutation(len(cs))
        sets.append([cs[i] for i in order])
    sets.append([rnd(rng, 100)])
    sets.append([])
    return sets


def test_random_fragmented_sets(gf):
    from gappadder_amd import MergeContigs as MC
    rec_sets = [recs_of(cs) for cs in random_sets(29)]
    got = gf.merge_sets_device(rec_sets)
    stats = dict(gf.last_merge_sets_stats)
    twins = host_twin(gf, rec_sets)
    n_checked = 0
    for si, (r, d, tw) in enumerate(zip(rec_sets, got, twins)):
        n_nodup = len(tw[0])
        if 2 <= n_nodup <= 128:
            assert d["status"] in ("merged", "nothing"), si
            assert (d["status"] == "merged") == (len(tw[1]["nodes"]) >= 2), si
            assert_equals_twin(d, tw, si)
            n_checked += 1
        elif n_nodup < 2:
            assert d["status"] == "nothing" and d["nodup"] == tw[0] and d["new"] == [] and d["final"] == tw[0], si
        else:
            assert d["status"] == "size" and d["nodup"] == tw[0], si
    assert n_checked >= 100 and got[-2]["status"] == "nothing" and got[-1]["status"] == "nothing" and got[-1]["nodup"] == []
    by = lambda s: sum(1 for d in got if d["status"] == s)
    assert (stats["tried"], stats["nothing"], stats["skipped_size"], stats["skipped_graph"]) == (by("merged"), by("nothing"), by("size"), by("graph"))
    assert stats["paths"] == sum(len(d["new"]) for d in got if d["new"]) and stats["paths"] > 100
    assert stats["edges"] == sum(len(d["edges"]) for d in got if d["edges"]) and stats["edges"] > 300 and stats["flags"] == 0
    assert any(len(d["final"]) < len(d["new"]) + len(d["nodup"]) for d in got if d["new"])      # the second dedup dropped something


def test_a_path_that_outgrows_the_overlap_kernel_is_reported_truncated(gf, tmp_path):
    from gappadder_amd import MergeContigs as MC
    cs = truncation_set(np.random.default_rng(31))
    recs = recs_of(cs)
    d = gf.merge_sets_device([recs])[0]
    stats = dict(gf.last_merge_sets_stats)
    tw = host_twin(gf, [recs])[0]
    assert_equals_twin(d, tw, "truncation")
    (name, seq, path), = d["new"]
    whole = cs[0] + cs[1][100:] + cs[2][100:] + cs[3][100:]
    assert len(path) == 3 and len(seq) == 11800 and seq in (whole[:11800], whole[3900:], rc(whole[:11800]), rc(whole[3900:]))
    assert stats["truncated_paths"] == 1 and stats["paths"] == 1
    wf = str(tmp_path) + "/"
    os.makedirs(wf + "velvet_temp/t")
    MC._write_fasta(wf + "velvet_temp/t/contigs.fa", recs)
    assert MC.merge_contigs(gf, wf, ["t"], engine="device") == {"t": 1}
    line, = open(wf + "velvet_temp/t/contigs.fa_no_dup.fa.merge.info").read().splitlines()
    assert len(line.split()) == 1 + 3


def test_limits_and_pass_through(gf):
    L = limit_sets(np.random.default_rng(32))
    order = ["three", "big", "three", "pass_through", "lower", "both_strands", "three"]
    rec_sets = [recs_of(L[k]) for k in order]
    got = gf.merge_sets_device(rec_sets)
    twins = host_twin(gf, rec_sets)
    assert [d["status"] for d in got] == ["merged", "size", "merged", "merged", "merged", "merged", "merged"]
    for si in (0, 2, 3, 4, 5, 6):
        assert_equals_twin(got[si], twins[si], order[si])
    assert got[0]["new"] and got[0] == got[2] == got[6]                         # the neighbours of the set left alone
    assert got[1]["nodup"] == twins[1][0] and got[1]["new"] is None and got[1]["final"] is None
    pt = got[3]
    assert len(pt["nodup"]) == 5 and len(pt["nodes"]) == 3 and pt["new"]
    assert rec_sets[3][0] in pt["final"] and rec_sets[3][4] in pt["final"]       # 20 and 9 000 bases: no nodes, they pass through
    assert got[4]["nodup"] == rec_sets[4] and [s for _, s, _ in got[4]["new"]] == [s for _, s, _ in got[0]["new"]]     # lower case in, upper case merged
    assert len(got[5]["nodup"]) == 2                                             # a contig and its reverse complement: the first stays
    small = gf.merge_sets_device(rec_sets[:3], max_set=2)
    assert [d["status"] for d in small] == ["size", "size", "size"] and small[0]["nodup"] == twins[0][0]
    assert gf.last_merge_sets_stats["skipped_size"] == 3 and gf.last_merge_sets_stats["paths"] == 0


def _write_sets(wf, named_sets):
    from gappadder_amd import MergeContigs as MC
    for gid, recs in named_sets:
        os.makedirs(wf + "velvet_temp/" + gid)
        if recs is not None:
            MC._write_fasta(wf + "velvet_temp/%s/contigs.fa" % gid, recs)


def _same_trees(a, b):
    names = []
    for root, _, files in os.walk(a):
        for fn in files:
            p = os.path.join(root, fn)
            q = os.path.join(b, os.path.relpath(p, a))
            assert os.path.exists(q) and filecmp.cmp(p, q, shallow=False), p
            names.append(fn)
    assert sum(len(f) for _, _, f in os.walk(b)) == len(names)
    return set(names)


def test_both_engines_leave_the_same_tree(gf, kat, tmp_path):
    from gappadder_amd import MergeContigs as MC
    rng = np.random.default_rng(33)
    L = limit_sets(rng)
    named = [("3_%d" % (i + 1), r) for i, r in enumerate(kat[1])]
    named += [("t_1", recs_of(truncation_set(rng)))] + [("l_%s" % k, recs_of(v)) for k, v in sorted(L.items())]
    named += [("no_contigs", None), ("one_mb", recs_of([rnd(rng, 8190) for _ in range(125)]))]
    ids = [gid for gid, _ in named]
    wfs = []
    for eng in ("host", "device"):
        wf = "%s/%s/" % (tmp_path, eng)
        _write_sets(wf, named)
        wfs.append(wf)
    before = dict(MC.DEVICE_COUNTS)
    done_h = MC.merge_contigs(gf, wfs[0], ids, engine="host")
    done_d = MC.merge_contigs(gf, wfs[1], ids, engine="device")
    assert done_h == done_d and sum(done_d.values()) >= 40 and "no_contigs" not in done_d and done_d["one_mb"] == 0
    seen = _same_trees(wfs[0] + "velvet_temp", wfs[1] + "velvet_temp")
    assert seen == {"contigs.fa", "contigs.fa_no_dup.fa", "contigs.fa_no_dup.fa.merge.info", "contigs.fa_no_dup.fa.merged.fa", "merge_edges.txt",
                    "original_contigs_before_merging.fa"}
    assert MC.LAST_FELL_BACK == ["l_big"]
    assert MC.DEVICE_COUNTS["fell_back_sets"] - before["fell_back_sets"] == 1 and MC.DEVICE_COUNTS["host_rule_sets"] - before["host_rule_sets"] == 1
    assert MC.DEVICE_COUNTS["device_sets"] - before["device_sets"] == len(named) - 3


def test_a_small_capacity_raises_and_nothing_is_truncated(gf, kat, kat_device):
    from gappadder_amd import _lib as B
    got, stats = kat_device
    assert stats["edges"] > 8 and stats["paths"] > 2
    for caps in [(8, 1 << 12, 1 << 16, 1 << 22, 1 << 14), (1 << 14, 2, 1 << 16, 1 << 22, 1 << 14), (1 << 14, 1 << 12, 4, 1 << 22, 1 << 14),
                 (1 << 14, 1 << 12, 1 << 16, 100, 1 << 14), (1 << 14, 1 << 12, 1 << 16, 1 << 22, 16)]:
        with pytest.raises(B.GapFillError) as e:
            gf.merge_sets_device(kat[1], caps=caps)
        assert e.value.code == B.GF_E_NOSPACE, caps
    assert gf.merge_sets_device(kat[1]) == got


def _one_gap_folder(root, left, right, reads):
    wf = root + "/wf/"
    for sub in ("merged/gap_reads", "merged/gap_reads_high_quality", "merged/velvet_temp", "flank_regions"):
        os.makedirs(wf + sub)
    open(wf + "flank_regions/0_1.fa", "w").write(">0_1_left\n%s\n>0_1_right\n%s\n" % (left, right))
    open(wf + "merged/gap_reads/0_1.fastq", "w").write("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    open(root + "/d.fai", "w").write("scf0\t100000\t6\t60\t61\n")
    open(wf + "gap_positions.txt", "w").write("5000 5600 600 scf0\n")
    return wf


def _tile(g, L=100, step=5):
    out = []
    for s in list(range(0, len(g) - L + 1, step)) + [len(g) - L]:
        out += [g[s:s + L], rc(g[s:s + L])]
    return out


def test_whole_pipeline_is_the_same_with_either_engine(gf, tmp_path):
    """The one-gap layout of test_gpu_merge.py::test_a_gap_that_only_the_contig_merging_closes through assemble_pipeline."""
    from gappadder_amd import assemble_gaps as AG
    rng = np.random.default_rng(77)
    g = rnd(rng, 1400)
    left, right = g[100:395], g[1005:1300]
    branch = g[560:680] + rnd(rng, 80)
    reads = _tile(g[60:1340]) + _tile(branch, step=4)
    out = {}
    for eng in ("host", "device"):
        root = "%s/%s" % (tmp_path, eng)
        os.makedirs(root)
        wf = _one_gap_folder(root, left, right, reads)
        ga = AG.GapAssembler(root + "/d.fai", wf + "gap_positions.txt", 1, wf + "merged/", kmer_list=[(31, 29)], gf=gf, contig_merger=eng)
        out[eng] = (ga.assemble_pipeline(), open(wf + "picked_seqs.fa").read(), wf)
    assert out["host"][0] == out["device"][0] and out["device"][0]["closed"] == 1 and out["device"][0]["gaps_with_merged_contigs"] >= 1
    assert out["host"][1] == out["device"][1] and out["device"][1].startswith(">0_1_NEW_CONTIG_MERGE_")
    assert "merge_edges.txt" in _same_trees(out["host"][2] + "merged/velvet_temp", out["device"][2] + "merged/velvet_temp")
