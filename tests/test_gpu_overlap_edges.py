"""overlap_eval_kernel / ov_evaluate (csrc/merge.hip) where it can go wrong, through the C ABI: the directed families of
tests/overlap_cases.py -- contigs up to OV_MAXLEN = 8 190 bases (the three rolling LDS diagonals full, up to eight cells per thread
along a diagonal), lengths around a wave, around the 1 024-thread strip and around two strips, end cells that share the maximum
(score descending, clip ascending, column scan before row scan, index ascending: the 64-bit rank of the in-wave and the 16-wave
reduce), max_clip 0 .. 1 000 and contigs shorter than it, a mismatch score that truncates, overlaps around the class thresholds, and
Evaluate's relaxed mode (what mg_strings_kernel concatenates by) -- against

  * tests/golden/evaluate_edge_kat.json.gz, the reference's own Evaluate on the 2-kb scale of the strict families, and
  * the oracle (or_overlap_evaluate, itself pinned on those vectors in test_oracle_golden.py), every result field of every pair,
    at full length.

The counts that keep a comparison from being vacuous (overlap_cases.MINIMUM / TOTALS) are asserted on the expected answers alone."""
import gzip
import json
import os

import numpy as np
import pytest

import overlap_cases as OC
from golden_util import GOLDEN

pytestmark = pytest.mark.gpu

OVL_FIELDS = ("res", "row_end", "col_end", "nclip", "score", "contained", "merged_len", "overlap", "containment", "first_goes_first")
FAMILIES = OC.STRICT + OC.RELAXED


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


def _qcpairs(triples):
    from gappadder_amd import _lib as B
    out = np.zeros(len(triples), dtype=B.QCPAIR)
    out["set"], out["i"], out["j"] = [t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples]
    return out


def _evaluate(gf, cases):
    """gf.overlap_evaluate on all pairs of `cases` (one parameter set, one mode): ONE call, the cases as its sets -> a result array per case"""
    assert len({(c["params"], c["relax"]) for c in cases}) == 1
    triples = [(s, i, j) for s, c in enumerate(cases) for i, j in c["pairs"]]
    got = gf.overlap_evaluate([c["contigs"] for c in cases], _qcpairs(triples), cases[0]["params"], relax=cases[0]["relax"])
    out, at = [], 0
    for c in cases:
        out.append(got[at:at + len(c["pairs"])])
        at += len(c["pairs"])
    return out


def _by_params(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c["params"], c["relax"]), []).append(c)
    return list(groups.values())


def _same(case, got, exp):
    assert len(got) == len(exp)
    for (i, j), g, e in zip(case["pairs"], got, exp):
        assert {f: int(g[f]) for f in OVL_FIELDS} == e, (case["name"], i, j)


def test_overlap_evaluate_equals_the_reference_edge_vectors(gf):
    """Every ordered node pair of every set of evaluate_edge_kat.json.gz against what the reference's own Evaluate printed; one call
    per parameter set, the sets of that parameter set side by side."""
    cases = json.loads(gzip.open(os.path.join(GOLDEN, "evaluate_edge_kat.json.gz"), "rt").read())
    mine = [dict(c, params=tuple(c["params"]), relax=False, pairs=OC.all_ordered(c["contigs"])) for c in cases]
    n_ovl = n_ties = 0
    for group in _by_params(mine):
        for c, got in zip(group, _evaluate(gf, group)):
            assert c["pairs"] == [(r[0], r[1]) for r in c["results"]]
            for g, r in zip(got, c["results"]):
                assert int(g["res"]) == r[2], (c["name"], r, g)
                if r[2]:
                    assert [int(g[f]) for f in ("row_end", "nclip", "overlap", "merged_len", "containment")] == r[3:], (c["name"], r, g)
                    n_ovl += 1
                    n_ties += c["name"].startswith("ties/")
    assert n_ovl >= 500 and n_ties >= OC.TIES_CLASS_1_2


@pytest.mark.parametrize("family", FAMILIES)
def test_family_equals_the_oracle_in_every_field(gf, family):
    """All result fields of every evaluated pair of one family, at full length, one call per parameter set."""
    cases = OC.families(True)[family]
    exp = OC.expected_all(cases)
    n = OC.check_minimum(family, cases, exp)
    if family.startswith("relax_"):
        assert n["res2"] == sum(len(c["pairs"]) for c in cases)          # relaxed: no significance test, every pair is class 2
    by_name = {c["name"]: e for c, e in zip(cases, exp)}
    for group in _by_params(cases):
        for c, got in zip(group, _evaluate(gf, group)):
            _same(c, got, by_name[c["name"]])
            if c["relax"]:
                assert (got["res"] == 2).all()


def test_expected_answers_reach_the_required_counts():
    """On the oracle's answers alone, summed over the families: clipped ends, second-node-first overlaps, contained nodes,
    containments, all three classes, pairs of two nodes at the LDS row end, single-base nodes, and ties of class 1 or 2."""
    fam = OC.families(True)
    total = dict.fromkeys(OC.TOTALS, 0)
    for name in FAMILIES:
        exp = OC.expected_all(fam[name])
        for k, v in OC.check_minimum(name, fam[name], exp).items():
            total[k] += v
        if name == "ties":
            assert sum(r["res"] in (1, 2) for e in exp for r in e) >= OC.TIES_CLASS_1_2
    for k, v in OC.TOTALS.items():
        assert total[k] >= v, (k, total[k], v)


def test_many_pairs_in_one_call_in_either_order(gf):
    """All families of the merger's own parameter set in ONE call.  The call opens with more copies of an 8 190 x 8 190 pair than the
    device has compute units, so that (pairs are handed out in order) every workgroup has swept a full-length pair before it takes
    the short ones behind them -- down to a single base -- on the same LDS rows.  Then the same pairs in reversed order: each pair's
    answer is the oracle's both times."""
    import torch
    fam = OC.families(True)
    cases = [c for name in OC.STRICT for c in fam[name] if c["params"] == OC.GAPPADDER]
    assert OC.big_pairs(cases) <= OC.BIG_PAIR_BUDGET
    exp = OC.expected_all(cases)
    assert {"limit/long_1", "strips/63_2049", "ties/polyA_8190_31", "clip/short_clip50"} <= {"%s/%s" % (n, c["name"]) for n in OC.STRICT for c in fam[n]}
    long_set = next(s for s, c in enumerate(cases) if c["name"] == "clean")
    long_pair = cases[long_set]["pairs"][0]
    nd = OC.nodes_of(cases[long_set]["contigs"])
    assert len(nd[long_pair[0]]) == len(nd[long_pair[1]]) == OC.OV_MAXLEN
    n_long = torch.cuda.get_device_properties(0).multi_processor_count + 64
    rest = [(s, i, j, e) for s, (c, ex) in enumerate(zip(cases, exp)) for (i, j), e in zip(c["pairs"], ex)]
    assert sum(min(len(cases[s]["contigs"][i // 2]), len(cases[s]["contigs"][j // 2])) == 1 for s, i, j, _ in rest) >= 4
    order = [(long_set, long_pair[0], long_pair[1], exp[long_set][0])] * n_long + rest
    sets = [c["contigs"] for c in cases]
    for seq in (order, order[::-1]):
        got = gf.overlap_evaluate(sets, _qcpairs([t[:3] for t in seq]), OC.GAPPADDER)
        for t, g in zip(seq, got):
            assert {f: int(g[f]) for f in OVL_FIELDS} == t[3], (cases[t[0]]["name"], t[1], t[2])


def test_ties_are_repeatable(gf):
    """The ties family twice: byte-identical outputs (which workgroup takes which pair changes from run to run; no answer may)."""
    cases = OC.families(True)["ties"]
    runs = [b"".join(r.tobytes() for group in _by_params(cases) for r in _evaluate(gf, group)) for _ in range(2)]
    assert runs[0] == runs[1] and len(runs[0]) == sum(len(c["pairs"]) for c in cases) * 40


def _dev_call(gf, contigs, pairs, params, fill=0xAB, n_pairs=None):
    """gf_overlap_evaluate_dev on torch buffers: ONE set `contigs` (any lengths, 0 included), `pairs` = [(i, j)] -> (return code, the
    whole output buffer as OVL_RESULT records, filled with `fill` before the call)"""
    import torch
    from gappadder_amd import _lib as B
    blob = "".join(contigs).encode()
    coff = np.zeros(len(contigs) + 1, dtype=np.uint64)
    coff[1:] = np.cumsum([len(c) for c in contigs])
    soff = np.array([0, len(contigs)], dtype=np.uint64)
    dev = lambda a: torch.from_numpy(np.frombuffer(a.tobytes() + b"\0" * 64, dtype=np.uint8).copy()).cuda()
    d_seq, d_co, d_so = dev(np.frombuffer(blob, dtype=np.uint8)), dev(coff), dev(soff)
    d_pairs = dev(_qcpairs([(0, i, j) for i, j in pairs]))
    d_out = torch.full((max(1, len(pairs)) * B.OVL_RESULT.itemsize,), fill, dtype=torch.uint8, device="cuda")
    pr = np.zeros(1, dtype=B.OVL_PARAMS)
    pr[0] = tuple(params)[:7] + (0.0,)
    torch.cuda.synchronize()
    rc = B.lib().gf_overlap_evaluate_dev(gf.handle, d_seq.data_ptr(), d_co.data_ptr(), d_so.data_ptr(), d_pairs.data_ptr(),
                                         len(pairs) if n_pairs is None else n_pairs, B._p(pr), d_out.data_ptr())
    gf.sync()
    return rc, np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.OVL_RESULT)


def test_device_entry_point_marks_what_it_cannot_evaluate(gf):
    """gf_overlap_evaluate_dev on device buffers: pairs with a contig of 8 191 bases or of none come back as res = -1 and zeros, the
    other pairs of the same call as the oracle has them; no pairs: GF_OK and the output untouched; a fractional indel score:
    GF_E_UNSUPPORTED; the host form refuses 8 191 bases with GF_E_INVAL; both forms take 8 190."""
    import random
    from gappadder_amd import _lib as B
    from oracle import c_oracle as CO
    rng = random.Random(8191)
    g = "".join(rng.choice("ACGT") for _ in range(8191 + 500))
    contigs = [g[0:8191], "", g[8000:8300], g[8191:8691], g[8190]]
    pairs = OC.all_ordered(contigs)
    rc, got = _dev_call(gf, contigs, pairs, OC.GAPPADDER)
    assert rc == B.GF_OK
    nd = OC.nodes_of(contigs)
    n_bad = n_ovl = 0
    for (i, j), r in zip(pairs, got):
        if i // 2 in (0, 1) or j // 2 in (0, 1):
            assert int(r["res"]) == -1 and not any(int(r[f]) for f in OVL_FIELDS[1:]), (i, j, r)
            n_bad += 1
        else:
            e = CO.overlap_evaluate(nd[i], nd[j], OC.GAPPADDER)
            assert {f: int(r[f]) for f in OVL_FIELDS} == e, (i, j)
            n_ovl += e["res"] == 2
    assert n_bad == len(pairs) - 6 * 5 and n_ovl >= 2
    # no pairs: nothing is written; a fractional indel score: refused before anything is written
    for params, n_pairs, want in ((OC.GAPPADDER, 0, B.GF_OK), ((-2.0, -1.5, 50.0, 0.005, 0.4, 12.0, 6.0), None, B.GF_E_UNSUPPORTED)):
        rc, got = _dev_call(gf, contigs, pairs, params, fill=0xAB, n_pairs=n_pairs)
        assert rc == want and got.tobytes() == b"\xab" * (len(pairs) * B.OVL_RESULT.itemsize), (params, n_pairs)
    # the host form refuses what the device form marks
    with pytest.raises(B.GapFillError) as e:
        gf.overlap_evaluate([contigs[:1] + contigs[2:]], _qcpairs([(0, 0, 2)]), OC.GAPPADDER)
    assert e.value.code == B.GF_E_INVAL
    # 8 190 bases: both forms evaluate
    case = next(c for c in OC.families(True)["limit"] if c["name"] == "long_30")
    exp = OC.expected(case)
    rc, got = _dev_call(gf, case["contigs"], case["pairs"], case["params"])
    assert rc == B.GF_OK
    _same(case, got, exp)
    _same(case, _evaluate(gf, [case])[0], exp)
