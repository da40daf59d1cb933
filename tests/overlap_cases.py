"""Directed inputs for the contig merger's pairwise overlap evaluation (ContigsCompactor::Evaluate; csrc/merge.hip ov_evaluate,
oracle/gp_oracle.c or_overlap_evaluate), shared by the CPU tests (test_oracle_golden.py), the GPU tests (test_gpu_overlap_edges.py)
and the writer of the reference vectors (golden/make_golden.py evaluate_edge_kat).  Plain module: fixed seeds, no GPU import.

A case is a dict
    name      unique inside its family
    contigs   ONE contig set; its nodes are [c0, revcomp(c0), c1, ...] (node = 2 * contig + strand)
    params    the seven merger parameters (mismatch, indel, max_clip, frac_min_overlap, frac_loss, min_overlap, min_overlap_scaffold)
    relax     Evaluate's fRelax mode (what the merged strings are built with)
    pairs     the ordered node pairs (i, j) to evaluate
and a family is a list of cases: families(full) -> {name: [case]}.

full=True is what the GPU tests run: the limit / ties / relax families reach OV_MAXLEN = 8 190 bases.  full=False replaces every
contig above 2 100 bases by a 2-kb scale model of the same construction and lists ALL ordered node pairs of every set: that is
what the reference's own driver (oracle/_ref/evaluate_kat: every ordered pair, a 16-byte-per-cell table) can evaluate, and what
tests/golden/evaluate_edge_kat.json.gz holds.

The oracle costs ~0.45 s per 8 190 x 8 190 pair, so no family lists more than BIG_PAIR_BUDGET distinct pairs in which both nodes exceed
4 000 bases (limit: 8, ties: 3; copies of one pair count once, the oracle sweeps it once), and expected() computes every
(node, node, params, relax) once per process.

MINIMUM holds, per family, the counts its EXPECTED answers (oracle or reference, never the code under test) must reach, so that no
comparison is vacuous; TOTALS is what they must add up to over the families."""
import functools
import random

LENGTHS = (1, 2, 29, 30, 31, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 8189, 8190)
STRIP_LENGTHS = (63, 64, 65, 1023, 1024, 1025, 2047, 2049)
OV_MAXLEN = 8190
GOLDEN_MAXLEN = 2100
BIG = 4000
BIG_PAIR_BUDGET = 12
GAPPADDER = (-2.0, -2.0, 50.0, 0.005, 0.4, 12.0, 6.0)      # MergeContigs.py:75 + ContigsMerger's defaults
DEFAULTS = (-1.0, -1.0, 0.0, 0.005, 0.01, 100000.0, 6.0)    # ContigsMerger's own defaults (main.cpp:24-27)
PARAM_SETS = ((-1.5, -2.0, 50.0, 0.005, 0.4, 12.0, 6.0),    # the mismatch score truncates to -1
              (-3.0, -1.0, 50.0, 0.005, 0.4, 12.0, 6.0),
              (0.0, -2.0, 50.0, 0.005, 0.4, 12.0, 6.0),
              (-2.0, -2.0, 10.0, 0.3, 0.2, 25.0, 15.0),      # with overlaps of 14 .. 26 bases: classes 0, 1 and 2
              DEFAULTS)
THRESHOLD_OVERLAPS = (14, 15, 24, 25, 26)
CLIP_TAILS = (0, 1, 49, 50, 51, 150)
CLIP_VALUES = (0, 1, 49, 50, 51, 200, 1000)

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    return "".join(_COMP.get(c, c) for c in reversed(s))


def nodes_of(contigs):
    return [x for c in contigs for x in (c.upper(), rc(c.upper()))]


def all_ordered(contigs):
    n = 2 * len(contigs)
    return [(i, j) for i in range(n) for j in range(n) if i != j]


def cross_pairs(a=0, b=1):
    """the ordered node pairs between contigs a and b, both strands (not a contig against its own reverse complement)"""
    na, nb = (2 * a, 2 * a + 1), (2 * b, 2 * b + 1)
    return [(i, j) for i in na for j in nb] + [(j, i) for i in na for j in nb]


def _rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _noisy(rng, s, subs, indels, lo=1, hi=None):
    """`subs` substitutions and `indels` single-base indels at random places of s[lo:hi]"""
    s = list(s)
    hi = len(s) - 1 if hi is None else hi
    for _ in range(subs):
        i = rng.randrange(lo, hi)
        s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
    for _ in range(indels):
        i = rng.randrange(lo, hi)
        if rng.random() < 0.5:
            del s[i]
        else:
            s.insert(i, rng.choice("ACGT"))
    return "".join(s)


def _case(name, contigs, params=GAPPADDER, pairs=None, relax=False):
    return {"name": name, "contigs": list(contigs), "params": tuple(float(x) for x in params), "relax": bool(relax),
            "pairs": all_ordered(contigs) if pairs is None else list(pairs)}


# ---- limit: the LDS row end -------------------------------------------------------------------------------------------------
def _limit(full):
    rng = random.Random(8190)
    n = OV_MAXLEN if full else 2048
    ov = 2190 if full else 548
    g = _rnd(rng, 2 * n)
    a, b = g[0:n], g[n - ov:2 * n - ov]
    out = [_case("clean", [a, b], pairs=None if not full else [(0, 2), (2, 0), (3, 1)])]
    # ~20 substitutions and 10 indels inside the overlap (the first contig's suffix); the length is kept
    an = a[:n - ov] + _noisy(rng, a[n - ov:], 20, 10, 5, ov - 5)
    an = an[len(an) - n:] if len(an) >= n else _rnd(rng, n - len(an)) + an
    out.append(_case("noisy", [an, b], pairs=None if not full else [(0, 2), (3, 1)]))
    near = _noisy(rng, a[1:], 3, 0, n // 4, 3 * n // 4)                                  # n - 1 bases, inside a: a containment
    out.append(_case("containment", [a, near], pairs=None if not full else [(0, 2), (2, 0)]))
    out.append(_case("unrelated", [a, _rnd(rng, n)], pairs=None if not full else [(0, 2)]))
    m = g[n // 2:n // 2 + n]                                                            # the long node of the mixed pairs
    lo, hi = n // 2, n // 2 + n
    # 1 and 30 lie inside the long node (contained, far off the corner diagonals); 1 023 hangs over its start, 1 025 over its end
    small = {"1": m[-1], "30": m[n - n // 4 - 30:n - n // 4], "1023": g[lo - 500:lo + 523], "1025": g[hi - 500:hi + 525]}
    for k, s in small.items():
        assert len(s) == int(k)
        # (n, k) and (k, n), both strands of both
        out.append(_case("long_%s" % k, [m, s], pairs=cross_pairs()))
    return out


# ---- strips: one, two and three cells per thread along a diagonal -----------------------------------------------------------
def _strips():
    rng = random.Random(1024)
    g = _rnd(rng, 2 * max(STRIP_LENGTHS))
    out = []
    for n in STRIP_LENGTHS:
        for m in STRIP_LENGTHS:
            h = min(n, m) // 2                                                         # x's last h bases are y's first h
            x, y = g[0:n], g[n - h:n - h + m]
            # two indels inside the overlap: a deletion and an insertion in y's prefix (the length is kept)
            p = sorted(rng.sample(range(3, h - 3), 2))
            y = y[:p[0]] + y[p[0] + 1:p[1]] + rng.choice("ACGT") + y[p[1]:]
            assert len(x) == n and len(y) == m
            out.append(_case("%d_%d" % (n, m), [x, y], pairs=[(0, 2), (2, 0), (3, 1), (0, 3)]))
    return out


# ---- ties: many end cells share the maximum ---------------------------------------------------------------------------------
def _ties(full):
    rng = random.Random(64)
    out = []
    poly = ((8190, 8190), (8190, 31), (2049, 1025), (64, 65)) if full else ((2049, 2049), (2049, 31), (2049, 1025), (64, 65))
    for n, m in poly:
        out.append(_case("polyA_%d_%d" % (n, m), ["A" * n, "A" * m], pairs=None if not full else [(0, 2), (2, 0)]))
    # ACGT x k against GTAC x k' + a random tail (both repeats are their own reverse complements: one strand says it all)
    out.append(_case("tandem_2k", ["ACGT" * 500, "GTAC" * 480 + _rnd(rng, 80)], pairs=None if not full else [(0, 2), (2, 0), (0, 3), (3, 0)]))
    if full:
        out.append(_case("tandem_8k", ["ACGT" * 2047, "GTAC" * 2005 + _rnd(rng, 80)], pairs=[(0, 2), (2, 0)]))
        assert [len(c) for c in out[-1]["contigs"]] == [8188, 8100]
    out.append(_case("period_2_4", ["AC" * 700, "ACGT" * 500]))
    c = _rnd(rng, 600)
    t1, t2 = _rnd(rng, 40), _rnd(rng, 40)
    out.append(_case("self_tails", [c, t1 + c, c + t2, t1 + c + t2]))
    blk = _rnd(rng, 200)
    out.append(_case("shared_ends", [blk + _rnd(rng, 800) + blk, blk + _rnd(rng, 600) + blk]))
    return out


# ---- clip: the end cell shifted in by 0 .. max_clip -------------------------------------------------------------------------
def _clip():
    rng = random.Random(50)
    g = _rnd(rng, 800)
    out = []
    for t in CLIP_TAILS:
        x = g[0:500] + _rnd(rng, t)                                                    # 200 clean bases, then t bases that y does not have
        y = g[300:800]
        for c in CLIP_VALUES:
            out.append(_case("tail%d_clip%d" % (t, c), [x, y], (-2.0, -2.0, float(c), 0.005, 0.4, 12.0, 6.0)))
    # contigs shorter than max_clip: every cell is an end-cell candidate
    s = _rnd(rng, 45)
    short = [s[0:1], s[0:2], s[0:30], s[15:44], s[14:45]]
    assert [len(x) for x in short] == [1, 2, 30, 29, 31]
    out.append(_case("short_clip50", short, GAPPADDER))
    h = _rnd(rng, 450)
    out.append(_case("300_clip1000", [h[0:300], h[150:450]], (-2.0, -2.0, 1000.0, 0.005, 0.4, 12.0, 6.0)))
    return out


# ---- params: truncation of the mismatch score, the three classes ------------------------------------------------------------
def _params():
    rng = random.Random(7)
    g = _rnd(rng, 5000)
    c1 = _noisy(rng, g[1500:3500], 25, 6)
    noisy2k = [_noisy(rng, g[0:2000], 25, 6), c1, rc(_noisy(rng, g[3000:5000], 25, 6)), c1[800:1200]]   # the last: clean, contained in c1
    # the tiling's overlaps in both orders and on both strands, one unrelated pair, and the contained contig against its host
    pairs = [(0, 2), (2, 0), (3, 1), (2, 5), (5, 2), (4, 3), (2, 4), (0, 5)] + cross_pairs(1, 3)
    out = []
    for pi, pr in enumerate(PARAM_SETS):
        out.append(_case("noisy2k_p%d" % pi, noisy2k, pr, pairs=pairs))
    for k in THRESHOLD_OVERLAPS:                                                       # 40-base contigs: k / 40 >= frac_min_overlap = 0.3
        u = _rnd(rng, 40)
        out.append(_case("overlap%d" % k, [u, u[-k:] + _rnd(rng, 40 - k)], PARAM_SETS[3]))
    return out


# ---- relax: no significance test; the fields mg_strings_kernel concatenates by -----------------------------------------------
def _relaxed(cases, prefix):
    return [dict(c, name="%s_%s" % (prefix, c["name"]), relax=True) for c in cases]


def _running_string():
    rng = random.Random(300)
    g = _rnd(rng, OV_MAXLEN + 250)
    return [_case("running_string", [g[0:OV_MAXLEN], g[OV_MAXLEN - 50:OV_MAXLEN + 250]], pairs=[(0, 2), (2, 0), (3, 1)], relax=True)]


@functools.lru_cache(maxsize=None)
def families(full=True):
    """{family: [case]}; the relax family is split in three so that no test exceeds the budget of long pairs"""
    fam = {"limit": _limit(full), "strips": _strips(), "ties": _ties(full), "clip": _clip(), "params": _params()}
    if full:
        fam["relax_limit"] = _relaxed(fam["limit"], "relax") + _running_string()
        fam["relax_ties"] = _relaxed(fam["ties"], "relax")
        fam["relax_clip"] = _relaxed(fam["clip"], "relax")
    for name, cases in fam.items():
        assert len({c["name"] for c in cases}) == len(cases)
        assert big_pairs(cases) <= BIG_PAIR_BUDGET, name
        cap = OV_MAXLEN if full else GOLDEN_MAXLEN
        assert all(1 <= len(x) <= cap for c in cases for x in c["contigs"]), name
    return fam


STRICT = ("limit", "strips", "ties", "clip", "params")
RELAXED = ("relax_limit", "relax_ties", "relax_clip")


def big_pairs(cases):
    """distinct evaluated pairs in which both nodes exceed BIG bases"""
    seen = set()
    for c in cases:
        nd = nodes_of(c["contigs"])
        seen |= {(nd[i], nd[j], c["params"], c["relax"]) for i, j in c["pairs"] if len(nd[i]) > BIG and len(nd[j]) > BIG}
    return len(seen)


def golden_sets():
    """(name, contigs, params) of every strict-mode case at the 2-kb scale, in a fixed order: what evaluate_edge_kat() feeds to the
    reference's driver, which evaluates all ordered node pairs of a set"""
    fam = families(False)
    return [("%s/%s" % (f, c["name"]), c["contigs"], c["params"]) for f in STRICT for c in fam[f]]


@functools.lru_cache(maxsize=None)
def _oracle(s1, s2, params, relax):
    from oracle import c_oracle as CO
    return CO.overlap_evaluate(s1, s2, params, relax=relax)


def expected(case):
    """the oracle's answer (dict of all result fields) for every pair of the case, in order; each distinct evaluation runs once"""
    nd = nodes_of(case["contigs"])
    return [_oracle(nd[i], nd[j], case["params"], case["relax"]) for i, j in case["pairs"]]


def expected_all(cases, threads=8):
    """[expected(c) for c in cases], the distinct evaluations spread over a few threads (the C oracle runs outside the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    jobs = {}
    for c in cases:
        nd = nodes_of(c["contigs"])
        for i, j in c["pairs"]:
            jobs[(nd[i], nd[j], c["params"], c["relax"])] = None
    order = sorted(jobs, key=lambda k: -len(k[0]) * len(k[1]))                          # longest first
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda k: _oracle(*k), order))
    return [expected(c) for c in cases]


# ---- non-vacuity --------------------------------------------------------------------------------------------------------------
def counts(cases, results):
    """the counted properties of the expected `results` (one list of result dicts per case)"""
    n = dict.fromkeys(TOTALS, 0)
    for c, rs in zip(cases, results):
        nd = nodes_of(c["contigs"])
        assert len(rs) == len(c["pairs"])
        for (i, j), r in zip(c["pairs"], rs):
            n["nclip"] += r["nclip"] > 0
            n["second_first"] += r["res"] != 0 and r["first_goes_first"] == 0
            n["contained"] += r["contained"] == 1
            n["containment"] += r["containment"] == 1
            n["res0"] += r["res"] == 0
            n["res1"] += r["res"] == 1
            n["res2"] += r["res"] == 2
            n["both_8189"] += min(len(nd[i]), len(nd[j])) >= 8189
            n["single_base"] += min(len(nd[i]), len(nd[j])) == 1
    return n


TOTALS = {"nclip": 10, "second_first": 10, "contained": 10, "containment": 5, "res0": 20, "res1": 5, "res2": 20, "both_8189": 6,
          "single_base": 4}
TIES_CLASS_1_2 = 8          # in the ties family: pairs of class 1 or 2, whose compared fields depend on which of the equal cells won
MINIMUM = {
    "limit": {"both_8189": 6, "single_base": 4, "contained": 2, "containment": 2, "res2": 6, "res0": 6},
    "strips": {"res2": 20, "second_first": 10, "res0": 20},
    "ties": {"contained": 6, "containment": 2, "res2": TIES_CLASS_1_2},
    "clip": {"nclip": 10},
    "params": {"res1": 5, "contained": 2, "containment": 2},
    "relax_limit": {"res2": 20},
    "relax_ties": {"res2": 20},
    "relax_clip": {"res2": 20, "nclip": 10},
}


def check_minimum(family, cases, results):
    got = counts(cases, results)
    for k, v in MINIMUM[family].items():
        assert got[k] >= v, (family, k, got[k], v)
    return got
