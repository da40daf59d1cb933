"""The pair-span kernel (gf_fill_pairs_dev, csrc/fill_pairs.hip) against its host twin (gappadder_amd/pair_span.py) through the C ABI —
records and statistics equal — on hand-built contig lists and per-library pools of read PAIRS sampled FR on each gap's truth (0.5 %
substitutions, mates dropped here and there): contigs of 300 to 1 300 bases with pools of 20 to 150 pairs; a fill with 60 bases missing,
one with an inverted segment, an exact tandem repeat; pools of exactly 256, 257 and about 700 rows (a batch is 256 rows: mates in
different batches); id slices with only side-0 or only side-1 rows, and slices whose first and last pair are complete (the mate is the
first / last id of its segment); pairs planted so that a span is clipped at column 0 and one ends exactly at n (the difference array's
last entry); an empty pool; an open gap; a contig with an N; a word whose span the contig does not carry; a contig of exactly the
kernel's longest length and one a base longer; tombstones and decoys in the contig list.  Two libraries with different (mean, sd, z),
one call each, into the two planes of one record array.  L = 150, and L = 100 with N masks; seeds of 12, 16 and 32 bases; exact
anchors and the pick table; forward and reverse words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A_LONG, A_SHORT = 30, 15
MAX_CONTIG = 8192   # GF_PL_MAX_CONTIG
BATCH = 256         # rows of one batch of the kernel's place phase at both read lengths
LIBS = [(260, 20, 3), (450, 35, 2)]     # (is_mean, is_sd, z) per library
# seed -> (max_mismatch at L = 150, at L = 100, min_overlap): floor(L / seed) > max_mismatch
PARAMS = {12: (4, 4, 40), 16: (4, 4, 48), 32: (3, 2, 48)}
KINDS = ["plain", "deletion", "rows256", "tandem", "plain", "empty", "open", "rows700", "side0", "non_acgt", "at_max", "inverted", "over_max",
         "mismatch", "rows257", "side1", "deletion", "plain"]
_CASES, _TWINS = {}, {}


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def _word(a, span, ci, rev):
    return (a << 56) | (min(span + 1, 0xFFFFFF) << 32) | ((0x7FFFFFFF - ci) << 1) | int(rev)


def _noisy(rng, read, masked, exact):
    r = list(read)
    if not exact:
        for p in np.nonzero(rng.random(len(r)) < 0.005)[0]:
            r[p] = _other(r[p], int(rng.integers(1, 4)))
        if masked and rng.integers(0, 4) == 0:
            r[int(rng.integers(0, len(r)))] = "N"
    return "".join(r)


def _pool(rng, truth, n_pairs, L, mean, sd, masked, planted=(), sides=(0, 1), keep_all=False):
    """([read ids], [reads]) of one gap and one library in the pool's order (mate side, then pair): n_pairs FR pairs sampled on `truth`
    with inserts around (mean, sd), the forward mate on either side at random, about a tenth of the mates dropped — never one of the
    first or the last pair —, then the `planted` (forward mate's start, insert) pairs as exact copies; sides: the mate sides kept."""
    from gappadder_amd.pick_contigs import revcomp
    numbers = np.sort(rng.choice(20000, n_pairs + len(planted), replace=False)).tolist()
    rows = []
    for k, pair in enumerate(numbers):
        exact = k >= n_pairs
        if exact:
            p, ins = planted[k - n_pairs]
        else:
            ins = int(np.clip(np.rint(rng.normal(mean, sd)), L, len(truth)))
            p = int(rng.integers(0, len(truth) - ins + 1))
        reads = [truth[p:p + L], revcomp(truth[p + ins - L:p + ins])]
        flip = int(rng.integers(0, 2))
        drop = -1 if (keep_all or exact or k in (0, n_pairs - 1) or rng.integers(0, 10)) else int(rng.integers(0, 2))
        for m in range(2):
            if m != drop and (m ^ flip) in sides:
                rows.append((2 * pair + (m ^ flip), _noisy(rng, reads[m], masked, exact)))
    rows.sort(key=lambda x: (x[0] & 1, x[0] >> 1))
    return [r for r, _ in rows], [s for _, s in rows]


def _build(L, masked, style, seed):
    """One run's input (cached): per gap its flanks, stored contig, stored body and per library (ids, reads); the contig list with decoys
    and tombstones; the words and pick entries; what locate has to answer."""
    key = (L, masked, style, seed)
    if key in _CASES:
        return _CASES[key]
    from gappadder_amd.pick_contigs import revcomp
    rng = np.random.default_rng(seed)
    gaps = []
    for g, kind in enumerate(KINDS):
        if kind == "mismatch" and style != "exact":
            kind = "plain"
        rev, a = bool(g % 2), (A_LONG if g % 4 < 2 else A_SHORT)
        lf, rf = _seq(rng, 100), _seq(rng, 100)
        left_n, right_n = 60 + g % 7, 55 + g % 5
        n_pairs = [int(rng.integers(20, 151)), int(rng.integers(20, 61))]
        sides, keep_all = (0, 1), False
        if kind == "tandem":
            body = _seq(rng, 80) + _seq(rng, 170) * 3 + _seq(rng, 80)
        elif kind in ("at_max", "over_max"):
            body = _seq(rng, MAX_CONTIG + (kind == "over_max") - left_n - right_n)
            n_pairs = [40, 20]
        elif kind in ("rows256", "rows257", "rows700"):
            body = _seq(rng, 1300 - left_n - right_n)
            n_pairs[0], keep_all = {"rows256": 125, "rows257": 126, "rows700": 347}[kind], True      # + the three planted pairs
        elif kind == "deletion":                              # a fill short enough for the pairs of both libraries to span
            body = _seq(rng, 260)
        elif kind == "inverted":                              # ... and one whose inverted half holds whole reads
            body = _seq(rng, 800)
        else:
            body = _seq(rng, int(rng.integers(300, 1100)) - left_n - right_n)
        if kind in ("side0", "side1"):
            sides = (int(kind[-1]),)
        truth = lf + body + rf
        fill = body
        if kind == "deletion":
            x = len(body) // 2
            fill = body[:x] + body[x + 60:]
        elif kind == "inverted":
            x, y = len(body) // 4, 3 * len(body) // 4
            fill = body[:x] + revcomp(body[x:y]) + body[y:]
        contig = lf[-left_n:] + fill + rf[:right_n]
        n = len(contig)
        if kind == "non_acgt":
            contig = contig[:left_n + 40] + "N" + contig[left_n + 41:]
        t0 = 100 - left_n                                      # the truth's coordinate of the contig's first base
        pools = []
        for l, (mean, sd, _) in enumerate(LIBS):
            planted = []
            if l == 0 and fill is body and kind not in ("empty", "side0", "side1"):
                # spans clipped at column 0, starting exactly there, and ending exactly at n (either one, by the stored orientation)
                planted = [(t0 - 20, mean), (t0, mean), (t0 + n - mean, mean)]
            ids, reads = _pool(rng, truth, 0 if kind == "empty" else n_pairs[l], L, mean, sd, masked, planted, sides, keep_all)
            if kind == "rows257" and l == 0:                   # 129 pairs without the last row: the last pair's mate is absent
                ids, reads = ids[:-1], reads[:-1]
            pools.append((ids, reads))
        stored = revcomp(contig) if rev else contig
        sb = (n - left_n - len(fill), n - left_n) if rev else (left_n, left_n + len(fill))
        gaps.append({"kind": kind, "flanks": (lf, rf), "stored": stored, "body": sb, "rev": rev, "a": a, "pools": pools,
                     "decoys": [_seq(rng, int(rng.integers(20, 120))) for _ in range(int(rng.integers(0, 3)))]})
    recs, words, picks, expect = [], [0] * len(gaps), {}, [None] * len(gaps)
    for g in rng.permutation(len(gaps)).tolist():
        G = gaps[g]
        recs += [(g, d) for d in G["decoys"]]
        if g % 3 == 0:
            recs.append((g, None))                            # a tombstone before the winner
        ci = len(recs)
        recs.append((g, G["stored"]))
        if G["kind"] == "open":
            continue
        sb0, sb1 = G["body"]
        words[g] = _word(G["a"], sb1 - sb0 + (7 if G["kind"] == "mismatch" else 0), ci, G["rev"])
        expect[g] = "mismatch" if G["kind"] == "mismatch" else (sb0, sb1)
        if style == "pick":
            lm, rm = min(40, sb0), min(35, len(G["stored"]) - sb1)
            picks[ci] = (sb1 + 1, sb0 - lm + 1, rm, lm, 1, G["a"], 0) if G["rev"] else (sb0 - lm + 1, sb1 + 1, lm, rm, 0, G["a"], 0)
    _CASES[key] = {"gaps": gaps, "recs": recs, "words": words, "picks": picks, "expect": expect}
    return _CASES[key]


def _params(s, L):
    mm_150, mm_100, mo = PARAMS[s]
    return s, (mm_150 if L == 150 else mm_100), mo


def _twin(case, L, masked, style, s):
    """(records [n_lib, n_gaps], a statistics dictionary per library, the placements per (library, gap)) from the twin (cached)."""
    key = (id(case), s)
    if key in _TWINS:
        return _TWINS[key]
    from gappadder_amd import _lib as B
    from gappadder_amd import pair_span as PS
    from gappadder_amd import read_support as RS
    prm = _params(s, L)
    want = np.zeros((len(LIBS), len(case["gaps"])), dtype=B.FILL_PAIRS)
    stats = [dict.fromkeys(PS.STAT_KEYS, 0) for _ in LIBS]
    where = {}
    for g, G in enumerate(case["gaps"]):
        w = case["words"][g]
        if not w:
            continue
        ci = 0x7FFFFFFF - ((w >> 1) & 0x7FFFFFFF)
        assert case["recs"][ci] == (g, G["stored"])
        entry = None
        if style == "pick":
            entry = np.zeros((), dtype=B.CTG_PICK)
            entry[()] = case["picks"][ci]
        body = RS.locate(w, G["stored"], G["flanks"], entry)
        assert body == (None if case["expect"][g] == "mismatch" else case["expect"][g]), (g, G["kind"], body, case["expect"][g])
        for l, (mean, sd, z) in enumerate(LIBS):
            if body is None:
                stats[l]["mismatches"] += 1
                continue
            ids, reads = G["pools"][l]
            reads = reads if masked else [r.replace("N", "A") for r in reads]      # without the mask words an N of a read is the base A
            want[l, g], where[l, g] = PS.pair_span_host(reads, ids, G["stored"], body[0], body[1], mean, sd, *prm, z=z, detail=True)
            PS.add_to_stats(stats[l], want[l, g])
    _TWINS[key] = (want, stats, where)
    return _TWINS[key]


def _run_device(case, L, masked, style, prm):
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    gaps, recs = case["gaps"], case["recs"]
    n_gaps, n = len(gaps), len(recs)
    gp = np.zeros(n_gaps, dtype=B.GAP)
    for g in range(n_gaps):
        gp[g] = (0, 20000 * (g + 1), 20000 * (g + 1) + 100, g + 1)
    gf = GapFill(0)
    gf.set_gaps(gp, 1, [G["flanks"] for G in gaps])
    ctg = np.zeros(n, dtype=B.CONTIG)
    o = 0
    for i, (g, s) in enumerate(recs):
        ctg[i] = (g, 31, 29, 1, len(s), 0, 0, o) if s is not None else (g, 31, 29, 3, 0, 5, 0, 0)
        o += len(s or "")
    seq = "".join(s or "" for _, s in recs).encode()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_ctg, d_seq = dev(ctg.view(np.uint8)), dev(np.frombuffer(seq, dtype=np.uint8))
    d_n = torch.tensor([n + 3], dtype=torch.int32, device="cuda")             # the counter counts records beyond the capacity
    d_best = dev(np.array(case["words"], dtype=np.uint64).view(np.int64))
    d_pick = None
    if style == "pick":
        pk = np.zeros(n, dtype=B.CTG_PICK)
        for ci, p in case["picks"].items():
            pk[ci] = p
        d_pick = dev(pk.view(np.uint8))
    plane = n_gaps * B.FILL_PAIRS.itemsize
    d_out = torch.full((len(LIBS) * plane,), 0x55, dtype=torch.uint8, device="cuda")
    stats, keep = [], []
    for l, (mean, sd, z) in enumerate(LIBS):
        reads = [r for G in gaps for r in G["pools"][l][1]]
        ids = np.array([r for G in gaps for r in G["pools"][l][0]], dtype=np.uint32)
        off = np.cumsum([0] + [len(G["pools"][l][0]) for G in gaps]).astype(np.uint64)
        packed, nm = GapFill.pack_reads(reads, L, with_mask=True)
        d_pool = dev(np.concatenate([packed.reshape(-1), np.zeros(64, dtype=np.uint8)]))
        d_nm = dev(nm.view(np.int32)) if masked else None
        d_off, d_ids = dev(off.view(np.int64)), dev(np.concatenate([ids, np.zeros(4, dtype=np.uint32)]).view(np.int32))
        d_scr = torch.full((len(reads) + 4,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        d_st = torch.full((B.PS_WORDS,), 7, dtype=torch.int32, device="cuda")
        keep += [d_pool, d_nm, d_off, d_ids, d_scr]
        torch.cuda.synchronize()
        rc = B.lib().gf_fill_pairs_dev(gf.handle, d_pool.data_ptr(), d_nm.data_ptr() if masked else None, d_off.data_ptr(), d_ids.data_ptr(),
                                       len(reads), L, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), d_best.data_ptr(),
                                       d_pick.data_ptr() if d_pick is not None else None, A_LONG, A_SHORT, *prm, mean, sd, z,
                                       d_scr.data_ptr(), d_out.data_ptr() + l * plane, d_st.data_ptr())
        assert rc == 0, (rc, B.lib().gf_last_error(gf.handle))
        gf.sync()
        assert int(d_scr[len(reads)]) == 0x7F7F7F7F                             # nothing beyond the pool's rows
        stats.append(d_st.cpu().numpy())
    got = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.FILL_PAIRS).reshape(len(LIBS), n_gaps)
    return got, stats, gf


def _cases_are_there(case, want, where, L):
    """What the cases are there for, from the twin alone."""
    from gappadder_amd import _lib as B
    gaps = case["gaps"]
    by_kind = {}
    for g, G in enumerate(gaps):
        by_kind.setdefault(G["kind"], []).append(g)
    for f in ("n_short", "n_long", "n_misoriented", "n_span", "n_unspanned", "min_cover"):
        assert int(want[f].sum()) > 0, f
    assert (want["pairs_complete"] > want["pairs_placed"]).any() and (want[1]["n_in_range"] > 0).any()
    clipped = at_zero = at_n = beyond = False
    for (l, g), rows in where.items():                        # the planted spans, among the placed pairs of library 0
        ids, n = gaps[g]["pools"][l][0], len(gaps[g]["stored"])
        at = {r: w for r, w in zip(ids, rows) if w not in (None, "ambiguous")}
        for r, w in at.items():
            if r & 1 or r + 1 not in at or at[r + 1][0] == w[0]:
                continue
            d_f, d_r = (w[1], at[r + 1][1]) if w[0] == 0 else (at[r + 1][1], w[1])
            clipped |= d_f < 0
            at_zero |= d_f == 0
            at_n |= d_r + L == n
            beyond |= d_r + L > n
    assert clipped and at_zero and at_n and beyond
    for g in by_kind["deletion"]:                             # 60 bases missing: the spanning pairs' mean insert is about 60 below is_mean
        assert int(want[1, g]["n_span"]) >= 5 and int(want[1, g]["span_insert_sum"]) // int(want[1, g]["n_span"]) < LIBS[1][0] - 30
    for g in by_kind["tandem"]:
        assert any(w == "ambiguous" for w in where[0, g])
    for g in by_kind["inverted"]:
        assert int(want[1, g]["n_misoriented"]) > 0             # (the mates of library 0 overlap: none lies apart from the other)
    for kind, rows in (("rows256", BATCH), ("rows257", BATCH + 1)):
        (g,) = by_kind[kind]
        assert int(want[0, g]["rows"]) == rows and int(want[0, g]["pairs_complete"]) > 100
    (g,) = by_kind["rows700"]
    assert int(want[0, g]["rows"]) > 2 * BATCH + 100 and int(want[0, g]["pairs_placed"]) > 300
    for kind in ("side0", "side1"):
        (g,) = by_kind[kind]
        assert {r & 1 for r in gaps[g]["pools"][0][0]} == {int(kind[-1])} and int(want[0, g]["rows"]) > 0 and int(want[0, g]["pairs_complete"]) == 0
        assert int(want[0, g]["n_unspanned"]) == int(want[0, g]["n_cols"]) > 0
    (g,) = by_kind["at_max"]
    assert len(gaps[g]["stored"]) == MAX_CONTIG == B.PL_MAX_CONTIG and int(want[0, g]["flags"]) == 0 and int(want[0, g]["pairs_placed"]) > 0
    (g,) = by_kind["over_max"]
    assert len(gaps[g]["stored"]) == MAX_CONTIG + 1 and int(want[0, g]["flags"]) == B.PS_F_LONG and int(want[0, g]["rows"]) > 0
    (g,) = by_kind["non_acgt"]
    assert int(want[1, g]["flags"]) == B.PS_F_NON_ACGT and int(want[1, g]["rows"]) > 0 and int(want[1, g]["n_cols"]) == 0
    (g,) = by_kind["empty"]
    assert int(want[0, g]["rows"]) == 0 and int(want[0, g]["n_unspanned"]) == int(want[0, g]["n_cols"]) > 0
    (g,) = by_kind["open"]
    assert case["words"][g] == 0 and not want[:, g].tobytes().strip(b"\0")
    for G in gaps:                                            # the first and the last pair of a sampled slice are complete
        ids = G["pools"][1][0]
        if G["kind"] in ("plain", "deletion", "tandem"):
            side1 = [r for r in ids if r & 1]
            assert side1[0] == ids[0] + 1 and side1[-1] - 1 in ids


@pytest.mark.parametrize("style", ["exact", "pick"])
@pytest.mark.parametrize("L,masked", [(150, False), (100, True)])
@pytest.mark.parametrize("s", sorted(PARAMS))
def test_kernel_equals_the_twin(s, L, masked, style):
    from gappadder_amd import pair_span as PS
    case = _build(L, masked, style, 9000 + L)
    want, stats, where = _twin(case, L, masked, style, s)
    _cases_are_there(case, want, where, L)
    got, st, _ = _run_device(case, L, masked, style, _params(s, L))
    for l in range(len(LIBS)):
        print("library %d: %s" % (l, PS.stats_of(st[l])))
        assert PS.stats_of(st[l]) == stats[l] and stats[l]["mismatches"] == (1 if style == "exact" else 0)
    bad = [(l, g) for l in range(len(LIBS)) for g in range(want.shape[1]) if got[l, g].tobytes() != want[l, g].tobytes()]
    assert not bad, [(l, g, case["gaps"][g]["kind"], got[l, g], want[l, g]) for l, g in bad[:4]]


def test_arguments():
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    import torch
    gf = GapFill(0)
    gp = np.zeros(1, dtype=B.GAP)
    gp[0] = (0, 1000, 1100, 1)
    gf.set_gaps(gp, 1, [("A" * 100, "C" * 100)])
    lib = B.lib()
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = z.data_ptr()
    args = lambda s=16, mm=4, mo=48, sd=30, zz=3, a_long=30, a_short=15: (gf.handle, p, None, p, p, 0, 150, p, p, 0, p, p, None, a_long, a_short,
                                                                         s, mm, mo, 400, sd, zz, p, p, p)
    assert lib.gf_fill_pairs_dev(*args()) == 0
    gf.sync()
    for kw in (dict(s=11), dict(s=33), dict(mm=-1), dict(mm=16), dict(mo=15), dict(mo=151), dict(zz=0), dict(zz=-1), dict(sd=-1),
               dict(s=32, mm=4), dict(s=20, mm=7)):
        assert lib.gf_fill_pairs_dev(*args(**kw)) == B.GF_E_UNSUPPORTED, kw
    assert lib.gf_fill_pairs_dev(*args(a_long=40)) == B.GF_E_INVAL and lib.gf_fill_pairs_dev(*args(a_long=30, a_short=30)) == B.GF_E_INVAL
