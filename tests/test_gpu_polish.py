"""The polish kernel (gf_fill_polish_dev, csrc/fill_polish.hip) against its host twin (gappadder_amd/polish.py) through the C ABI —
records, statistics and polished bytes equal, per gap and order-free in `off` — on hand-built pools and contig lists: contigs of 300 to
1 300 bases with pools of 40 to 250 sampled rows (0.5 % substitutions, both strands, overhanging either contig end) and edits planted in
the fill; a near repeat and an exact tandem repeat; an empty pool; an open gap; a contig with an N; a word whose span the contig does not
carry; a contig of exactly the kernel's longest length and one a base longer, each with a tiny pool; and, the kernel taking its votes in
passes of 1 024 body columns, an edit in the last column before every pass boundary and in the first after it.  L = 150, and L = 100 with
N masks; seeds of 12, 16, 20 and 32 bases; exact anchors and the pick table; forward and reverse words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A_LONG, A_SHORT = 30, 15
VCHUNK = 1024       # fill_polish.hip PL_VCHUNK
MAX_CONTIG = 8192   # GF_PL_MAX_CONTIG
# seed -> (max_mismatch at L = 150, at L = 100, min_overlap, min_votes): floor(L / seed) > max_mismatch
PARAMS = {12: (4, 4, 40, 1), 16: (4, 4, 48, 2), 20: (4, 4, 60, 2), 32: (3, 2, 48, 3)}
KINDS = ["plain", "plain", "near", "tandem", "plain", "empty", "open", "boundary", "plain", "non_acgt", "at_max", "plain", "over_max", "mismatch",
         "plain", "near", "tandem", "boundary"]
_CASES, _TWINS = {}, {}


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def _sub(text, at, step=1):
    return text[:at] + _other(text[at], step) + text[at + 1:]


def _word(a, span, ci, rev):
    return (a << 56) | (min(span + 1, 0xFFFFFF) << 32) | ((0x7FFFFFFF - ci) << 1) | int(rev)


def _reads(rng, truth, n_rows, L, masked, where=None):
    """Rows of `truth`, either strand: sampled anywhere with 0.5 % substitutions and, when masked, a quarter with one N; or exact copies at
    the offsets `where`."""
    from gappadder_amd.pick_contigs import revcomp
    out = []
    for i in range(n_rows):
        o = int(rng.integers(0, len(truth) - L + 1)) if where is None else where[i]
        r = list(truth[o:o + L])
        for p in np.nonzero(rng.random(L) < (0.005 if where is None else 0.0))[0]:
            r[p] = _other(r[p], int(rng.integers(1, 4)))
        if masked and where is None and rng.integers(0, 4) == 0:
            r[int(rng.integers(0, L))] = "N"
        r = "".join(r)
        out.append(revcomp(r) if rng.integers(0, 2) else r)
    return out


def _build(L, masked, style, seed):
    """One run's input (cached): per gap its flanks, stored contig, stored body, reads; the contig list with decoys and tombstones; the
    words and pick entries; what locate has to answer."""
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
        n_rows, where, edits = int(rng.integers(40, 251)), None, []
        if kind == "near":                                    # two copies of 150 bases that differ at 50 and 99; an error planted in copy 1
            rep = _seq(rng, 150)
            body = _seq(rng, 70) + rep + _seq(rng, 90) + _sub(_sub(rep, 50), 99) + _seq(rng, 60)
            edits = [70 + 50] if g % 2 else []
            n_rows = 200
        elif kind == "tandem":
            body = _seq(rng, 80) + _seq(rng, 130) * 4 + _seq(rng, 80)
            n_rows = 200
        elif kind == "boundary":                              # a body of more than one pass of vote columns
            body = _seq(rng, 1300 - left_n - right_n)
            n_rows = 250
        elif kind in ("at_max", "over_max"):
            body = _seq(rng, MAX_CONTIG + (kind == "over_max") - left_n - right_n)
        else:
            body = _seq(rng, int(rng.integers(300, 1100)) - left_n - right_n if kind != "empty" else 400)
            edits = sorted(int(x) for x in rng.choice(len(body), 4, replace=False))
        truth = lf + body + rf
        n = left_n + len(body) + right_n
        # the stored contig's body [sb0, sb1) and the pass boundaries in it, mapped back to the natural orientation of `body`
        sb0 = right_n if rev else left_n
        if kind in ("boundary", "at_max", "over_max"):
            cols = [sb0 + VCHUNK * k + e for k in range(1, (len(body) - 1) // VCHUNK + 1) for e in (-1, 0)]
            edits = sorted((n - 1 - c if rev else c) - left_n for c in cols)
            if kind != "boundary":                            # a tiny pool: three rows over every planted pair
                where = [100 + e - L // 2 + d for e in edits[::2] for d in (-20, 0, 20)]
                n_rows = len(where)
        fill = body
        for e in edits:
            fill = _sub(fill, e, 1 + e % 3)
        contig = lf[-left_n:] + fill + rf[:right_n]
        if kind == "non_acgt":
            contig = contig[:left_n + 40] + "N" + contig[left_n + 41:]
        reads = _reads(rng, truth, 0 if kind == "empty" else n_rows, L, masked, where)
        stored = revcomp(contig) if rev else contig
        sb = (n - left_n - len(body), n - left_n) if rev else (left_n, left_n + len(body))
        assert sb[0] == sb0
        gaps.append({"kind": kind, "flanks": (lf, rf), "stored": stored, "body": sb, "rev": rev, "a": a, "reads": reads, "n_edits": len(edits),
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
    mm_150, mm_100, mo, mv = PARAMS[s]
    return s, (mm_150 if L == 150 else mm_100), mo, mv


def _twin(case, L, masked, style, s):
    """(records with off = 0, {gap: polished text}, stats, the placements of every gap) from the twin (cached per input and seed length)."""
    key = (id(case), s)
    if key in _TWINS:
        return _TWINS[key]
    from gappadder_amd import _lib as B
    from gappadder_amd import polish as PL
    from gappadder_amd import read_support as RS
    prm = _params(s, L)
    want, texts, where = np.zeros(len(case["gaps"]), dtype=B.FILL_POLISH), {}, {}
    stats = dict.fromkeys(PL.STAT_KEYS, 0)
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
        if body is None:
            stats["mismatches"] += 1
            continue
        reads = G["reads"] if masked else [r.replace("N", "A") for r in G["reads"]]      # without the mask words an N of a read is the base A
        texts[g], want[g], where[g] = PL.polish_host(reads, G["stored"], body[0], body[1], *prm, detail=True)
        f = int(want[g]["flags"])
        stats["skipped_long"] += bool(f & B.PL_F_LONG)
        stats["skipped_non_acgt"] += bool(f & B.PL_F_NON_ACGT)
        stats["gaps"] += not f
        stats["changed"] += int(want[g]["n_changed"])
        stats["placed"] += int(want[g]["reads_placed"])
        stats["ambiguous"] += int(want[g]["reads_ambiguous"])
        stats["bases"] += len(G["stored"])
    _TWINS[key] = (want, texts, stats, where)
    return _TWINS[key]


def _run_device(case, L, masked, style, prm, base_cap=None):
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
    reads = [r for G in gaps for r in G["reads"]]
    off = np.cumsum([0] + [len(G["reads"]) for G in gaps]).astype(np.uint64)
    packed, nm = GapFill.pack_reads(reads, L, with_mask=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_pool = dev(np.concatenate([packed.reshape(-1), np.zeros(64, dtype=np.uint8)]))
    d_nm = dev(nm.view(np.int32)) if masked else None
    d_off, d_ctg, d_seq = dev(off.view(np.int64)), dev(ctg.view(np.uint8)), dev(np.frombuffer(seq, dtype=np.uint8))
    d_n = torch.tensor([n + 3], dtype=torch.int32, device="cuda")             # the counter counts records beyond the capacity
    d_best = dev(np.array(case["words"], dtype=np.uint64).view(np.int64))
    d_pick = None
    if style == "pick":
        pk = np.zeros(n, dtype=B.CTG_PICK)
        for ci, p in case["picks"].items():
            pk[ci] = p
        d_pick = dev(pk.view(np.uint8))
    if base_cap is None:                                                      # exactly what the closed gaps' contigs take
        base_cap = sum(len(G["stored"]) for g, G in enumerate(gaps) if case["words"][g] and case["expect"][g] != "mismatch")
    d_out = torch.full((n_gaps * B.FILL_POLISH.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    d_bases = torch.full((base_cap + 256,), 0x2E, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B.PL_WORDS,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = B.lib().gf_fill_polish_dev(gf.handle, d_pool.data_ptr(), d_nm.data_ptr() if masked else None, d_off.data_ptr(), len(reads), L,
                                    d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), d_best.data_ptr(),
                                    d_pick.data_ptr() if d_pick is not None else None, A_LONG, A_SHORT, *prm, d_out.data_ptr(),
                                    d_bases.data_ptr(), base_cap, d_st.data_ptr())
    assert rc == 0, (rc, B.lib().gf_last_error(gf.handle))
    gf.sync()
    return np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.FILL_POLISH), d_bases.cpu().numpy().tobytes(), d_st.cpu().numpy(), gf, base_cap


def _cases_are_there(case, want, texts, where, L):
    """What the cases are there for, from the twin alone."""
    from gappadder_amd import _lib as B
    gaps = case["gaps"]
    by_kind = {}
    for g, G in enumerate(gaps):
        by_kind.setdefault(G["kind"], []).append(g)
    assert sum(int(r["n_changed"]) for r in want) > 0 and sum(int(r["reads_ambiguous"]) for r in want) > 0
    assert sum(int(r["n_uncovered"]) for r in want) > 0
    placed = [(w, len(gaps[g]["stored"])) for g in where for w in where[g] if w not in (None, "ambiguous")]
    assert any(w[1] < 0 for w, n in placed) and any(w[1] + L > n for w, n in placed) and {w[0] for w, _ in placed} == {0, 1}
    for g in by_kind["tandem"]:
        assert int(want[g]["reads_ambiguous"]) > 0 and int(want[g]["n_uncovered"]) > 0, want[g]
    for g in by_kind["near"]:
        assert int(want[g]["n_changed"]) >= gaps[g]["n_edits"]
    for g in by_kind["boundary"] + by_kind["at_max"]:         # every planted pair around a pass boundary is repaired: the passes see all votes
        sb0, sb1 = gaps[g]["body"]
        assert sb1 - sb0 > VCHUNK and int(want[g]["n_changed"]) >= gaps[g]["n_edits"] > 0 and int(want[g]["flags"]) == 0
        cols = [sb0 + VCHUNK * k + e for k in range(1, (sb1 - sb0 - 1) // VCHUNK + 1) for e in (-1, 0)]
        assert len(cols) == gaps[g]["n_edits"] and all(texts[g][c] != gaps[g]["stored"][c] for c in cols)
    (g,) = by_kind["at_max"]
    assert len(gaps[g]["stored"]) == MAX_CONTIG == B.PL_MAX_CONTIG and gaps[g]["n_edits"] == 14
    (g,) = by_kind["over_max"]
    assert len(gaps[g]["stored"]) == MAX_CONTIG + 1 and int(want[g]["flags"]) == B.PL_F_LONG and texts[g] == gaps[g]["stored"]
    (g,) = by_kind["non_acgt"]
    assert int(want[g]["flags"]) == B.PL_F_NON_ACGT and texts[g] == gaps[g]["stored"]
    (g,) = by_kind["empty"]
    assert int(want[g]["n_uncovered"]) == int(want[g]["n_cols"]) > 0 and texts[g] == gaps[g]["stored"]
    (g,) = by_kind["open"]
    assert case["words"][g] == 0 and not want[g].tobytes().strip(b"\0")


@pytest.mark.parametrize("style", ["exact", "pick"])
@pytest.mark.parametrize("L,masked", [(150, False), (100, True)])
@pytest.mark.parametrize("s", sorted(PARAMS))
def test_kernel_equals_the_twin(s, L, masked, style):
    from gappadder_amd import polish as PL
    case = _build(L, masked, style, 7000 + L)
    want, texts, stats, where = _twin(case, L, masked, style, s)
    _cases_are_there(case, want, texts, where, L)
    got, bases, st, _, base_cap = _run_device(case, L, masked, style, _params(s, L))
    assert PL.stats_of(st) == stats and stats["mismatches"] == (1 if style == "exact" else 0) and stats["bases"] == base_cap
    bad, spans = [], []
    for g in range(len(want)):                                # every gap: the record but for `off`, and the bytes at `off`
        a, b = got[g].copy(), want[g].copy()
        o, n = int(a["off"]), int(a["len"])
        a["off"] = 0
        if a.tobytes() != b.tobytes() or (g in texts and bases[o:o + n].decode() != texts[g]) or (g not in texts and (o or n)):
            bad.append(g)
        if g in texts:
            spans.append((o, o + n))
    assert not bad, [(g, case["gaps"][g]["kind"], got[g], want[g]) for g in bad[:4]]
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == base_cap and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    assert set(bases[base_cap:]) == {0x2E}                    # nothing beyond what was handed out


def test_arguments_and_the_base_buffers_capacity():
    from gappadder_amd import _lib as B
    from gappadder_amd import polish as PL
    import torch
    case = _build(150, False, "exact", 7150)
    want, texts, stats, _ = _twin(case, 150, False, "exact", 16)
    # a buffer that takes none of the contigs: every closed gap is flagged, nothing is written, the counts are still the twin's
    got, bases, st, gf, _ = _run_device(case, 150, False, "exact", _params(16, 150), base_cap=100)
    dev = PL.stats_of(st)
    assert dev == dict(stats, overflow=len(texts)) and dev["bases"] > 100 and set(bases) == {0x2E}
    for g in texts:
        assert int(got[g]["flags"]) == int(want[g]["flags"]) | B.PL_F_OVERFLOW and int(got[g]["len"]) == 0 and int(got[g]["off"]) == 0
        assert all(int(got[g][f]) == int(want[g][f]) for f in ("n_cols", "n_changed", "n_uncovered", "reads_placed", "reads_ambiguous"))
    lib = B.lib()
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = z.data_ptr()
    args = lambda s=16, mm=4, mo=48, mv=2, a_long=30, a_short=15: (gf.handle, p, None, p, 0, 150, p, p, 0, p, p, None, a_long, a_short, s, mm, mo, mv,
                                                                   p, p, 0, p)
    for kw in (dict(s=11), dict(s=33), dict(mm=-1), dict(mm=16), dict(mo=15), dict(mo=151), dict(mv=0), dict(s=32, mm=4), dict(s=20, mm=7)):
        assert lib.gf_fill_polish_dev(*args(**kw)) == B.GF_E_UNSUPPORTED, kw
    assert lib.gf_fill_polish_dev(*args(a_long=40)) == B.GF_E_INVAL and lib.gf_fill_polish_dev(*args(a_long=30, a_short=30)) == B.GF_E_INVAL
