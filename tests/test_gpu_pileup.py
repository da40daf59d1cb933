"""The pile-up kernel (gf_fill_pileup_dev, csrc/fill_pileup.hip) against its host twin (gappadder_amd/pileup.py) through the C ABI — records
equal byte for byte but for `off`, the track entries at `off` equal, the spans tiling what was handed out, nothing written beyond — on
hand-built pools and contig lists made the way test_gpu_polish.py makes them: contigs of 300 to 1 300 bases with pools of 40 to 250
sampled rows (0.5 % substitutions, both strands, overhanging either contig end) and edits planted in the fill; a near repeat and an exact
tandem repeat; an empty pool; an open gap; a contig with an N; a word whose span the contig does not carry; decoys and tombstones in the
list.  On top, what this kernel alone can get wrong — it takes its votes in passes of 1 024 CONTIG columns and carries the open run of low
columns from pass to pass —: rows left out around a pass boundary (a low run across it), a contig of exactly the longest length tiled with
rows, with a single contested column before or after every pass boundary and rows left out across two of them, two more such contigs
(one stored reverse-complemented) with rows left out across EVERY one of the seven pass boundaries, a contig one base longer,
rows left out across both ends of the body (runs that start on its first and end on its last column, low flank columns beside them),
saturating counters, the track's capacity, the records-only mode and the arguments.  L = 150, and L = 100 with N masks; seeds of 12, 16
and 32 bases; exact anchors and the pick table; forward and reverse words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A_LONG, A_SHORT = 30, 15
VCHUNK = 1024       # fill_pileup.hip PU_VCHUNK
MAX_CONTIG = 8192   # GF_PL_MAX_CONTIG
MIN_DEPTH, MIN_AGREE = 3, 80
# seed -> (max_mismatch at L = 150, at L = 100, min_overlap): floor(L / seed) > max_mismatch
PARAMS = {12: (4, 4, 40), 16: (4, 4, 48), 32: (3, 2, 48)}
KINDS = ["plain", "plain", "near", "tandem", "plain", "empty", "open", "boundary", "plain", "non_acgt", "at_max", "plain", "over_max", "mismatch",
         "plain", "near", "tandem", "boundary", "edges", "edges", "all_straddled", "all_straddled"]
STRADDLED = (3, 6)  # at_max: the pass boundaries rows are left out across; the others get one contested column
_CASES, _TWINS = {}, {}


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def _sub(text, at, step=1):
    return text[:at] + _other(text[at], step) + text[at + 1:]


def _word(a, span, ci, rev):
    return (a << 56) | (min(span + 1, 0xFFFFFF) << 32) | ((0x7FFFFFFF - ci) << 1) | int(rev)


def _reads(rng, truth, n_rows, L, masked, where=None, avoid=()):
    """Rows of `truth`, either strand: sampled anywhere — but touching none of the `avoid` windows — with 0.5 % substitutions and, when
    masked, a quarter with one N; or exact copies at the offsets `where`."""
    from gappadder_amd.pick_contigs import revcomp
    out = []
    while len(out) < (n_rows if where is None else len(where)):
        o = int(rng.integers(0, len(truth) - L + 1)) if where is None else where[len(out)]
        if where is None and any(o < hi and lo < o + L for lo, hi in avoid):
            continue
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
        n_rows, where, edits, holes = int(rng.integers(40, 251)), None, [], []       # holes: windows of STORED columns no row may touch
        if kind == "near":                                    # two copies of 150 bases that differ at 50 and 99; an error planted in copy 1
            rep = _seq(rng, 150)
            body = _seq(rng, 70) + rep + _seq(rng, 90) + _sub(_sub(rep, 50), 99) + _seq(rng, 60)
            edits = [70 + 50] if g % 2 else []
            n_rows = 200
        elif kind == "tandem":
            body = _seq(rng, 80) + _seq(rng, 130) * 4 + _seq(rng, 80)
            n_rows = 200
        elif kind == "boundary":                              # a contig of more than one pass of vote columns
            body = _seq(rng, 1300 - left_n - right_n)
            n_rows = 250
        elif kind in ("at_max", "over_max", "all_straddled"):
            body = _seq(rng, MAX_CONTIG + (kind == "over_max") - left_n - right_n)
        else:
            body = _seq(rng, int(rng.integers(300, 1100)) - left_n - right_n if kind != "empty" else 400)
            edits = sorted(int(x) for x in rng.choice(len(body), 4, replace=False)) if kind != "edges" else []
        truth = lf + body + rf
        n = left_n + len(body) + right_n
        sb0 = right_n if rev else left_n
        sb1 = sb0 + len(body)
        natural = lambda c: n - 1 - c if rev else c           # a stored column on the contig as the truth reads
        if kind == "boundary":                                # rows left out across the pass boundary
            holes = [(VCHUNK - 8, VCHUNK + 8)]
        elif kind == "at_max":                                # one contested column before (odd k) or after (even k) the k-th boundary
            holes = [(VCHUNK * k - 7, VCHUNK * k + 9) for k in STRADDLED]
            edits = sorted(natural(VCHUNK * k - k % 2) - left_n for k in range(1, 8) if k not in STRADDLED)
        elif kind == "all_straddled":                         # rows left out across every pass boundary: an open run carried out of every pass
            holes = [(VCHUNK * k - 7, VCHUNK * k + 9) for k in range(1, 8)]
        elif kind == "edges":                                 # rows left out across either end of the body
            holes = [(sb0 - 20, sb0 + (5 if g % 2 else 25)), (sb1 - (25 if g % 2 else 5), sb1 + 20)]
            n_rows = 250
        avoid = [tuple(sorted((natural(lo) + 100 - left_n, natural(hi - 1) + 100 - left_n))) for lo, hi in holes]
        avoid = [(lo, hi + 1) for lo, hi in avoid]
        if kind in ("at_max", "all_straddled"):               # tiled: three rows deep wherever no row is left out
            where = [o for o in range(0, len(truth) - L + 1, L // 3) if not any(o < hi and lo < o + L for lo, hi in avoid)]
        elif kind == "over_max":
            where = [100, 4000, 8000]
        fill = body
        for e in edits:
            fill = _sub(fill, e, 1 + e % 3)
        contig = lf[-left_n:] + fill + rf[:right_n]
        if kind == "non_acgt":
            contig = contig[:left_n + 40] + "N" + contig[left_n + 41:]
        reads = _reads(rng, truth, 0 if kind == "empty" else n_rows, L, masked, where, avoid)
        stored = revcomp(contig) if rev else contig
        gaps.append({"kind": kind, "flanks": (lf, rf), "stored": stored, "body": (sb0, sb1), "rev": rev, "a": a, "reads": reads, "n_edits": len(edits),
                     "holes": holes, "decoys": [_seq(rng, int(rng.integers(20, 120))) for _ in range(int(rng.integers(0, 3)))]})
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
    return s, (mm_150 if L == 150 else mm_100), mo, MIN_DEPTH, MIN_AGREE


def _twin(case, L, masked, style, s):
    """(records with off = 0, {gap: entries}, stats, {gap: (placements, unsaturated counts)}) from the twin (cached per input and seed length)."""
    key = (id(case), s)
    if key in _TWINS:
        return _TWINS[key]
    from gappadder_amd import _lib as B
    from gappadder_amd import pileup as PU
    from gappadder_amd import read_support as RS
    prm = _params(s, L)
    want, tracks, detail = np.zeros(len(case["gaps"]), dtype=B.FILL_PILEUP), {}, {}
    stats = dict.fromkeys(PU.STAT_KEYS, 0)
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
        e, want[g], where, counts = PU.pileup_host(reads, G["stored"], body[0], body[1], *prm, detail=True)
        detail[g] = (where, counts)
        if e is not None:
            tracks[g] = e
        PU.add_stats(stats, want[g], len(G["stored"]))
    _TWINS[key] = (want, tracks, stats, detail)
    return _TWINS[key]


def _run_device(case, L, masked, style, prm, track_cap=None, track=True):
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
    if track_cap is None:                                                     # exactly what the piled-up gaps' contigs take
        track_cap = sum(len(G["stored"]) for g, G in enumerate(gaps) if case["words"][g] and case["expect"][g] != "mismatch"
                        and G["kind"] not in ("non_acgt", "over_max"))
    if not track:
        track_cap = 0
    d_out = torch.full((n_gaps * B.FILL_PILEUP.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    d_track = torch.full(((track_cap + 16) * 16,), 0x2E, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B.PU_WORDS,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = B.lib().gf_fill_pileup_dev(gf.handle, d_pool.data_ptr(), d_nm.data_ptr() if masked else None, d_off.data_ptr(), len(reads), L,
                                    d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), d_best.data_ptr(),
                                    d_pick.data_ptr() if d_pick is not None else None, A_LONG, A_SHORT, *prm, d_out.data_ptr(),
                                    d_track.data_ptr() if track else None, track_cap, d_st.data_ptr())
    assert rc == 0, (rc, B.lib().gf_last_error(gf.handle))
    gf.sync()
    entries = np.frombuffer(d_track.cpu().numpy().tobytes(), dtype="<u2").reshape(-1, 8)
    return np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.FILL_PILEUP), entries, d_st.cpu().numpy(), gf, track_cap


def _low(case, detail, g):
    """The low flag of every STORED column of gap g's contig (False outside the body), from the twin's unsaturated counts."""
    from gappadder_amd import pileup as PU
    from gappadder_amd.fill_rounds import _LUT
    G = case["gaps"][g]
    sb0, sb1 = G["body"]
    cc = _LUT[np.frombuffer(G["stored"].encode(), dtype=np.uint8)]
    unc, thin, con = PU._classes(detail[g][1][sb0:sb1], cc[sb0:sb1], MIN_DEPTH, MIN_AGREE)[:3]
    out = np.zeros(len(cc), dtype=bool)
    out[sb0:sb1] = unc | thin | con
    return out


def _cases_are_there(case, want, tracks, detail, L):
    """What the cases are there for, from the twin alone."""
    from gappadder_amd import _lib as B
    gaps = case["gaps"]
    by_kind = {}
    for g, G in enumerate(gaps):
        by_kind.setdefault(G["kind"], []).append(g)
    for f in ("n_uncovered", "n_thin", "n_contested", "n_minority", "n_one_strand", "reads_ambiguous", "low_run"):
        assert sum(int(r[f]) for r in want) > 0, f
    placed = [(w, len(gaps[g]["stored"])) for g in detail for w in detail[g][0] if w not in (None, "ambiguous")]
    assert any(w[1] < 0 for w, n in placed) and any(w[1] + L > n for w, n in placed) and {w[0] for w, _ in placed} == {0, 1}
    assert any(tracks[g][:, :4].any() and tracks[g][:, 4:].any() for g in tracks)          # both strands' counters
    assert any(tracks[g][:gaps[g]["body"][0]].any() and tracks[g][gaps[g]["body"][1]:].any() for g in tracks)     # votes on the flank columns
    for g in by_kind["tandem"]:
        assert int(want[g]["reads_ambiguous"]) > 0 and int(want[g]["n_uncovered"]) > 0, want[g]
    for g in by_kind["boundary"]:                             # a low run across the pass boundary, wholly inside the body
        low, (sb0, sb1) = _low(case, detail, g), gaps[g]["body"]
        assert sb0 < VCHUNK - 8 and VCHUNK + 8 < sb1 and low[VCHUNK - 8:VCHUNK + 8].all()
        lo, hi = VCHUNK - 8, VCHUNK + 8
        while low[lo - 1]:
            lo -= 1
        while low[hi]:
            hi += 1
        assert sb0 < lo and hi < sb1 and int(want[g]["low_run"]) >= hi - lo >= 16
    (g,) = by_kind["at_max"]
    low, (sb0, sb1) = _low(case, detail, g), gaps[g]["body"]
    assert len(gaps[g]["stored"]) == MAX_CONTIG == B.PL_MAX_CONTIG and int(want[g]["flags"]) == 0 and gaps[g]["n_edits"] == 5
    for k in range(1, 8):
        c = VCHUNK * k
        if k in STRADDLED:                                    # a run across the boundary ...
            assert low[c - 7:c + 9].all()
        else:                                                 # ... or of exactly one column: the last before it (odd k) or the first behind it
            assert low[c - 3:c + 3].tolist() == [False, False, k % 2 == 1, k % 2 == 0, False, False], (k, low[c - 3:c + 3])
    runs = np.diff(np.nonzero(np.diff(np.concatenate([[0], low.astype(np.int8), [0]])))[0])[::2]
    assert sorted(runs)[-2] >= 16 and (runs == 1).sum() == 5 and int(want[g]["low_run"]) == runs.max()
    assert len(by_kind["all_straddled"]) == 2 and {gaps[g]["rev"] for g in by_kind["all_straddled"]} == {False, True}
    for g in by_kind["all_straddled"]:                        # seven separate runs, each across its boundary, each wholly inside the body
        low, (sb0, sb1) = _low(case, detail, g), gaps[g]["body"]
        assert len(gaps[g]["stored"]) == MAX_CONTIG and int(want[g]["flags"]) == 0
        spans = []
        for k in range(1, 8):
            lo, hi = VCHUNK * k - 7, VCHUNK * k + 9
            assert low[lo:hi].all()
            while low[lo - 1]:
                lo -= 1
            while low[hi]:
                hi += 1
            assert sb0 < lo < VCHUNK * k < hi < sb1 and (not spans or spans[-1][1] < lo)
            spans.append((lo, hi))
        longest = max(spans, key=lambda s: (s[1] - s[0], -s[0]))
        assert int(want[g]["low_run"]) >= longest[1] - longest[0] >= 16
        if int(want[g]["low_run"]) == longest[1] - longest[0]:
            assert int(want[g]["low_run_col"]) == longest[0] - sb0
    (g,) = by_kind["over_max"]
    assert len(gaps[g]["stored"]) == MAX_CONTIG + 1 and int(want[g]["flags"]) == B.PU_F_LONG and g not in tracks and int(want[g]["len"]) == 0
    (g,) = by_kind["non_acgt"]
    assert int(want[g]["flags"]) == B.PU_F_NON_ACGT and g not in tracks and int(want[g]["n_cols"]) > 0
    (g,) = by_kind["empty"]
    assert int(want[g]["n_uncovered"]) == int(want[g]["n_cols"]) == int(want[g]["low_run"]) > 0 and not tracks[g].any()
    (g,) = by_kind["open"]
    assert case["words"][g] == 0 and not want[g].tobytes().strip(b"\0")
    starts, ends = 0, 0
    for g in by_kind["edges"]:                                # runs on the first and on the last body column, low flank columns beside them
        low, (sb0, sb1) = _low(case, detail, g), gaps[g]["body"]
        depth = detail[g][1].sum(axis=1)
        assert low[sb0:sb0 + 5].all() and low[sb1 - 5:sb1].all() and (depth[sb0 - 20:sb0] < MIN_DEPTH).all() and (depth[sb1:sb1 + 20] < MIN_DEPTH).all()
        run0 = int(np.argmin(low[sb0:sb1]))                   # the run that starts on the first body column
        run1 = int(np.argmin(low[sb0:sb1][::-1]))
        starts += int(want[g]["low_run"]) == run0 and int(want[g]["low_run_col"]) == 0
        ends += int(want[g]["low_run"]) == run1 and int(want[g]["low_run_col"]) == sb1 - sb0 - run1
        assert int(want[g]["low_run"]) >= max(run0, run1) >= 25 and min(run0, run1) >= 5
    return starts, ends


def _compare(case, want, tracks, got, entries, handed_out):
    """Every gap: the record but for `off`, and the entries at `off`; the spans tile [0, handed_out); nothing beyond them is written."""
    bad, spans = [], []
    for g in range(len(want)):
        a, b = got[g].copy(), want[g].copy()
        o, n = int(a["off"]), int(a["len"])
        a["off"] = 0
        if a.tobytes() != b.tobytes() or (g in tracks and not (entries[o:o + n] == tracks[g]).all()) or (g not in tracks and (o or n)):
            bad.append(g)
        if g in tracks:
            spans.append((o, o + n))
    assert not bad, [(g, case["gaps"][g]["kind"], got[g], want[g]) for g in bad[:4]]
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == handed_out and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    assert (entries[handed_out:] == 0x2E2E).all()


@pytest.mark.parametrize("style", ["exact", "pick"])
@pytest.mark.parametrize("L,masked", [(150, False), (100, True)])
@pytest.mark.parametrize("s", sorted(PARAMS))
def test_kernel_equals_the_twin(s, L, masked, style):
    from gappadder_amd import pileup as PU
    case = _build(L, masked, style, 7000 + L)
    want, tracks, stats, detail = _twin(case, L, masked, style, s)
    _cases_are_there(case, want, tracks, detail, L)
    got, entries, st, _, cap = _run_device(case, L, masked, style, _params(s, L))
    assert PU.stats_of(st) == stats and stats["mismatches"] == (1 if style == "exact" else 0) and stats["entries"] == cap
    assert stats["skipped_long"] == stats["skipped_non_acgt"] == 1
    _compare(case, want, tracks, got, entries, cap)


def test_both_body_edges_carry_the_longest_run_somewhere():
    """Over the inputs of the parametrised test, a longest run that starts on the first body column and one that ends on the last."""
    starts = ends = 0
    for L, masked in ((150, False), (100, True)):
        case = _build(L, masked, "exact", 7000 + L)
        want, tracks, _, detail = _twin(case, L, masked, "exact", 16)
        a, b = _cases_are_there(case, want, tracks, detail, L)
        starts, ends = starts + a, ends + b
    assert starts > 0 and ends > 0


def test_track_capacity_one_entry_short_and_records_only():
    from gappadder_amd import _lib as B
    from gappadder_amd import pileup as PU
    case = _build(150, False, "exact", 7150)
    prm = _params(16, 150)
    want, tracks, stats, _ = _twin(case, 150, False, "exact", 16)
    full = stats["entries"]
    got, entries, st, _, cap = _run_device(case, 150, False, "exact", prm, track_cap=full - 1)
    dev = PU.stats_of(st)
    assert dev == dict(stats, overflow=1) and cap == full - 1
    flagged = [g for g in tracks if int(got[g]["flags"]) & B.PU_F_OVERFLOW]
    assert len(flagged) == 1
    (f,) = flagged
    assert int(got[f]["off"]) == 0 and int(got[f]["len"]) == 0 and int(got[f]["flags"]) == B.PU_F_OVERFLOW
    assert all(int(got[f][x]) == int(want[f][x]) for x in B.FILL_PILEUP.names if x not in ("off", "len", "flags"))
    # the others are the twin's and tile what was handed out but for the flagged contig's entries, which nobody wrote
    spans = []
    for g in tracks:
        if g == f:
            continue
        a = got[g].copy()
        o, n = int(a["off"]), int(a["len"])
        a["off"] = 0
        assert a.tobytes() == want[g].tobytes() and (entries[o:o + n] == tracks[g]).all(), (g, got[g], want[g])
        spans.append((o, o + n))
    spans.sort()
    holes = [(x[1], y[0]) for x, y in zip([(0, 0)] + spans, spans + [(full, full)]) if x[1] != y[0]]
    assert holes == [(holes[0][0], holes[0][0] + len(case["gaps"][f]["stored"]))]
    written = np.zeros(len(entries), dtype=bool)
    for o, e in spans:
        written[o:e] = True
    assert (entries[~written] == 0x2E2E).all()
    # records only: a null track with capacity 0 is a mode, not an overflow
    want0, tracks0, stats0 = want.copy(), {}, dict(stats, entries=0)
    want0["len"] = 0
    got, entries, st, _, _ = _run_device(case, 150, False, "exact", prm, track=False)
    assert PU.stats_of(st) == stats0 and got.tobytes() == want0.tobytes() and (entries == 0x2E2E).all()
    e, rec = PU.pileup_host(case["gaps"][0]["reads"], case["gaps"][0]["stored"], *case["gaps"][0]["body"], *prm, track=False)
    assert e is None and rec.tobytes() == want0[0].tobytes()


def test_counters_saturate_in_the_track_only():
    """65 540 identical rows at one offset of a 300-base contig: the expectation is written by hand."""
    from gappadder_amd import _lib as B
    from gappadder_amd import pileup as PU
    rng = np.random.default_rng(99)
    L, rows, at = 100, 65540, 120
    lf, rf, body = _seq(rng, 100), _seq(rng, 100), _seq(rng, 180)
    contig = lf[-60:] + body + rf[:60]                        # the body: columns 60..239; the rows cover 120..219
    case = {"gaps": [{"kind": "deep", "flanks": (lf, rf), "stored": contig, "body": (60, 240), "rev": False, "a": A_LONG,
                      "reads": [contig[at:at + L]] * rows, "decoys": []}],
            "recs": [(0, contig)], "words": [_word(A_LONG, 180, 0, False)], "picks": {}, "expect": [(60, 240)]}
    got, entries, st, _, cap = _run_device(case, L, False, "exact", _params(16, L))
    rec = got[0]
    assert cap == 300 and (int(rec["off"]), int(rec["len"]), int(rec["flags"]), int(rec["n_cols"])) == (0, 300, 0, 180)
    assert (int(rec["reads_placed"]), int(rec["reads_ambiguous"])) == (rows, 0) and int(rec["depth_sum"]) == rows * L
    assert (int(rec["n_uncovered"]), int(rec["n_thin"]), int(rec["n_contested"]), int(rec["n_minority"]), int(rec["n_one_strand"])) == (80, 0, 0, 0, 100)
    assert (int(rec["low_run"]), int(rec["low_run_col"]), int(rec["min_depth_seen"]), int(rec["min_depth_col"])) == (60, 0, 0, 0)
    expect = np.zeros((300, 8), dtype=np.uint16)
    for j in range(at, at + L):
        expect[j, "ACGT".index(contig[j])] = 65535
    assert (entries[:300] == expect).all() and (entries[300:] == 0x2E2E).all()
    assert PU.stats_of(st) == {"gaps": 1, "mismatches": 0, "skipped_long": 0, "skipped_non_acgt": 0, "placed": rows, "ambiguous": 0, "entries": 300,
                               "low": 80, "overflow": 0}


def test_arguments():
    from gappadder_amd import _lib as B
    import torch
    from gappadder_amd.hip_api import GapFill
    gf = GapFill(0)
    gp = np.zeros(1, dtype=B.GAP)
    gp[0] = (0, 20000, 20100, 1)
    gf.set_gaps(gp, 1, [("ACGT" * 25, "TGCA" * 25)])
    lib = B.lib()
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = z.data_ptr()
    args = lambda s=16, mm=4, mo=48, md=3, ma=80, a_long=30, a_short=15, track=p, cap=0: (
        gf.handle, p, None, p, 0, 150, p, p, 0, p, p, None, a_long, a_short, s, mm, mo, md, ma, p, track, cap, p)
    for kw in (dict(s=11), dict(s=33), dict(mm=-1), dict(mm=16), dict(mo=15), dict(mo=151), dict(md=0), dict(ma=0), dict(ma=101), dict(s=32, mm=4),
               dict(s=20, mm=7)):
        assert lib.gf_fill_pileup_dev(*args(**kw)) == B.GF_E_UNSUPPORTED, kw
    assert lib.gf_fill_pileup_dev(*args(a_long=40)) == B.GF_E_INVAL and lib.gf_fill_pileup_dev(*args(a_long=30, a_short=30)) == B.GF_E_INVAL
    assert lib.gf_fill_pileup_dev(*args(track=None, cap=8)) == B.GF_E_INVAL and lib.gf_fill_pileup_dev(*args(track=p + 8, cap=8)) == B.GF_E_INVAL
    gf.sync()
