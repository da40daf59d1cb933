"""The indel-aware polish kernel (gf_fill_polish_gapped_dev, csrc/fill_polish_gapped.hip) against its host twin
(gappadder_amd/polish_gapped.py) through the C ABI — records, statistics and polished bytes equal, per gap and order-free in `off` — on
hand-built pools and contig lists: contigs of 300 to 700 bases with pools of 40 to 150 rows and every case of the host tests (planted
insertions and deletions, a homopolymer and a tandem unit, an event in the anchor, a minority indel, indels at either edge of the body;
and, as a few hand-made rows each, the tie with a gapless candidate, the indel's cost of two, two touching events with unequal and
with equal votes, masked inserted bases);
an empty pool, an open gap, a word whose span the contig does not carry, a contig with an N; a contig of 1 300 bases with a deletion of
the last column before the kernel's vote-pass boundary and the first after it; contigs of 8 192 and 8 193 bases with a three-row pool over
one planted indel; 65 hand-made rows with 65 distinct insertions (the EVENTS flag) and 64 (no flag); five passing 16-base insertions (the
INS_CAP flag on the fifth); the base buffer exactly full and one byte short.  L = 150, and L = 100 with N masks; seeds of 12, 16 and 32
bases with max_indel 1, 8 and 16; exact anchors and the pick table; forward and reverse words."""
import numpy as np
import pytest

import polish_gapped_cases as C

pytestmark = pytest.mark.gpu

A_LONG, A_SHORT = 30, 15
VCHUNK = 768        # fill_polish_gapped.hip PLG_VCHUNK
MAX_CONTIG = 8192   # GF_PL_MAX_CONTIG
# (seed, max_indel) -> (max_mismatch at L = 150, at L = 100, min_overlap, min_votes): floor(L / seed) > max_mismatch
PARAMS = {(12, 1): (4, 4, 40, 2), (16, 8): (4, 4, 48, 2), (32, 16): (3, 2, 48, 3)}
KINDS = ["missing", "extra", "homopolymer", "tandem", "anchor", "minority", "ins_b0", "ins_b1", "del_b1", "plain", "empty", "open", "non_acgt",
         "boundary", "at_max", "over_max", "events65", "events64", "ins_cap", "mismatch", "extra", "missing", "tandem", "homopolymer",
         "tie", "cost", "overlap", "overlap_tie", "masked"]
_GAPS, _CASES, _TWINS = {}, {}, {}


def _word(a, span, ci, rev):
    return (a << 56) | (min(span + 1, 0xFFFFFF) << 32) | ((0x7FFFFFFF - ci) << 1) | int(rev)


def _avoid(*bases):
    return next(c for c in "ACGT" if c not in bases)


def _gap(rng, g, kind, L, masked):
    """One gap: flanks, the contig in its natural orientation (left_n anchor bases, the fill, right_n anchor bases), the reads."""
    from gappadder_amd.pick_contigs import revcomp
    lf, rf = C.seq(rng, 100), C.seq(rng, 100)
    left_n, right_n = 60 + g % 7, 55 + g % 5
    indel = kind in ("missing", "extra", "homopolymer", "tandem", "anchor", "minority", "ins_b0", "ins_b1", "del_b1")
    n_rows = int(rng.integers(110, 151)) if indel else int(rng.integers(40, 151))      # (an indel needs rows with a seed on either side of it)
    rev = bool(g % 2)
    mid = lambda: int(rng.integers(150, 250))
    fill_t = C.seq(rng, int(rng.integers(300, 400 if indel else 560)))    # the true fill; fill_c: what the contig has in its place
    fill_c, rows, anchor_c, extra = fill_t, None, None, {}
    natural = lambda fill: lf[-left_n:] + fill + rf[:right_n]             # the contig, or the truth, around a fill
    both = lambda texts: [x for t in texts for x in (t, revcomp(t))]
    if kind == "missing":
        at, gone = mid(), C.seq(rng, int(rng.integers(1, 9)))
        fill_t = fill_t[:at] + gone + fill_t[at:]
    elif kind == "extra":
        at = mid()
        fill_c = fill_t[:at] + C.seq(rng, int(rng.integers(1, 9))) + fill_t[at:]
    elif kind == "homopolymer":
        at = mid()
        fill_t = fill_t[:at - 1] + "C" + "A" * 7 + "G" + fill_t[at + 8:]
        fill_c = fill_t[:at] + "A" * (1 + g % 2) + fill_t[at:]
    elif kind == "tandem":
        at = mid()
        fill_c = fill_t[:at - 1] + "T" + "ACG" * 4 + "T" + fill_t[at + 13:]
        fill_t = fill_c[:at] + "ACG" + fill_c[at:]
    elif kind == "anchor":                                                # three bases of the left flank are missing left of the anchor
        left_n = 95
        anchor_c = (lf[-left_n:-40] + lf[-37:], rf[:right_n])
        rows = C.sample(rng, lf + fill_t + rf, n_rows, L, 0.005, masked) + C.exact_rows(lf + fill_t + rf, [0, 4, 8, 12, 16, 20], L)
    elif kind == "plain":
        for at in (40, 141, 250):
            fill_c = C.sub(fill_c, at)
    elif kind == "minority":
        at = mid()
        variant = fill_t[:at] + fill_t[at + 3:]
        n_var = int(0.3 * n_rows)
        rows = C.sample(rng, lf + fill_t + rf, n_rows - n_var, L, 0.005, masked) + C.sample(rng, lf + variant + rf, n_var, L, 0.005, masked)
    elif kind == "ins_b0":                                                # the contig lacks the fill's first two bases: an insertion at p = b0
        fill_t = _avoid(lf[-1], fill_t[2]) * 2 + fill_t[2:]
        fill_c = fill_t[2:]
    elif kind == "ins_b1":                                                # ... its last two: at p = b1
        fill_t = fill_t[:-2] + _avoid(fill_t[-3], rf[0]) * 2
        fill_c = fill_t[:-2]
    elif kind == "del_b1":                                                # two bases too many at the fill's end: a deletion that ends at b1
        fill_c = fill_t + _avoid(fill_t[-1], rf[0]) * 2
    elif kind == "boundary":                                              # the stored body's columns VCHUNK - 1 and VCHUNK go away
        fill_t = C.seq(rng, 1300 - left_n - right_n - 2)
        col = (right_n if rev else left_n) + VCHUNK - 1                   # stored column; natural: the two columns end at n - col
        at = (1300 - col - 2 if rev else col) - left_n
        fill_c = fill_t[:at] + _avoid(fill_t[at - 1], fill_t[at]) * 2 + fill_t[at:]
        n_rows = 150
    elif kind in ("at_max", "over_max"):                                  # one planted insertion, three rows over it
        fill_t = C.seq(rng, MAX_CONTIG + (kind == "over_max") - left_n - right_n + 2)
        at = 4000
        fill_c = fill_t[:at] + fill_t[at + 2:]
        rows = C.exact_rows(lf + fill_t + rf, [100 + at - L // 2 + d for d in (-20, 0, 20)], L)
    elif kind in ("events65", "events64"):                                # rows with one inserted base each, at columns three apart
        truth, rows = lf + fill_t + rf, []
        for k in range(65 if kind == "events65" else 64):
            o = 110 + 3 * k
            rows.append((truth[o:o + 60] + _avoid(truth[o + 59], truth[o + 60]) + truth[o + 60:])[:L])
            rows[-1] = revcomp(rows[-1]) if k % 2 else rows[-1]
    elif kind == "ins_cap":                                               # five times 16 bases missing, three exact rows over each
        sites = [40 + 90 * k for k in range(5)]
        fill_t = C.seq(rng, 500)
        fill_c = "".join(fill_t[a + 16 if a else 0:b] for a, b in zip([0] + sites, sites + [500]))
        rows = C.exact_rows(lf + fill_t + rf, [100 + s + 8 - L // 2 + d for s in sites for d in (-6, 0, 6)], L)
    elif kind == "tie":                                                   # the host test's tie: a gapless candidate with the split one's key
        fill_t = fill_c = C.seq(rng, 159) + "AG" + "T" * 40 + "CA" + C.seq(rng, 80)
        K, pg = natural(fill_c), left_n + 160                             # pg: the G's column; the rows lack the G
        tie = K[pg - (L - 41):pg] + "T" * 40 + "C"                        # split: 0 + 2; gapless on the left diagonal: T on G, C on T: 2; overlap L both
        alone = K[pg - (L - 42):pg] + "T" * 40 + "CA"                     # one base more: a third gapless mismatch, the split candidate stands alone
        rows = both([tie] * 3 + [alone])
    elif kind in ("cost", "overlap", "overlap_tie", "masked"):
        left, right = C.unique_pair(rng, 170, 170, "GTC")
        fill_t = fill_c = left + "GTC" + right
        K, p, h = natural(fill_c), left_n + 170, L // 2                   # p: the G's column; nothing here can slide (unique_pair)
        lacks = K[:p] + K[p + 3:]
        if kind == "cost":                                                # the indel costs two: two more mismatches are placed, three are not
            r2 = C.sub(C.sub(lacks[p - h:p - h + L], 20), L - 20)
            rows = both([r2, C.sub(r2, 30)])
        elif kind == "masked":                                            # the contig lacks GTC; a row with the T masked cannot insert it
            fill_c = left + right
            r = K[p - h:p - h + L]
            rows = both([r, r[:h + 1] + "N" + r[h + 2:]])
            extra = {"d1": p - h, "h": h}
        else:                                                             # a deletion of [p, p + 3) and an insertion before p + 2: they touch
            more = K[:p + 2] + "AA" + K[p + 2:]
            d_ins = (-8, -4, 0, 4, 8) if kind == "overlap" else (-4, 0, 4)
            rows = C.exact_rows(lacks, [p - h + d for d in (-4, 0, 4)], L) + C.exact_rows(more, [p + 2 - h + d for d in d_ins], L)
    elif kind == "empty":
        rows = []
    contig = (anchor_c[0] if anchor_c else lf[-left_n:]) + fill_c + (anchor_c[1] if anchor_c else rf[:right_n])
    if kind == "non_acgt":
        contig = contig[:left_n + 40] + "N" + contig[left_n + 41:]
    if rows is None:
        rows = C.sample(rng, lf + fill_t + rf, n_rows, L, 0.005, masked)
    left_n = len(contig) - len(fill_c) - right_n
    n = len(contig)
    sb = (n - left_n - len(fill_c), n - left_n) if rev else (left_n, left_n + len(fill_c))
    return {"kind": kind, "flanks": (lf, rf), "stored": revcomp(contig) if rev else contig, "body": sb, "rev": rev, "a": A_LONG if g % 4 < 2 else A_SHORT,
            "reads": rows, "extra": extra, "truth": lf[-left_n:] + fill_t + rf[:right_n] if not anchor_c else None,
            "decoys": [C.seq(rng, int(rng.integers(20, 120))) for _ in range(int(rng.integers(0, 3)))]}


def _build(L, masked, style):
    """One run's input (cached): the gaps (shared by the styles), the contig list with decoys and tombstones, the words and pick entries."""
    if (L, masked) not in _GAPS:
        rng = np.random.default_rng(9000 + L)
        _GAPS[L, masked] = [_gap(rng, g, kind, L, masked) for g, kind in enumerate(KINDS)]
    if (L, masked, style) in _CASES:
        return _CASES[L, masked, style]
    gaps = _GAPS[L, masked]
    rng = np.random.default_rng(77)
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
        wrong = G["kind"] == "mismatch" and style == "exact"
        words[g] = _word(G["a"], sb1 - sb0 + (7 if wrong else 0), ci, G["rev"])
        expect[g] = "mismatch" if wrong else (sb0, sb1)
        if style == "pick":
            lm, rm = min(40, sb0), min(35, len(G["stored"]) - sb1)
            picks[ci] = (sb1 + 1, sb0 - lm + 1, rm, lm, 1, G["a"], 0) if G["rev"] else (sb0 - lm + 1, sb1 + 1, lm, rm, 0, G["a"], 0)
    _CASES[L, masked, style] = {"gaps": gaps, "recs": recs, "words": words, "picks": picks, "expect": expect}
    return _CASES[L, masked, style]


def _params(key, L):
    mm_150, mm_100, mo, mv = PARAMS[key]
    return key[0], (mm_150 if L == 150 else mm_100), mo, mv, key[1]


def _twin(case, L, masked, style, key):
    """(records with off = 0, {gap: polished text}, stats) from the twin; a gap's answer is computed once for both styles."""
    from gappadder_amd import _lib as B
    from gappadder_amd import polish_gapped as PG
    from gappadder_amd import read_support as RS
    prm = _params(key, L)
    want, texts = np.zeros(len(case["gaps"]), dtype=B.FILL_POLISH_GAPPED), {}
    stats = dict.fromkeys(PG.STAT_KEYS, 0)
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
        tk = (L, masked, key, g)
        if tk not in _TWINS:
            reads = G["reads"] if masked else [r.replace("N", "A") for r in G["reads"]]      # without the mask words an N of a read is the base A
            _TWINS[tk] = PG.polish_gapped_host(reads, G["stored"], body[0], body[1], *prm)
        texts[g], want[g] = _TWINS[tk]
        PG.add_stats(stats, want[g], len(texts[g]))
    return want, texts, stats


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
    d_out = torch.full((n_gaps * B.FILL_POLISH_GAPPED.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    d_bases = torch.full((base_cap + 256,), 0x2E, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B.PLG_WORDS,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = B.lib().gf_fill_polish_gapped_dev(gf.handle, d_pool.data_ptr(), d_nm.data_ptr() if masked else None, d_off.data_ptr(), len(reads), L,
                                           d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), d_best.data_ptr(),
                                           d_pick.data_ptr() if d_pick is not None else None, A_LONG, A_SHORT, *prm, d_out.data_ptr(),
                                           d_bases.data_ptr(), base_cap, d_st.data_ptr())
    assert rc == 0, (rc, B.lib().gf_last_error(gf.handle))
    gf.sync()
    return np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.FILL_POLISH_GAPPED), d_bases.cpu().numpy().tobytes(), d_st.cpu().numpy(), gf


def _cases_are_there(case, want, texts, key):
    """What the cases are there for, from the twin alone (the repairs at the default rule: seed 16, max_indel 8)."""
    from gappadder_amd import _lib as B
    gaps = case["gaps"]
    by_kind = {}
    for g, G in enumerate(gaps):
        by_kind.setdefault(G["kind"], []).append(g)
    one = lambda kind: by_kind[kind][0]
    if key == (16, 8):
        # (not the homopolymer and the tandem unit: a row whose leftmost seed ends inside the repeat cannot name the leftmost breakpoint and
        # names the same indel further right, and two such rows pass as an event of their own — DESIGN.md §22, limits)
        for g in by_kind["tandem"] + by_kind["homopolymer"]:
            assert int(want[g]["n_events"]) >= 1 and (int(want[g]["n_inserted"]) > 0) != (int(want[g]["n_deleted"]) > 0)
        for kind in ("missing", "extra", "ins_b0", "ins_b1", "del_b1", "boundary", "at_max"):
            for g in by_kind[kind]:
                G = gaps[g]
                truth = C.revcomp(G["truth"]) if G["rev"] else G["truth"]
                assert texts[g] == truth != G["stored"] and int(want[g]["n_events"]) == 1 and int(want[g]["flags"]) == 0, (kind, g, want[g])
        assert all({gaps[g]["rev"] for g in by_kind[kind]} == {False, True} for kind in ("missing", "extra", "homopolymer", "tandem"))
        g = one("anchor")
        assert int(want[g]["events_outside"]) >= 3 and int(want[g]["n_events"]) == 0 and texts[g] == gaps[g]["stored"]
        g = one("minority")
        assert int(want[g]["events_seen"]) >= 1 and int(want[g]["n_events"]) == 0 and int(want[g]["reads_split"]) >= 3
        g = one("boundary")
        sb0, sb1 = gaps[g]["body"]
        assert sb1 - sb0 > VCHUNK and int(want[g]["n_deleted"]) == 2 and len(gaps[g]["stored"]) == 1300
        g = one("events65")
        assert int(want[g]["flags"]) == B.PL_F_EVENTS and int(want[g]["events_seen"]) == 65 and int(want[g]["reads_split"]) == 65
        g = one("events64")
        assert int(want[g]["flags"]) == 0 and int(want[g]["events_seen"]) == 64 and int(want[g]["n_events"]) == 0
    if key[1] == 16:
        g = one("ins_cap")
        assert int(want[g]["flags"]) == B.PL_F_INS_CAP and int(want[g]["n_events"]) == 4 and int(want[g]["n_inserted"]) == 64 == B.PLG_MAX_INSERTED
        assert int(want[g]["events_seen"]) == 5 and int(want[g]["len"]) == len(gaps[g]["stored"]) + 64
    assert sum(int(r["reads_split"]) for r in want) > 0
    if key == (16, 8):
        _directed_cases_fire(gaps, one, want)
    g = one("at_max")
    assert len(gaps[g]["stored"]) == MAX_CONTIG == B.PL_MAX_CONTIG
    g = one("over_max")
    assert len(gaps[g]["stored"]) == MAX_CONTIG + 1 and int(want[g]["flags"]) == B.PL_F_LONG and texts[g] == gaps[g]["stored"]
    g = one("non_acgt")
    assert int(want[g]["flags"]) == B.PL_F_NON_ACGT and texts[g] == gaps[g]["stored"]
    g = one("empty")
    assert int(want[g]["n_uncovered"]) == int(want[g]["n_cols"]) > 0 and texts[g] == gaps[g]["stored"]
    g = one("open")
    assert case["words"][g] == 0 and not want[g].tobytes().strip(b"\0")


def _directed_cases_fire(gaps, one, want):
    """The four host cases that no sampled pool is sure to hold, from the twin at seed 16, max_mismatch 4, max_indel 8."""
    from gappadder_amd import polish_gapped as PG
    w = want[one("tie")]              # six rows tie between the gapless and the split candidate; the two with one base more are placed split
    assert (int(w["reads_ambiguous"]), int(w["reads_placed"]), int(w["reads_split"])) == (6, 2, 2), w
    w = want[one("cost")]             # mm 2 + an indel: placed (and their deletion passes with two votes); mm 3 + an indel: refused
    assert (int(w["reads_placed"]), int(w["reads_split"]), int(w["reads_ambiguous"]), int(w["n_events"]), int(w["n_deleted"])) == (2, 2, 0, 1, 3), w
    w = want[one("overlap")]          # five votes for the insertion, three for the deletion it touches: the votes decide, against the key order
    assert (int(w["events_seen"]), int(w["n_events"]), int(w["n_inserted"]), int(w["n_deleted"]), int(w["reads_split"])) == (2, 1, 2, 0, 8), w
    w = want[one("overlap_tie")]      # three votes each: the smaller key, the deletion
    assert (int(w["events_seen"]), int(w["n_events"]), int(w["n_inserted"]), int(w["n_deleted"]), int(w["reads_split"])) == (2, 1, 0, 3, 6), w
    G = gaps[one("masked")]
    L, d1, h = len(G["reads"][0]), G["extra"]["d1"], G["extra"]["h"]
    assert not G["rev"] and int(want[one("masked")]["reads_split"]) == 4
    if "N" in G["reads"][2]:          # (read by the run with masks; without them the N is the base A)
        assert PG.placements_gapped(G["reads"][::2], G["stored"], 16, 4, 48, 8) == [(0, d1, 0, L - 3, d1 - 3, h), (0, d1, 1, L - 3, d1 - 3, h - 2)]


def _compare(case, got, bases, want, texts, base_cap):
    bad, spans = [], []
    for g in range(len(want)):                                # every gap: the record but for `off`, and the bytes at `off`
        a, b = got[g].copy(), want[g].copy()
        o, n = int(a["off"]), int(a["len"])
        a["off"] = 0
        if a.tobytes() != b.tobytes() or (g in texts and bases[o:o + n].decode() != texts[g]) or (g not in texts and (o or n)):
            bad.append(g)
        if g in texts:
            spans.append((o, o + n))
    assert not bad, [(g, case["gaps"][g]["kind"], case["gaps"][g]["rev"], got[g], want[g]) for g in bad[:4]]
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == base_cap and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    assert set(bases[base_cap:]) == {0x2E}                    # nothing beyond what was handed out


@pytest.mark.parametrize("L,masked,key,style", [(L, m, key, "exact") for L, m in ((150, False), (100, True)) for key in sorted(PARAMS)] +
                         [(150, False, (16, 8), "pick"), (100, True, (16, 8), "pick")])
def test_kernel_equals_the_twin(L, masked, key, style):
    from gappadder_amd import polish_gapped as PG
    case = _build(L, masked, style)
    want, texts, stats = _twin(case, L, masked, style, key)
    _cases_are_there(case, want, texts, key)
    base_cap = sum(len(t) for t in texts.values())            # exactly what the polished contigs take
    got, bases, st, _ = _run_device(case, L, masked, style, _params(key, L), base_cap)
    assert PG.stats_of(st) == stats and stats["mismatches"] == (1 if style == "exact" else 0) and stats["bases"] == base_cap
    _compare(case, got, bases, want, texts, base_cap)


def test_arguments_and_the_base_buffers_capacity():
    from gappadder_amd import _lib as B
    from gappadder_amd import polish_gapped as PG
    import torch
    case = _build(150, False, "exact")
    want, texts, stats = _twin(case, 150, False, "exact", (16, 8))
    total = sum(len(t) for t in texts.values())
    # one byte short: exactly one contig — whichever asks last — does not fit; the counts are still the twin's
    got, bases, st, gf = _run_device(case, 150, False, "exact", _params((16, 8), 150), base_cap=total - 1)
    dev = PG.stats_of(st)
    assert dev == dict(stats, overflow=1) and dev["bases"] == total
    (lost,) = [g for g in texts if int(got[g]["flags"]) & B.PL_F_OVERFLOW]
    assert int(got[lost]["len"]) == 0 and int(got[lost]["off"]) == 0 and int(got[lost]["flags"]) == int(want[lost]["flags"]) | B.PL_F_OVERFLOW
    for g in texts:
        assert all(int(got[g][f]) == int(want[g][f]) for f in B.FILL_POLISH_GAPPED.names[3:] if f != "reserved")
        if g != lost:
            o = int(got[g]["off"])
            assert bases[o:o + int(got[g]["len"])].decode() == texts[g]
    assert set(bases[total - 1:]) == {0x2E}
    lib = B.lib()
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = z.data_ptr()
    args = lambda s=16, mm=4, mo=48, mv=2, mi=8, a_long=30, a_short=15: (gf.handle, p, None, p, 0, 150, p, p, 0, p, p, None, a_long, a_short, s, mm, mo,
                                                                         mv, mi, p, p, 0, p)
    for kw in (dict(s=11), dict(s=33), dict(mm=-1), dict(mm=16), dict(mo=15), dict(mo=151), dict(mv=0), dict(s=32, mm=4), dict(mi=0), dict(mi=17)):
        assert lib.gf_fill_polish_gapped_dev(*args(**kw)) == B.GF_E_UNSUPPORTED, kw
    assert lib.gf_fill_polish_gapped_dev(*args(a_long=40)) == B.GF_E_INVAL and lib.gf_fill_polish_gapped_dev(*args(mi=16)) == B.GF_OK
