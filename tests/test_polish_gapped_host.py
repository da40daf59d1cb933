"""The host twin of the indel-aware polish (gappadder_amd/polish_gapped.py): hand-derived answers clause by clause — planted indels stored
forward and reversed, the tie between equal breakpoints in a homopolymer and a tandem repeat, the indel's cost of two, the ambiguity with
a gapless candidate, events outside the body, `against`, the order in which events are accepted, the body's edges, masked inserted bases
— the seeded search against a brute-force restatement of the definition over all (d1, d2, x), and a pool without any split candidate
against polish.polish_host."""
import numpy as np
import pytest

import polish_gapped_cases as C
from gappadder_amd import _lib as B
from gappadder_amd import polish as PL
from gappadder_amd import polish_gapped as PG
from gappadder_amd import read_support as SUP
from gappadder_amd.pick_contigs import revcomp

DEL, INS = PG.DEL, PG.INS


def _run(case, **kw):
    text, rec, where, events = PG.polish_gapped_host(case["reads"], case["contig"], *case["body"], detail=True, **kw)
    return text, rec, where, events


# ---- planted indels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("build,seed", [(C.missing_bases, 21), (C.extra_bases, 22)])
def test_a_planted_indel_is_repaired(build, seed, reverse):
    case = C.stored(build(np.random.default_rng(seed)), reverse)
    text, rec, where, events = _run(case)
    kind, p, g, _ = case["event"]
    assert text == case["truth"] and int(rec["len"]) == len(case["truth"]) != len(case["contig"])
    assert int(rec["n_events"]) == 1 and int(rec["n_inserted"]) == (g if kind == INS else 0) and int(rec["n_deleted"]) == (g if kind == DEL else 0)
    votes, against = events[case["event"]]
    assert votes >= 15 and against == 0 and all(v <= 1 for e, (v, _) in events.items() if e != case["event"])     # (stray events: one row each)
    assert int(rec["reads_split"]) == sum(len(w) == 6 for w in where if w not in (None, "ambiguous")) >= votes
    assert {w[0] for w in where if w not in (None, "ambiguous") and len(w) == 6} == {0, 1}
    # (a row that ends a few bases beyond the indel is placed without a gap and votes its shifted bases there: columns the deletion removes)
    assert int(rec["n_changed"]) <= (g if kind == DEL else 0) and int(rec["flags"]) == 0 and int(rec["events_seen"]) == len(events)
    # the plain polish cannot repair it, and no read is placed across it
    plain, prec = PL.polish_host(case["reads"], case["contig"], *case["body"])
    assert plain != case["truth"] and len(plain) == len(case["contig"]) and int(prec["reads_placed"]) < int(rec["reads_placed"])


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("build,seed", [(C.homopolymer, 23), (C.tandem, 24)])
def test_equal_breakpoints_collapse_to_one_key_at_the_leftmost_column(build, seed, reverse):
    case = C.stored(build(np.random.default_rng(seed)), reverse)
    text, rec, where, events = _run(case)
    assert set(events) == {case["event"]} and events[case["event"]] == (len(case["reads"]), 0)      # one key, from the rows of both strands
    assert {w[0] for w in where} == {0, 1} and all(len(w) == 6 for w in where)
    assert text == case["truth"] and int(rec["events_seen"]) == 1 and int(rec["reads_split"]) == len(case["reads"])


# ---- the cost of an indel, ambiguity ------------------------------------------------------------------------------------------------------
def _split_read(rng):
    """A contig of 400 bases and a read of 100 that lacks its columns 200..202 (read bases 0..49 on diagonal 150, 50..99 on 153)."""
    left, right = C.unique_pair(rng, 200, 197, "GTC")
    contig = left + "GTC" + right
    return contig, contig[150:200] + contig[203:253]


def test_an_indel_costs_two_mismatches():
    rng = np.random.default_rng(25)
    contig, read = _split_read(rng)
    for subs, want in (((20, 80), (0, 150, 2, 100, 153, 50)), ((20, 30, 80), None)):      # mm 2 + 2 = 4 is placed, mm 3 + 2 = 5 is refused
        r = read
        for at in subs:
            r = C.sub(r, at)
        assert PG.placements_gapped([r], contig, 16, 4, 48, 8) == [want]
        assert PG.placements_gapped([revcomp(r)], contig, 16, 4, 48, 8) == [want and (1,) + want[1:]]
    assert PG.placements_gapped([read], contig, 16, 1, 48, 8) == [None] and PG.placements_gapped([read], contig, 16, 2, 48, 8)[0][2] == 0
    assert PG.placements_gapped([read], contig, 16, 4, 48, 2) == [None]                    # max_indel 2: the diagonals are three apart


def test_a_gapless_candidate_of_equal_cost_and_overlap_makes_the_row_ambiguous():
    rng = np.random.default_rng(26)
    u, v = C.seq(rng, 100)[:-1] + "A", "A" + C.seq(rng, 60)
    contig = u + "G" + "T" * 40 + "C" + v
    # the read lacks the G.  Split: a deletion at column 100, cost 0 + 2, overlap 100.  Gapless on the left diagonal: T on the G, the
    # read's C on the last T: cost 2, overlap 100 — the same key
    read = u[-59:] + "T" * 40 + "C"
    assert PG.placements_gapped([read], contig, 16, 4, 48, 8) == ["ambiguous"]
    # one base more: the gapless candidate has a third mismatch (v[0] = A on the C) and the split one stands alone
    read = u[-58:] + "T" * 40 + "C" + v[0]
    assert PG.placements_gapped([read], contig, 16, 4, 48, 8) == [(0, 42, 0, 100, 43, 58)]
    text, rec = PG.polish_gapped_host([u[-59:] + "T" * 40 + "C"] * 5, contig, 80, 160)
    assert text == contig and int(rec["reads_ambiguous"]) == 5 and int(rec["reads_placed"]) == 0 and int(rec["n_uncovered"]) == 80


# ---- the body -----------------------------------------------------------------------------------------------------------------------------
def test_an_event_in_the_anchor_is_dropped_and_counted():
    case = C.missing_bases(np.random.default_rng(27), body=(310, 500))
    text, rec, where, events = _run(case)
    assert case["event"] not in events and int(rec["events_outside"]) >= 15 and int(rec["n_events"]) == 0
    assert text == case["contig"] and int(rec["reads_split"]) >= int(rec["events_outside"])       # the rows stay placed


@pytest.mark.parametrize("body,applied", [((300, 500), True), ((301, 500), False), ((100, 300), True), ((100, 299), False)])
def test_an_insertion_at_either_edge_of_the_body(body, applied):
    case = C.missing_bases(np.random.default_rng(28), body=body)          # INS at p = 300: b0 <= p <= b1
    text, rec, _, events = _run(case)
    assert (case["event"] in events) == applied and (text == case["truth"]) == applied and int(rec["n_events"]) == int(applied)


@pytest.mark.parametrize("body,applied", [((100, 302), True), ((100, 301), False), ((300, 500), True), ((301, 500), False)])
def test_a_deletion_at_either_edge_of_the_body(body, applied):
    case = C.extra_bases(np.random.default_rng(29), body=body)            # DEL of columns 300, 301: b0 <= p and p + g <= b1
    text, rec, _, events = _run(case)
    assert (case["event"] in events) == applied and (text == case["truth"]) == applied and int(rec["n_deleted"]) == 2 * int(applied)


# ---- against, the order of acceptance ------------------------------------------------------------------------------------------------------
def test_a_minority_indel_changes_nothing():
    case = C.minority(np.random.default_rng(30))
    text, rec, where, events = _run(case)
    votes, against = events[case["event"]]
    # enough votes to pass min_votes: it is `against` that stops it — the rows of the contig itself that cross the site outnumber them
    assert votes >= 10 and against > votes and text == case["contig"] and int(rec["n_events"]) == 0 and int(rec["events_seen"]) >= 1
    assert int(rec["reads_split"]) >= votes and int(rec["n_changed"]) == 0


def test_against_counts_the_rows_that_cross_the_site_in_one_piece():
    rng = np.random.default_rng(31)
    case = C.minority(rng, n_reads=0, share=0)
    contig, variant = case["contig"], case["contig"][:300] + case["contig"][303:]
    # site of (DEL, 300, 3) with s = 16: columns [284, 319).  Rows of the contig itself at 134 (ends at 284: not), 169 (covers 169..318:
    # yes), 170 (covers 170..319: yes), 284 (yes), 285 (no)
    rows = [contig[o:o + 150] for o in (134, 169, 170, 284, 285)]
    voters = [variant[o:o + 150] for o in (200, 220, 240)]
    _, rec, _, events = PG.polish_gapped_host(voters + rows, contig, 100, 500, detail=True)
    assert events == {(DEL, 300, 3, 0): (3, 3)} and int(rec["n_events"]) == 0            # 3 > 3 fails
    text, rec, _, events = PG.polish_gapped_host(voters + rows[:2] + rows[3:], contig, 100, 500, detail=True)
    assert events == {(DEL, 300, 3, 0): (3, 2)} and int(rec["n_events"]) == 1 and text == variant


def test_the_order_in_which_events_are_accepted():
    a, b = (DEL, 100, 3, 0), (INS, 102, 2, 7)                 # [100, 103] and [102, 102] meet
    assert PG.decide_events({a: 5, b: 7}, {}, 2) == ([b], False) and PG.decide_events({a: 7, b: 5}, {}, 2) == ([a], False)
    assert PG.decide_events({a: 5, b: 5}, {}, 2) == ([a], False)                                  # the smaller column
    assert PG.decide_events({a: 5, (INS, 103, 2, 7): 5}, {}, 2) == ([a], False)                   # [103, 103] still touches [100, 103]
    assert PG.decide_events({a: 5, (INS, 104, 2, 7): 4}, {}, 2) == ([a, (INS, 104, 2, 7)], False)
    assert PG.decide_events({(INS, 100, 2, 7): 5, (DEL, 100, 2, 0): 5}, {}, 2)[0] == [(DEL, 100, 2, 0)]        # a deletion before an insertion
    assert PG.decide_events({(DEL, 100, 3, 0): 5, (DEL, 100, 2, 0): 5}, {}, 2)[0] == [(DEL, 100, 2, 0)]        # the shorter
    assert PG.decide_events({(INS, 100, 2, 7): 5, (INS, 100, 2, 6): 5}, {}, 2)[0] == [(INS, 100, 2, 6)]        # the smaller base-4 number
    assert PG.decide_events({a: 1, b: 3}, {b: 3}, 2) == ([], False)                               # too few votes; no more votes than against
    five = {(INS, 100 + 20 * i, 16, i): 9 - i for i in range(5)}                                 # 4 x 16 = GF_PLG_MAX_INSERTED: the fifth is dropped
    assert PG.decide_events(five, {}, 2) == (sorted(five)[:4], True)
    assert PG.decide_events({**five, (DEL, 300, 16, 0): 2}, {}, 2) == (sorted(five)[:4] + [(DEL, 300, 16, 0)], True)


# ---- masked bases --------------------------------------------------------------------------------------------------------------------------
def test_masked_inserted_bases_give_no_candidate():
    rng = np.random.default_rng(32)
    left, right = C.unique_pair(rng, 200, 200, "GTC")
    contig, truth = left + right, left + "GTC" + right
    read = truth[150:250]                                       # the inserted bases are the read's 50..52
    assert PG.placements_gapped([read], contig, 16, 4, 48, 8) == [(0, 150, 0, 97, 147, 50)]
    # the middle one masked: no three inserted bases may hold it.  x = 48 (the read's C on the contig's last left base) and x = 52 (its
    # G on the first right base) cost one mismatch each — unique_pair keeps those bases apart —: the smaller x
    masked = read[:51] + "N" + read[52:]
    assert PG.placements_gapped([masked], contig, 16, 4, 48, 8) == [(0, 150, 1, 97, 147, 48)]
    masked = read[:49] + "N" + read[50:]                        # a masked ALIGNED base next to them costs nothing
    assert PG.placements_gapped([masked], contig, 16, 4, 48, 8) == [(0, 150, 0, 97, 147, 50)]


# ---- the seeded search against the definition, by brute force -------------------------------------------------------------------------------
def _brute(codes, valid, cc, s, mm_max, mo, G):
    n, L = len(cc), codes.shape[1]
    out = []
    for r in range(len(codes)):
        cands = []
        for strand in (0, 1):
            q, v = (codes[r], valid[r]) if strand == 0 else (3 - codes[r][::-1], valid[r][::-1])
            seeds = {}                                         # d -> the clean seed windows that equal the contig there
            for d in range(-L, n + 1):
                js = [j for j in range(L // s) if 0 <= d + j * s and d + j * s + s <= n and v[j * s:j * s + s].all()
                      and (q[j * s:j * s + s] == cc[d + j * s:d + j * s + s]).all()]
                if js:
                    seeds[d] = js
            mm_of = lambda d, a, b: sum(1 for i in range(a, b) if v[i] and q[i] != cc[d + i])
            for d in seeds:
                i0, i1 = max(0, -d), min(L, n - d)
                if i1 - i0 >= mo and mm_of(d, i0, i1) <= mm_max:
                    cands.append((mm_of(d, i0, i1), -(i1 - i0), (strand, d, mm_of(d, i0, i1), i1 - i0)))
            for d1 in seeds:
                for d2 in seeds:
                    if not 0 < abs(d2 - d1) <= G:
                        continue
                    gi = max(0, d1 - d2)
                    i0, i1 = max(0, -d1), min(L, n - d2)
                    best = None
                    for x in range((min(seeds[d1]) + 1) * s, max(seeds[d2]) * s - gi + 1):
                        if not v[x:x + gi].all():
                            continue
                        mm = mm_of(d1, i0, x) + mm_of(d2, x + gi, i1)
                        if best is None or mm < best[0]:
                            best = (mm, x)
                    if best is not None and i1 - i0 - gi >= mo and best[0] + 2 <= mm_max:
                        cands.append((best[0] + 2, -(i1 - i0 - gi), (strand, d1, best[0], i1 - i0 - gi, d2, best[1])))
        if not cands:
            out.append(None)
            continue
        key = min(c[:2] for c in cands)
        top = [c for c in cands if c[:2] == key]
        out.append(top[0][2] if len(top) == 1 else "ambiguous")
    return out


@pytest.mark.parametrize("seed,G", [(41, 1), (42, 4), (43, 8), (44, 16)])
def test_the_seeded_search_equals_the_definition_by_brute_force(seed, G):
    rng = np.random.default_rng(seed)
    L, s, mm_max, mo = 60, 12, 3, 24
    kinds = set()
    for trial in range(3):
        unit = C.seq(rng, int(rng.integers(1, 5)))
        truth = C.seq(rng, 70) + unit * int(rng.integers(3, 9)) + C.seq(rng, 70)
        truth = truth[:int(rng.integers(150, 201))]
        reads = []
        for _ in range(24):                                    # rows of the truth with an indel of their own, a substitution, an N
            o = int(rng.integers(0, len(truth) - L - G))
            r = truth[o:o + L + G]
            at, g = int(rng.integers(5, L - 5)), int(rng.integers(1, G + 1))
            r = (r[:at] + r[at + g:], r[:at] + C.seq(rng, g) + r[at:], r)[int(rng.integers(0, 3))][:L]
            if rng.integers(0, 2):
                r = C.sub(r, int(rng.integers(0, L)))
            if rng.integers(0, 4) == 0:
                r = r[:at + 1] + "N" + r[at + 2:]
            reads.append(revcomp(r) if rng.integers(0, 2) else r)
        codes, valid = SUP.codes_of(reads)
        cc = PG._LUT[np.frombuffer(truth.encode(), dtype=np.uint8)]
        got = PG.placements_gapped((codes, valid), truth, s, mm_max, mo, G)
        assert got == _brute(codes, valid, cc, s, mm_max, mo, G)
        kinds |= {"ambiguous" if w == "ambiguous" else "none" if w is None else ("split", w[4] > w[1]) if len(w) == 6 else "gapless" for w in got}
    assert {"gapless", ("split", True), ("split", False)} <= kinds, kinds


# ---- without a split candidate: the plain polish -------------------------------------------------------------------------------------------
def test_a_pool_without_a_split_candidate_gives_the_plain_polish():
    rng = np.random.default_rng(45)
    truth = C.seq(rng, 600)
    contig = truth
    for at in (200, 301, 455):
        contig = C.sub(contig, at)
    reads = C.sample(rng, truth, 90, 100)
    text, rec, where, events = PG.polish_gapped_host(reads, contig, 100, 500, detail=True)
    plain, prec = PL.polish_host(reads, contig, 100, 500)
    assert not events and all(w is None or w == "ambiguous" or len(w) == 4 for w in where)
    assert text == plain == truth and rec.tobytes()[:40] == prec.tobytes() and not rec.tobytes()[40:].strip(b"\0")
    assert where == PL.placements(reads, contig)


def test_skips_and_parameters_are_the_plain_polishs():
    rng = np.random.default_rng(46)
    case = C.missing_bases(rng)
    n_contig = case["contig"][:250] + "N" + case["contig"][251:]
    text, rec = PG.polish_gapped_host(case["reads"], n_contig, *case["body"])
    assert text == n_contig and int(rec["flags"]) == B.PL_F_NON_ACGT and int(rec["n_cols"]) == 400 and int(rec["reads_placed"]) == 0
    long = C.seq(rng, B.PL_MAX_CONTIG + 1)
    text, rec = PG.polish_gapped_host(case["reads"], long, 100, 500)
    assert text == long and int(rec["flags"]) == B.PL_F_LONG and int(rec["len"]) == len(long)
    for kw in (dict(max_indel=0), dict(max_indel=17), dict(seed=11), dict(max_mismatch=16), dict(min_overlap=151), dict(min_votes=0)):
        with pytest.raises(ValueError):
            PG.check_params(150, **kw)
    assert PG.check_params(150) == (16, 4, 48, 2, 8) and PG.check_params(150, max_indel=16)[4] == 16 and PG.check_params(150, max_indel=1)[4] == 1
    assert B.FILL_POLISH_GAPPED.itemsize == 64 and B.FILL_POLISH_GAPPED.names[:9] == B.FILL_POLISH.names


# ---- the cut of a fill whose length changed --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("build,seed", [(C.missing_bases, 51), (C.extra_bases, 52)])
def test_polished_sequences_cuts_a_fill_whose_length_changed(build, seed, reverse):
    """Pipeline.polished_sequences on a Results built by hand around the twin's answer (pick-table mode: the cut comes from the contig's
    gf_ctg_pick entry): the cut [b0, b1 + 1) of the contig becomes [b0, b1 + 1 + the change of length) of the polished contig."""
    import types
    from gappadder_amd.pipeline import Pipeline
    case = C.stored(build(np.random.default_rng(seed)), reverse)
    contig, (b0, b1) = case["contig"], case["body"]
    text, rec = PG.polish_gapped_host(case["reads"], contig, b0, b1)
    assert text == case["truth"] and len(text) != len(contig)
    res = types.SimpleNamespace(best=np.array([(30 << 56) | ((b1 - b0 + 1) << 32) | (0x7FFFFFFF << 1) | int(reverse)], dtype=np.uint64),
                                contigs=np.zeros(1, dtype=B.CONTIG), seq=contig.encode(), ctg_pick=np.zeros(1, dtype=B.CTG_PICK),
                                polish=np.zeros(1, dtype=B.FILL_POLISH_GAPPED), polish_bases=text.encode())
    res.contigs[0]["length"] = len(contig)
    res.ctg_pick[0] = (b1 + 1, b0 - 40 + 1, 35, 40, 1, 30, 0) if reverse else (b0 - 40 + 1, b1 + 1, 40, 35, 0, 30, 0)
    res.polish[0] = rec
    me = types.SimpleNamespace(gf=types.SimpleNamespace(flanks=None))
    me._pick_cut = lambda r, g: Pipeline._pick_cut(me, r, g)
    picked, polished = Pipeline.picked_sequences(me, res), Pipeline.polished_sequences(me, res)
    cut, new = contig[b0:b1 + 1], case["truth"][b0:b1 + 1 + len(text) - len(contig)]
    assert picked == {0: (0, revcomp(cut) if reverse else cut, bool(reverse))}
    assert polished == {0: (0, revcomp(new) if reverse else new, bool(reverse))} and len(new) - len(cut) == len(text) - len(contig)
    assert new[-1] == cut[-1] and new[0] == cut[0]              # the anchors' bases at either end of the cut stay
