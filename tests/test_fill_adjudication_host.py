"""The host twin of the read adjudication (gappadder_amd/fill_adjudication.py) on the CPU: the hand-derived cases of
tests/fill_adj_cases.py through adjudicate_host (the oriented fills given) and through adjudicate_gaps (the fills located on a contig list
by the alternatives' rule, the records of fill_alternatives.alts_host); best_keys against polish.placements wherever that is unique and
against a brute force over all diagonals; the invariant that a row none of whose accepted pairs touches the differing window never votes;
the parameter checks and the Pipeline's refusals."""
import random

import numpy as np
import pytest

import fill_adj_cases as JC
from gappadder_amd import _lib as B
from gappadder_amd import fill_adjudication as ADJ
from gappadder_amd import fill_alternatives as FA
from gappadder_amd import polish as PL
from gappadder_amd import read_support as RS

CASES = JC.cases()


def as_dict(rec):
    return {k: int(rec[k]) for k in ("locus_w", "locus_r", "verdict", "flags") + JC.COUNTERS}


def test_the_cases_file_states_the_modules_defaults_and_constants():
    assert (JC.SEED, JC.MAX_MISMATCH, JC.MIN_OVERLAP, JC.MIN_VOTES, JC.RATIO) == (ADJ.SEED, ADJ.MAX_MISMATCH, ADJ.MIN_OVERLAP, ADJ.MIN_VOTES, ADJ.RATIO)
    assert (JC.KEEP, JC.SWITCH, JC.UNDECIDED) == (B.AJ_KEEP, B.AJ_SWITCH, B.AJ_UNDECIDED)
    assert (JC.LONG, JC.NON_ACGT, JC.RIVAL_FAR, JC.NO_ROWS) == (B.AJ_F_LONG, B.AJ_F_NON_ACGT, B.AJ_F_RIVAL_FAR, B.AJ_F_NO_ROWS)
    assert JC.MAX_LOCUS == B.PL_MAX_CONTIG and B.FILL_ADJ.itemsize == 48 and B.AJ_WORDS == 16
    assert {c["L"] for c in CASES} == {100, 150} and len({c["name"] for c in CASES}) == len(CASES)
    assert {c["want"]["verdict"] for c in CASES} == {0, 1, 2, 3}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_derived_case(case):
    rec = ADJ.adjudicate_host(case["reads"], case["lf"], case["rf"], case["fill_w"], case["fill_r"], context=case["L"], contig=7, rival=9,
                              rival_far=case["rival_far"], read_len=case["L"])
    assert as_dict(rec) == case["want"], case["name"]
    assert (int(rec["contig"]), int(rec["rival"]), int(rec["reserved"])) == (7, 9, 0)
    n = len(case["reads"]) if int(rec["verdict"]) else 0
    assert int(rec["votes_w"]) + int(rec["votes_r"]) + int(rec["ties"]) + int(rec["unplaced"]) == n


@pytest.mark.parametrize("L", [150, 100])
def test_the_cases_on_a_contig_list(L):
    """The fills are located by the alternatives' rule on stored contigs of either strand; open and uncontested gaps get zero records."""
    cs = [c for c in CASES if c["L"] == L]
    contigs, flanks, best, reads, gap_of = JC.assemble(cs)
    alts, _, ast = FA.alts_host(contigs, flanks, best)
    assert ast["contested"] == len(cs) and ast["lost"] == 0
    recs, st = ADJ.adjudicate_gaps(alts, contigs, flanks, best, lambda g: reads[g], L)
    for x, c in enumerate(cs):
        g = gap_of[x]
        assert as_dict(recs[g]) == c["want"], c["name"]
        assert (int(recs[g]["contig"]), int(recs[g]["rival"])) == (int(alts[g]["contig"]), int(alts[g]["rival"]))
        assert bool(int(alts[g]["dist"]) == B.FA_DIST_FAR) == c["rival_far"], c["name"]
    others = sorted(set(range(len(flanks))) - set(gap_of.values()))
    assert len(others) == 2 * len(cs) and not recs[others].tobytes().strip(b"\0")
    wants = [c["want"] for c in cs]
    assert st == {"contested": len(cs), "adjudicated": sum(w["verdict"] != 0 for w in wants), "keep": sum(w["verdict"] == 1 for w in wants),
                  "switch": sum(w["verdict"] == 2 for w in wants), "undecided": sum(w["verdict"] == 3 for w in wants),
                  "skipped_long": sum(bool(w["flags"] & JC.LONG) for w in wants), "skipped_non_acgt": sum(bool(w["flags"] & JC.NON_ACGT) for w in wants),
                  "mismatches": 0, "votes_w": sum(w["votes_w"] for w in wants), "votes_r": sum(w["votes_r"] for w in wants),
                  "ties": sum(w["ties"] for w in wants)}
    # a record that states another length, strand or contig than the list carries: a mismatch, zero record
    g = gap_of[0]
    for field, value in (("rival_len", int(alts[g]["rival_len"]) + 1), ("fill_len", 3), ("flags", int(alts[g]["flags"]) ^ B.FA_F_REVERSE),
                         ("flags", int(alts[g]["flags"]) ^ B.FA_F_RIVAL_REVERSE), ("rival", int(alts[g]["rival"]) + 2), ("contig", int(alts[g]["contig"]) + 1)):
        bad = alts.copy()
        bad[g][field] = value
        r2, s2 = ADJ.adjudicate_gaps(bad, contigs, flanks, best, lambda g: reads[g], L)
        assert s2["mismatches"] == 1 and s2["contested"] == len(cs) and not r2[g].tobytes().strip(b"\0"), field
        assert np.delete(r2, g).tobytes() == np.delete(recs, g).tobytes()


def accepted_pairs(q, v, cc, s, mm_max, mo):
    """Brute force over every diagonal: [(mm, ov, d)] of the accepted pairs of one oriented row on the locus codes cc."""
    L, n = len(q), len(cc)
    out = []
    for d in range(-(L - 1), n):
        i0, i1 = max(0, -d), min(L, n - d)
        if i1 - i0 < mo:
            continue
        eq = q[i0:i1] == cc[d + i0:d + i1]
        mm = int((~eq & v[i0:i1]).sum())
        if mm > mm_max:
            continue
        if any(j * s >= i0 and j * s + s <= i1 and v[j * s:j * s + s].all() and eq[j * s - i0:j * s + s - i0].all() for j in range(L // s)):
            out.append((mm, i1 - i0, d))
    return out


def brute_pairs(read, text, s, mm_max, mo):
    """[(mm, ov, strand, d)] of the row's accepted pairs on both strands."""
    (codes,), (valid,) = RS.codes_of([read])
    cc = RS.codes_of([text])[0][0]
    out = []
    for strand, (q, v) in enumerate(((codes, valid), ((3 - codes[::-1]).astype(np.uint8), valid[::-1]))):
        out += [(mm, ov, strand, d) for mm, ov, d in accepted_pairs(q, v, cc, s, mm_max, mo)]
    return out


def sampled_rows(rng, G, L, n, errors=0.02, masked=0.3):
    out = []
    for _ in range(n):
        o = rng.randrange(0, len(G) - L + 1)
        r = [JC.flip(c, 0) if rng.random() < errors else c for c in G[o:o + L]]
        if rng.random() < masked:
            r[rng.randrange(L)] = "N"
        r = "".join(r)
        out.append(JC.rc(r) if rng.random() < 0.5 else r)
    return out


@pytest.mark.parametrize("s, mm_max, mo", [(16, 4, 48), (12, 4, 40), (32, 2, 48)])
def test_best_keys_agree_with_the_polish_placements_and_with_a_brute_force(s, mm_max, mo):
    rng = random.Random(s)
    L = 100
    n_unique = n_multi = n_none = 0
    for trial in range(6):
        unit = JC.rnd(rng, 37)
        text = JC.rnd(rng, 150) + unit * 4 + JC.rnd(rng, 150) if trial % 2 else JC.rnd(rng, 400)
        reads = sampled_rows(rng, JC.rnd(rng, 60) + text + JC.rnd(rng, 60), L, 25)
        keys = ADJ.best_keys(reads, text, s, mm_max, mo)
        placed = PL.placements(reads, text, s, mm_max, mo)
        for r, (k, p) in enumerate(zip(keys, placed)):
            pairs = brute_pairs(reads[r], text, s, mm_max, mo)
            if not pairs:
                assert k is None and p is None
                n_none += 1
                continue
            mm, ov = min((a[0], -a[1]) for a in pairs)
            strands = {a[2] for a in pairs if (a[0], -a[1]) == (mm, ov)}
            assert k == (mm, -ov, 0 if 0 in strands else 1), (trial, r, k, pairs)
            if p == "ambiguous":
                assert sum((a[0], -a[1]) == (mm, ov) for a in pairs) > 1
                n_multi += 1
            else:
                assert (p[2], p[3], p[0]) == k                        # (strand, d, mm, ov) of the unique placement
                n_unique += 1
    assert n_unique >= 60 and n_multi >= 3 and n_none >= 3, (n_unique, n_multi, n_none)


def random_pair(rng):
    """(F_w, F_r): F_r is F_w with a block of 0..30 bases replaced by a block of 0..30 other bases."""
    F = JC.rnd(rng, rng.randrange(60, 200))
    at, cut, put = rng.randrange(0, len(F) - 30), rng.randrange(0, 31), rng.randrange(0, 31)
    if cut == put == 0:
        put = 1
    return F, F[:at] + JC.rnd(rng, put) + F[at + cut:]


def test_a_row_that_never_touches_the_differing_window_never_votes():
    rng = random.Random(26)
    L, C, s, mm_max, mo = 100, 100, 16, 4, 48
    n_clear = n_votes = 0
    for _ in range(200):
        lf, rf = JC.rnd(rng, 160), JC.rnd(rng, 160)
        Fw, Fr = random_pair(rng)
        while Fw == Fr:                          # (a block replaced by itself: draw again, so that 200 differing pairs are checked)
            Fw, Fr = random_pair(rng)
        lcp, lcs, _ = FA.distance(Fw.encode(), Fr.encode(), 16)
        ll = min(C, len(lf))
        Tw, Tr = ADJ.locus(lf, Fw, rf, C), ADJ.locus(lf, Fr, rf, C)
        reads = sampled_rows(rng, lf + Fw + rf, L, 3) + sampled_rows(rng, lf + Fr + rf, L, 3)
        rec, keys = ADJ.adjudicate_host(reads, lf, rf, Fw, Fr, s, mm_max, mo, C, detail=True)
        for r, (kw, kr) in enumerate(keys):
            vote = (kw is None) != (kr is None) or (kw is not None and kw[:2] != kr[:2])
            n_votes += vote
            touches = False
            for T, F in ((Tw, Fw), (Tr, Fr)):
                lo, hi = ll + lcp, ll + len(F) - lcs
                if lo == hi:
                    lo, hi = lo - 1, hi + 1
                for mm, ov, strand, d in brute_pairs(reads[r], T, s, mm_max, mo):
                    c0 = max(0, d)
                    touches |= c0 < hi and c0 + ov > lo
            if not touches:
                n_clear += 1
                assert not vote, (Fw, Fr, reads[r], kw, kr)
        assert int(rec["votes_w"]) + int(rec["votes_r"]) == sum((a is None) != (b is None) or (a is not None and a[:2] != b[:2]) for a, b in keys)
    assert n_clear >= 200 and n_votes >= 100, (n_clear, n_votes)


def test_locus_and_verdict():
    assert ADJ.locus("AAACCC", "GG", "TTTAAA", 4) == "ACCCGGTTTA" and ADJ.locus("AC", "", "T", 50) == "ACT"
    assert ADJ.locus(b"AAACCC", b"GG", b"TTTAAA", 6) == "AAACCCGGTTTAAA"
    v = ADJ.verdict_of
    assert (v(3, 0), v(2, 0), v(6, 3), v(5, 3), v(0, 3), v(3, 6), v(3, 5), v(0, 0), v(1, 0, 1, 2), v(8, 1, 3, 8), v(7, 1, 3, 8)) == (1, 3, 1, 3, 2, 2, 3, 3, 1, 1, 3)


def test_check_params():
    assert ADJ.check_params(150) == (16, 4, 48, 150, 3, 2)
    assert ADJ.check_params(100, 12, 0, 12, 12, 1, 16) == (12, 0, 12, 12, 1, 16)
    assert ADJ.check_params(150, context=1000)[3] == 1000
    for kw in (dict(seed=11), dict(seed=33), dict(max_mismatch=16), dict(max_mismatch=-1), dict(min_overlap=15), dict(min_overlap=151),
               dict(seed=32, max_mismatch=4), dict(context=47), dict(context=1001), dict(context=60.5), dict(min_votes=0), dict(min_votes=True),
               dict(min_votes="3"), dict(ratio=1), dict(ratio=17), dict(ratio=2.5)):
        with pytest.raises(ValueError, match="^adjudicate "):
            ADJ.check_params(150, **kw)


def test_the_pipeline_refuses_what_the_round_excludes():
    from gappadder_amd.pipeline import Pipeline, Results
    assert Results.adjudication is None and Results.adj_stats is None
    for kw, msg in ((dict(adjudicate=True), "adjudicate needs alternatives"),
                    (dict(adjudicate=True, alternatives=True, world=2), "runs on a single rank"),
                    (dict(adjudicate=True, alternatives=True, second_round=True), "adjudicate with second_round"),
                    (dict(adjudicate=True, alternatives=True, anchor_mode="align"), "alternatives works with the exact anchors")):
        with pytest.raises(ValueError, match=msg):
            Pipeline(None, 4, 150, [(31, 29)], **kw)
    with pytest.raises(ValueError, match="^adjudicate ratio"):
        Pipeline(None, 4, 150, [(31, 29)], alternatives=True, adjudicate=True, adj_ratio=1)


def test_stats_dict_and_flank_context():
    words = np.zeros(B.AJ_WORDS, dtype=np.uint32)
    words[:8] = range(1, 9)
    words[B.AJ_VOTES_W:B.AJ_VOTES_W + 2] = (5, 1)
    words[B.AJ_VOTES_R], words[B.AJ_TIES] = 9, 11
    assert ADJ.stats_dict(words.view(np.int32)) == {"contested": 1, "adjudicated": 2, "keep": 3, "switch": 4, "undecided": 5, "skipped_long": 6,
                                                    "skipped_non_acgt": 7, "mismatches": 8, "votes_w": (1 << 32) + 5, "votes_r": 9, "ties": 11}
    text, lens = ADJ.flank_context([("AAACCC", "GGT"), ("AC", "TTTTTTT")], 4)
    assert text.shape == (2, 2, 4) and lens.tolist() == [[4, 3], [2, 4]]
    assert text[0, 0].tobytes() == b"ACCC" and text[0, 1].tobytes() == b"GGT\0" and text[1, 0].tobytes() == b"AC\0\0" and text[1, 1].tobytes() == b"TTTT"


# ---- the CLI keys and the writers -------------------------------------------------------------------------------------------------------

def test_the_cli_keys(tmp_path):
    from test_fill_alternatives_host import _config
    from gappadder_amd import main as M
    cfg = M.parse_configuration(_config(tmp_path))
    assert cfg["fill_adjudication"] is False and "fill_adjudication_context" not in cfg
    assert [cfg["fill_adjudication_" + k] for k in ("seed", "max_mismatch", "min_overlap", "min_votes", "ratio")] == [16, 4, 48, 3, 2]
    cfg = M.parse_configuration(_config(tmp_path, fill_alternatives=True, fill_adjudication=True, fill_adjudication_seed=12, fill_adjudication_max_mismatch=2,
                                        fill_adjudication_min_overlap=40, fill_adjudication_context=80, fill_adjudication_min_votes=5, fill_adjudication_ratio=16))
    assert cfg["fill_adjudication"] is True
    assert [cfg["fill_adjudication_" + k] for k in ("seed", "max_mismatch", "min_overlap", "context", "min_votes", "ratio")] == [12, 2, 40, 80, 5, 16]
    for bad in (dict(fill_adjudication_seed=11), dict(fill_adjudication_max_mismatch=16), dict(fill_adjudication_min_overlap=8), dict(fill_adjudication_context=1001),
                dict(fill_adjudication_context=11), dict(fill_adjudication_min_votes=0), dict(fill_adjudication_ratio=1), dict(fill_adjudication_ratio=17),
                dict(fill_adjudication_ratio="x")):
        with pytest.raises(SystemExit) as e:
            M.parse_configuration(_config(tmp_path, fill_alternatives=True, fill_adjudication=True, **bad))
        assert list(bad)[0] in str(e.value)
    cfgp = _config(tmp_path, fill_adjudication=True)                  # without fill_alternatives: main ends with a message
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert "fill_adjudication needs fill_alternatives" in str(e.value)
    # the keywords the collector hands the Pipeline, checked against the read length
    from gappadder_amd import device_collect as DC
    kw = DC.round_keywords(cfg, 150, "adjudication", "adj", ("seed", "max_mismatch", "min_overlap", "context", "min_votes", "ratio"), ADJ.check_params, "adjudicate")
    assert kw == dict(adjudicate=True, adj_seed=12, adj_max_mismatch=2, adj_min_overlap=40, adj_context=80, adj_min_votes=5, adj_ratio=16)
    cfg["fill_adjudication_context"] = 30
    with pytest.raises(SystemExit, match="fill_adjudication_"):
        DC.round_keywords(cfg, 150, "adjudication", "adj", ("seed", "max_mismatch", "min_overlap", "context", "min_votes", "ratio"), ADJ.check_params, "adjudicate")


def test_the_writers_on_a_made_up_results():
    from test_fill_alternatives_host import made_up_results
    from gappadder_amd import device_collect as DC
    from gappadder_amd.pipeline import Pipeline
    pipe, res, cs = made_up_results()                                  # gap 0 contested (a reverse rival), 1 and 2 closed and uncontested, 3 open
    contigs = FA.contigs_of_results(res)
    lf, rf = pipe.gf.flanks[0]
    rival = FA.candidate(contigs[int(res.alts[0]["rival"])][1], lf.encode(), rf.encode(), 30, 15)[3].decode()
    G = lf + rival + rf
    reads = {0: [G[s:s + 100] for s in range(len(lf) - 80, len(lf) + len(rival) - 20, 10)]}
    res.adjudication, res.adj_stats = ADJ.adjudicate_gaps(res.alts, contigs, pipe.gf.flanks, res.best, lambda g: reads.get(g, []), 100)
    assert int(res.adjudication[0]["verdict"]) == B.AJ_SWITCH and res.adj_stats["contested"] == res.adj_stats["switch"] == 1
    pipe.adjudicated_sequences = lambda r: Pipeline.adjudicated_sequences(pipe, r)
    tsv, fa = DC.fill_adjudication_files(pipe, res, [(31, 29)])
    lines = [l.split("\t") for l in tsv.splitlines()]
    picked = DC.picked_names(res, [(31, 29)])
    assert lines[0] == ["name"] + list(DC.ADJ_FIELDS) + ["verdict_word"] and "reserved" not in lines[0] and len(lines) == 2
    row = dict(zip(lines[0], lines[1]))
    assert row["name"] == picked[0] and row["verdict_word"] == "switch" and all(int(row[f]) == int(res.adjudication[0][f]) for f in DC.ADJ_FIELDS)
    # the sequences: every closed gap under its picked name; the rival's text at the SWITCH gap, the picked text elsewhere
    recs = {r.split("\n")[0]: "".join(r.split("\n")[1:]) for r in fa.split(">")[1:]}
    assert list(recs) == [picked[g] for g in sorted(picked)] and len(recs) == 3 and all(len(l) <= 60 for l in fa.split("\n"))
    assert recs[picked[0]] == pipe.alternative_sequences(res)[0][1] != pipe.picked_sequences(res)[0][1]
    for g in (1, 2):
        assert recs[picked[g]] == pipe.picked_sequences(res)[g][1]
    # KEEP: the file is picked_seqs.fa's text
    res.adjudication = res.adjudication.copy()
    res.adjudication[0]["verdict"] = B.AJ_KEEP
    assert {g: s for g, (s, _) in pipe.adjudicated_sequences(res).items()} == {g: v[1] for g, v in pipe.picked_sequences(res).items()}
    res.adjudication = None
    with pytest.raises(ValueError, match="adjudicate=True"):
        pipe.adjudicated_sequences(res)


def test_an_empty_pool_is_checked_against_the_given_read_length():
    """(the context may be shorter than a read: an empty pool must not take the context for the read length)"""
    c = next(c for c in CASES if c["name"] == "an empty pool")
    rec = ADJ.adjudicate_host([], c["lf"], c["rf"], c["fill_w"], c["fill_r"], context=48, read_len=150)
    assert (int(rec["locus_w"]), int(rec["verdict"]), int(rec["flags"])) == (48 + 120 + 48, B.AJ_UNDECIDED, B.AJ_F_NO_ROWS)
    contigs, flanks, best, reads, gap_of = JC.assemble([c])
    alts, _, _ = FA.alts_host(contigs, flanks, best)
    recs, st = ADJ.adjudicate_gaps(alts, contigs, flanks, best, lambda g: reads[g], 150, context=48)
    assert st["adjudicated"] == st["undecided"] == 1 and int(recs[gap_of[0]]["locus_r"]) == 216
    with pytest.raises(ValueError, match="min_overlap"):
        ADJ.adjudicate_host([], c["lf"], c["rf"], c["fill_w"], c["fill_r"], context=48, read_len=40)
    with pytest.raises(ValueError, match="needs read_len"):
        ADJ.adjudicate_host([], c["lf"], c["rf"], c["fill_w"], c["fill_r"])
