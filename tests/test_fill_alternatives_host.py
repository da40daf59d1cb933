"""The host side of the fill alternatives: the twin fill_alternatives.alts_host on hand-derived cases
(tests/fill_alt_cases.py), its distance against a textbook Levenshtein, check_params, the CLI keys in main.parse_configuration, and the
writers of fill_alternatives.tsv and alt_seqs.fa on a made-up Results."""
import random
import types

import numpy as np
import pytest

import fill_alt_cases as AC
from test_pair_span_config_host import _config

CASES = AC.cases()


def record(w):
    """The hand-written dictionary as a gf_fill_alt record (fields it leaves out are zero)."""
    from gappadder_amd import _lib as B
    r = np.zeros(1, dtype=B.FILL_ALT)
    for k, v in (w or {}).items():
        r[0][k] = v
    return r[0]


def _check(got, cs, index):
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_alternatives as FA
    recs, per, stats = got
    want, want_per, want_stats = AC.expected(cs, index)
    for g, (c, w) in enumerate(zip(cs, want)):
        assert recs[g].tobytes() == record(w).tobytes(), (c["name"], recs[g], record(w))
        assert FA.contested(recs[g]) == bool(w and w["flags"] & AC.HAS_RIVAL), c["name"]
    assert len(per) == len(want_per)
    for at, p in want_per.items():
        assert tuple(int(x) for x in per[at]) == p, (at, per[at], p)
    assert stats == want_stats
    assert recs.dtype == B.FILL_ALT and per.dtype == B.FILL_ALT_CONTIG


@pytest.mark.parametrize("interleave", [False, True])
def test_twin_gives_the_hand_derived_records_and_statistics(interleave):
    from gappadder_amd import fill_alternatives as FA
    contigs, flanks, best, index = AC.assemble(CASES, interleave)
    got = FA.alts_host(contigs, flanks, best, AC.ANCHORS, AC.B)
    assert got[0].dtype.itemsize == 48 and got[1].dtype.itemsize == 8 and len(got[0]) == len(CASES) >= 30
    _check(got, CASES, index)
    again = FA.alts_host(contigs, flanks, best)          # the defaults are the cases' parameters
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2]
    assert got[2]["lost"] == 4 and got[2]["outranked"] == 4 and got[2]["contested"] >= 15


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_alone(case):
    from gappadder_amd import fill_alternatives as FA
    if isinstance(case["best"], tuple) and isinstance(case["best"][2], tuple):       # (names a contig of another case: it needs that case)
        cs = [next(c for c in CASES if c["name"] == case["best"][2][0]), case]
    else:
        cs = [case]
    contigs, flanks, best, index = AC.assemble(cs)
    _check(FA.alts_host(contigs, flanks, best, AC.ANCHORS, AC.B), cs, index)


def test_the_hand_written_words_are_the_picks_own():
    """Where a case is not doctored, its word is the largest word over its candidates: what the pick's atomicMax keeps."""
    from gappadder_amd import fill_alternatives as FA
    contigs, flanks, best, index = AC.assemble(CASES)
    for g, c in enumerate(CASES):
        words = []
        for n in range(len(c["contigs"])):
            k = FA.candidate(contigs[index[(g, n)]][1].encode(), flanks[g][0].encode(), flanks[g][1].encode(), *AC.ANCHORS)
            if k is not None:
                words.append(FA.pick_word(k[0], k[1], index[(g, n)], k[2]))
        assert (max(words) == best[g]) == (not c["doctored"]), c["name"]


def test_first_skips_the_candidates_before_it_but_finds_the_winner():
    from gappadder_amd import fill_alternatives as FA
    case = next(c for c in CASES if c["name"] == "the runner-up is the longer span")
    contigs, flanks, best, _ = AC.assemble([case])
    recs, per, st = FA.alts_host(contigs, flanks, best, first=2)          # the winner at 0 and the closer rival at 1 lie before `first`
    assert int(recs[0]["contig"]) == 0 and int(recs[0]["rival"]) == 2 and int(recs[0]["n_candidates"]) == 2 and int(recs[0]["len_min"]) == 159
    assert [int(p["cls"]) for p in per] == [AC.WINNER, AC.NONE, AC.NEAR] and st["candidates"] == 2
    recs, per, st = FA.alts_host(contigs, flanks, best, first=3)
    assert int(recs[0]["n_candidates"]) == 1 and int(recs[0]["flags"]) == 0 and int(recs[0]["fill_len"]) == 160 and st["contested"] == 0


def test_a_single_anchor_length_and_a_smaller_bound():
    from gappadder_amd import fill_alternatives as FA
    by = {c["name"]: c for c in CASES}
    contigs, flanks, best, _ = AC.assemble([by["lower"]])
    recs, _, st = FA.alts_host(contigs, flanks, best, (30,))              # no short level: the broken contig is no candidate at all
    assert int(recs[0]["n_candidates"]) == 1 and st["lower"] == 0
    contigs, flanks, best, _ = AC.assemble([by["short level only"]])
    assert int(FA.alts_host(contigs, flanks, best, (30,))[0][0]["flags"]) == AC.LOST
    contigs, flanks, best, _ = AC.assemble([by["16 substitutions"]])
    assert int(FA.alts_host(contigs, flanks, best, max_dist=15)[0][0]["dist"]) == 0xFFFF
    assert int(FA.alts_host(contigs, flanks, best, max_dist=16)[0][0]["dist"]) == 16


def _textbook(a, b):
    """Wagner-Fischer, the full matrix."""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D[len(a)][len(b)]


def random_pairs(seed=25, n=200, longest=120):
    """Seeded pairs of fills: a random text and a copy with 0 .. 40 random edits (some pairs unrelated, some empty)."""
    rng = random.Random(seed)
    out = []
    for x in range(n):
        a = AC.rnd(rng, rng.randrange(longest + 1))
        if x % 10 == 9:
            b = AC.rnd(rng, rng.randrange(longest + 1))
        else:
            b = list(a)
            for _ in range(rng.choice((0, 1, 1, 1, 2, 4, 5, 6, 16, 30, 31, 32, 40))):
                op, at = rng.randrange(3), rng.randrange(len(b) + 1)
                if op == 0 and at < len(b):
                    b[at] = rng.choice("ACGT")
                elif op == 1 and at < len(b):
                    del b[at]
                elif len(b) < longest:
                    b.insert(at, rng.choice("ACGT"))
            b = "".join(b)
        out.append((a, b))
    return out


@pytest.mark.parametrize("bound", [1, 5, 31])
def test_distance_is_the_textbook_levenshtein_thresholded(bound):
    from gappadder_amd import fill_alternatives as FA
    n_near = 0
    for a, b in random_pairs():
        d = _textbook(a, b)
        lcp, lcs, got = FA.distance(a.encode(), b.encode(), bound)
        assert got == (d if d <= bound else 0xFFFF), (a, b, d, got)
        assert a[:lcp] == b[:lcp] and (lcp == min(len(a), len(b)) or a[lcp] != b[lcp]) and lcp + lcs <= min(len(a), len(b))
        assert lcs == 0 or a[len(a) - lcs:] == b[len(b) - lcs:]
        n_near += 0 < d <= bound
    assert n_near >= 10


@pytest.mark.parametrize("v", [0, 32, -1, 2.5, "16", True, None])
def test_check_params_refuses(v):
    from gappadder_amd import fill_alternatives as FA
    with pytest.raises(ValueError, match="alt_max_dist"):
        FA.check_params(v)


def test_check_params_takes_the_edges():
    from gappadder_amd import fill_alternatives as FA
    assert FA.check_params() == 16 and FA.check_params(1) == 1 and FA.check_params(31) == 31
    for bad in ((33, 15), (30, 7), (15, 30), (7,)):
        with pytest.raises(ValueError):
            FA.alts_host([], [], [], bad)


# ---- the CLI keys -------------------------------------------------------------------------------------------------------------------

def test_fill_alternatives_is_off_by_default_with_the_twins_default(tmp_path):
    from gappadder_amd import fill_alternatives as FA
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path))
    assert cfg["fill_alternatives"] is False and cfg["fill_alternatives_max_dist"] == FA.MAX_DIST == 16


def test_fill_alternatives_and_its_parameter_are_read(tmp_path):
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path, fill_alternatives=True, fill_alternatives_max_dist=5))
    assert cfg["fill_alternatives"] is True and cfg["fill_alternatives_max_dist"] == 5
    for v in (1, 31):
        assert parse_configuration(_config(tmp_path, fill_alternatives_max_dist=v))["fill_alternatives_max_dist"] == v


@pytest.mark.parametrize("v", [0, 32, "16", True, 2.5])
def test_a_value_out_of_range_makes_main_exit_with_a_message(tmp_path, v):
    from gappadder_amd import main as M
    cfgp = _config(tmp_path, fill_alternatives=True, fill_alternatives_max_dist=v)
    with pytest.raises(SystemExit) as e:
        M.parse_configuration(cfgp)
    assert "fill_alternatives_max_dist" in str(e.value)
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert "fill_alternatives_max_dist" in str(e.value)


# ---- the writers --------------------------------------------------------------------------------------------------------------------

def made_up_results():
    """Four gaps from the cases: a contested one with a reverse rival, one with only identical candidates, one with a single candidate and
    an open one; the records are the twin's.  Returns (stub pipeline, Results, cases)."""
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_alternatives as FA
    from gappadder_amd.pipeline import Pipeline, Results
    by = {c["name"]: c for c in CASES}
    cs = [by["rival on the reverse strand"], by["the same contig twice"], by["one candidate"], by["open gap"]]
    contigs, flanks, best, index = AC.assemble(cs)
    res = Results()
    ctg = np.zeros(len(contigs), dtype=B.CONTIG)
    off = 0
    for i, (g, s) in enumerate(contigs):
        ctg[i] = (g, 31, 29, len(s) - 30, len(s), 3 * (len(s) - 30), 0, off)
        off += len(s)
    res.contigs, res.seq, res.best, res.ctg_pick = ctg, "".join(s for _, s in contigs).encode(), np.array(best, dtype=np.uint64), None
    res.keys = ["0_%d" % (g + 1) for g in range(len(cs))]
    res.alts, res.alt_contigs, res.alt_stats = FA.alts_host(contigs, flanks, best)
    pipe = types.SimpleNamespace(gf=types.SimpleNamespace(flanks=flanks))
    pipe._pick_cut = lambda *a: Pipeline._pick_cut(pipe, *a)
    pipe.alternative_sequences = lambda r: Pipeline.alternative_sequences(pipe, r)
    pipe.picked_sequences = lambda r: Pipeline.picked_sequences(pipe, r)
    return pipe, res, cs


def test_the_writers_on_a_made_up_results():
    from gappadder_amd import device_collect as DC
    pipe, res, cs = made_up_results()
    tsv, fa = DC.fill_alternatives_files(pipe, res, [(31, 29)])
    lines = [l.split("\t") for l in tsv.splitlines()]
    assert lines[0] == ["gap"] + list(DC.ALT_FIELDS) + ["contested", "name", "rival_name"] and "reserved" not in lines[0]
    assert [l[0] for l in lines[1:]] == ["0_1", "0_2"]                      # more than one candidate: not the single one, not the open gap
    rows = [dict(zip(lines[0], l)) for l in lines[1:]]
    for g, row in enumerate(rows):
        assert all(int(row[f]) == int(res.alts[g][f]) for f in DC.ALT_FIELDS)
    assert rows[0]["contested"] == "1" and rows[1]["contested"] == "0" and rows[1]["rival_name"] == ""
    picked = DC.picked_names(res, [(31, 29)])
    assert rows[0]["name"] == picked[0] and rows[1]["name"] == picked[1]
    assert rows[0]["rival_name"].startswith("0_1_31_29_NODE_") and rows[0]["rival_name"] != rows[0]["name"]
    # the sequences: the contested gap alone, named with the picked name; the rival's sequence is the winner's with the one substitution,
    # cut by the same rule and turned to the draft's strand
    recs = fa.split(">")[1:]
    assert len(recs) == 1 and recs[0].split("\n")[0] == picked[0] + "_alt"
    rival_seq = "".join(recs[0].split("\n")[1:])
    assert all(len(l) <= 60 for l in recs[0].split("\n"))
    winner_seq = pipe.picked_sequences(res)[0][1]
    # (ContigsSelection's cut keeps one anchor base: the right anchor's first behind a forward selection, the left anchor's last in front
    # of a reverse one; between them the 140 bases of the two fills differ in the one substituted column)
    assert len(rival_seq) == len(winner_seq) == 141 and [x for x in range(140) if rival_seq[1 + x] != winner_seq[x]] == [20]
    seqs = pipe.alternative_sequences(res)
    assert list(seqs) == [0] and seqs[0][0] == int(res.alts[0]["rival"]) and seqs[0][1] == rival_seq and seqs[0][2] is True
    res.alts = None
    with pytest.raises(ValueError, match="alternatives=True"):
        pipe.alternative_sequences(res)
