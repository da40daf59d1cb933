"""The twins of the partitioned screen filter (screen_cand_twin.py) against the oracle, and the preconditions of the GPU tests that use them
(test_gpu_screen_passb.py) on the very inputs those tests build: what the tests need of their inputs is decided here, without a GPU."""
import numpy as np
import pytest

import probe_column_twin as T
import screen_cand_twin as W
import screen_passb_cases as K
import synth_small as S
from oracle import c_oracle as CO


@pytest.mark.parametrize("k,seed", [(31, 7), (51, 43)])
def test_every_oracle_hit_is_a_candidate(k, seed):
    """A read that shares a k-mer with a flank holds a probe that is a flank 16-mer with the flank's bases behind it: the oracle's reads
    are candidates, with and without the neighbour check, and the check only ever removes candidates."""
    c = S.small_case(seed=seed, n_pairs=4000)
    L = c["L"]
    packed = W.pack_ascii(c["reads_blob"], L)
    hits = np.unique(CO.screen_reads(c["reads_blob"], L, c["flanks"], k, min_hits=1)["read"])
    assert len(hits) > 100
    seeds = W.flank_seed_set(c["flanks"], k)
    assert len(seeds[0]) > 4000 and (np.diff(seeds[0].astype(np.int64)) > 0).all()
    got = {}
    for ext_allowed in (True, False):
        assert (T.geometry(L, k, ext_allowed)[3] > 0) == ext_allowed
        cand, qual = W.candidates(packed, L, k, c["flanks"], ext_allowed, seeds=seeds)
        assert np.isin(hits, cand).all(), (k, ext_allowed, np.setdiff1d(hits, cand)[:8])
        assert np.array_equal(cand, np.nonzero(qual.any(axis=1))[0])
        got[ext_allowed] = cand
    loose, _ = W.candidates(packed, L, k, c["flanks"], True, check_ext=False, seeds=seeds)
    assert np.isin(got[True], loose).all() and len(loose) >= len(got[True])


def test_neighbour_masks_on_a_hand_made_flank():
    """Run ends (room 0 and 1), a reverse-strand occurrence, a palindrome and a non-ACGT break, checked by hand."""
    pal = "ACGTACGTACGTACGT"                       # its own reverse complement
    assert W.word16(pal) == W.word16(pal.translate(W._COMP)[::-1])
    run = "G" + pal + "CA"                         # 19 bases
    keys, left, right = W.flank_seed_set([(run + "N" + "A" * 18, "acgt")], 18)
    d = {int(x): (int(l), int(r)) for x, l, r in zip(keys, left, right)}
    # the palindrome: text reading left = G with nothing behind (room 1), right = C then A; the other reading swaps and complements:
    # left = G then T (complement of C, A), right = C with anything (complement of G)
    lp, rp = d[W.word16(pal)]
    assert lp == (0xF << (4 * 2)) | (1 << (4 * 2 + 3)) and rp == (1 << (4 * 1 + 0)) | (0xF << (4 * 1))
    # poly-A: the canonical form is A x 16 (not T x 16); three occurrences in the run of 18: rooms (0, 2), (1, 1), (2, 0)
    la, ra = d[0]
    assert la == (0xF << 0) | (1 << 0) and ra == (1 << 0) | (0xF << 0)
    # the run's first 16-mer GACGT...ACG and its third, CGTAC...GTC, are each other's reverse complement: one key, the canonical form the
    # third's text.  Third: left A then G, right A alone (room 1).  First (reverse reading): nothing left of the text -> no statement about
    # the canonical right; the text's right T then C -> canonical left A then G, the same bit.
    w, rc = W.word16(run[:16]), W.word16(run[2:18])
    assert rc == W.word16(run[:16].translate(W._COMP)[::-1]) < w
    assert d[rc] == (1 << (4 * 0 + 2), 0xF << 0)
    # the run's last 16-mer GTACG...TCA: nothing right of the text, left C then A
    w3, rc3 = W.word16(run[3:19]), W.word16(run[3:19].translate(W._COMP)[::-1])
    assert d[min(w3, rc3)] == ((1 << (4 * 1 + 0), 0) if w3 < rc3 else (0, 1 << (4 * 2 + 3)))
    assert len(keys) == 3 + 1                                       # three keys of the first run's four 16-mers, one of the second run; none of "acgt"


@pytest.mark.parametrize("k", [31, 41, 51])
def test_pass_a_state_holds_every_probe_once(k):
    c = K.draft()
    L, n = 150, 10_007
    case = W.planted_case(n, L, k, c["flanks"], seed=5)
    n_probes = T.geometry(L, k)[2]
    for nw in (1, 2, 5):
        st = W.pass_a_state(case["packed"], L, k, nw)
        assert st["count"].sum() == n * n_probes == len(st["pairs"]) == len(st["runs"])
        assert st["fills"].shape == (256 * nw, st["n_groups"] + 1) and (st["fills"][:, 0] == 0).all()
        assert (np.diff(st["runs"]) >= 0).all() and np.array_equal(np.bincount(st["runs"], minlength=256 * nw * st["n_groups"]),
                                                                   np.diff(st["fills"].astype(np.int64), axis=1).ravel())
        assert st["n_groups"] == W.plan(n, L, k, 256, nw)["n_groups"]
        # a pair's entry names its read's octet inside the batch: with the run (-> writer, iteration) the octet of the read follows
        octets = set()
        for e, run in zip(st["pairs"][::97], st["runs"][::97]):
            part, g = divmod(int(run), st["n_groups"])
            octets.add(((g // st["n_grp"]) * nw + part % nw) * 256 + (int(e) & 255))
        assert max(octets) <= (n - 1) // 8 and len(octets) > 100


def test_default_plan_of_the_twin_is_the_documented_one():
    """plan() with no writer cap, at sizes whose plans are on record in DESIGN.md / the issue: 100 000 reads under one writer are 49 groups."""
    p = W.plan(100_000, 150, 51, 256, 1)
    assert (p["n_writers"], p["n_iter"], p["n_groups"], p["n_grp"]) == (1, 49, 49, 1) and p["cap"] % 64 == 0 and 1500 < p["cap"] < 1700
    q = W.plan(100_000, 150, 51, 256)
    assert (q["n_writers"], q["n_iter"]) == (49, 1) and W.plan(100_000, 150, 51, 256, 0) == q and W.plan(100_000, 150, 51, 256, 64) == q


@pytest.mark.parametrize("n,writers", K.TRIP_RUNS)
def test_trip_runs_meet_their_preconditions(n, writers):
    """Case (a) of the GPU tests, per run and seed geometry: the input is sized so that every precondition the GPU test asserts on the dumped
    state holds for the twin's state (the two are asserted equal there)."""
    assert n % 8 and n % 64 and n % 2048
    for ext in (1, 0):
        r = K.trip_run(n, writers, ext)
        assert len(r["confirmed"]) > 0.2 * n and np.isin(r["confirmed"], r["cand"]).all()
        f = W.tail_facts(r["state"]["count"], r["state"]["fills"])
        assert (r["state"]["count"] > 1024).mean() > 0.9, f          # nearly every part takes more than one trip
        assert W.planted_in_last_group(r["state"], r["state"]["count"], r["state"]["fills"], r["confirmed"], r["qual"]) >= 0.5
        assert r["state"]["count"].max() < W.plan(n, K.L, 51, 256, writers, bool(ext))["cap"]      # no part runs full: the state compares whole


def test_trip_runs_together_meet_the_union_preconditions():
    """What each run is to contribute (TRIP_WANT: the GPU test asserts it on the run's dumped counts) adds up to every tail class and a run
    beyond two full trips — and each run does contribute it, with every residue of count % 4."""
    assert set().union(*(t for t, _ in K.TRIP_WANT.values())) == {0, 1, 2, 3} and any(top for _, top in K.TRIP_WANT.values())
    for n, writers in K.TRIP_RUNS:
        for ext in (1, 0):
            st = K.trip_run(n, writers, ext)["state"]
            f = W.tail_facts(st["count"], st["fills"])
            assert K.TRIP_WANT[n][0] <= f["tails"] and f["mod4"] == {0, 1, 2, 3} and (f["max"] > 2048) == K.TRIP_WANT[n][1], (n, writers, ext, f)


@pytest.mark.parametrize("k", [51, 31, 41])
def test_short_list_inputs(k):
    r = K.short_list_run(k)
    n_groups = r["state"]["n_groups"]
    assert n_groups >= 20 * r["state"]["n_grp"] and r["state"]["n_grp"] == (1 if k == 51 else 2)
    on_list = W.exact_set_pairs(r["state"]["pairs"], r["state"]["runs"], 1, n_groups, K.seeds(k)[0])
    assert on_list > 4 * 1024 and on_list >= len(r["confirmed"])
    assert np.isin(r["cand"], r["loose"]).all() and len(r["loose"]) > len(r["cand"])          # the neighbour check removes decoys


def test_spill_input_fills_the_poly_a_part_after_the_first_iteration():
    r = K.spill_case()
    st, p = r["state"], W.plan(r["n"], K.L, 31, 256, 2)
    assert p["n_writers"] == 2 and st["n_groups"] == p["n_groups"] > st["n_grp"] == 2
    assert K.spill_facts(st, p["cap"])["first_full_group"] >= st["n_grp"]
    assert len(np.unique(r["exp"]["read"])) > 60000 and np.isin(np.unique(r["exp"]["read"]), r["cand"]).all()


def test_crowded_home_groups_input():
    r = K.crowded_case()
    assert len(r["keys"]) >= 32
    # every crowded key is planted, and found by the twin in a confirmed read
    bases = W.unpack(r["case"]["packed"])
    first, stride, n_probes, _ = T.geometry(K.L, 51)
    seen = set()
    for j in range(n_probes):
        w = T.canon16(W._words(bases, first + j * stride)).astype(np.uint32)
        rows = r["confirmed"][r["qual"][r["confirmed"], j]]
        seen |= set(w[rows].tolist())
    assert set(r["keys"].tolist()) <= seen
