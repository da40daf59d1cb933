"""Repeated recruitment rounds of the device step (csrc/round_n.hip, second_round.py): the new entry points are declared, exported and
typed; the host twin second_round.rounds_host on a hand-made chain of reads; the constructor's refusals (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND_N = ["gf_contig_kmer_table_from_dev", "gf_round_carry_dev", "gf_round_pools_dev"]
K = 21


def test_round_n_entry_points_are_declared_exported_and_typed():
    import __graft_entry__ as G
    G.build()
    from gappadder_amd import _lib as B
    txt = open(os.path.join(ROOT, "include", "gapfill_hip.h")).read()
    L = ctypes.CDLL(B.LIB_PATH)
    lib = B.lib()
    for name in ROUND_N:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert getattr(lib, name).argtypes, name
    assert (B.R2_NEW, B.R2_GROWN, B.R2_GATED) == (12, 13, 14) and B.R2_WORDS == 16


# ---- the twin on a chain ----------------------------------------------------------------------------------------------------------
# Gap 0: a sequence of 400 bases; the first pick leaves one contig, its first 100 bases.  Candidate pair j of library 0 holds the bases
# [60 + 40 j, 160 + 40 j) twice (both mates alike): it overlaps pair j - 1 by 60 >= K bases and the contig only for j = 0, so every round
# adds exactly one link; both anchors lie in link 5 and in no other.
# Gap 1: the same with a chain of two links and no more: its recruits stop, it stays open.
# Gap 2: closed; a pair shares a k-mer with its contig and must never be recruited.
def _chain():
    rng = np.random.default_rng(5)
    text = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    seq = [text(400), text(400), text(200)]
    link = lambda g, j: seq[g][60 + 40 * j:160 + 40 * j]
    cand = {(0, j): (link(0, j), link(0, j)) for j in range(6)}
    cand.update({(1, 100 + j): (link(1, j), link(1, j)) for j in range(2)})      # (a second library)
    cand[(0, 50)] = (seq[2][20:120], seq[2][20:120])
    cand[(0, 51)] = (text(100), "N" * 100)                                      # noise and a fully masked mate
    contigs = [(0, seq[0][:100]), (1, seq[1][:100]), (2, seq[2]), (0, ""), (1, seq[1][:K - 1])]     # a tombstone, a contig shorter than k
    pools = {0: [seq[0][:100]], 1: [seq[1][:100]], 2: [seq[2][:100]]}
    anchors = {0: (seq[0][270:300], seq[0][330:360]), 1: (seq[1][270:300], seq[1][330:360])}
    return seq, cand, contigs, pools, anchors


def _toys(anchors, calls):
    def assemble(g, rows):          # every distinct row is a contig
        calls.append((g, len(rows)))
        return sorted(set(rows))

    def pick(g, texts):             # some contig holds both anchors
        a, b = anchors[g]
        return any(a in t and b in t for t in texts)
    return assemble, pick


def test_rounds_host_adds_one_link_per_round_and_closes_when_the_chain_completes():
    from gappadder_amd.second_round import rounds_host
    seq, cand, contigs, pools, anchors = _chain()
    calls = []
    assemble, pick = _toys(anchors, calls)
    rounds, run = rounds_host(pools, cand, contigs, {0, 1}, K, assemble, pick, 10)
    assert len(rounds) == 10
    # gap 0: link j arrives in round j + 1 and is the only new pair of the gap in that round
    for j in range(6):
        assert rounds[j]["new"][0] == {(0, j)}, j
        assert 0 in rounds[j]["grown"]
        assert rounds[j]["reads"][0] == [(0, i) for i in range(j + 1)]         # cumulative, in (library, pair) order
    # the anchors [270, 300) and [330, 360) lie in link 5 = [260, 360): the gap closes in round 6, not before
    assert [0 in d["closed"] for d in rounds[:7]] == [False] * 5 + [True, False]
    # gap 1: two links, then nothing: open, and not assembled again after round 2
    assert rounds[0]["new"][1] == {(1, 100)} and rounds[1]["new"][1] == {(1, 101)}
    assert all(1 not in d["grown"] and 1 not in d["new"] for d in rounds[2:])
    assert [g for g, _ in calls].count(1) == 2
    assert all(1 not in d["closed"] for d in rounds)
    # gap 2 is closed: its contig recruits nothing, whatever shares a k-mer with it
    assert all(2 not in d["hits"] and 2 not in d["grown"] for d in rounds)
    # round 7 finds gap 0 closed and gap 1 without contigs: it grows nothing, it is the empty round that is counted; 8..10 are gated
    assert run == 7 and rounds[6]["grown"] == [] and not rounds[6]["gated"]
    assert all(d["gated"] and not d["contigs"] for d in rounds[7:])
    # round 3's table holds round 2's contigs (the pool's rows: the round-1 row, links 0 and 1): it hits links 0, 1, 2, and 2 alone is new
    assert rounds[2]["hits"][0] == {(0, 0), (0, 1), (0, 2)} and rounds[2]["new"][0] == {(0, 2)}


def test_rounds_host_stops_at_max_rounds_and_counts_them():
    from gappadder_amd.second_round import rounds_host
    seq, cand, contigs, pools, anchors = _chain()
    assemble, pick = _toys(anchors, [])
    rounds, run = rounds_host(pools, cand, contigs, {0, 1}, K, assemble, pick, 3)
    assert run == 3 and len(rounds) == 3 and not any(d["gated"] for d in rounds)
    assert not any(d["closed"] for d in rounds)
    # nothing open: the first round is the empty one
    rounds, run = rounds_host(pools, cand, contigs, set(), K, assemble, pick, 4)
    assert run == 1 and [d["gated"] for d in rounds] == [False, True, True, True]


def test_constructor_refusals():
    from gappadder_amd.pipeline import Pipeline
    kk = [(31, 29)]
    for bad in (0, 17, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="recruit_rounds"):
            Pipeline(None, 4, 100, kk, second_round=True, recruit_rounds=bad)
    with pytest.raises(ValueError, match="second_round"):
        Pipeline(None, 4, 100, kk, recruit_rounds=2)
