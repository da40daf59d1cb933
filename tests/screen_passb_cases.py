"""The inputs of test_gpu_screen_passb.py with what the twins (screen_cand_twin.py) say about them.  numpy only: the host tests
(test_screen_cand_twin_host.py) check on these very inputs that the preconditions of the GPU tests hold."""
from functools import lru_cache

import numpy as np

import screen_cand_twin as W
import synth_small as S
from oracle import c_oracle as CO

L = 150
# Case (a): (reads, writers).  A part of bucket b and writer w holds about reads * 3 / (256 * writers) pairs (k = 51: three probes), a
# trip of pass B 1 024: the four runs put the parts' counts around 1 344, 1 800, 2 231 and 1 176 — tail classes 0/1, 2/3, beyond two full
# trips, and two writers.  No count is a multiple of 8, 64 or 2 048, and every writer's last batch of 2 048 reads is nearly full, so that
# most parts' last group holds two dozen pairs (two of them planted, on average).
TRIP_RUNS = [(56 * 2048 - 5, 1), (75 * 2048 - 11, 1), (93 * 2048 - 77, 1), (49 * 4096 - 13, 2)]
# What every run contributes, asserted on its dumped counts: tail classes ((count - 1) % 1024) // 256 among its parts of more than 1 024
# pairs, and whether a part passes 2 048 pairs.  Together: every tail class, and one run beyond two full trips.
TRIP_WANT = {TRIP_RUNS[0][0]: ({0, 1}, False), TRIP_RUNS[1][0]: ({2, 3}, False), TRIP_RUNS[2][0]: ({0}, True), TRIP_RUNS[3][0]: ({0}, False)}


@lru_cache(maxsize=None)
def draft(n_scaffolds=3):
    """A synth_small draft: its gaps and flanks (nine gaps, 18 flanks of 295 bases)."""
    c = S.small_case(seed=29, n_pairs=4, n_scaffolds=n_scaffolds)
    return {"gaps": c["gaps"], "n_scaffolds": c["n_scaffolds"], "flanks": c["flanks"]}


@lru_cache(maxsize=None)
def seeds(k, n_scaffolds=3):
    return W.flank_seed_set(draft(n_scaffolds)["flanks"], k)


def _run(n, k, writers, ext, seed, flanks, sd, **kw):
    case = W.planted_case(n, L, k, flanks, seed, ext_allowed=bool(ext), **kw)
    cand, qual = W.candidates(case["packed"], L, k, flanks, bool(ext), seeds=sd)
    return {"case": case, "cand": cand, "qual": qual, "confirmed": W.confirmed(case["planted"], qual),
            "state": W.pass_a_state(case["packed"], L, k, writers, ext_allowed=bool(ext)) if writers else None}


@lru_cache(maxsize=2)
def trip_run(n, writers, ext):
    return _run(n, 51, writers, ext, 7 * n + ext, draft()["flanks"], seeds(51))


@lru_cache(maxsize=1)
def short_list_run(k):
    """Case (b): 50 003 reads under one writer are 25 iterations (25 or 50 groups), the planted pairs several times the short pair lists."""
    r = _run(50_003, k, 1, 1, 11 * k, draft()["flanks"], seeds(k))
    r["loose"] = W.candidates(r["case"]["packed"], L, k, draft()["flanks"], True, check_ext=False, seeds=seeds(k))[0]
    return r


@lru_cache(maxsize=1)
def spill_case():
    """Case (c): 60 000 poly-A reads behind the first 5 000 reads — under two writers (4 096 reads per iteration) none of them in the first
    iteration — all in ONE bucket; gap 0's left flank ends in a poly-A run, so they are hits."""
    c = S.small_case(seed=43, n_pairs=3000)
    flanks = [list(f) for f in c["flanks"]]
    flanks[0][0] = flanks[0][0][:-60] + "A" * 60
    flanks = [tuple(f) for f in flanks]
    blob = c["reads_blob"][:5000 * L] + b"A" * (60000 * L) + c["reads_blob"][5000 * L:-3 * L]
    packed = W.pack_ascii(blob, L)
    sd = W.flank_seed_set(flanks, 31)
    return {"gaps": c["gaps"], "n_scaffolds": c["n_scaffolds"], "flanks": flanks, "blob": blob, "packed": packed, "n": packed.shape[0],
            "cand": W.candidates(packed, L, 31, flanks, True, seeds=sd)[0], "loose": W.candidates(packed, L, 31, flanks, True, check_ext=False, seeds=sd)[0],
            "state": W.pass_a_state(packed, L, 31, 2), "exp": CO.screen_reads(blob, L, flanks, 31)}


def spill_facts(state, cap):
    """The poly-A bucket (key 0 -> bucket 0) of every writer: the first group whose pairs pass the part's capacity."""
    n_writers = state["count"].shape[0] // W.NB
    over = state["fills"][:n_writers, 1:].astype(np.int64) > cap
    assert over.any(axis=1).all()
    return {"first_full_group": int(np.argmax(over, axis=1).min())}


@lru_cache(maxsize=1)
def crowded_case():
    """Case (d): the keys whose home group of the grouped exact set is the home of more than four keys, every one planted; the draft grows
    until there are 32 of them."""
    n_scaffolds = 3
    while len(W.crowded_keys(seeds(51, n_scaffolds)[0])) < 32:
        n_scaffolds += 3
    keys = W.crowded_keys(seeds(51, n_scaffolds)[0])
    r = _run(20_011, 51, 0, 1, 13, draft(n_scaffolds)["flanks"], seeds(51, n_scaffolds), only_keys=keys)
    r.update(keys=keys, draft=draft(n_scaffolds))
    return r
