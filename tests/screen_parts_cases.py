"""Inputs of test_gpu_screen_parts.py that screen_passb_cases.py does not have, with what the twins (screen_cand_twin.py) say about them.
numpy only."""
from functools import lru_cache

import numpy as np

import screen_cand_twin as W
import screen_passb_cases as K
import synth_small as S
from oracle import c_oracle as CO

L = K.L
N_MAX = 100_003
COUNTS = (1, 63, 65, 2047, 2049, N_MAX)      # below, at and beyond a tile (64), a batch (2 048), and many writers


def parts_layout(n_writers, cap, gs):
    """(first fill word, first pair word, words in all) of a parts buffer [count | fills | pairs | 64 words]: include/gapfill_hip.h."""
    at_fills = (W.NB * n_writers * 4 + 255) // 256 * 64
    at_pairs = at_fills + W.NB * n_writers * gs
    return at_fills, at_pairs, at_pairs + W.NB * n_writers * cap + 64


@lru_cache(maxsize=None)
def draft_b():
    """A second draft beside screen_passb_cases.draft(): other scaffolds, other flanks."""
    c = S.small_case(seed=31, n_pairs=4, n_scaffolds=3)
    return {"gaps": c["gaps"], "n_scaffolds": c["n_scaffolds"], "flanks": c["flanks"]}


@lru_cache(maxsize=1)
def reads_for_both_drafts():
    """N_MAX reads: the first half planted from draft A's flanks, the rest from draft B's — either draft finds hits, and not the same ones.
    A prefix of n reads is the input of the tests at n reads."""
    a = W.planted_case(N_MAX // 2, L, 51, K.draft()["flanks"], 5)
    b = W.planted_case(N_MAX - N_MAX // 2, L, 51, draft_b()["flanks"], 6)
    return {"packed": np.concatenate([a["packed"], b["packed"]]), "blob": a["blob"] + b["blob"]}


@lru_cache(maxsize=1)
def full_part_case():
    """screen_passb_cases.spill_case at k = 51: 6 000 poly-A reads behind the first 5 000 reads, under two writers (4 096 reads per
    iteration) — three probes each, all in bucket 0, against parts of a few hundred entries; gap 0's left flank ends in a poly-A run, so
    they are hits."""
    c = S.small_case(seed=43, n_pairs=3000)
    flanks = [list(f) for f in c["flanks"]]
    flanks[0][0] = flanks[0][0][:-60] + "A" * 60
    flanks = [tuple(f) for f in flanks]
    blob = c["reads_blob"][:5000 * L] + b"A" * (6000 * L) + c["reads_blob"][5000 * L:-3 * L]
    packed = W.pack_ascii(blob, L)
    n = packed.shape[0]
    return {"gaps": c["gaps"], "n_scaffolds": c["n_scaffolds"], "flanks": flanks, "blob": blob, "packed": packed, "n": n,
            "state": W.pass_a_state(packed, L, 51, 2), "exp": CO.screen_reads(blob, L, flanks, 51)}
