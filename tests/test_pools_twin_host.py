"""The definition of the per-gap pools (tests/pools_twin.py) against brute force, without a device: the twin is what
tests/test_gpu_pools.py holds the kernels to, so the definition itself stays under test."""
import numpy as np
import pytest

import pools_twin as T
from gappadder_amd import _lib as B

N_GAPS, N_READS, RB = 11, 60, 5


def _brute(keys, n_gaps, reads, pool_cap):
    """A dict of lists built key by key; a read enters a gap's list once; lists ordered left mates by pair, then right mates by pair."""
    lists = {}
    for k in keys.tolist():
        g, r = k >> 32, k & 0xFFFFFFFF
        if g >= n_gaps:
            continue
        lst = lists.setdefault(g, [])
        if r not in lst:
            lst.append(r)
    off, ids = [0], []
    for g in range(n_gaps):
        lst = lists.get(g, [])
        left = [r for r in lst if r % 2 == 0]
        right = [r for r in lst if r % 2 == 1]
        left.sort(key=lambda r: r // 2)
        right.sort(key=lambda r: r // 2)
        ids += left + right
        off.append(len(ids))
    total = len(ids)
    ids = ids[:pool_cap]
    rows = [bytes(reads[r]) if r < len(reads) else bytes(reads.shape[1]) for r in ids]
    return off, ids, rows, total > pool_cap


def _keys(seed):
    rng = np.random.RandomState(seed)
    gap = rng.randint(0, N_GAPS, 300)
    gap[rng.rand(300) < 0.3] = 4                                          # one deep gap
    read = rng.randint(0, N_READS, 300)
    keys = T.make_keys(gap, read)
    keys = np.concatenate([keys, keys[rng.randint(0, 300, 80)],           # duplicates
                           T.make_keys([3, 3, 3, 3], [10, 11, 11, 10]),    # both mates of one pair, twice
                           T.make_keys([N_GAPS, N_GAPS + 1, T.NO_GAP, T.NO_GAP], [1, 2, 3, 0xFFFFFFFF])])   # gaps out of range
    rng.shuffle(keys)
    keys = keys[(keys >> np.uint64(32)) != np.uint64(7)]                  # and an empty gap in the middle
    return keys, rng.randint(0, 256, (N_READS, RB)).astype(np.uint8)


def _check(keys, reads, cap, n_gaps=N_GAPS):
    off, ids, rows, flag = T.build_pools(keys, n_gaps, reads, cap)
    b_off, b_ids, b_rows, b_flag = _brute(keys, n_gaps, reads, cap)
    assert off.dtype == np.uint64 and off.tolist() == b_off
    assert ids.dtype == np.uint32 and ids.tolist() == b_ids
    assert rows.shape == (len(b_ids), reads.shape[1]) and [bytes(r) for r in rows] == b_rows
    assert flag == b_flag
    return off, ids


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_equals_the_key_by_key_definition_at_every_capacity_cut(seed):
    keys, reads = _keys(seed)
    off, ids = _check(keys, reads, 10 ** 6)
    total = int(off[-1])
    assert total == len(ids) > 100 and off[8] == off[7] and off[5] - off[4] > 40
    in_gap = int(off[4]) + 3
    for cap in (0, 1, in_gap, int(off[4]), int(off[5]), total - 1, total, total + 3):      # 0, inside a gap, at gap edges, exact, roomy
        _check(keys, reads, cap)
    assert T.build_pools(keys, N_GAPS, reads, total)[3] is False and T.build_pools(keys, N_GAPS, reads, total - 1)[3] is True


def test_twin_orders_both_mates_of_a_pair_and_drops_duplicates():
    reads = np.arange(40, dtype=np.uint8).reshape(8, 5)
    keys = T.make_keys([1, 1, 1, 1, 1, 0, 1], [5, 4, 1, 4, 0, 7, 5])
    off, ids, rows, flag = T.build_pools(keys, 2, reads, 8)
    assert off.tolist() == [0, 1, 5] and ids.tolist() == [7, 0, 4, 1, 5] and not flag          # left mates 0, 4; then right mates 1, 5
    assert (rows == reads[[7, 0, 4, 1, 5]]).all()
    _check(keys, reads, 8, n_gaps=2)


def test_twin_drops_gaps_out_of_range_and_counts_reads_out_of_range():
    reads = np.full((4, 3), 9, dtype=np.uint8)
    keys = T.make_keys([0, 2, 3, T.NO_GAP, 1], [2, 2, 2, 2, 77])
    off, ids, rows, flag = T.build_pools(keys, 2, reads, 4)
    assert off.tolist() == [0, 1, 2] and ids.tolist() == [2, 77] and not flag
    assert rows.tolist() == [[9, 9, 9], [0, 0, 0]]                       # read 77 of 4: counted, listed, its row undefined (zeros here)
    assert T.build_pools(np.zeros(0, np.uint64), 3, reads, 0)[0].tolist() == [0, 0, 0, 0]
    _check(keys, reads, 4, n_gaps=2)


def test_twin_key_producers():
    hits = np.array([(3, 10), (0, 7)], dtype=B.HIT)
    assert T.keys_from_screen(hits, 0).tolist() == [(3 << 32) | 10, 7]
    assert T.keys_from_screen(hits, 1).tolist() == [(3 << 32) | 10, (3 << 32) | 11, 7, 6]
    recs = np.zeros(3, dtype=B.ALNREC)
    recs["read"] = [20, 0xFFFFFFFF, 31]
    th = np.array([(0, 1, 0, 0), (0, 1, 0, 1), (1, 1, 0, 0), (1, 0, 0, 1), (2, 2, 0, 3)], dtype=B.TAGHIT)
    no = T.NO_GAP << 32
    assert T.keys_from_tags(recs, th, None).tolist() == [(1 << 32) | 20, (1 << 32) | 21, no | 0xFFFFFFFF, no | 0xFFFFFFFE, (2 << 32) | 30]
    row_gap = np.array([5, 6, 4], dtype=np.uint32)
    assert T.keys_from_tags(recs, th, row_gap).tolist() == [(6 << 32) | 20, (6 << 32) | 21, no | 0xFFFFFFFF, no | 0xFFFFFFFE, (4 << 32) | 30]
    every = T.keys_all(hits, 1, recs, th, th[:2], row_gap)
    assert every.tolist() == T.keys_from_screen(hits, 1).tolist() + T.keys_from_tags(recs, th, None).tolist() + T.keys_from_tags(recs, th[:2], row_gap).tolist()
    assert T.keys_all(hits, 0, recs, None, th[:2], row_gap).tolist() == T.keys_from_screen(hits, 0).tolist() + T.keys_from_tags(recs, th[:2], row_gap).tolist()
    assert T.keys_all(hits, 0, recs, th, None, None).tolist() == T.keys_from_screen(hits, 0).tolist() + T.keys_from_tags(recs, th, None).tolist()
