"""Directed device tests of gappadder_amd/csrc/pools.hip: every build of the per-gap pools (LDS and global-atomic histogram and
scatter, the LDS sort and its chunked global passes, the in-place unique, both gather paths), every key producer and the exact-size
owner exchange — each compared exactly with the plain definition in tests/pools_twin.py (the exchange: with the numpy definitions
of tests/test_distributed_cpu.py).  Every output buffer sits between guard bytes that must survive."""
import collections

import numpy as np
import pytest

import pools_twin as T

pytestmark = pytest.mark.gpu

GUARD, PAD = 0xEE, 256


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """A device buffer of `nbytes` between two runs of guard bytes; the body starts out as guard bytes too (an unwritten place shows)."""

    def __init__(self, nbytes, fill=GUARD):
        import torch
        self.n = int(nbytes)
        self.t = torch.full((PAD + self.n + PAD,), GUARD, dtype=torch.uint8, device="cuda:0")
        if fill != GUARD:
            self.t[PAD:PAD + self.n] = fill

    @property
    def ptr(self):
        return self.t.data_ptr() + PAD

    def host(self, dtype=np.uint8):
        """The body as a numpy array, after checking both guards."""
        h = self.t.cpu().numpy()
        assert (h[:PAD] == GUARD).all(), "bytes in front of the buffer were overwritten"
        assert (h[PAD + self.n:] == GUARD).all(), "bytes behind the buffer were overwritten"
        return h[PAD:PAD + self.n].copy().view(dtype)


def _dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).copy()).to("cuda:0")


def _gaps(n_gaps, per=7):
    """B.GAP array without flanks: `per` gaps per scaffold, ascending and apart — all gf_set_gaps asks for."""
    from gappadder_amd import _lib as B
    i = np.arange(n_gaps, dtype=np.uint32)
    gaps = np.zeros(n_gaps, dtype=B.GAP)
    gaps["scaffold"], gaps["idx_in_scaffold"] = i // per, i % per + 1
    gaps["start"] = (i % per) * 100 + 50
    gaps["end"] = gaps["start"] + 10
    return gaps, max(1, (n_gaps + per - 1) // per)


def _set_gaps(gf, n_gaps):
    gaps, n_scaffolds = _gaps(n_gaps)
    gf.set_gaps(gaps, n_scaffolds)


def _build(gf, d_reads, n_reads, L, keys_buf_ptr, n_keys, key_cap, pool_cap, with_ids=True, null_pool=False):
    """One gf_build_pools_dev call into guarded buffers -> (pool_off u64, ids u32 or None, rows u8 [pool_cap, rb], error word)."""
    import torch
    from gappadder_amd import _lib as B
    rb = (L + 3) // 4
    n_gaps = gf.n_gaps
    pool = None if null_pool else Guarded(pool_cap * rb)
    ids = Guarded(pool_cap * 4) if with_ids else None
    off = Guarded((n_gaps + 1) * 8)
    err = Guarded(4)
    d_nk = torch.tensor([n_keys], dtype=torch.int64, device="cuda:0").view(torch.int32)
    rc = B.lib().gf_build_pools_dev(gf.handle, d_reads.data_ptr(), n_reads, L, keys_buf_ptr, d_nk.data_ptr(), key_cap,
                                    pool.ptr if pool else None, pool_cap, off.ptr, ids.ptr if ids else None, err.ptr)
    assert rc == 0
    gf.sync()
    return (off.host(np.uint64), ids.host(np.uint32) if ids else None,
            pool.host().reshape(pool_cap, rb) if pool else None, int(err.host(np.uint32)[0]))


def _check_build(out, keys, n_gaps, reads, pool_cap):
    """pool_off, ids, row bytes and the error word of one build against the twin; what lies behind the pooled rows is untouched."""
    off, ids, rows, err = out
    w_off, w_ids, w_rows, w_flag = T.build_pools(keys, n_gaps, reads, pool_cap)
    assert off.tobytes() == w_off.tobytes()
    assert err == (T.POOL_OVERFLOW if w_flag else 0)
    n = len(w_ids)
    assert n == min(int(w_off[-1]), pool_cap)
    if ids is not None:
        bad = np.flatnonzero(ids[:n] != w_ids)
        assert len(bad) == 0, "first wrong id in gap %d" % (np.searchsorted(w_off, bad[0], side="right") - 1)
        assert (ids[n:] == 0xEEEEEEEE).all()
    if rows is not None:
        known = w_ids < len(reads)
        assert rows[:n][known].tobytes() == w_rows[known].tobytes()
        assert (rows[:n][~known] == GUARD).all()          # the row of a read >= n_reads is left as it was (include/gapfill_hip.h)
        assert (rows[n:] == GUARD).all()
    return w_off, w_ids


def _keys_call(keys, n_keys=None, tail=None):
    """Keys on the device (plus `tail`, keys behind n_keys that must not be read) -> (device tensor, n_keys, key_cap)."""
    buf = keys if tail is None else np.concatenate([keys, tail])
    return _dev(buf), len(keys) if n_keys is None else n_keys, len(buf)


# ------------------------------------------------------------------------------------------- histogram and scatter, both forms

def _hist_keys(n_gaps, seed, n_reads):
    """About 59 000 keys: first and last gap non-empty, most gaps empty, one gap with 5 000 keys, runs of equal gap and fully shuffled
    stretches, ~20 % duplicates, and a few hundred keys of gaps n_gaps, n_gaps + 1 and 0xFFFFFFFF."""
    rng = np.random.RandomState(seed)
    used = np.unique(np.concatenate([[0, n_gaps - 1, n_gaps // 2], rng.randint(0, n_gaps, max(1, n_gaps // 8))]))
    rd = lambda n: rng.randint(0, n_reads, n)
    runs = lambda k: [T.make_keys(np.full(n, used[rng.randint(len(used))]), rd(n)) for n in rng.randint(1, 200, k)]
    shuffled = T.make_keys(used[rng.randint(0, len(used), 24000)], rd(24000))
    outside = T.make_keys(np.repeat([n_gaps, n_gaps + 1, T.NO_GAP], 100), rd(300))
    deep = T.make_keys(np.full(5000, n_gaps // 2), rd(5000))
    ends = T.make_keys([0, 0, n_gaps - 1, n_gaps - 1], rd(4))
    first = np.concatenate(runs(100) + [ends])
    so_far = np.concatenate([first, shuffled, deep])
    stretch = np.concatenate([shuffled, outside, so_far[rng.randint(0, len(so_far), 12000)]])      # the duplicates: shuffled in
    rng.shuffle(stretch)
    return np.concatenate([first, stretch[:20000], deep, stretch[20000:]] + runs(80))


@pytest.mark.parametrize("n_gaps", [1, 1025, 32768, 32769, 70001])
def test_histogram_and_scatter_in_both_forms(gf, n_gaps):
    """One LDS counter per gap up to 32 768 gaps (exactly 128 KiB at the boundary), the wave-grouped global atomics beyond; 1 025 gaps give
    the scan a chunk of 2.  Same pools from the exact key count and from a count below key_cap (the keys behind it are not read)."""
    import torch
    _set_gaps(gf, n_gaps)
    n_reads, L = 400000, 150
    keys = _hist_keys(n_gaps, n_gaps, n_reads)
    assert 55000 < len(keys) < 65000
    d_reads = torch.randint(0, 256, (n_reads, 38), dtype=torch.uint8, device="cuda:0")
    reads = d_reads.cpu().numpy()
    w_off = T.build_pools(keys, n_gaps, reads, len(keys))[0]
    total = int(w_off[-1])
    cnt = np.diff(w_off.astype(np.int64))
    assert cnt[0] > 0 and cnt[-1] > 0 and cnt.max() > 4096 and (n_gaps < 8 or (cnt == 0).sum() > n_gaps // 2)
    assert 0.15 * len(keys) < len(keys) - 300 - total < 0.3 * len(keys)        # the duplicates
    d_keys, nk, cap = _keys_call(keys)
    _check_build(_build(gf, d_reads, n_reads, L, d_keys.data_ptr(), nk, cap, total + 3), keys, n_gaps, reads, total + 3)
    tail = T.make_keys(np.full(4097, n_gaps - 1), np.arange(4097))            # would be pooled if read
    d_keys, nk, cap = _keys_call(keys, tail=tail)
    _check_build(_build(gf, d_reads, n_reads, L, d_keys.data_ptr(), nk, cap, total), keys, n_gaps, reads, total)


# ------------------------------------------------------------------------------------------------------- sort and unique

SORT_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289, 20000]
SORT_CONTENTS = ["distinct", "one_key", "twice", "descending_pairs"]


def _sort_reads(n, content, rng, n_reads):
    """n raw reads of one gap."""
    if n == 0:
        return np.zeros(0, np.int64)
    if content == "distinct":
        return rng.choice(n_reads, n, replace=False)
    if content == "one_key":
        return np.full(n, rng.randint(n_reads))
    if content == "twice":      # sorted: the smallest once, then equal neighbours at (2i + 1, 2i + 2) — among them 255 | 256 from 257 keys on
        d = rng.choice(n_reads, n // 2 + 1, replace=False)
        d = np.array(sorted(d.tolist(), key=lambda r: (r & 1, r >> 1)))
        out = np.concatenate([d[:1], np.repeat(d[1:], 2)])[:n]
        assert len(out) == n
        rng.shuffle(out)
        return out
    p = np.sort(rng.choice(n_reads // 2, (n + 1) // 2, replace=False))[::-1]      # both mates of the same pairs, reads descending
    return np.stack([2 * p + 1, 2 * p], axis=1).reshape(-1)[:n]


def test_sort_and_unique_at_their_edges_with_blocks_that_take_several_gaps(gf):
    """More gaps than workgroups, so every block of pool_sort_unique_kernel takes gaps g, g + grid, g + 2 grid in turn (its kept count
    starts again for each): two gaps with more keys than one LDS sort holds and a shallow one behind them share a block.  Key counts around
    every power of two the network and the 256-key compaction rounds care about, and around one, two and three LDS chunks."""
    import torch
    grid = 8 * _cus()
    n_gaps = 3 * grid + 5
    cases = [(n, c) for n in SORT_COUNTS for c in SORT_CONTENTS]
    deep = [x for x in cases if x[0] > 4096]
    shallow = [x for x in cases if x[0] <= 4096]
    h = len(deep) // 2
    assert len(deep) == 32 and grid >= h + len(shallow) - h
    place = {}
    for i in range(h):                         # column i: deep, deep, shallow — one block's three gaps
        place[i], place[grid + i], place[2 * grid + i] = deep[i], deep[h + i], shallow[i]
    for i, x in enumerate(shallow[h:]):
        place[h + i] = x
    _set_gaps(gf, n_gaps)
    n_reads, L, rb = 200000, 16, 4
    rng = np.random.RandomState(5)
    parts = []
    for g, (n, content) in sorted(place.items()):
        parts.append(T.make_keys(np.full(n, g), _sort_reads(n, content, rng, n_reads)))
    other = np.setdiff1d(np.arange(n_gaps), np.array(sorted(place)))
    g_other = np.repeat(other, rng.randint(0, 41, len(other)))
    k_other = T.make_keys(g_other, rng.randint(0, 2000, len(g_other)))           # few reads: duplicates inside the shallow gaps too
    rng.shuffle(k_other)
    keys = np.concatenate(parts + [k_other])
    d_reads = torch.randint(0, 256, (n_reads, rb), dtype=torch.uint8, device="cuda:0")
    reads = d_reads.cpu().numpy()
    d_keys, nk, cap = _keys_call(keys)
    pool_cap = len(keys)
    w_off, _ = _check_build(_build(gf, d_reads, n_reads, L, d_keys.data_ptr(), nk, cap, pool_cap), keys, n_gaps, reads, pool_cap)
    cnt = np.diff(w_off.astype(np.int64))
    for g, (n, content) in place.items():      # the cases are what they claim to be
        assert cnt[g] == {"distinct": n, "one_key": min(n, 1), "twice": n // 2 + (n > 0), "descending_pairs": n}[content], (g, n, content)


# ---------------------------------------------------------------------------------------------------------------- gather

@pytest.mark.parametrize("L", [1, 4, 5, 16, 150, 160, 251])      # rows of 1, 1, 2, 4, 38 (the fast path), 40 and 63 bytes
def test_gather_rows_of_every_size_at_every_capacity_cut(gf, L):
    """The 38-byte fast path and the general path with and without a tail (rb & 3), rows shorter than a dword included: exact and roomy
    capacity, a cut at a gap's first row, inside a gap and one row short of the end (bit 31, pool_off exact, everything below the cut
    exact), with and without the id list, offsets only, and a key whose read does not exist."""
    import torch
    n_gaps, n_reads, rb = 40, 3000, (L + 3) // 4
    _set_gaps(gf, n_gaps)
    rng = np.random.RandomState(L)
    gap = rng.randint(0, n_gaps, 1800)
    gap[gap % 5 == 3] = 17                                                     # 300 and more rows in one gap, some gaps empty
    keys = np.concatenate([T.make_keys(gap, rng.randint(0, n_reads, 1800)),
                           T.make_keys([9, 9, 17], [n_reads, 0xFFFFFFFE, n_reads + 1])])      # reads that do not exist
    rng.shuffle(keys)
    d_reads = torch.randint(0, 256, (n_reads, rb), dtype=torch.uint8, device="cuda:0")
    reads = d_reads.cpu().numpy()
    d_keys, nk, cap = _keys_call(keys)
    w_off, w_ids, _, _ = T.build_pools(keys, n_gaps, reads, len(keys))
    total = int(w_off[-1])
    assert w_off[18] - w_off[17] > 256 and (np.diff(w_off.astype(np.int64)) == 0).any() and (w_ids >= n_reads).sum() == 3
    cuts = [total, total + 3, int(w_off[17]), int(w_off[17]) + 259, int(w_off[9]) + 1, total - 1]
    for pool_cap in cuts:
        for with_ids in (True, False):
            out = _build(gf, d_reads, n_reads, L, d_keys.data_ptr(), nk, cap, pool_cap, with_ids=with_ids)
            _check_build(out, keys, n_gaps, reads, pool_cap)
            assert (out[3] == T.POOL_OVERFLOW) == (pool_cap < total)
    off, ids, rows, err = _build(gf, d_reads, n_reads, L, d_keys.data_ptr(), nk, cap, 0, with_ids=False, null_pool=True)      # offsets only
    assert off.tobytes() == w_off.tobytes() and err == 0          # no pool asked for: no overflow to report (include/gapfill_hip.h)


# ------------------------------------------------------------------------------------------------------------ key producers

N_PROD_GAPS, N_PROD_RECS, N_PROD_ROWS = 23, 5000, 40


def _producer_inputs(n, seed):
    """n screen hits, n tagger hits and n second-hop hits (+ 37 further entries behind each list that a clamped count must not
    reach), alignment records (some without a read), and a row -> gap table in both forms (gf_dpos rows and the resolved u32)."""
    from gappadder_amd import _lib as B
    rng = np.random.RandomState(seed)
    m = n + 37
    hits = np.zeros(m, dtype=B.HIT)
    hits["gap"], hits["read"] = rng.randint(0, N_PROD_GAPS, m), rng.randint(0, 100000, m)
    hits["gap"][rng.rand(m) < 0.02] = N_PROD_GAPS + 1                           # a producer copies the gap as it is
    recs = np.zeros(N_PROD_RECS, dtype=B.ALNREC)
    recs["read"] = rng.randint(0, 100000, N_PROD_RECS)
    recs["read"][::41] = 0xFFFFFFFF                                            # no FASTQ record of that name
    th, lh = np.zeros(m, dtype=B.TAGHIT), np.zeros(m, dtype=B.TAGHIT)
    for a, n_targets in ((th, N_PROD_GAPS), (lh, N_PROD_ROWS)):
        a["rec"], a["gap"] = rng.randint(0, N_PROD_RECS, m), rng.randint(0, n_targets, m)
        a["kind"], a["to_mate"] = rng.randint(0, 4, m), rng.randint(0, 2, m)
    gaps, _ = _gaps(N_PROD_GAPS)
    row_gap = rng.randint(0, N_PROD_GAPS, N_PROD_ROWS).astype(np.uint32)
    table = np.zeros(N_PROD_ROWS, dtype=B.DPOS)
    table["mate_scaffold"], table["mate_pos"] = rng.randint(0, 4, N_PROD_ROWS), rng.randint(0, 9999, N_PROD_ROWS)
    table["src_scaffold"], table["src_gap"] = gaps["scaffold"][row_gap], gaps["idx_in_scaffold"][row_gap]
    return hits, recs, th, lh, row_gap, table


def _big_hits():
    return 4 * _cus() * 256 + 77          # one more trip of every producer's grid-stride loop


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, "big"])
def test_key_producers_give_the_defined_keys(gf, n, pairs, clamp):
    """The three atomic producers one after the other into one list (the keys of the definition as a multiset, *n_keys their number), and
    gf_pool_keys_all_dev with all three lists, without tagger hits and without second-hop hits (every key in its fixed place).  `clamp`:
    the device count says 37 hits more than hit_cap, and hit_cap holds."""
    import torch
    from gappadder_amd import _lib as B
    n = _big_hits() if n == "big" else n
    _set_gaps(gf, N_PROD_GAPS)
    hits, recs, th, lh, row_gap, table = _producer_inputs(n, 1000 * pairs + n % 1000)
    hit_cap, said = (n, n + 37) if clamp else (n + 37, n)
    d_hits, d_recs, d_th, d_lh, d_rg = _dev(hits), _dev(recs), _dev(th), _dev(lh), _dev(row_gap)
    d_cnt = torch.tensor([said], dtype=torch.int64, device="cuda:0").view(torch.int32)
    Lb, h = B.lib(), gf.handle
    per = 2 if pairs else 1
    want = [T.keys_from_screen(hits[:n], pairs), T.keys_from_tags(recs, th[:n], None), T.keys_from_tags(recs, lh[:n], row_gap),
            T.keys_from_tags(recs, lh[:n], row_gap)]
    total = (per + 3) * n
    keys, nk = Guarded(total * 8), Guarded(4)
    args = (keys.ptr, total, nk.ptr)
    assert Lb.gf_pool_keys_reset(h, nk.ptr) == 0
    assert Lb.gf_pool_keys_from_screen_dev(h, d_hits.data_ptr(), d_cnt.data_ptr(), hit_cap, pairs, *args) == 0
    assert Lb.gf_pool_keys_from_tags_dev(h, d_recs.data_ptr(), d_th.data_ptr(), d_cnt.data_ptr(), hit_cap, None, 0, *args) == 0
    assert Lb.gf_pool_keys_from_tags_dev(h, d_recs.data_ptr(), d_lh.data_ptr(), d_cnt.data_ptr(), hit_cap, B._p(table), len(table), *args) == 0
    assert Lb.gf_pool_keys_from_second_hop_dev(h, d_recs.data_ptr(), d_lh.data_ptr(), d_cnt.data_ptr(), hit_cap, d_rg.data_ptr(), *args) == 0
    gf.sync()
    assert int(nk.host(np.uint32)[0]) == total
    got = keys.host(np.uint64)
    edges = np.cumsum([0] + [len(w) for w in want])
    for i, w in enumerate(want):               # the calls run in stream order: each list's keys lie behind the previous list's
        assert np.array_equal(np.sort(got[edges[i]:edges[i + 1]]), np.sort(w)), i
    for with_tags, with_hop in ((True, True), (False, True), (True, False)):
        w = T.keys_all(hits[:n], pairs, recs, th[:n] if with_tags else None, lh[:n] if with_hop else None, row_gap)
        keys, nk = Guarded(len(w) * 8), Guarded(4)
        assert Lb.gf_pool_keys_all_dev(h, d_hits.data_ptr(), d_cnt.data_ptr(), hit_cap, pairs, d_recs.data_ptr(),
                                       d_th.data_ptr() if with_tags else None, d_cnt.data_ptr() if with_tags else None, hit_cap,
                                       d_lh.data_ptr() if with_hop else None, d_cnt.data_ptr() if with_hop else None, hit_cap,
                                       d_rg.data_ptr(), keys.ptr, len(w), nk.ptr) == 0
        gf.sync()
        assert int(nk.host(np.uint32)[0]) == len(w)
        assert keys.host(np.uint64).tobytes() == w.tobytes(), (with_tags, with_hop)


@pytest.mark.parametrize("cut", ["odd_inside_the_screen_keys", "inside_the_tagger_keys", "zero"])
@pytest.mark.parametrize("n", [700, "big"])
def test_key_cap_below_the_produced_total(gf, n, cut):
    """*n_keys still reports the total, the stores stop at key_cap (an odd cap inside the screen keys separates a hit from its mate),
    nothing is written behind it, and gf_build_pools_dev clamps: its pools are those of keys[:key_cap]."""
    import torch
    from gappadder_amd import _lib as B
    n = _big_hits() if n == "big" else n
    _set_gaps(gf, N_PROD_GAPS)
    hits, recs, th, lh, row_gap, table = _producer_inputs(n, 7)
    hits, th, lh = hits[:n], th[:n], lh[:n]
    d_hits, d_recs, d_th, d_lh, d_rg = _dev(hits), _dev(recs), _dev(th), _dev(lh), _dev(row_gap)
    d_cnt = torch.tensor([n], dtype=torch.int64, device="cuda:0").view(torch.int32)
    total = 4 * n
    key_cap = {"odd_inside_the_screen_keys": n + 1 - n % 2, "inside_the_tagger_keys": 2 * n + n // 3, "zero": 0}[cut]
    n_reads, L = 100000, 100
    d_reads = torch.randint(0, 256, (n_reads, 25), dtype=torch.uint8, device="cuda:0")
    reads = d_reads.cpu().numpy()
    Lb, h = B.lib(), gf.handle

    def pools_of(got):
        pool_cap = len(got) + 1
        _check_build(_build(gf, d_reads, n_reads, L, keys.ptr, total, key_cap, pool_cap), got, N_PROD_GAPS, reads, pool_cap)

    want = T.keys_all(hits, 1, recs, th, lh, row_gap)
    assert len(want) == total
    keys, nk = Guarded(key_cap * 8), Guarded(4)
    assert Lb.gf_pool_keys_all_dev(h, d_hits.data_ptr(), d_cnt.data_ptr(), n, 1, d_recs.data_ptr(), d_th.data_ptr(), d_cnt.data_ptr(), n,
                                   d_lh.data_ptr(), d_cnt.data_ptr(), n, d_rg.data_ptr(), keys.ptr, key_cap, nk.ptr) == 0
    gf.sync()
    assert int(nk.host(np.uint32)[0]) == total
    got = keys.host(np.uint64)
    assert got.tobytes() == want[:key_cap].tobytes()
    pools_of(got)

    keys, nk = Guarded(key_cap * 8), Guarded(4)          # the atomic producers: places are taken in any order, so a sub-multiset
    args = (keys.ptr, key_cap, nk.ptr)
    assert Lb.gf_pool_keys_reset(h, nk.ptr) == 0
    assert Lb.gf_pool_keys_from_screen_dev(h, d_hits.data_ptr(), d_cnt.data_ptr(), n, 1, *args) == 0
    assert Lb.gf_pool_keys_from_tags_dev(h, d_recs.data_ptr(), d_th.data_ptr(), d_cnt.data_ptr(), n, None, 0, *args) == 0
    assert Lb.gf_pool_keys_from_second_hop_dev(h, d_recs.data_ptr(), d_lh.data_ptr(), d_cnt.data_ptr(), n, d_rg.data_ptr(), *args) == 0
    gf.sync()
    assert int(nk.host(np.uint32)[0]) == total
    got = keys.host(np.uint64)
    assert not collections.Counter(got.tolist()) - collections.Counter(want.tolist())
    pools_of(got)


# ------------------------------------------------------------------------------------------------------- exact-size exchange

def _rank_pools(world, n_lib, n_gaps, rb, seed, thin=False):
    """[rank][lib] -> (rows u8 [n, rb], pool_off i64 [n_gaps + 1]): 0 .. 5 rows per gap, a third of the gaps empty."""
    rng = np.random.RandomState(seed)
    counts = rng.randint(0, 6, (world, n_lib, n_gaps)) * (rng.rand(world, n_lib, n_gaps) > 0.33)
    if thin:                                   # no gap with more rows than before, other bytes
        counts, rng = counts // 2, np.random.RandomState(seed + 1)
    out = []
    for r in range(world):
        libs = []
        for l in range(n_lib):
            off = np.concatenate([[0], np.cumsum(counts[r, l])]).astype(np.int64)
            libs.append((rng.randint(0, 256, (int(off[-1]), rb)).astype(np.uint8), off))
        out.append(libs)
    return out


def _rows_table(pools, world, n_lib, n_gaps, batch):
    """rows[src][dst][lib] of the sizing pass."""
    owner = (np.arange(n_gaps) // batch) % world
    table = np.zeros((world, world, n_lib), dtype=np.int64)
    for r in range(world):
        for l in range(n_lib):
            np.add.at(table[r, :, l], owner, np.diff(pools[r][l][1]))
    return table


class _Ranks:
    """The ranks of one exchange on one device: a sharding.ExactOwnerExchange per rank, its numpy double, and the all-to-all done by
    slicing host copies along the split sizes."""

    def __init__(self, gf, world, n_lib, n_gaps, batch, L, table):
        import torch
        from gappadder_amd import sharding as SH
        self.gf, self.world, self.n_lib, self.n_gaps, self.batch, self.L, self.rb = gf, world, n_lib, n_gaps, batch, L, (L + 3) // 4
        self.x = [SH.ExactOwnerExchange(world, r, n_lib, n_gaps, table, self.rb, "cuda", "nccl") for r in range(world)]
        self.np_send = [torch.zeros(len(x.send), dtype=torch.uint8) for x in self.x]
        self.np_cnt = [np.zeros((n_lib, n_gaps), dtype=np.uint32) for _ in self.x]
        self.err = Guarded(4, fill=0)

    def pack(self, r, pools, send_cap=None):
        """Rank r's libraries into x.send on the device, and into the numpy double by the definition (send_cap: another slot_cap table
        for the device call alone)."""
        from gappadder_amd import _lib as B
        from test_distributed_cpu import _np_pack_for_owners_v
        x = self.x[r]
        for l in range(self.n_lib):
            rows, off = pools[r][l]
            d_rows, d_off = _dev(rows), _dev(off)
            cnt = x.lib_cnt[l * self.n_gaps:(l + 1) * self.n_gaps]
            cap = x.send_cap if send_cap is None else send_cap
            assert B.lib().gf_pools_pack_for_owners_v_dev(self.gf.handle, d_rows.data_ptr(), d_off.data_ptr(), self.n_gaps, self.L, self.world,
                                                          self.batch, l, self.n_lib, x.send.data_ptr(), x.send_base.data_ptr(), cap.data_ptr(),
                                                          x.send_cnt.data_ptr(), cnt.data_ptr(), self.err.ptr) == 0
            self.gf.sync()
            if send_cap is None:
                _np_pack_for_owners_v(rows, off, self.world, self.batch, l, self.n_lib, self.np_send[r], x.send_base.cpu().numpy(),
                                      x.send_cap.cpu().numpy(), x.send_cnt.cpu().numpy(), self.np_cnt[r][l], self.rb)

    def all_to_all(self):
        """recv of rank r = the chunks every rank sends to r, in source order."""
        import torch
        sends = [x.send.cpu() for x in self.x]
        for r, x in enumerate(self.x):
            parts = []
            for s, xs in enumerate(self.x):
                at = sum(xs.in_splits[:r])
                parts.append(sends[s][at:at + xs.in_splits[r]])
                assert len(parts[-1]) == x.out_splits[s]
            recv = torch.cat(parts) if sum(x.out_splits) else torch.zeros(0, dtype=torch.uint8)
            x.recv[:len(recv)] = recv.to("cuda")

    def merge(self, r, merged_cap):
        """gf_pools_merge_v_dev on rank r's recv -> (rows [merged_cap, rb], merged_off u64, error word)."""
        from gappadder_amd import _lib as B
        x = self.x[r]
        merged, moff = Guarded(merged_cap * self.rb), Guarded((self.n_gaps + 1) * 8)
        assert B.lib().gf_pools_merge_v_dev(self.gf.handle, x.recv.data_ptr(), x.recv_base.data_ptr(), x.recv_cnt.data_ptr(), self.n_lib, self.world,
                                            self.n_gaps, self.L, r, self.world, self.batch, merged.ptr if merged_cap else None, merged_cap, moff.ptr,
                                            self.err.ptr) == 0
        self.gf.sync()
        return merged.host().reshape(merged_cap, self.rb), moff.host(np.uint64), int(self.err.host(np.uint32)[0])

    def np_merge(self, r):
        from test_distributed_cpu import _np_merge_v
        x = self.x[r]
        rows, moff = _np_merge_v(x.recv.cpu(), x.recv_base.cpu().numpy(), x.recv_cnt.cpu().numpy(), self.n_lib, self.world, self.n_gaps, r,
                                 self.batch, self.rb)
        return rows, np.asarray(moff, dtype=np.uint64)

    def step(self, pools):
        """One whole step, every byte against the definitions."""
        for r in range(self.world):
            self.pack(r, pools)
            assert self.x[r].send.cpu().numpy().tobytes() == self.np_send[r].numpy().tobytes(), r          # headers and rows
            assert self.x[r].lib_cnt.cpu().numpy().view(np.uint32).tobytes() == self.np_cnt[r].tobytes(), r
        self.all_to_all()
        n_all = 0
        for r in range(self.world):
            w_rows, w_off = self.np_merge(r)
            rows, moff, err = self.merge(r, len(w_rows))
            assert err == 0 and moff.tobytes() == w_off.tobytes() and rows.tobytes() == w_rows.tobytes(), r
            n_all += len(w_rows)
        assert n_all == sum(len(rows) for libs in pools for rows, _ in libs)          # every row reaches exactly one owner


XCHG = [(3, 1, 37, 4, 150), (4, 2, 1030, 256, 150), (2, 2, 19, 3, 101), (1, 3, 50, 256, 100)]      # rows of 38, 38, 26 (even) and 25 (odd) bytes


@pytest.mark.parametrize("world,n_lib,n_gaps,batch,L", XCHG)
def test_exact_size_exchange_equals_its_definitions(gf, world, n_lib, n_gaps, batch, L):
    """gf_pools_pack_for_owners_v_dev and gf_pools_merge_v_dev — what Pipeline.step() runs at N > 1 — for every rank of a simulated world:
    the send buffer with its count headers (zero for gaps the peer does not own), lib_cnt, the merged rows and merged_off, byte for
    byte; a second step with fewer rows reuses the buffers."""
    rb = (L + 3) // 4
    pools = _rank_pools(world, n_lib, n_gaps, rb, seed=n_gaps)
    ranks = _Ranks(gf, world, n_lib, n_gaps, batch, L, _rows_table(pools, world, n_lib, n_gaps, batch))
    ranks.step(pools)
    ranks.step(_rank_pools(world, n_lib, n_gaps, rb, seed=n_gaps, thin=True))      # fewer rows per slot: old headers and rows must not show


@pytest.mark.parametrize("world,n_lib,n_gaps,batch,L", XCHG)
def test_exact_size_exchange_short_slot_and_short_merged_buffer(gf, world, n_lib, n_gaps, batch, L):
    """A slot with room for fewer rows than the rank produces: bit 30, the rows that fit are sent, and every byte outside that slot's
    rows is as in the unflagged run.  A merged buffer three rows short: bit 31, merged_off exact, the rows below the capacity
    exact, nothing behind it."""
    rb = (L + 3) // 4
    pools = _rank_pools(world, n_lib, n_gaps, rb, seed=n_gaps)
    table = _rows_table(pools, world, n_lib, n_gaps, batch)
    good = _Ranks(gf, world, n_lib, n_gaps, batch, L, table)
    for r in range(world):
        good.pack(r, pools)
    r = world - 1
    x = good.x[r]
    cap = x.send_cap.cpu().numpy()
    s = int(np.argmax(cap))
    assert cap[s] >= 3
    short_cap = cap.copy()
    short_cap[s] -= 2
    short = _Ranks(gf, world, n_lib, n_gaps, batch, L, table)
    short.pack(r, pools, send_cap=_dev(short_cap).view(x.send_cap.dtype))
    assert int(short.err.host(np.uint32)[0]) == 0x40000000 and int(good.err.host(np.uint32)[0]) == 0
    a, b = x.send.cpu().numpy(), short.x[r].send.cpu().numpy()
    base = int(x.send_base.cpu().numpy()[s])
    cut, end = base + int(short_cap[s]) * rb, base + int(cap[s]) * rb
    assert a[:cut].tobytes() == b[:cut].tobytes() and a[end:].tobytes() == b[end:].tobytes()
    assert (b[cut:end] == 0).all() and a[cut:end].any()                           # the rows that did not fit were not sent
    assert short.x[r].lib_cnt.cpu().numpy().tobytes() == x.lib_cnt.cpu().numpy().tobytes()

    good.all_to_all()
    w_rows, w_off = good.np_merge(r)
    assert len(w_rows) > 3
    rows, moff, err = good.merge(r, len(w_rows) - 3)
    assert err == 0x80000000 and moff.tobytes() == w_off.tobytes() and rows.tobytes() == w_rows[:-3].tobytes()
    _, moff, err = good.merge(r, 0)                                                # offsets only: err keeps the bit (these calls do not reset it)
    assert err == 0x80000000 and moff.tobytes() == w_off.tobytes()
