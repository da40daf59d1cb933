"""The device second hop (csrc/hop.hip + the look-up of csrc/tag_low.hip) restated in plain numpy, and the directed inputs its tests use.

Part 1 is the twin: what the three device calls must return, written from the reference's definitions (the inversion + sort(1) of
run_multi_threads_discordant.py, the look-up of collect_discordant_low_mapq_reads.py) with sorts and searches of numpy — no project
kernel, no GPU.  `bucket_geometry` / `bucket_of` restate the kernels' bucket rule; the tests use them ONLY to assert that an input lands
where it was aimed ("the largest bucket holds 3000 rows"), never as an expected result.

Part 2 builds the inputs.  Every builder asserts its own edge conditions, so a builder that stops producing its edge fails on the CPU
(test_second_hop_twin_host.py builds every case) as well as on the device (test_gpu_second_hop.py)."""
import numpy as np

from oracle.c_oracle import ALNREC, DPOS, GAP, TAGHIT

LOWREC = np.dtype([("pos", "<u4"), ("ref", "<u4"), ("rec", "<u4")])
KIND_CLIP, KIND_DISCORDANT, KIND_UNMAP, KIND_LOWMAPQ = 0, 1, 2, 3
NONE = 0xFFFFFFFF
# constants of the kernels that decide which path an input takes (hop.hip, gf_internal.hpp)
BUCKETS_LOG2, SORT_LDS, TABLE_BLOCKS = 14, 1024, 256
WIN_BELOW, WIN_ABOVE = 199, 299     # a record at pos sees a row at q iff q - 199 <= pos <= q + 299
U64 = np.uint64


def _key(scaffold, pos):
    return (np.asarray(scaffold).astype(U64) << U64(32)) | np.asarray(pos).astype(U64)


def row_keys(rows):
    return _key(rows["mate_scaffold"], rows["mate_pos"])


# ------------------------------------------------------------------------------------------------ part 1: the twin
def bucket_geometry(n_scaffolds, max_pos):
    """(sub_bits, pos_shift, n_buckets) of the counting sort: buckets = (scaffold, top sub_bits bits of the position)."""
    scaf_bits = int(n_scaffolds).bit_length()
    sub_bits = max(BUCKETS_LOG2 - scaf_bits, 0)
    pos_shift = max(int(max_pos).bit_length() - sub_bits, 0)
    return sub_bits, pos_shift, (n_scaffolds + 1) << sub_bits


def bucket_of(mate_scaffold, mate_pos, n_scaffolds, max_pos):
    sub_bits, pos_shift, _ = bucket_geometry(n_scaffolds, max_pos)
    sub = np.asarray(mate_pos).astype(U64) >> U64(pos_shift)
    sub = np.minimum(sub, U64((1 << sub_bits) - 1))
    return (np.asarray(mate_scaffold).astype(U64) << U64(sub_bits)) | sub


def table_rows(recs, hits, gaps, n_scaffolds):
    """(rows, row_gap): one row per DISCORDANT hit whose record's mate lies on a known scaffold, sorted by
    (mate scaffold, mate position, gap index)."""
    d = hits[hits["kind"] == KIND_DISCORDANT]
    d = d[recs["mate_ref"][d["rec"]] < n_scaffolds]
    ms, mp, g = recs["mate_ref"][d["rec"]], recs["mate_pos"][d["rec"]], d["gap"]
    order = np.lexsort((g, mp, ms))
    rows = np.zeros(len(d), dtype=DPOS)
    rows["mate_scaffold"], rows["mate_pos"] = ms[order], mp[order]
    rows["src_scaffold"], rows["src_gap"] = gaps["scaffold"][g[order]], gaps["idx_in_scaffold"][g[order]]
    return rows, g[order].astype(np.uint32)


def merge_parts(parts, part_cap):
    """Union of sorted parts [(rows, row_gap)], each cut to part_cap rows: stable by (mate scaffold, mate position) — among equal keys an
    earlier part comes first, and the rows of one part keep their order."""
    rows = np.concatenate([np.asarray(r, dtype=DPOS)[:part_cap] for r, _ in parts]) if parts else np.zeros(0, DPOS)
    gap = np.concatenate([np.asarray(g, dtype=np.uint32)[:part_cap] for _, g in parts]) if parts else np.zeros(0, np.uint32)
    order = np.argsort(row_keys(rows), kind="stable")
    return rows[order], gap[order]


def low_mapq_hits(low, rows, n_scaffolds):
    """Hits (TAGHIT, kind 3, to_mate 0, gap = row index) of the MAPQ-0 records `low` against the SORTED table `rows`: the record's
    focal position is the largest unique position <= pos + 199 on its scaffold, if that + 299 >= pos; one hit per row of it.
    Sorted by (rec, row)."""
    keys = row_keys(rows)
    assert np.all(keys[1:] >= keys[:-1]), "the table must be sorted by (mate scaffold, mate position)"
    ukey, ufirst, ucount = np.unique(keys, return_index=True, return_counts=True)
    low = np.asarray(low, dtype=LOWREC)
    pos, ref = low["pos"].astype(U64), low["ref"].astype(U64)
    lim = (ref << U64(32)) | np.minimum(pos + U64(WIN_BELOW), U64(0xFFFFFFFF))
    at = np.searchsorted(ukey, lim, side="right").astype(np.int64) - 1
    ok = (low["ref"] < n_scaffolds) & (at >= 0)
    at = np.where(ok, at, 0)
    if len(ukey):
        q = ukey[at]
        ok &= ((q >> U64(32)) == ref) & ((q & U64(0xFFFFFFFF)) + U64(WIN_ABOVE) >= pos)
    else:
        ok[:] = False
    cnt = np.where(ok, ucount[at] if len(ukey) else 0, 0).astype(np.int64)
    first = np.where(ok, ufirst[at] if len(ukey) else 0, 0).astype(np.int64)
    total = int(cnt.sum())
    out = np.zeros(total, dtype=TAGHIT)
    src = np.repeat(np.arange(len(low)), cnt)
    within = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    out["rec"] = low["rec"][src]
    out["gap"] = first[src] + within
    out["kind"] = KIND_LOWMAPQ
    return out[np.lexsort((out["gap"], out["rec"]))]


# ------------------------------------------------------------------------------------------------ part 2: directed inputs
def make_gaps(n_gaps, n_scaffolds):
    """n_gaps gaps spread over the scaffolds in scaffold order; gap index = place in the array."""
    g = np.zeros(n_gaps, dtype=GAP)
    g["scaffold"] = (np.arange(n_gaps, dtype=np.uint64) * n_scaffolds // max(n_gaps, 1)).astype(np.uint32)
    first = np.searchsorted(g["scaffold"], g["scaffold"])
    g["idx_in_scaffold"] = np.arange(n_gaps) - first + 1
    g["start"] = 1000 * g["idx_in_scaffold"]
    g["end"] = g["start"] + 100
    return g


def table_input(n_scaffolds, n_gaps, mate_scaffold, mate_pos, gap, density=3, n_hits=None, seed=0):
    """Records and tagger hits whose DISCORDANT hits on known scaffolds are exactly the rows (mate_scaffold, mate_pos, gap), shuffled.
    One record per distinct (scaffold, position): hits that share a key share the record.  Every `density`-th hit is DISCORDANT, the
    rest are of the other kinds (on any record, the dropped ones included); a twentieth more DISCORDANT hits point at records whose
    mate_ref is 0xFFFFFFFF or n_scaffolds and must be dropped.  n_hits: the exact length of the hit list (the discordant ones among
    them, kept + dropped, number ceil(n_hits / density))."""
    rng = np.random.default_rng(seed)
    ms, mp, gap = (np.asarray(x, dtype=np.uint32) for x in (mate_scaffold, mate_pos, gap))
    n = len(ms)
    ukey, inv = np.unique(_key(ms, mp), return_inverse=True)
    n_fill = 8
    recs = np.zeros(len(ukey) + 2 + n_fill, dtype=ALNREC)
    perm = rng.permutation(len(recs))                     # where each logical record lives
    place = perm[:len(ukey)]
    recs["pos"] = rng.integers(0, 1 << 20, len(recs))
    recs["ref"] = rng.integers(0, n_scaffolds, len(recs))
    recs["mate_ref"] = rng.integers(0, n_scaffolds, len(recs))
    recs["mate_pos"] = rng.integers(0, 1 << 20, len(recs))
    recs["flag"], recs["mapq"], recs["tlen"] = 0x41, 40, 100000
    recs["read"] = np.arange(len(recs))
    recs["mate_ref"][place] = (ukey >> U64(32)).astype(np.uint32)
    recs["mate_pos"][place] = (ukey & U64(0xFFFFFFFF)).astype(np.uint32)
    dropped = perm[len(ukey):len(ukey) + 2]
    recs["mate_ref"][dropped] = (NONE, n_scaffolds)
    if n_hits is None:
        n_drop = (n + 19) // 20
    else:
        n_disc = (n_hits + density - 1) // density
        n_drop = n_disc - n
        assert n_drop >= 0
    disc = np.zeros(n + n_drop, dtype=TAGHIT)
    disc["rec"][:n], disc["gap"][:n] = place[inv], gap
    disc["rec"][n:] = dropped[rng.integers(0, 2, n_drop)]
    disc["gap"][n:] = rng.integers(0, n_gaps, n_drop)
    disc["kind"] = KIND_DISCORDANT
    disc["to_mate"] = rng.integers(0, 2, len(disc))
    disc = disc[rng.permutation(len(disc))]
    total = n_hits if n_hits is not None else len(disc) * density
    hits = np.zeros(total, dtype=TAGHIT)
    hits["rec"] = rng.integers(0, len(recs), total)
    hits["gap"] = rng.integers(0, n_gaps, total)
    hits["kind"] = rng.choice([KIND_CLIP, KIND_UNMAP, KIND_LOWMAPQ], total)
    slots = np.arange(0, total, density)
    assert len(slots) == len(disc)
    hits[slots] = disc
    case = {"n_scaffolds": n_scaffolds, "gaps": make_gaps(n_gaps, n_scaffolds), "recs": recs, "hits": hits}
    rows, _ = table_rows(recs, hits, case["gaps"], n_scaffolds)          # the builder's own condition: the rows asked for, no others
    assert np.array_equal(np.sort(row_keys(rows)), np.sort(_key(ms, mp))) and len(rows) == n
    assert n_drop == 0 or (recs["mate_ref"][hits["rec"][hits["kind"] == KIND_DISCORDANT]] >= n_scaffolds).sum() == n_drop
    assert total == len(disc) or (hits["kind"] != KIND_DISCORDANT).any()
    return case


def _bucket_sizes(case):
    rows, _ = table_rows(case["recs"], case["hits"], case["gaps"], case["n_scaffolds"])
    max_pos = int(rows["mate_pos"].max()) if len(rows) else 0
    b, c = np.unique(bucket_of(rows["mate_scaffold"], rows["mate_pos"], case["n_scaffolds"], max_pos), return_counts=True)
    return dict(zip(b.tolist(), c.tolist())), max_pos


BUCKET_ROWS = [0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 5000]


def bucket_case(n, mode):
    """n rows in ONE bucket (scaffold 2 of 5, sub-bucket 37 of 2048, 16 384 positions wide), a few in the buckets either side of it and
    150 spread elsewhere.  mode "distinct": n distinct positions, random gaps; "onepos": one position, n distinct gaps."""
    rng = np.random.default_rng(1000 + n)
    ns, top = 5, (1 << 24) + 5
    sub_bits, pos_shift, _ = bucket_geometry(ns, top)
    assert (sub_bits, pos_shift) == (11, 14)
    base = 37 << pos_shift
    n_gaps = 48 if mode == "distinct" else 6000
    if mode == "distinct":
        pos = base + rng.choice(1 << pos_shift, n, replace=False)
        gap = rng.integers(0, n_gaps, n)
    else:
        pos = np.full(n, base + 777)
        gap = rng.permutation(n_gaps)[:n]
    bg_s = rng.choice([0, 1, 3, 4], 150)
    bg_p = rng.integers(0, 1 << 24, 150)
    edge_p = np.array([base - 1, base - 1, base + (1 << pos_shift), top])       # neighbours of the bucket; the largest position
    edge_s = np.array([2, 2, 2, 4])
    ms = np.concatenate([np.full(n, 2), bg_s, edge_s])
    mp = np.concatenate([pos, bg_p, edge_p])
    g = np.concatenate([gap, rng.integers(0, n_gaps, 154)])
    case = table_input(ns, n_gaps, ms, mp, g, density=3, seed=n)
    sizes, max_pos = _bucket_sizes(case)
    target = int(bucket_of(2, base, ns, max_pos))
    assert max_pos == top and sizes.get(target, 0) == n
    assert max(c for b, c in sizes.items() if b != target) < 64
    if mode == "distinct":
        assert len(np.unique(pos)) == n
    else:
        assert len(np.unique(gap)) == n
    case["largest_bucket"] = n
    return case


SCAFFOLD_COUNTS = [1, 2, 3, 8191, 8192, 8193, 40000]


def scaffold_case(ns):
    """Rows on the first, the last and scattered scaffolds; from 8192 scaffolds on (one bucket per scaffold) one scaffold carries 1500."""
    rng = np.random.default_rng(2000 + ns)
    scat = rng.integers(0, ns, 300)
    ms = [np.zeros(40, np.int64), np.full(40, ns - 1), scat]
    heavy = None
    if ns >= 8192:
        heavy = ns - 1 if ns == 8192 else ns // 2
        ms.append(np.full(1500, heavy))
    ms = np.concatenate(ms)
    mp = rng.integers(0, 1_000_000, len(ms))
    mp[0] = 999_999
    case = table_input(ns, 48, ms, mp, rng.integers(0, 48, len(ms)), density=3, seed=ns)
    sizes, max_pos = _bucket_sizes(case)
    sub_bits, _, n_buckets = bucket_geometry(ns, max_pos)
    assert sub_bits == {1: 13, 2: 12, 3: 12, 8191: 1}.get(ns, 0)
    assert n_buckets == (ns + 1) << sub_bits
    rows, _ = table_rows(case["recs"], case["hits"], case["gaps"], ns)
    assert rows["mate_scaffold"].min() == 0 and rows["mate_scaffold"].max() == ns - 1
    if heavy is not None:
        assert sizes[int(bucket_of(heavy, 0, ns, max_pos))] >= 1500 > SORT_LDS
    case["largest_bucket"] = max(sizes.values())
    return case


MAX_POSITIONS = [0, 1, (1 << 12) - 1, 1 << 12, (1 << 24) + 5]


def maxpos_case(top):
    """Three scaffolds (4096 sub-buckets each), mate positions 0 .. top with top itself present.  top = 0: 700 rows per scaffold that
    differ only in the gap."""
    rng = np.random.default_rng(3000 + top % 977)
    ns, n_gaps = 3, 6000
    if top == 0:
        ms = np.repeat(np.arange(3), 700)
        mp = np.zeros(2100, np.int64)
        gap = rng.permutation(n_gaps)[:2100]
    else:
        ms = rng.integers(0, 3, 600)
        mp = rng.integers(0, top + 1, 600)
        mp[:3] = top
        mp[3:6] = 0
        gap = rng.integers(0, n_gaps, 600)
    case = table_input(ns, n_gaps, ms, mp, gap, density=3, seed=top % 977)
    sizes, max_pos = _bucket_sizes(case)
    assert max_pos == top
    assert bucket_geometry(ns, max_pos)[:2] == (12, {0: 0, 1: 0, 4095: 0, 4096: 1, (1 << 24) + 5: 13}[top])
    if top == 0:
        assert sorted(sizes.values()) == [700, 700, 700] and len(np.unique(gap)) == 2100
    case["largest_bucket"] = max(sizes.values())
    return case


def shift32_case():
    """8192 scaffolds (no sub-buckets) and one mate position >= 2^31: the bucket rule's position shift is 32."""
    rng = np.random.default_rng(4000)
    ns = 8192
    ms = np.concatenate([rng.integers(0, ns, 300), np.full(40, 5)])
    mp = np.concatenate([rng.integers(0, 1 << 31, 300), rng.integers(0, 1 << 31, 40)])
    mp[-1] = (1 << 31) + 12345
    mp[-2] = 0
    case = table_input(ns, 48, ms, mp, rng.integers(0, 48, len(ms)), density=3, seed=4000)
    sizes, max_pos = _bucket_sizes(case)
    assert max_pos >= 1 << 31 and bucket_geometry(ns, max_pos)[:2] == (0, 32)
    assert sizes[5] >= 40
    case["largest_bucket"] = max(sizes.values())
    return case


HIT_COUNTS = [1, 63, 64, 65, 97]
DENSITIES = [1, 3, 64]


def big_hit_count(n_cu):
    return n_cu * 4 * 256 + 65        # one more trip of the extraction kernel's grid-stride loop, ending inside a wave


def count_case(n_hits, density, seed=0):
    """A hit list of exactly n_hits hits, every density-th of them DISCORDANT, over at most 2000 records on 50 scaffolds."""
    rng = np.random.default_rng(5000 + n_hits % 9973 + density)
    ns, n_gaps = 50, 48
    n_disc = (n_hits + density - 1) // density
    n = n_disc - n_disc // 16                      # the rest: dropped (unknown mate scaffold)
    pool_s, pool_p = rng.integers(0, ns, 2000), rng.integers(0, 3_000_000, 2000)
    pick = rng.integers(0, 2000, n)
    case = table_input(ns, n_gaps, pool_s[pick], pool_p[pick], rng.integers(0, n_gaps, n), density=density, n_hits=n_hits, seed=seed + n_hits % 9973)
    assert len(case["hits"]) == n_hits and len(case["recs"]) <= 2010
    assert (case["hits"]["kind"] == KIND_DISCORDANT).sum() == n_disc
    return case


def _sorted_rows(scaffold, pos, rng):
    key = np.sort(_key(scaffold, pos))
    rows = np.zeros(len(key), dtype=DPOS)
    rows["mate_scaffold"], rows["mate_pos"] = (key >> U64(32)).astype(np.uint32), (key & U64(0xFFFFFFFF)).astype(np.uint32)
    rows["src_scaffold"] = rng.integers(0, 1000, len(key))
    rows["src_gap"] = rng.integers(1, 50, len(key))
    return rows


def _low(pos, ref, rng=None, first_rec=1000):
    low = np.zeros(len(pos), dtype=LOWREC)
    low["pos"], low["ref"] = pos, ref
    low["rec"] = first_rec + np.arange(len(pos))
    return low[rng.permutation(len(low))] if rng is not None else low


# ---- the union
def _part(rng, n, tag0, scaffolds=4, positions=50, s0=0, p0=0):
    rows = _sorted_rows(s0 + rng.integers(0, scaffolds, n), p0 + rng.integers(0, positions, n), rng)
    return rows, (tag0 + np.arange(n)).astype(np.uint32)


MERGE_CASES = ["one_part", "two_parts", "three_parts", "eight_parts", "1024_parts_of_4", "empty_first_middle_last", "all_empty",
               "one_exactly_full", "count_above_part_cap", "one_key_in_every_part", "identical_parts", "descending_ranges", "row_cap_below_total"]


def merge_case(name):
    """{"parts": [(rows, row_gap)], "part_cap", "row_cap"}: sorted parts with unique row_gap tags; a part longer than part_cap stands
    for a slot that is full with a count above part_cap."""
    rng = np.random.default_rng(6000 + MERGE_CASES.index(name))
    sizes, part_cap, row_cap, kw = None, 700, None, {}
    if name == "one_part":
        sizes = [613]
    elif name == "two_parts":
        sizes = [700 - 3, 255]
    elif name == "three_parts":
        sizes = [1, 699, 257]
    elif name == "eight_parts":
        sizes = [65, 300, 0, 512, 513, 64, 63, 700]
    elif name == "1024_parts_of_4":
        part_cap = 4
        sizes = rng.integers(0, 7, 1024).tolist()           # 5 and 6: counts above the slot
        kw = {"positions": 2000}
    elif name == "empty_first_middle_last":
        sizes = [0, 300, 0, 0, 301, 0]
    elif name == "all_empty":
        sizes = [0, 0, 0]
    elif name == "one_exactly_full":
        sizes = [100, 700, 100]
    elif name == "count_above_part_cap":
        sizes = [100, 700 + 50, 30, 700 + 1]
    elif name == "row_cap_below_total":
        sizes = [400, 401, 402]
        row_cap = 777
    parts, tag = [], 0
    if sizes is not None:
        for n in sizes:
            parts.append(_part(rng, n, tag, **kw))
            tag += n
    elif name == "one_key_in_every_part":
        for p in range(5):
            rows, g = _part(rng, 200, tag, scaffolds=1, positions=1, s0=2, p0=25)      # 200 rows of the key (2, 25) ...
            more, g2 = _part(rng, 100 + p, tag + 200)                                   # ... among other keys
            both = np.concatenate([rows, more])
            order = np.argsort(row_keys(both), kind="stable")
            parts.append((both[order], np.concatenate([g, g2])[order]))
            tag += 300 + p
        assert all((row_keys(r) == _key(2, 25)).sum() >= 200 for r, _ in parts)
    elif name == "identical_parts":
        rows, _ = _part(rng, 333, 0)
        for p in range(4):
            parts.append((rows.copy(), (tag + np.arange(333)).astype(np.uint32)))
            tag += 333
    elif name == "descending_ranges":
        for p in range(4):
            parts.append(_part(rng, 250 + p, tag, s0=10 * (3 - p)))
            tag += 250 + p
        assert all(row_keys(parts[p][0]).min() > row_keys(parts[p + 1][0]).max() for p in range(3))
    total = sum(min(len(r), part_cap) for r, _ in parts)
    case = {"parts": parts, "part_cap": part_cap, "row_cap": row_cap if row_cap is not None else max(total, 1), "total": total}
    tags = np.concatenate([g[:part_cap] for _, g in parts])
    assert len(np.unique(tags)) == len(tags) == total                       # a collision or a hole would show
    for r, _ in parts:
        assert np.all(row_keys(r)[1:] >= row_keys(r)[:-1])
    if name == "count_above_part_cap" or name == "1024_parts_of_4":
        assert any(len(r) > part_cap for r, _ in parts)
    if name == "one_exactly_full":
        assert any(len(r) == part_cap for r, _ in parts)
    if name == "row_cap_below_total":
        assert case["row_cap"] < total
    if name not in ("all_empty", "descending_ranges", "one_part"):          # equal keys in different parts: the tie rule is exercised
        in_parts = np.concatenate([np.unique(row_keys(r[:part_cap])) for r, _ in parts])
        assert np.unique(in_parts, return_counts=True)[1].max() > 1
    return case


# ---- the look-up
LOOKUP_ROWS = [0, 1, 255, 256, 257, 65537, 150001]


def lookup_rows_case(n):
    """A sorted table of n rows on scaffolds 2, 3 and 6 of 9 (0, 1, 4, 5, 7 and the last, 8, have none) in runs of equal keys (a row
    repeats the key before it with probability 0.6), and records in and around the windows of a sample of its positions.  From 65 537
    rows on, the 256 chunks of the table build have more than 256 rows, and the runs at their edges are PLACED: with 65 537 rows a run
    lies across every chunk boundary and across every row 256 * j inside a chunk; with 150 001 rows every second of these places has
    such a run and at the others a new key starts exactly there.  The positions at these places are all among the records' targets."""
    rng = np.random.default_rng(7000 + n)
    ns = 9
    same = rng.random(n) < 0.6                           # row i repeats the key of row i - 1
    places = np.zeros(0, np.int64)
    if n >= 65537:
        chunk = (n + TABLE_BLOCKS - 1) // TABLE_BLOCKS
        assert chunk > 256
        edges = np.arange(chunk, n, chunk)                                                   # first row of a chunk
        rounds = np.concatenate([np.arange(a + 256, min(a + chunk, n), 256) for a in range(0, n, chunk)])   # first row of a later round
        assert len(edges) == TABLE_BLOCKS - 1 and len(rounds) >= TABLE_BLOCKS - 1
        places = np.concatenate([edges, rounds])
        if n == 65537:
            same[places] = True
        else:
            same[edges[0::2]], same[edges[1::2]] = True, False
            same[rounds[0::2]], same[rounds[1::2]] = True, False
    same[:1] = False
    gid = np.cumsum(~same) - 1                           # the run of every row
    n_runs = int(gid[-1]) + 1 if n else 0
    third = n_runs // 3
    scaf = np.repeat([2, 3, 6], [third, third, n_runs - 2 * third])
    step = rng.integers(1, 700, n_runs).astype(np.int64)
    pos = np.concatenate([np.cumsum(step[scaf == s]) for s in (2, 3, 6)]) if n_runs else np.zeros(0, np.int64)
    rows = _sorted_rows(scaf[gid], pos[gid], rng)
    keys = row_keys(rows)
    assert len(rows) == n and np.array_equal(keys[1:] == keys[:-1], same[1:])
    if n == 65537:
        assert np.all(keys[places] == keys[places - 1])
    elif n > 65537:
        for at in (edges, rounds):
            assert np.all(keys[at[0::2]] == keys[at[0::2] - 1]) and np.all(keys[at[1::2]] != keys[at[1::2] - 1])
    ukey = np.unique(keys)
    pick = ukey[rng.permutation(len(ukey))[:1500]] if len(ukey) else np.zeros(0, U64)
    pick = np.unique(np.concatenate([pick, keys[places], keys[places - 1]]))                 # every placed run and its neighbour is looked up
    q, s = (pick & U64(0xFFFFFFFF)).astype(np.int64), (pick >> U64(32)).astype(np.uint32)
    lp, lr = [np.array([5, 100000], np.int64)], [np.array([0, 8], np.uint32)]                # records on scaffolds without rows
    for d in (-200, -199, 0, 299, 300):
        keep = q + d >= 0
        lp.append((q + d)[keep]); lr.append(s[keep])
    low = _low(np.concatenate(lp), np.concatenate(lr), rng)
    case = {"n_scaffolds": ns, "rows": rows, "low": low}
    assert n == 0 or len(low_mapq_hits(low, rows, ns)) > len(pick)
    assert set(np.unique(rows["mate_scaffold"]).tolist()) <= {2, 3, 6}
    return case


EDGE_Q = [0, 1, 198, 199, 200] + [512 * j + d for j in (1, 3, 1000) for d in (199, 198, -300, -299)]
EDGE_OFFSETS = {"below_out": -200, "below_in": -199, "at": 0, "above_in": 299, "above_out": 300}


def lookup_edges_case():
    """Every position of EDGE_Q alone on a scaffold of its own (1 .. 17 of 64; 0 and 18 .. 63 but 20 and 30 are empty) with records at
    the five EDGE_OFFSETS of it; scaffold 20: two positions 100 apart; records on scaffold n_scaffolds and 0xFFFFFFFF.
    "classes": name -> the records' rec ids; "expect": name -> True (each record has a hit) / False (none has)."""
    rng = np.random.default_rng(8000)
    ns = 64
    rs, rp = [], []
    for i, q in enumerate(EDGE_Q):
        k = 1 + i % 3
        rs += [1 + i] * k; rp += [q] * k
    q1, q2 = 5000, 5100
    rs += [20, 20, 20, 30]; rp += [q1, q2, q2, 7]
    rows = _sorted_rows(rs, rp, rng)
    lp, lr, cls = [], [], []
    for i, q in enumerate(EDGE_Q):
        for name, d in EDGE_OFFSETS.items():
            if q + d >= 0:
                lp.append(q + d); lr.append(1 + i); cls.append(name)
    for d in (q1 - 199, q1, q1 + 299, q1 + 300, q2 + 299):       # both windows hold for the middle three: the larger position wins
        lp.append(d); lr.append(20); cls.append("two_apart_q2" if d >= q1 else "two_apart_q1")
    lp += [q1 - 200, q2 + 300]; lr += [20, 20]; cls += ["two_apart_out"] * 2
    lp += [7, 7, 0]; lr += [ns, NONE, NONE]; cls += ["unknown_scaffold"] * 3
    low = _low(np.array(lp), np.array(lr, dtype=np.uint32))
    cls = np.array(cls)
    perm = rng.permutation(len(low))
    low, cls = low[perm], cls[perm]
    classes = {c: low["rec"][cls == c] for c in np.unique(cls)}
    expect = {"below_out": False, "below_in": True, "at": True, "above_in": True, "above_out": False, "two_apart_q1": True,
              "two_apart_q2": True, "two_apart_out": False, "unknown_scaffold": False}
    hits = low_mapq_hits(low, rows, ns)
    for c, recs in classes.items():
        got = np.isin(recs, hits["rec"])
        assert len(recs) > 0 and (got.all() if expect[c] else not got.any()), c
    assert len(classes["below_in"]) == len([q for q in EDGE_Q if q >= 199]) and len(classes["above_in"]) == len(EDGE_Q)
    assert np.all(rows["mate_pos"][hits["gap"][np.isin(hits["rec"], classes["two_apart_q2"])]] == q2)
    assert np.all(rows["mate_pos"][hits["gap"][np.isin(hits["rec"], classes["two_apart_q1"])]] == q1)
    # window ends on the edges of the 512-base bins of the near-bit map: first / last position of a bin, and its neighbours
    lo_end = [(q - 199) % 512 for q in EDGE_Q if q >= 199]
    hi_end = [(q + 299) % 512 for q in EDGE_Q]
    assert {0, 511} <= set(lo_end) and {0, 511} <= set(hi_end)
    return {"n_scaffolds": ns, "rows": rows, "low": low, "classes": classes, "expect": expect, "n_hits": len(hits)}


def lookup_high_case():
    """Positions next to 2^32 (the window's upper end and pos + 199 are clamped there): q = 0xFFFFFF00 on scaffold 1 of 3."""
    rng = np.random.default_rng(8100)
    q = 0xFFFFFF00
    rows = _sorted_rows([0, 1, 1, 1, 2], [100, 5, q, q, 0xFFFFFFFF], rng)
    lp = [q - 200, q - 199, q - 1, q, q + 1, q + 255, 0xFFFFFFFF, 0xFFFFFFFF - 199, 0xFFFFFFFF - 200, 0xFFFFFFFF]
    lr = [1, 1, 1, 1, 1, 1, 2, 2, 2, 0]
    low = _low(np.array(lp, dtype=np.uint64), np.array(lr, dtype=np.uint32), rng)
    hits = low_mapq_hits(low, rows, 3)
    assert len(hits) == 5 * 2 + 2
    return {"n_scaffolds": 3, "rows": rows, "low": low}


UPPER_LAYOUTS = ["even", "cluster_low", "cluster_high"]


def lookup_upper_case(layout):
    """One scaffold with 20 000 unique positions: evenly spread; all within 40 000 bases plus one at 2^30; the mirror image.  Probes
    whose pos + 199 is one below / exactly / one past every tenth position, the positions themselves, below the first, above the last."""
    rng = np.random.default_rng(9000 + UPPER_LAYOUTS.index(layout))
    n = 20000
    if layout == "even":
        pos = 1000 + 50000 * np.arange(n, dtype=np.int64)
    else:
        cl = np.sort(rng.choice(40000, n - 1, replace=False)).astype(np.int64)
        pos = np.concatenate([1000 + cl, [1 << 30]]) if layout == "cluster_low" else np.concatenate([[1000], (1 << 30) - 40000 + cl])
    assert len(np.unique(pos)) == n and pos.min() >= 1000
    rows = _sorted_rows(np.full(n, 1), pos, rng)
    q = np.sort(pos)[::10]
    lp = np.concatenate([q - 200, q - 199, q - 198, q, q + 1, [pos.min() - 200, pos.min() - 500, pos.max() + 299, pos.max() + 300, (1 << 31)],
                         rng.integers(0, 1 << 30, 500)])
    low = _low(lp, np.full(len(lp), 1, np.uint32), rng)
    hits = low_mapq_hits(low, rows, 2)
    assert len(hits) >= 4 * len(q)
    if layout != "even":        # the interpolated guess is thousands of entries off: the gallop runs, in each direction for one of the layouts
        srt = np.sort(pos)
        guess = (q[1000] - srt[0]) * (n - 1) // (srt[-1] - srt[0])
        assert abs(int(guess) - 10000) > 5000
    return {"n_scaffolds": 2, "rows": rows, "low": low, "n_hits": len(hits)}


FANOUT_LANES = [3, 17, 31, 40, 63]


def lookup_fanout_case():
    """One position owns 3000 rows; of 64 records (one wave of the look-up) the five at FANOUT_LANES see it."""
    rng = np.random.default_rng(9500)
    rows = _sorted_rows([0] * 3 + [1] * 3000 + [2] * 2, [50, 60, 70] + [10000] * 3000 + [9, 10000], rng)
    lp = 500000 + 1000 * np.arange(64, dtype=np.int64)
    lp[FANOUT_LANES] = [10000 - 199, 10000, 10000 + 1, 10000 + 150, 10000 + 299]
    low = _low(lp, np.full(64, 1, np.uint32))
    hits = low_mapq_hits(low, rows, 4)
    assert len(hits) == 5 * 3000 and set(hits["rec"].tolist()) == set(low["rec"][FANOUT_LANES].tolist())
    return {"n_scaffolds": 4, "rows": rows, "low": low, "n_hits": len(hits)}


def lookup_cases():
    """name -> builder of every directed look-up case (for the checks that run over all of them)."""
    c = {"rows_%d" % n: (lambda n=n: lookup_rows_case(n)) for n in LOOKUP_ROWS}
    c.update({"upper_" + l: (lambda l=l: lookup_upper_case(l)) for l in UPPER_LAYOUTS})
    c.update({"edges": lookup_edges_case, "high": lookup_high_case, "fanout": lookup_fanout_case})
    return c
