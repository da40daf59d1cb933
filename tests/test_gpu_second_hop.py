"""The device second hop, piece by piece, against its numpy twin (tests/second_hop_twin.py; pinned on the CPU by
test_second_hop_twin_host.py): gf_second_hop_table_dev (extraction, counting sort, bucket sort), gf_second_hop_table_merge_dev (union by
rank-merge) and gf_tag_low_mapq_table_dev (table arrays, near-bit map, interpolate-and-gallop look-up), on inputs built in numpy that aim
at one branch each.  Bit-exact, with no re-sorting of a table the device wrote; every output buffer is followed by a guard region of
0xEE bytes that must come back untouched."""
import numpy as np
import pytest

from golden_util import CASES, Case
from oracle import gp_oracle as O
import records_util as RU
import second_hop_twin as T

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


def _dev_in(arr):
    """the bytes of arr on the device, followed by 0xEE: what a kernel that ignores a cap or a count would read"""
    import torch
    b = np.concatenate([np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8), np.full(GUARD, 0xEE, np.uint8)])
    return torch.from_numpy(b).to("cuda:0")


class _Out:
    """an output buffer of n items prefilled with 0xEE, guard behind it"""
    def __init__(self, n, dtype):
        import torch
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.t = torch.full((self.n * self.dtype.itemsize + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.t.data_ptr()

    def take(self, k):
        """the first min(k, n) items; asserts that everything behind them — the unused tail and the guard — is still 0xEE"""
        k = min(int(k), self.n)
        host = self.t.cpu().numpy()
        assert np.all(host[k * self.dtype.itemsize:] == 0xEE), "written behind the %d items the call reported or could hold" % k
        return np.frombuffer(host[:k * self.dtype.itemsize].tobytes(), dtype=self.dtype)

    def guard_intact(self):
        return bool((self.t[self.n * self.dtype.itemsize:] == 0xEE).all())


def _counts(*vals):
    """16 device counters, the first ones preset"""
    import torch
    return torch.from_numpy(np.array(list(vals) + [0] * (16 - len(vals)), dtype=np.uint32).view(np.int32)).to("cuda:0")


def _lib():
    from gappadder_amd import _lib as B
    return B.lib()


def run_table(gf, c, row_cap=None, hit_cap=None, claimed=None):
    """gf_second_hop_table_dev on the case's records and hits -> (rows, row_gap, *d_n_rows).  The whole hit list is uploaded also
    where hit_cap is below its length: what lies behind the cap is live hits, and a call that read them would show it"""
    gf.set_gaps(c["gaps"], c["n_scaffolds"])
    hits = c["hits"]
    hit_cap = len(hits) if hit_cap is None else hit_cap
    exp_rows, _ = T.table_rows(c["recs"], hits[:hit_cap], c["gaps"], c["n_scaffolds"])
    row_cap = max(len(exp_rows), 1) if row_cap is None else row_cap
    d_recs, d_hits = _dev_in(c["recs"]), _dev_in(hits)
    d_cnt = _counts(len(hits) if claimed is None else claimed, 0xEEEEEEEE)
    rows, rg = _Out(row_cap, T.DPOS), _Out(row_cap, np.uint32)
    assert _lib().gf_second_hop_table_dev(gf.handle, d_recs.data_ptr(), d_hits.data_ptr(), d_cnt.data_ptr(), hit_cap, rows.ptr, rg.ptr, row_cap,
                                          d_cnt.data_ptr() + 4) == 0
    gf.sync()
    n = int(d_cnt.cpu().numpy().view(np.uint32)[1])
    return rows.take(n), rg.take(n), n


def check_table(gf, c, **kw):
    hits = c["hits"][:kw["hit_cap"]] if kw.get("hit_cap") is not None else c["hits"]
    exp_rows, exp_gap = T.table_rows(c["recs"], hits, c["gaps"], c["n_scaffolds"])
    rows, rg, n = run_table(gf, c, **kw)
    assert n == len(exp_rows)
    assert rows.tobytes() == exp_rows.tobytes()            # as the device wrote them: equal keys in gap order
    assert rg.tobytes() == exp_gap.tobytes()
    return n


# ---------------------------------------------------------------------------------- a. the table build
@pytest.mark.parametrize("mode", ["distinct", "onepos"])
@pytest.mark.parametrize("n", T.BUCKET_ROWS)
def test_table_bucket_of_n_rows(gf, n, mode):
    """n rows in one bucket: the LDS sort up to 1024, chunks through LDS + compare-exchanges in global memory beyond"""
    c = T.bucket_case(n, mode)
    assert c["largest_bucket"] == n
    assert check_table(gf, c) == n + 154


@pytest.mark.parametrize("ns", T.SCAFFOLD_COUNTS)
def test_table_scaffold_counts(gf, ns):
    """the bucket rule either side of 8192 scaffolds (one sub-bucket bit -> none); from there on a scaffold of 1500 rows is one bucket"""
    c = T.scaffold_case(ns)
    assert (c["largest_bucket"] > T.SORT_LDS) == (ns >= 8192)
    assert check_table(gf, c) >= 380


@pytest.mark.parametrize("top", T.MAX_POSITIONS)
def test_table_largest_position(gf, top):
    """the split of the position follows the largest one seen; all positions zero: the rows differ in the gap alone"""
    assert check_table(gf, T.maxpos_case(top)) >= 600


def test_table_position_shift_of_32(gf):
    """8192 scaffolds and a mate position >= 2^31: the bucket rule's shift is 32.  Pins the table for this geometry; it cannot tell the
    guarded shift of hop_bucket_of from an unguarded one (the hardware takes the low five bits of the count, and without sub-buckets
    the result is clamped to 0 either way) — the guard is there for the language's sake"""
    assert check_table(gf, T.shift32_case()) == 340


@pytest.mark.parametrize("density", T.DENSITIES)
@pytest.mark.parametrize("n_hits", T.HIT_COUNTS + ["grid + 65"])
def test_table_hit_counts_and_densities(gf, n_hits, density):
    """hit lists that end inside / on / behind a wave, DISCORDANT hits 1 in 1, 3 and 64 among the other kinds and among hits whose mate
    scaffold is unknown; the long one takes the extraction kernel's grid-stride loop into a second trip"""
    if n_hits == "grid + 65":
        import torch
        n_hits = T.big_hit_count(torch.cuda.get_device_properties(0).multi_processor_count)
    c = T.count_case(n_hits, density)
    n_disc = (n_hits + density - 1) // density
    assert check_table(gf, c) == n_disc - n_disc // 16


def test_table_hit_count_above_hit_cap_is_clamped(gf):
    """*d_n_taghits = 300 with hit_cap = 200, and the 100 hits behind the cap are on the device: 30 rows that must not appear"""
    c = T.count_case(300, 3)
    beyond = c["hits"][200:]
    beyond = beyond[beyond["kind"] == T.KIND_DISCORDANT]
    assert (c["recs"]["mate_ref"][beyond["rec"]] < c["n_scaffolds"]).sum() > 10
    n_all = len(T.table_rows(c["recs"], c["hits"], c["gaps"], c["n_scaffolds"])[0])
    n = check_table(gf, c, hit_cap=200, claimed=300)
    assert 0 < n <= n_all - 10


def test_table_row_cap_below_the_rows_found(gf):
    """the count reports every row; nothing is written at or behind row_cap (which rows fill the table is unspecified)"""
    c = T.count_case(1500, 1)
    exp_rows, _ = T.table_rows(c["recs"], c["hits"], c["gaps"], c["n_scaffolds"])
    rows, rg, n = run_table(gf, c, row_cap=100)           # (take() asserts the guard)
    assert n == len(exp_rows) > 1000 and len(rows) == len(rg) == 100
    k = T.row_keys(rows)
    assert np.all(k[1:] >= k[:-1]) and np.all(np.isin(k, T.row_keys(exp_rows)))


@pytest.mark.parametrize("name", CASES)
def test_golden_files_through_the_device_chain(gf, name):
    """tagger with MAPQ-0 list -> table -> look-up, all on the device: the rows are the reference's sorted file, the look-up's lines its lists"""
    case = Case(name)
    gaps = O.gap_positions(case.fasta_records(), case.meta["min_gap"])
    garr = RU.gaps_array(case.fai_names, gaps)
    gf.set_gaps(garr, len(case.fai_names))
    L, h = _lib(), gf.handle
    for lib in case.libs:
        recs, fields = RU.sam_to_records(lib["sam"], case.fai_names)
        n, cap = len(recs), max(1024, 4 * len(recs))
        d_recs, d_cnt = _dev_in(recs), _counts()
        cp = d_cnt.data_ptr()
        th, low, rows, rg, lh = _Out(cap, T.TAGHIT), _Out(n, T.LOWREC), _Out(cap, T.DPOS), _Out(cap, np.uint32), _Out(cap, T.TAGHIT)
        assert L.gf_tag_alignments_low_dev(h, d_recs.data_ptr(), n, lib["is"], lib["sd"], case.meta["clip_dist"], case.meta["anchor_mapq"],
                                           th.ptr, cap, cp, low.ptr, n, cp + 4) == 0
        assert L.gf_second_hop_table_dev(h, d_recs.data_ptr(), th.ptr, cp, cap, rows.ptr, rg.ptr, cap, cp + 8) == 0
        assert L.gf_tag_low_mapq_table_dev(h, low.ptr, cp + 4, n, rows.ptr, cp + 8, cap, lh.ptr, cap, cp + 12) == 0
        gf.sync()
        cnt = d_cnt.cpu().numpy()
        table = rows.take(cnt[2])
        text = "".join("%d %d %d %d\n" % tuple(r) for r in table.tolist())
        assert text == case.expected[lib["folder"] + "/discordant_reads_pos.txt.sorted.txt"], lib["folder"]
        assert np.array_equal(garr["scaffold"][rg.take(cnt[2])], table["src_scaffold"])
        hits = np.sort(lh.take(cnt[3]), order=["rec", "gap"])
        got = RU.lowmapq_hits_to_lines(hits, fields, table, case.fai_names)
        exp = case.exp_dir(lib["folder"] + "/discordant_reads_list/")
        for fname, txt in exp.items():
            scf, side = fname.rsplit("_cluster_by_discordant_reads_", 1)
            assert got.get(scf, {}).get(side.split(".")[0], []) == txt.splitlines(), (lib["folder"], fname)
        assert th.guard_intact() and low.guard_intact()


# ---------------------------------------------------------------------------------- b. the union
def run_merge(gf, parts, part_cap, row_cap):
    """gf_second_hop_table_merge_dev on slots of part_cap rows (0xEE behind a part's rows; a longer part fills its slot and keeps its
    count) -> (rows, row_gap, *d_n_rows)"""
    n_parts = len(parts)
    rows_all = np.full((n_parts, part_cap * T.DPOS.itemsize), 0xEE, np.uint8)
    gap_all = np.full((n_parts, part_cap * 4), 0xEE, np.uint8)
    for p, (r, g) in enumerate(parts):
        k = min(len(r), part_cap)
        rows_all[p, :k * 16] = np.frombuffer(r[:k].tobytes(), np.uint8)
        gap_all[p, :k * 4] = np.frombuffer(np.ascontiguousarray(g[:k], dtype=np.uint32).tobytes(), np.uint8)
    n_all = np.array([len(r) for r, _ in parts], dtype=np.uint32)
    d_rows_all, d_gap_all, d_n_all, d_cnt = _dev_in(rows_all), _dev_in(gap_all), _dev_in(n_all), _counts(0xEEEEEEEE)
    rows, rg = _Out(row_cap, T.DPOS), _Out(row_cap, np.uint32)
    gf.set_gaps(T.make_gaps(4, 64), 64)
    assert _lib().gf_second_hop_table_merge_dev(gf.handle, d_rows_all.data_ptr(), d_gap_all.data_ptr(), d_n_all.data_ptr(), n_parts, part_cap,
                                                rows.ptr, rg.ptr, row_cap, d_cnt.data_ptr()) == 0
    gf.sync()
    n = int(d_cnt.cpu().numpy().view(np.uint32)[0])
    return rows.take(n), rg.take(n), n


@pytest.mark.parametrize("name", T.MERGE_CASES)
def test_union_equals_the_stable_merge(gf, name):
    c = T.merge_case(name)
    exp_rows, exp_gap = T.merge_parts(c["parts"], c["part_cap"])
    rows, rg, n = run_merge(gf, c["parts"], c["part_cap"], c["row_cap"])
    assert n == c["total"] == len(exp_rows)                 # the clamped total, also where row_cap is below it
    assert rows.tobytes() == exp_rows[:c["row_cap"]].tobytes()
    assert rg.tobytes() == exp_gap[:c["row_cap"]].tobytes()  # unique tags: no row twice, none missing, no 0xEE from a slot's tail


def test_union_of_three_device_tables_is_the_single_table(gf):
    """one hit list split over three "ranks" by index stride: three device tables, merged == the device table of all hits as a multiset
    per key; the look-up through either table gives the same (record, gap) pairs"""
    c = T.count_case(6000, 1)
    full_rows, full_gap, n_full = run_table(gf, c)
    parts = []
    for r in range(3):
        rows, rg, n = run_table(gf, dict(c, hits=c["hits"][r::3]))
        parts.append((rows.copy(), rg.copy()))
    assert sum(len(r) for r, _ in parts) == n_full > 5000
    part_cap = max(len(r) for r, _ in parts) + 5
    rows, rg, n = run_merge(gf, parts, part_cap, n_full)
    assert n == n_full and np.array_equal(T.row_keys(rows), T.row_keys(full_rows))
    o1, o2 = np.lexsort((rg, T.row_keys(rows))), np.lexsort((full_gap, T.row_keys(full_rows)))
    assert rows[o1].tobytes() == full_rows[o2].tobytes() and np.array_equal(rg[o1], full_gap[o2])
    rng = np.random.default_rng(5)
    pick = rng.permutation(n_full)[:2000]
    low = T._low(full_rows["mate_pos"][pick].astype(np.int64) + rng.integers(-150, 250, 2000).clip(-full_rows["mate_pos"][pick].astype(np.int64)),
                 full_rows["mate_scaffold"][pick], rng)
    pairs = []
    for table, gap_of in ((rows, rg), (full_rows, full_gap)):
        hits, n_hits = run_lookup(gf, {"n_scaffolds": c["n_scaffolds"], "rows": table, "low": low})
        pairs.append(np.sort(hits["rec"].astype(np.uint64) << np.uint64(32) | gap_of[hits["gap"]].astype(np.uint64)))
    assert len(pairs[0]) > 2000 and np.array_equal(pairs[0], pairs[1])


# ---------------------------------------------------------------------------------- c. table arrays and look-up
def run_lookup(gf, c, low_cap=None, claimed_low=None, row_cap=None, claimed_rows=None, cap=None):
    """gf_tag_low_mapq_table_dev on a sorted table and a MAPQ-0 list -> (hits sorted by (rec, row), *d_n_out).  The whole table and
    the whole list are uploaded also where row_cap / low_cap are below their lengths: live rows and records lie behind the caps"""
    rows, low, ns = c["rows"], c["low"], c["n_scaffolds"]
    gf.set_gaps(T.make_gaps(4, ns), ns)
    row_cap = max(len(rows), 1) if row_cap is None else row_cap
    low_cap = len(low) if low_cap is None else low_cap
    exp = T.low_mapq_hits(low[:low_cap], rows[:row_cap], ns)
    cap = max(len(exp), 1) if cap is None else cap
    d_rows, d_low = _dev_in(rows), _dev_in(low)
    d_cnt = _counts(len(low) if claimed_low is None else claimed_low, len(rows) if claimed_rows is None else claimed_rows, 0xEEEEEEEE)
    cp = d_cnt.data_ptr()
    out = _Out(cap, T.TAGHIT)
    assert _lib().gf_tag_low_mapq_table_dev(gf.handle, d_low.data_ptr(), cp, low_cap, d_rows.data_ptr(), cp + 4, row_cap, out.ptr, cap, cp + 8) == 0
    gf.sync()
    n = int(d_cnt.cpu().numpy().view(np.uint32)[2])
    hits = out.take(n)
    return hits[np.lexsort((hits["gap"], hits["rec"]))], n


def check_lookup(gf, c, **kw):
    low = c["low"][:kw["low_cap"]] if kw.get("low_cap") is not None else c["low"]
    rows = c["rows"][:kw["row_cap"]] if kw.get("row_cap") is not None else c["rows"]
    exp = T.low_mapq_hits(low, rows, c["n_scaffolds"])
    hits, n = run_lookup(gf, c, **kw)
    assert n == len(exp)
    assert hits.tobytes() == exp.tobytes()
    return n


@pytest.mark.parametrize("n", T.LOOKUP_ROWS)
def test_lookup_table_sizes(gf, n):
    """tables that end inside / on / behind a block of the table build, runs of equal keys across its chunk and round boundaries,
    scaffolds without rows before, between and behind the populated ones"""
    assert check_lookup(gf, T.lookup_rows_case(n)) > (0 if n else -1)


def test_lookup_row_count_above_row_cap_is_clamped(gf):
    """*d_n_rows = 257 with row_cap = 200, the 57 sorted rows behind the cap on the device and records in their windows: hits that
    must not appear"""
    c = T.lookup_rows_case(257)
    n_all = len(T.low_mapq_hits(c["low"], c["rows"], c["n_scaffolds"]))
    n = check_lookup(gf, c, row_cap=200, claimed_rows=257)
    assert 0 < n <= n_all - 57


def test_lookup_window_edges(gf):
    """q - 199 <= pos <= q + 299 at both ends and one outside, for q < 199 and for window ends on the edges of the near-bit map's bins;
    of two positions 100 apart the larger wins; records on scaffolds the table does not know"""
    c = T.lookup_edges_case()
    hits, n = run_lookup(gf, c)
    for name, recs in c["classes"].items():                 # which class loses or gains a hit, before the byte comparison
        got = np.isin(recs, hits["rec"])
        assert got.all() if c["expect"][name] else not got.any(), name
    assert n == c["n_hits"] and hits.tobytes() == T.low_mapq_hits(c["low"], c["rows"], c["n_scaffolds"]).tobytes()


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65])
def test_lookup_low_counts(gf, k):
    """a MAPQ-0 list that ends inside / on / behind a wave, its last record one with a hit"""
    c = T.lookup_edges_case()
    low = c["low"]
    last = low[low["rec"] == c["classes"]["above_in"][0]]
    sub = np.concatenate([low[low["rec"] != last["rec"][0]][:max(k - 1, 0)], last])[:k]
    assert check_lookup(gf, dict(c, low=sub)) >= min(k, 1)


def test_lookup_low_count_above_low_cap_is_clamped(gf):
    """*d_n_low = 88 with low_cap = 70, the 18 records behind the cap on the device, some of them with hits that must not appear"""
    c = T.lookup_edges_case()
    assert len(T.low_mapq_hits(c["low"][70:], c["rows"], c["n_scaffolds"])) >= 5
    assert 0 < check_lookup(gf, c, low_cap=70, claimed_low=len(c["low"])) <= c["n_hits"] - 5


@pytest.mark.parametrize("layout", T.UPPER_LAYOUTS)
def test_lookup_search_on_spread_and_clustered_positions(gf, layout):
    """20 000 positions on one scaffold: the interpolated start is right (evenly spread) or thousands of entries off (clustered, with an
    outlier at either end): long gallops up and down"""
    c = T.lookup_upper_case(layout)
    assert check_lookup(gf, c) == c["n_hits"]


def test_lookup_fan_out_and_output_cap(gf):
    """one position owns 3000 rows and five lanes of one wave emit them; with an output cap below the hits the count is the full one
    and nothing is written behind the cap"""
    c = T.lookup_fanout_case()
    assert check_lookup(gf, c) == 15000
    hits, n = run_lookup(gf, c, cap=1000)                  # (take() asserts the guard)
    assert n == 15000 and len(hits) == 1000
    pair = lambda h: h["rec"].astype(np.uint64) << np.uint64(32) | h["gap"].astype(np.uint64)
    assert len(np.unique(pair(hits))) == 1000 and np.all(np.isin(pair(hits), pair(T.low_mapq_hits(c["low"], c["rows"], c["n_scaffolds"]))))
    assert np.all(hits["kind"] == T.KIND_LOWMAPQ) and np.all(hits["to_mate"] == 0)


def test_lookup_positions_next_to_2_32(gf):
    assert check_lookup(gf, T.lookup_high_case()) == 12
