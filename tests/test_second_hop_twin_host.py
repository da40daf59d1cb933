"""The numpy twin of the device second hop (tests/second_hop_twin.py) pinned on the CPU: against the quadratic C definition of the
look-up, against the reference's own sorted table (byte for byte: "by gap index" IS the reference's order of equal keys), and the
directed inputs of tests/test_gpu_second_hop.py against their own conditions — every builder asserts them when it runs."""
import numpy as np
import pytest

from golden_util import CASES, Case
from oracle import c_oracle as CO
from oracle import gp_oracle as O
import records_util as RU
import second_hop_twin as T


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return Case(request.param)


def _low_of(recs):
    at = np.flatnonzero(recs["mapq"] == 0)
    low = np.zeros(len(at), dtype=T.LOWREC)
    low["pos"], low["ref"], low["rec"] = recs["pos"][at], recs["ref"][at], at
    return low


def _c_hits(low, rows):
    """or_tag_low_mapq over records made from the low list: the C oracle numbers its hits by record index."""
    recs = np.zeros(len(low), dtype=CO.ALNREC)
    recs["pos"], recs["ref"] = low["pos"], low["ref"]
    got = CO.tag_low_mapq(recs, rows).copy()
    got["rec"] = low["rec"][got["rec"]]
    return got[np.lexsort((got["gap"], got["rec"]))]


def test_table_rows_are_the_references_sorted_file_byte_for_byte(case):
    gaps = O.gap_positions(case.fasta_records(), case.meta["min_gap"])
    garr = RU.gaps_array(case.fai_names, gaps)
    n_rows = 0
    for lib in case.libs:
        recs, _ = RU.sam_to_records(lib["sam"], case.fai_names)
        hits = CO.tag_alignments(recs, garr, lib["is"], lib["sd"], case.meta["clip_dist"], case.meta["anchor_mapq"])
        rows, row_gap = T.table_rows(recs, hits, garr, len(case.fai_names))
        text = "".join("%d %d %d %d\n" % tuple(r) for r in rows.tolist())
        assert text == case.expected[lib["folder"] + "/discordant_reads_pos.txt.sorted.txt"], lib["folder"]
        assert np.array_equal(garr["scaffold"][row_gap], rows["src_scaffold"]) and np.array_equal(garr["idx_in_scaffold"][row_gap], rows["src_gap"])
        n_rows += len(rows)
    assert n_rows > 10


def test_low_mapq_hits_equal_the_c_oracle_on_the_golden_tables(case):
    n_hits = 0
    for lib in case.libs:
        rows = RU.dpos_array([tuple(int(x) for x in l.split()) for l in case.exp_lines(lib["folder"] + "/discordant_reads_pos.txt.sorted.txt")])
        recs, _ = RU.sam_to_records(lib["sam"], case.fai_names)
        got = T.low_mapq_hits(_low_of(recs), rows, len(case.fai_names))
        exp = CO.tag_low_mapq(recs, rows)            # (in record order, rows ascending: sorted by (rec, row) already)
        assert got.tobytes() == exp.tobytes(), lib["folder"]
        n_hits += len(exp)
    assert n_hits > 0


@pytest.mark.parametrize("name", sorted(T.lookup_cases()))
def test_low_mapq_hits_equal_the_c_oracle_on_the_directed_tables(name):
    c = T.lookup_cases()[name]()
    rng = np.random.default_rng(1)
    rows = c["rows"][:3000]                           # (a prefix of a sorted table is sorted; the C definition is quadratic)
    low = c["low"]
    if len(low) > 3000:
        low = low[np.sort(rng.permutation(len(low))[:3000])]
    got = T.low_mapq_hits(low, rows, c["n_scaffolds"])
    exp = _c_hits(low, rows)
    assert got.tobytes() == exp.tobytes()
    assert len(exp) > 0 or len(rows) == 0
    if len(c["rows"]) <= 3000 and len(c["low"]) <= 3000 and "n_hits" in c:
        assert len(exp) == c["n_hits"]


def test_merge_parts_of_any_split_is_the_table_per_key():
    rng = np.random.default_rng(11)
    rows, tags = T._part(rng, 5000, 0, scaffolds=6, positions=120)
    by_tag = lambda r, g: np.lexsort((g, T.row_keys(r)))
    for n_parts in (1, 2, 3, 7, 64):
        owner = rng.integers(0, n_parts, len(rows))
        parts = [(rows[owner == p], tags[owner == p]) for p in range(n_parts)]
        r, g = T.merge_parts(parts, 1 << 20)
        assert np.array_equal(T.row_keys(r), T.row_keys(rows))                       # sorted, the same keys
        o1, o2 = by_tag(r, g), by_tag(rows, tags)
        assert r[o1].tobytes() == rows[o2].tobytes() and np.array_equal(g[o1], tags[o2])   # the same rows under every key
        # equal keys: an earlier part first, a part's own rows in their order (tags ascend inside a part)
        part_of = owner[g]
        same = T.row_keys(r)[1:] == T.row_keys(r)[:-1]
        assert np.all(part_of[1:][same] >= part_of[:-1][same])
        assert np.all(g[1:][same & (part_of[1:] == part_of[:-1])] > g[:-1][same & (part_of[1:] == part_of[:-1])])
    r, g = T.merge_parts([(rows[:10], tags[:10]), (rows[5:100], tags[5:100])], 7)     # clamped parts
    assert len(r) == 14 and set(g.tolist()) == set(range(7)) | set(range(5, 12))


def test_bucket_rule_of_the_twin():
    """hand-worked values of the bucket rule the builders aim with"""
    assert T.bucket_geometry(8191, 1000) == (1, 9, 8192 << 1)
    assert T.bucket_geometry(8192, 1000) == (0, 10, 8193)
    assert T.bucket_geometry(5, (1 << 24) + 5) == (11, 14, 6 << 11)
    assert T.bucket_geometry(3, 0) == (12, 0, 4 << 12)
    assert T.bucket_geometry(8192, 1 << 31) == (0, 32, 8193)
    assert int(T.bucket_of(2, 37 << 14, 5, (1 << 24) + 5)) == (2 << 11) | 37
    assert int(T.bucket_of(7, 0xFFFFFFFF, 8192, 0xFFFFFFFF)) == 7
    assert int(T.bucket_of(1, 4096, 3, 4096)) == (1 << 12) | 2048


# ---- the directed inputs meet their own conditions (asserted inside the builders)
@pytest.mark.parametrize("mode", ["distinct", "onepos"])
@pytest.mark.parametrize("n", T.BUCKET_ROWS)
def test_bucket_cases_hold_n_rows_in_one_bucket(n, mode):
    assert T.bucket_case(n, mode)["largest_bucket"] == n


def test_table_cases_meet_their_conditions():
    for ns in T.SCAFFOLD_COUNTS:
        c = T.scaffold_case(ns)
        assert (c["largest_bucket"] > T.SORT_LDS) == (ns >= 8192)
    for top in T.MAX_POSITIONS:
        T.maxpos_case(top)
    assert T.shift32_case()["largest_bucket"] >= 40
    for n_hits in T.HIT_COUNTS + [T.big_hit_count(256)]:
        for density in T.DENSITIES:
            T.count_case(n_hits, density)


@pytest.mark.parametrize("name", T.MERGE_CASES)
def test_merge_cases_meet_their_conditions(name):
    c = T.merge_case(name)
    r, g = T.merge_parts(c["parts"], c["part_cap"])
    assert len(r) == len(g) == c["total"]


def test_lookup_cases_meet_their_conditions():
    for name, build in T.lookup_cases().items():
        c = build()
        k = T.row_keys(c["rows"])
        assert np.all(k[1:] >= k[:-1]), name
    e = T.lookup_edges_case()
    assert all(len(v) > 0 for v in e["classes"].values()) and e["n_hits"] > 0
