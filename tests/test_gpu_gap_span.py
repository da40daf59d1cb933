"""gf_gap_span_dev (csrc/gap_span.hip) through the C ABI against its host twin (gappadder_amd/gap_span.py): records and statistics equal,
byte for byte — on the hand-built records of gap_span_util (where the expectation is also written down by hand), on record counts of 0, 1,
63, 64, 65, 257 and 5 003, in the key-column form, the record form (d_keys null) and in shuffled record order, on out-of-range and '*'
scaffolds and a scaffold without gaps, on two libraries (1 500 +/- 100 and 5 000 +/- 500) over gaps of 200 to 3 000 bases of which some
lie closer together than L and some closer than dist2, and on gap tables large enough for every form of bin map the launch chooses among.

Which form a case reaches is established by _map_form below, a restatement in Python of the rule the library builds its maps by
(tag_map.hip, ensure_bin_map: a 16-KiB map; the 64-KiB one when more than a tenth of its bins are set; a fine map behind it when more
than a twentieth still is and the fine bins cover at most 0.6 of what the coarse ones do) — asserted per case:
  the hand-built table, the two-library table           the small LDS map (4-wave workgroups)
  9 000 gaps over 2.6 Gb, library 1 500 +/- 100         the 64-KiB map without a fine map (16-wave workgroups)
  20 000 gaps over 2.6 Gb, library 1 500 +/- 100        the 64-KiB map with a fine map
  20 000 gaps over 2.6 Gb, library 5 000 +/- 500        the 64-KiB map, the fine map rejected (its windows are wider than the bins)"""
import numpy as np
import pytest

import gap_span_util as U

pytestmark = pytest.mark.gpu

def _dev(gf, recs, L, mu, sd, z, shift, q, keys=True, n=None):
    """(gf_gap_span per gap, statistics dictionary, raw statistics words) of gf_gap_span_dev on the first n records."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import gap_span as GS
    lib, h = B.lib(), gf.handle
    n = len(recs) if n is None else n
    d_recs = torch.from_numpy(np.frombuffer(recs.tobytes() + b"\0" * 64, dtype=np.uint8).copy()).cuda()
    d_keys = torch.empty(n + 2, dtype=torch.int64, device="cuda")
    d_rec = torch.full((max(1, gf.n_gaps) * 64,), 0xAB, dtype=torch.uint8, device="cuda")       # (the call clears its outputs)
    d_stats = torch.full((B.GS_WORDS,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if keys:
        gf._chk(lib.gf_alnrec_keys_dev(h, d_recs.data_ptr(), n, d_keys.data_ptr()), "gf_alnrec_keys_dev")
    gf._chk(lib.gf_gap_span_dev(h, d_recs.data_ptr(), d_keys.data_ptr() if keys else None, n, L, mu, sd, z, shift, q, d_rec.data_ptr(),
                                d_stats.data_ptr()), "gf_gap_span_dev")
    gf.sync()
    out = np.frombuffer(d_rec.cpu().numpy().tobytes(), dtype=B.GAP_SPAN)[:gf.n_gaps]
    st = d_stats.cpu().numpy()
    return out, GS.stats_of(st), st


def _same(got, want):
    bad = [g for g in range(len(want)) if got[g].tobytes() != want[g].tobytes()]
    assert not bad, [(g, got[g], want[g]) for g in bad[:4]]


@pytest.fixture(scope="module")
def hand():
    from gappadder_amd.hip_api import GapFill
    gf = GapFill(0)
    gf.set_gaps(U.GAPS, U.N_SCAFFOLDS)
    return gf


@pytest.mark.parametrize("keys", [True, False], ids=["keys", "records"])
@pytest.mark.parametrize("shift", [0, 200, 1000])
def test_hand_built_records(hand, shift, keys):
    from gappadder_amd import gap_span as GS
    cases = U.hand_cases()
    recs = U.records([c[2] for c in cases if c[1] == shift])
    want, stats = GS.gap_span_host(recs, U.GAPS, U.N_SCAFFOLDS, U.L, U.MU, U.SD, U.Z, shift, U.Q)
    assert want.tobytes() == U.expected(cases, shift).tobytes() and stats["accepted"] > 0
    assert _map_form(U.GAPS, U.N_SCAFFOLDS, U.DIST2) == ("small", False)
    got, gstats, _ = _dev(hand, recs, U.L, U.MU, U.SD, U.Z, shift, U.Q, keys)
    _same(got, want)
    assert gstats == stats
    # one record at a time, where a wave holds nothing else
    for name, d, row, exp in cases[::3]:
        if d == shift:
            got, _, _ = _dev(hand, U.records([row]), U.L, U.MU, U.SD, U.Z, shift, U.Q, keys)
            _same(got, U.expected([(name, d, row, exp)], shift))


def test_records_that_must_be_ignored_index_nothing(hand):
    """Out-of-range and '*' scaffolds, a scaffold without gaps, positions beyond the map: an all-zero answer, in both forms."""
    rows = [c[2] for c in U.hand_cases() if c[0] in ("scaffold out of range", "scaffold = n_scaffolds", "unplaced", "scaffold without gaps",
                                                     "beyond the last window", "at the largest position", "pos 0")]
    assert len(rows) == 7
    recs = U.records(rows * 40)
    for keys in (True, False):
        got, stats, raw = _dev(hand, recs, U.L, U.MU, U.SD, U.Z, 0, U.Q, keys)
        assert not got.tobytes().strip(b"\0") and not raw.tobytes().strip(b"\0")


def test_errors(hand):
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    lib = B.lib()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    for mu, sd, z, shift, q, L in ((1500, 100, 0, 0, 30, 100), (1500, 100, 3, -1, 30, 100), (1500, -1, 3, 0, 30, 100), (-5, 0, 3, 0, 30, 100),
                                   (1500, 100, 3, 0, 256, 100), (1500, 100, 3, 0, -1, 100), (1500, 100, 3, 0, 30, 0),
                                   (1 << 20, 0, 1, 0, 30, 100), (1000000, 10000, 3, (1 << 20) - 1030000, 30, 100)):
        assert lib.gf_gap_span_dev(hand.handle, p, None, 1, L, mu, sd, z, shift, q, p + 1024, p + 2048) == B.GF_E_UNSUPPORTED
    empty = GapFill(0)
    assert lib.gf_gap_span_dev(empty.handle, p, None, 1, 100, 1500, 100, 3, 0, 30, p + 1024, p + 2048) == B.GF_E_STATE


# ---- generated libraries --------------------------------------------------------------------------------------------------------------
def _pairs(rng, gaps, sel, L, mu, sd, per_gap, n_scaffolds):
    """Coordinate-sorted records of read pairs planted around the gaps `sel`: the forward mate up to 30 bases outside either end of the
    left window, the insert from the library's normal with a twentieth of outliers, a twentieth each clipped and of low MAPQ; every
    pair's reverse record as well, and a few records that are unmapped, unplaced or on scaffolds beyond the table."""
    dist2 = mu + 3 * sd
    rows = []
    for g in sel:
        s, start = int(gaps[g]["scaffold"]), int(gaps[g]["start"])
        for _ in range(per_gap):
            a0 = start - int(rng.integers(L - 5, dist2 + 30))
            x = int(rng.normal(mu, sd)) if rng.random() > 0.05 else int(mu + rng.choice([-1, 1]) * rng.integers(3 * sd, 8 * sd + 50))
            x = max(x, L + 1)
            m0 = a0 + x - L
            if a0 < 0:
                continue
            mapq = 60 if rng.random() > 0.05 else int(rng.integers(0, 30))
            clip = 0 if rng.random() > 0.05 else int(rng.integers(1, 4))
            first = rng.random() < 0.5
            rows.append((a0 + 1, m0 + 1, x, s, s, 0x1 | 0x20 | (0x40 if first else 0x80), mapq, clip, 2 * len(rows)))
            rows.append((m0 + 1, a0 + 1, -x, s, s, 0x1 | 0x10 | (0x80 if first else 0x40), 60, 0, 2 * len(rows) + 1))
    for _ in range(max(4, len(rows) // 50)):
        ref = int(rng.choice([n_scaffolds, n_scaffolds + 3, 0xFFFFFFFF, 0x7FFFFFFF]))
        rows.append((int(rng.integers(1, 1 << 20)), 0, 0, ref, ref, 0x1 | 0x4 | 0x8, 0, 0, 0))
    recs = U.records(rows)
    return recs[np.lexsort((recs["pos"], recs["ref"]))]


def _table(rng, n_scaffolds, per_scaffold, spacing, near=()):
    """Gaps of 200 to 3 000 bases, `spacing` (lo, hi) bases apart; every k-th gap of `near` = {k: distance} follows its predecessor at
    that distance instead.  The last scaffold stays without gaps."""
    from gappadder_amd import _lib as B
    rows = []
    for s in range(n_scaffolds - 1):
        pos = 20_000
        for i in range(per_scaffold):
            d = int(rng.integers(*spacing))
            for k, dist in near.items():
                if i % k == k - 1:
                    d = dist
            pos += d
            ln = int(rng.integers(200, 3001))
            rows.append((s, pos, pos + ln, i + 1))
            pos += ln
    return np.array(rows, dtype=B.GAP)


def _map_form(gaps, n_scaffolds, dist2):
    """("small" | "big", has a fine map) of the bin map the library builds for these gaps and dist2 (module docstring)."""
    span = np.zeros(n_scaffolds, dtype=np.int64)
    np.maximum.at(span, gaps["scaffold"].astype(np.int64), gaps["end"].astype(np.int64) + dist2)

    def nbits(sh):
        return int(((span >> sh) + (span > 0)).sum())

    def n_set(sh):
        off = np.concatenate([[0], np.cumsum((span >> sh) + (span > 0))])
        lo = np.maximum(0, gaps["start"].astype(np.int64) - dist2 + 1) >> sh
        hi = (gaps["end"].astype(np.int64) + dist2 - 1) >> sh
        base = off[gaps["scaffold"].astype(np.int64)]
        cnt = hi - lo + 1
        idx = np.repeat(base + lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        return len(np.unique(idx))
    shift = 6
    while nbits(shift) > (1 << 17):
        shift += 1
    if shift > 8 and n_set(shift) * 10 > nbits(shift):
        while shift > 6 and nbits(shift - 1) <= (1 << 19):
            shift -= 1
    words = (nbits(shift) + 31) // 32 + 1
    set_bits = n_set(shift)
    fine = False
    if shift > 9 and set_bits * 20 > nbits(shift):
        fs = 7
        while nbits(fs) > (1 << 23):
            fs += 1
        if fs + 2 <= shift:
            fine = n_set(fs) * (1 << fs) <= 0.6 * set_bits * (1 << shift)
    return ("big" if words * 4 > 32 * 1024 else "small"), fine


LIBS = [(1500, 100), (5000, 500)]
L2 = 100


@pytest.fixture(scope="module")
def two_libs():
    from gappadder_amd.hip_api import GapFill
    rng = np.random.default_rng(20260021)
    # every 5th gap 60 bases (< L) behind its predecessor, every 7th 900 bases (< dist2 of either library)
    gaps = _table(rng, 3, 40, (9_000, 30_000), near={5: 60, 7: 900})
    d = gaps["start"][1:].astype(np.int64) - gaps["end"][:-1].astype(np.int64)
    assert ((d > 0) & (d < L2)).any() and ((d >= L2) & (d < 1800)).any() and int((gaps["end"] - gaps["start"]).min()) >= 200
    gf = GapFill(0)
    gf.set_gaps(gaps, 3)
    recs = [_pairs(rng, gaps, range(len(gaps)), L2, mu, sd, 70, 3) for mu, sd in LIBS]
    return gf, gaps, recs


def test_two_libraries_and_the_comparison_is_not_vacuous(two_libs):
    from gappadder_amd import gap_span as GS
    gf, gaps, recs = two_libs
    for (mu, sd), r in zip(LIBS, recs):
        assert _map_form(gaps, 3, mu + 3 * sd) == ("small", False)
        assert len(r) % 256 and len(r) % 1024 and len(r) > 4000
        for shift in (0, 300):
            want, stats = GS.gap_span_host(r, gaps, 3, L2, mu, sd, 3, shift, 30)
            print("library %d +/- %d, shift %d: %s" % (mu, sd, shift, stats))
            # from the twin alone: accepted pairs exist and every drop counter is non-zero somewhere
            # (a 1 500-base insert spans only the gaps below about 1 300 bases: a third of the table)
            assert stats["accepted"] > 200 and stats["gaps_with_pairs"] >= 15
            if shift == 0:
                assert all(stats[k] > 0 for k in ("multi", "clipped", "lowq", "low", "high")), stats
            assert int(want["n"].max()) >= 30
            got, gstats, _ = _dev(gf, r, L2, mu, sd, 3, shift, 30)
            _same(got, want)
            assert gstats == stats


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5003])
def test_record_counts(two_libs, n):
    from gappadder_amd import gap_span as GS
    gf, gaps, recs = two_libs
    full = GS.gap_span_host(recs[0], gaps, 3, L2, 1500, 100, 3, 0, 30)[0]
    g = int(np.argmax(full["n"]))            # the slice begins where the left window of the gap with the most pairs does
    first = int(np.searchsorted((recs[0]["ref"].astype(np.int64) << 32) | recs[0]["pos"], (int(gaps[g]["scaffold"]) << 32) | (int(gaps[g]["start"]) - 1800)))
    r = recs[0][first:first + n].copy()
    assert len(r) == n
    want, stats = GS.gap_span_host(r, gaps, 3, L2, 1500, 100, 3, 0, 30)
    assert n < 63 or stats["candidates"] > 0
    for keys in (True, False):
        got, gstats, _ = _dev(gf, r, L2, 1500, 100, 3, 0, 30, keys)
        _same(got, want)
        assert gstats == stats


def test_the_two_forms_and_a_shuffled_order_agree(two_libs):
    from gappadder_amd import gap_span as GS
    gf, gaps, recs = two_libs
    r = recs[1]
    want, stats = GS.gap_span_host(r, gaps, 3, L2, 5000, 500, 3, 100, 30)
    a, sa, _ = _dev(gf, r, L2, 5000, 500, 3, 100, 30, True)
    b, sb, _ = _dev(gf, r, L2, 5000, 500, 3, 100, 30, False)
    shuffled = r[np.random.default_rng(3).permutation(len(r))]
    c, sc, _ = _dev(gf, shuffled, L2, 5000, 500, 3, 100, 30, True)
    d, sd_, _ = _dev(gf, shuffled, L2, 5000, 500, 3, 100, 30, False)
    assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes() == want.tobytes() and sa == sb == sc == sd_ == stats
    assert stats["accepted"] > 1000


# ---- every form of the bin map --------------------------------------------------------------------------------------------------------
# name -> (gaps per scaffold — four scaffolds with gaps, about 640 Mb each, and a fifth without —, their spacing, is_mean, is_sd, the form)
BIG = {"64 KiB": (2250, (40_000, 650_000), 1500, 100, ("big", False)), "64 KiB + fine": (5000, (20_000, 290_000), 1500, 100, ("big", True)),
       "64 KiB, fine rejected": (5000, (20_000, 290_000), 5000, 500, ("big", False))}
_TABLES = {}


def _big_table(per_scaffold, spacing):
    if (per_scaffold, spacing) not in _TABLES:
        _TABLES[per_scaffold, spacing] = _table(np.random.default_rng(20260022), 5, per_scaffold, spacing, near={9: 70, 11: 1200})
    return _TABLES[per_scaffold, spacing]


@pytest.mark.parametrize("name", sorted(BIG))
def test_every_form_of_the_bin_map(name):
    from gappadder_amd import gap_span as GS
    from gappadder_amd.hip_api import GapFill
    per_scaffold, spacing, mu, sd, form = BIG[name]
    gaps = _big_table(per_scaffold, spacing)
    n_gaps = len(gaps)
    assert n_gaps == 4 * per_scaffold and int(gaps["end"].max()) > 600_000_000
    assert _map_form(gaps, 5, mu + 3 * sd) == form
    rng = np.random.default_rng(len(name))
    sel = np.sort(rng.choice(n_gaps, 150, replace=False))
    sel = np.unique(np.concatenate([sel, [0, 8, 9, n_gaps // 4 - 1, n_gaps // 4, n_gaps - 1]]))      # the table's ends, a close pair, a scaffold change
    recs = _pairs(rng, gaps, sel, 100, mu, sd, 24, 5)
    want, stats = GS.gap_span_host(recs, gaps, 5, 100, mu, sd, 3, 0, 30)
    print("%s: %d records, %s" % (name, len(recs), stats))
    assert stats["accepted"] > 200 and stats["gaps_with_pairs"] >= 30 and all(stats[k] > 0 for k in ("multi", "clipped", "lowq", "low", "high"))
    gf = GapFill(0)
    gf.set_gaps(gaps, 5)
    for keys in (True, False):
        got, gstats, _ = _dev(gf, recs, 100, mu, sd, 3, 0, 30, keys)
        _same(got, want)
        assert gstats == stats
