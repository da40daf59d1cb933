"""The tagger on the 4-byte LINEAR key column (gf_alnrec_linkeys_dev, gf_tag_alignments_linkeys_dev): the column and its MAPQ-0 bit plane
against the numpy twin (tag_linear_twin.py) word for word, and the tagging against the 8-byte-key entry, the record stream and the C oracle —
both insert-size branches, the 4-wave and the 16-wave kernel, each without and behind a fine map, windows at the scaffolds' ends, stale columns,
and one Pipeline.step with the linear column on and off."""
import ctypes as C

import numpy as np
import pytest

import tag_linear_twin as T

pytestmark = pytest.mark.gpu

LOWREC = np.dtype([("pos", "<u4"), ("ref", "<u4"), ("rec", "<u4")])
G = 1 << 20


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


def _build(gf, recs, n_scaffolds, n=None):
    """The linear column of the first n records: (device buffer, layout, host words)."""
    import torch
    from gappadder_amd import _lib as B
    lib = B.lib()
    n = len(recs) if n is None else n
    d_recs = torch.from_numpy(np.frombuffer(recs.tobytes() + bytes(32), dtype=np.uint8).copy()).cuda()
    words = lib.gf_alnrec_linkeys_bytes(n, n_scaffolds) // 4
    assert words == T.parts(n, n_scaffolds)[4]
    d_col = torch.full((words,), 0x55555555, dtype=torch.int32, device="cuda")
    lay = B.TagLayout()
    torch.cuda.synchronize()
    assert lib.gf_alnrec_linkeys_dev(gf.handle, d_recs.data_ptr(), n, d_col.data_ptr(), 4 * words, C.byref(lay)) == 0
    gf.sync()
    return d_recs, d_col, lay, d_col.cpu().numpy().view(np.uint32)


def _edge_records(n, n_scaffolds, ends):
    """n records that walk over the edges of a draft with these scaffold ends: position 0 and the last position of every scaffold (so both sides
    of every boundary), unplaced records, a scaffold behind the last one — each with MAPQ 0 and with MAPQ 30 —, then positions in between."""
    from gappadder_amd import _lib as B
    rng = np.random.default_rng(1000 + n)
    spots = []
    for s in range(n_scaffolds):
        spots += [(s, ends[s] - 1), (s, 0)]                # ... (s, last), (s + 1, 0) follow each other
    spots += [(0xFFFFFFFF, 17), (n_scaffolds, 3)]
    recs = np.zeros(n, dtype=B.ALNREC)
    for i in range(n):
        j = i // 2
        if j < len(spots):
            ref, pos = spots[j]
            mapq = 0 if i % 2 == 0 else 30
        else:
            ref = int(rng.integers(0, n_scaffolds))
            pos = int(rng.integers(0, ends[ref]))
            mapq = int(rng.choice([0, 0, 12, 60]))
        recs[i] = (pos, 0, 0, ref, ref, 0, mapq, 0, i)
    return recs


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4095, 4097, 9001])
def test_column_and_plane_equal_the_twin_word_for_word(gf, n):
    """Every boundary of the four-keys-per-lane load, of the 256-record wave load, of the wave's stage and of the 4 096-record run of the pass that
    measures the ends (the filler records hop between the scaffolds, so its lanes end on different ones); the pads carry the sentinel and zero
    bits, the buffer's last part the layout's base[]."""
    from gappadder_amd import _lib as B
    ns, ends = 3, [G, G + 1, 3 * G + 12345]                # one granule exactly, one granule plus 1, a non-multiple
    gf.set_gaps(np.zeros(0, dtype=B.GAP), ns)
    recs = _edge_records(n, ns, ends)
    _, _, lay, got = _build(gf, recs, ns)
    want = T.layout(T.ends_of(recs, ns), n)
    assert (lay.use, lay.n_recs, lay.n_scaffolds, lay.granule_log2, lay.span, lay.checksum) == \
           (1, n, ns, want["granule_log2"], want["span"], want["checksum"])
    keys, plane = T.column(recs, ns, want["base"])
    kw, p_at, pw, b_at, total = T.parts(n, ns)
    assert (got[:kw] == keys).all(), np.nonzero(got[:kw] != keys)[0][:8]
    assert (got[p_at:p_at + pw] == plane).all(), np.nonzero(got[p_at:p_at + pw] != plane)[0][:8]
    assert (got[b_at:total] == want["base"]).all()
    if n >= 16:       # the list's edge records are all there: keys on both sides of every boundary, sentinels, MAPQ-0 bits on each
        assert keys[0] == G - 1 and keys[2] == 0 and keys[4] == want["base"][1] + G and keys[6] == want["base"][1]
        assert keys[12] == keys[13] == keys[14] == keys[15] == T.SENTINEL and plane[0] & 0xFFFF == 0x0555


def _draft(kind):
    """(gaps, n_scaffolds, scaffold ends).  small: three scaffolds, the first exactly one granule long; a gap whose left window starts below 0,
    two gaps inside one 64-base bin, a gap whose right window passes the scaffold's last record, and a gap at the very start of the next
    scaffold.  wide: 4 x 5 Mb with eight gaps each.  many: 4 x 5 Mb with 100 gaps of 1 500 bases each, evenly spaced; vast: 64 x 5 Mb with 160
    gaps of 200 bases each — the two whose LDS map (at 2^13 / 2^19 bins) has wide bins, more than a twentieth of them set, and so a fine map."""
    from gappadder_amd import _lib as B
    if kind == "small":
        ends = [G, 40_000, 50_000]
        rows = [(0, 100, 300), (0, 20_000, 20_010), (0, 20_020, 20_030), (0, 500_000, 501_000), (0, G - 400, G - 100),
                (1, 5, 50), (1, 20_000, 21_000), (1, 39_700, 39_990), (2, 0, 40), (2, 25_000, 25_500)]
    elif kind in ("many", "vast"):
        n_scf, per, glen = {"many": (4, 100, 1500), "vast": (64, 160, 200)}[kind]
        ends = [5_000_000] * n_scf
        step = 5_000_000 // per
        rows = [(s, step // 2 + step * j + 7 * s, step // 2 + step * j + 7 * s + glen) for s in range(n_scf) for j in range(per)]
    else:
        ends = [5_000_000] * 4
        rows = [(s, 300_000 + 600_000 * j + 1000 * s, 300_000 + 600_000 * j + 1000 * s + 1500) for s in range(4) for j in range(8)]
        rows[0] = (0, 120, 900)
        rows[15] = (1, 4_999_200, 4_999_900)
    gaps = np.zeros(len(rows), dtype=B.GAP)
    idx = {}
    for i, (s, a, b) in enumerate(rows):
        idx[s] = idx.get(s, 0) + 1
        gaps[i] = (s, a, b, idx[s])
    return gaps, len(ends), ends


def _records(gaps, n_scaffolds, ends, dist2, n_far, seed):
    """Records around every gap's windows (both sides of every window edge), at the scaffolds' ends, far from every gap, unplaced and on an unknown
    scaffold; every branch of the hit rules: clipped, mate elsewhere, long and short templates, unmapped mates, low and zero MAPQ."""
    from gappadder_amd import _lib as B
    rng = np.random.default_rng(seed)
    where = []
    for g in gaps:
        s, a, b = int(g["scaffold"]), int(g["start"]), int(g["end"])
        for p in list(range(a - dist2 - 2, a - dist2 + 3)) + list(range(b + dist2 - 3, b + dist2 + 2)) + [a - 1, a, a + 1, b - 1, b, b + 1] + \
                rng.integers(a - dist2 - 40, b + dist2 + 40, size=60).tolist():
            if 0 <= p < ends[s]:
                where.append((s, int(p)))
    for s in range(n_scaffolds):
        where += [(s, 0), (s, 1), (s, ends[s] - 1), (s, ends[s] - 2)]
        where += [(s, int(p)) for p in rng.integers(0, ends[s], size=n_far // n_scaffolds)]
    where += [(0xFFFFFFFF, 200), (n_scaffolds, 150), (n_scaffolds + 7, 0), (0xFFFFFFFF, 0)]
    where.sort(key=lambda t: (t[0], t[1]))
    n = len(where)
    recs = np.zeros(n, dtype=B.ALNREC)
    recs["ref"] = [w[0] for w in where]
    recs["pos"] = [w[1] for w in where]
    recs["mate_ref"] = np.where(rng.random(n) < 0.25, (recs["ref"] + 1) % n_scaffolds, recs["ref"])
    recs["mate_pos"] = rng.integers(0, 30_000, size=n)
    recs["tlen"] = rng.choice([0, 150, -210, 280, 400, -900, 4000, -5200, 7000, 12_000], size=n)
    recs["flag"] = rng.choice([0x1, 0x1 | 0x10, 0x1 | 0x8, 0x1 | 0x4, 0x1 | 0x20], p=[0.4, 0.3, 0.15, 0.05, 0.1], size=n)
    recs["mapq"] = rng.choice([0, 10, 30, 60], p=[0.2, 0.1, 0.3, 0.4], size=n)
    recs["clipflag"] = rng.integers(0, 4, size=n)
    recs["read"] = np.arange(n)
    return recs


def _run(gf, entry, d_recs, n, is_, sd, d_col=None, lay=None, d_keys=None):
    """(sorted hits, sorted MAPQ-0 list, (waves per workgroup, stream form), gf_tag_kernel's name of the kernel) of one tagger entry."""
    import torch
    from gappadder_amd import _lib as B
    lib = B.lib()
    cap = max(4096, 4 * n)
    d_hits = torch.zeros(cap * 12, dtype=torch.uint8, device="cuda")
    d_low = torch.zeros(cap * 12, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tail = (n, is_, sd, 250, 30, d_hits.data_ptr(), cap, d_cnt.data_ptr(), d_low.data_ptr(), cap, d_cnt.data_ptr() + 4)
    if entry == "lin":
        rc = lib.gf_tag_alignments_linkeys_dev(gf.handle, d_recs.data_ptr(), d_col.data_ptr() if d_col is not None else None,
                                               C.byref(lay) if lay is not None else None, d_keys.data_ptr() if d_keys is not None else None, *tail)
    elif entry == "keys":
        rc = lib.gf_tag_alignments_keys_dev(gf.handle, d_recs.data_ptr(), d_keys.data_ptr(), *tail)
    else:
        rc = lib.gf_tag_alignments_low_dev(gf.handle, d_recs.data_ptr(), *tail)
    assert rc == 0, rc
    gf.sync()
    nw, form = C.c_int(), C.c_int()
    assert lib.gf_tag_last_launch(gf.handle, C.byref(nw), C.byref(form)) == 0
    nh, nl = int(d_cnt[0]), int(d_cnt[1])
    assert nh <= cap and nl <= cap
    hits = np.frombuffer(d_hits[:nh * 12].cpu().numpy().tobytes(), dtype=B.TAGHIT)
    low = np.frombuffer(d_low[:nl * 12].cpu().numpy().tobytes(), dtype=LOWREC)
    return np.sort(hits, order=["rec", "gap", "kind", "to_mate"]), np.sort(low, order=["rec"]), (nw.value, form.value), lib.gf_tag_kernel(gf.handle).decode()


def _keys8(gf, d_recs, n):
    import torch
    from gappadder_amd import _lib as B
    d_keys = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert B.lib().gf_alnrec_keys_dev(gf.handle, d_recs.data_ptr(), n, d_keys.data_ptr()) == 0
    gf.sync()
    return d_keys


@pytest.fixture(scope="module")
def cases(gf):
    """Per (draft, insert size): the records, and the hits and the MAPQ-0 list they must give — from the C oracle and from numpy, computed once."""
    from oracle import c_oracle as CO
    out = {}
    for kind, walk in (("small", 1), ("wide", 1), ("many", 7), ("vast", 157)):    # (records around every walk-th gap: a few thousand in all)
        gaps, ns, ends = _draft(kind)
        for is_, sd in ((300, 30), (5000, 500)) if walk == 1 else ((300, 30),):
            recs = _records(gaps[::walk], ns, ends, is_ + 3 * sd, 1200, seed=is_ + len(kind))
            want = np.sort(CO.tag_alignments(recs, gaps, is_, sd).astype(_taghit()), order=["rec", "gap", "kind", "to_mate"])
            z = np.nonzero((recs["mapq"] == 0) & (recs["ref"] < ns))[0]
            low = np.zeros(len(z), dtype=LOWREC)
            low["pos"], low["ref"], low["rec"] = recs["pos"][z], recs["ref"][z], z
            out[kind, is_] = (gaps, ns, ends, recs, want, low)
    return out


def _taghit():
    from gappadder_amd import _lib as B
    return B.TAGHIT


@pytest.mark.parametrize("kind,bins_log2,waves,is_,sd", [
    ("small", 17, 4, 300, 30), ("small", 17, 4, 5000, 500), ("wide", 19, 16, 300, 30), ("wide", 19, 16, 5000, 500),
    ("many", 13, 4, 300, 30), ("vast", 19, 16, 300, 30)])
def test_tagging_equals_the_other_entries_and_the_oracle(gf, cases, kind, bins_log2, waves, is_, sd):
    """Hit multiset and MAPQ-0 list of the linear entry = the 8-byte-key entry = the record stream (device and gf.tag_alignments) = the C oracle,
    each from the kernel the case is there for (gf_tag_kernel).  The small draft takes the 4-wave kernel; 4 x 5 Mb with 2^19 bins asked for gets
    a map above 32 KiB and the 16-wave kernel; both maps have 64-base bins and no fine map.  many (2^13 bins: 4 096-base bins, an eighth set)
    and vast (2^19 bins: 1 024-base bins, a sixteenth set — the form of the full-size benchmark) run the same two kernels behind a fine map:
    the candidate queue's fine-map test, and for the records the queued form of the kernel."""
    gaps, ns, ends, recs, want, want_low = cases[kind, is_]
    fine = kind in ("many", "vast")
    n = len(recs)
    gf.set_gaps(gaps, ns)
    gf.set_option("tag_bins_log2", bins_log2)
    try:
        d_recs, d_col, lay, _ = _build(gf, recs, ns)
        assert lay.use == 1 and lay.n_recs == n
        d_keys = _keys8(gf, d_recs, n)
        lin = _run(gf, "lin", d_recs, n, is_, sd, d_col, lay)
        keys = _run(gf, "keys", d_recs, n, is_, sd, d_keys=d_keys)
        rec = _run(gf, "recs", d_recs, n, is_, sd)
        host = np.sort(gf.tag_alignments(recs, is_, sd), order=["rec", "gap", "kind", "to_mate"])
    finally:
        gf.set_option("tag_bins_log2", 17)
    assert lin[2] == (waves, 2) and keys[2] == (waves, 1) and rec[2] == (waves, 0)
    tail = "+fine" if fine else ""
    assert lin[3] == "tag_kernel<%d, true, false, 2>%s" % (waves, tail) and keys[3] == "tag_kernel<%d, true, false, 1>%s" % (waves, tail)
    assert rec[3] == "tag_kernel<%d, true, %s, 0>%s" % (waves, "true" if fine else "false", tail)
    assert len(want) > 200 and len(want_low) > 100
    for hits, low, *_ in (lin, keys, rec):
        assert len(hits) == len(want) and (hits == want).all()
        assert len(low) == len(want_low) and (low == want_low).all()
    assert len(host) == len(want) and (host == want).all()
    # the edge gaps are hit from inside their own scaffold only: every hit's record lies on its gap's scaffold
    assert (recs["ref"][lin[0]["rec"]] == gaps["scaffold"][lin[0]["gap"]]).all()
    edge = {"small": (0, 4, 5, 8), "wide": (0, 15)}.get(kind, ())
    assert all((lin[0]["gap"] == g).any() for g in edge)


def test_a_stale_column_is_refused_and_the_call_answers_from_the_other_columns(gf, cases):
    from gappadder_amd import _lib as B
    gaps, ns, ends, recs, want, want_low = cases["small", 300]
    n = len(recs)
    gf.set_gaps(gaps, ns)
    d_recs, d_col, lay, _ = _build(gf, recs, ns)
    d_keys = _keys8(gf, d_recs, n)
    ok = _run(gf, "lin", d_recs, n, 300, 30, d_col, lay, d_keys)
    assert ok[2] == (4, 2) and (ok[0] == want).all()

    def other(**kw):
        o = B.TagLayout.from_buffer_copy(lay)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    # another record count, a granule base[] is not a multiple of, another base[] (checksum), another scaffold count, a layout that says "keep none"
    assert lay.granule_log2 == 20
    for bad in (other(n_recs=n - 1), other(granule_log2=21), other(checksum=lay.checksum ^ 1), other(n_scaffolds=ns + 1), other(use=0)):
        r8 = _run(gf, "lin", d_recs, n, 300, 30, d_col, bad, d_keys)
        r0 = _run(gf, "lin", d_recs, n, 300, 30, d_col, bad, None)
        assert r8[2] == (4, 1) and r0[2] == (4, 0)
        for hits, low, *_ in (r8, r0):
            assert len(hits) == len(want) and (hits == want).all() and len(low) == len(want_low) and (low == want_low).all()
    # a column built for one record less, asked about all of them
    _, d_col1, lay1, _ = _build(gf, recs, ns, n - 1)
    assert lay1.n_recs == n - 1 and _run(gf, "lin", d_recs, n, 300, 30, d_col1, lay1, d_keys)[2] == (4, 1)
    # the context's scaffolds changed under the column
    gf.set_gaps(gaps, ns + 2)
    r = _run(gf, "lin", d_recs, n, 300, 30, d_col, lay, d_keys)
    assert r[2] == (4, 1) and len(r[0]) == len(want)
    # no column at all
    gf.set_gaps(gaps, ns)
    assert _run(gf, "lin", d_recs, n, 300, 30, None, None, d_keys)[2] == (4, 1)


def test_a_draft_beyond_32_bits_is_served_by_the_8_byte_column(gf):
    """Three scaffolds with one record each near position 2^31: use = 0, no column; the linear entry answers from the 8-byte column, with the
    record stream's results."""
    from gappadder_amd import _lib as B
    gaps = np.zeros(2, dtype=B.GAP)
    gaps[0] = (0, (1 << 31) - 200, (1 << 31) - 100, 1)
    gaps[1] = (2, (1 << 31) + 100, (1 << 31) + 300, 1)
    gf.set_gaps(gaps, 3)
    recs = np.zeros(3, dtype=B.ALNREC)
    recs["ref"], recs["mate_ref"] = [0, 1, 2], [1, 1, 2]
    recs["pos"] = [(1 << 31) - 250, (1 << 31) + 5, (1 << 31) + 320]
    recs["flag"], recs["mapq"], recs["tlen"], recs["clipflag"], recs["read"] = 1, [60, 0, 60], [0, 0, 9000], [2, 0, 1], [0, 1, 2]
    d_recs, d_col, lay, _ = _build(gf, recs, 3)
    assert lay.use == 0
    d_keys = _keys8(gf, d_recs, 3)
    lin = _run(gf, "lin", d_recs, 3, 300, 30, d_col, lay, d_keys)
    rec = _run(gf, "recs", d_recs, 3, 300, 30)
    assert lin[2][1] == 1 and len(rec[0]) >= 3 and (lin[0] == rec[0]).all() and (lin[1] == rec[1]).all() and lin[1]["rec"].tolist() == [1]


def test_a_pipeline_step_with_the_linear_column_on_and_off(gf):
    """Hits, pools, contigs and picks of one step are the same with the linear column, with the 8-byte column alone and with gap_span switched
    on — which still gets its 8-byte column beside the linear one."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline, decode_best
    seed, slen, nscf, gps, glen, L, n_pairs = 31, 300_000, 2, 5, 150, 150, 20_000
    cfg = GapFill.synth_cfg(seed=seed, scaffold_len=slen, n_scaffolds=nscf, gaps_per_scaffold=gps, gap_len=glen, read_len=L)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf.set_gaps(gaps, nscf, flanks)
    out = []
    for linear, span in ((True, False), (False, False), (True, True)):
        d_reads = torch.empty(2 * n_pairs * 38 + 64, dtype=torch.uint8, device="cuda")
        d_recs = torch.empty(2 * n_pairs * 32, dtype=torch.uint8, device="cuda")
        gf.synth_pairs_dev(cfg, 0, n_pairs, d_reads.data_ptr(), d_recs.data_ptr())
        gf.sync()
        pipe = Pipeline(gf, len(gaps), L, [(31, 29)], keep_read_ids=True, linear_keys=linear, gap_span=span)
        lb = pipe.add_library(DeviceLibrary("x", 300, 30, 2 * n_pairs, d_reads, d_recs))
        assert (lb.d_lin_keys is not None) == linear and (lb.d_rec_keys is not None) == (span or not linear)
        assert not linear or (lb.lin_layout.use == 1 and lb.lin_layout.n_recs == 2 * n_pairs)
        pipe.prepare()
        pipe.finish()
        res = pipe.fetch(pools=True)
        nw, form = C.c_int(), C.c_int()
        assert B.lib().gf_tag_last_launch(gf.handle, C.byref(nw), C.byref(form)) == 0 and form.value == (2 if linear else 1)
        ctg = sorted((int(c["gap"]), res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])]) for c in res.contigs)
        picks = []
        for g, b in enumerate(res.best.tolist()):
            if b:
                a_len, span1, ci, rev = decode_best(b)
                c = res.contigs[ci]
                picks.append((g, a_len, span1, rev, res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])]))
        assert lb.counts["tagger_hits"] > 64 and (res.gap_span is not None) == span
        out.append((lb.counts, res.pool_off.tolist(), res.pool_rows.tobytes(), ctg, picks))
    assert out[0] == out[1] == out[2] and len(out[0][3]) > 5
