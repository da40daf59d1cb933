"""The step's contig list at and beyond its capacities (contig_cap records, seq_cap bases; DESIGN.md "Capacities").

Producer: gf_assemble_multi_dev writes every record below contig_cap either with its bases inside seq_cap or as a tombstone (length 0,
seq_off 0), counts everything in its counters, and writes nothing beyond either cap.  Consumers — both picks, the extended fill, the merge
round and the round-2 k-mer table — read only [first, min(n, contig_cap)) and skip tombstones; the merge round keeps an overflow it is
handed visible.  Pipeline: a step whose list outgrows a cap raises in fetch(), and the next step with the caps restored is clean."""
import collections

import numpy as np
import pytest

import pick_util as PK
from step_util import L, N_PAIRS, picks as _picks, setup as _setup

pytestmark = pytest.mark.gpu

CANARY_GAP = 0xFFFFFFFE
KK = [(31, 29), (41, 39), (51, 49)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


def _canary_records(n):
    from gappadder_amd import _lib as B
    c = np.frombuffer(b"\x5a" * (32 * n), dtype=B.CONTIG).copy()
    c["gap"] = CANARY_GAP
    return c


def _text(ctg, seq, i):
    c = ctg[i]
    return seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])].decode()


# ---- A. the producer: gf_assemble_multi_dev at its caps ----------------------------------------------------------------------------

def _assemble_capped(gf, d_pool, d_off, n_pools, rows, L, kk, contig_cap, seq_cap, slack=64):
    """One call with buffers `slack` records / 4 KiB larger than the caps it is told, the region beyond filled with canaries."""
    import torch
    from gappadder_amd import _lib as B
    d_ctg = _dev(_canary_records(contig_cap + slack).view(np.uint8))
    d_seq = torch.full((seq_cap + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    d_err = torch.zeros(n_pools, dtype=torch.int32, device="cuda")
    k_arr, kv_arr = np.array([a for a, _ in kk], dtype=np.int32), np.array([b for _, b in kk], dtype=np.int32)
    assert B.lib().gf_assemble_multi_dev(gf.handle, d_pool.data_ptr(), None, d_off.data_ptr(), n_pools, rows, L, B._p(k_arr), B._p(kv_arr),
                                         len(kk), 2, 40, d_ctg.data_ptr(), contig_cap, d_cnt.data_ptr(), d_seq.data_ptr(), seq_cap,
                                         d_cnt.data_ptr() + 8, d_err.data_ptr()) == 0
    gf.sync()
    ctg = np.frombuffer(d_ctg.cpu().numpy().tobytes(), dtype=B.CONTIG)
    cnt = d_cnt.cpu().numpy()
    return ctg, d_seq.cpu().numpy().tobytes(), int(cnt[0]), int(cnt[2:4].view(np.uint64)[0]), d_err.cpu().numpy()


@pytest.mark.parametrize("seed,kk", [(31, [(31, 29), (51, 49)]), (32, [(41, 39), (63, 61)])])
def test_assembly_at_its_caps_writes_tombstones_and_counts_everything(gf, seed, kk):
    import synth_small as S
    from gappadder_amd.hip_api import GapFill
    from test_gpu_assembly import _pools_from_case
    L = 150
    pools = _pools_from_case(S.small_case(seed=seed, n_pairs=12000, L=L, insert=300))
    packed, _ = GapFill.pack_reads(b"".join(pools), L)
    off = np.cumsum([0] + [len(p) // L for p in pools]).astype(np.int64)
    d_pool, d_off = _dev(packed.reshape(-1)), _dev(off)
    rows = int(off[-1])
    run = lambda cc, sc: _assemble_capped(gf, d_pool, d_off, len(pools), rows, L, kk, cc, sc)
    ctg0, seq0, n, bases, err0 = run(1 << 16, 1 << 24)
    assert n > 20 and not err0.any()
    key = lambda c: (int(c["gap"]), int(c["k"]), int(c["kv"]))
    full = collections.Counter((key(ctg0[i]), _text(ctg0, seq0, i), int(ctg0[i]["n_nodes"]), int(ctg0[i]["cov_sum"])) for i in range(n))
    assert sum(full.values()) == n and sum(len(t) for (_, t, _, _) in full.elements()) == bases
    for cc, sc, what in ((n // 2, 1 << 24, "contig_cap n/2"), (1 << 16, bases // 2, "seq_cap bases/2"), (1 << 16, bases, "seq_cap exact"),
                         (1 << 16, bases - 1, "seq_cap exact - 1"), (n, bases, "both exact")):
        ctg, seq, n1, b1, err = run(cc, sc)
        assert (n1, b1) == (n, bases), what                         # the counters count what did not fit
        assert (err == err0).all(), what
        left = full.copy()
        tomb = 0
        for i in range(min(n, cc)):
            c = ctg[i]
            assert int(c["gap"]) != CANARY_GAP, (what, i)            # every record below the cap is written
            if int(c["length"]) == 0:
                assert int(c["seq_off"]) == 0, (what, i)
                tomb += 1
                continue
            assert int(c["seq_off"]) + int(c["length"]) <= sc, (what, i)
            t = (key(c), _text(ctg, seq, i), int(c["n_nodes"]), int(c["cov_sum"]))
            assert left[t] > 0, (what, i, t[0])
            left[t] -= 1
        if sc >= bases:
            assert tomb == 0, what                                   # everything fits: no tombstone
        if cc >= n and sc >= bases:
            assert not +left, what                                   # ... and every contig is there
        if sc < bases:
            assert tomb > 0, what
        # nothing beyond either cap
        assert (ctg[min(n, cc):]["gap"] == CANARY_GAP).all() and ctg[cc:].tobytes() == _canary_records(len(ctg) - cc).tobytes(), what
        assert seq[sc:] == b"\x5a" * (len(seq) - sc), what


# ---- B. the consumers: hand-built lists with tombstones, records beyond the cap and (from-variants) records before *first -----------

def _closing(rng, l, r):
    """A contig that would close the gap (both flanks whole around an insert) if a consumer read it."""
    return l + PK.rand_seq(rng, int(rng.integers(20, 200))) + r


def _dirty_list(cases, rng, pairs, n_before, n_past):
    """[(gap, k, kv, bases, kind)]: n_before closing decoys, the cases' contigs with tombstones mixed in, n_past closing decoys.
    kind: 'ok' | 'tomb' | 'decoy'.  Returns the list and the cap (= end of the middle part)."""
    mid = [(g, *pairs[int(rng.integers(0, len(pairs)))], s, "ok") for g, (_, _, seqs) in enumerate(cases) for s in seqs]
    mid += [(int(rng.integers(0, len(cases))), *pairs[int(rng.integers(0, len(pairs)))], "", "tomb") for _ in range(len(mid) // 3)]
    mid = [mid[i] for i in rng.permutation(len(mid))]
    dec = lambda: [(g, *pairs[0], _closing(rng, cases[g][0], cases[g][1]), "decoy") for g in rng.integers(0, len(cases), 1)]
    before = [x for _ in range(n_before) for x in dec()]
    past = [x for _ in range(n_past) for x in dec()]
    lst = before + mid + past
    return lst, len(before) + len(mid)


def _upload(lst):
    """Device records + bases; a tombstone is length 0, seq_off 0 (its n_nodes / cov_sum left as the assembly leaves them)."""
    from gappadder_amd import _lib as B
    ctg = np.zeros(len(lst), dtype=B.CONTIG)
    o = 0
    for i, (g, k, kv, s, kind) in enumerate(lst):
        if kind == "tomb":
            ctg[i] = (g, k, kv, 7, 0, 3, 0, 0)
        else:
            ctg[i] = (g, k, kv, max(1, len(s) - 28), len(s), 0, 0, o)
            o += len(s)
    blob = np.frombuffer("".join(x[3] for x in lst).encode() + b"\0" * 64, dtype=np.uint8)
    return _dev(ctg.view(np.uint8)), _dev(blob)


def _gaps(gf, cases):
    from gappadder_amd import _lib as B
    gaps = np.zeros(len(cases), dtype=B.GAP)
    for g in range(len(cases)):
        gaps[g] = (0, 2000 * (g + 1), 2000 * (g + 1) + 100, g + 1)
    gf.set_gaps(gaps, 1, [(l, r) for l, r, _ in cases])


def _exact_twin(cases, lst, first):
    """gf_pick_anchored2_dev's words from pick_contigs.pick_gap_sequence over the valid records (index >= first), scores 30 then 15."""
    from gappadder_amd.pick_contigs import pick_gap_sequence
    best = np.zeros(len(cases), dtype=np.uint64)
    for g, (l, r, _) in enumerate(cases):
        idx = [i for i, x in enumerate(lst) if x[0] == g and x[4] == "ok" and i >= first]
        mine = [("%d" % i, lst[i][3]) for i in idx]
        for a in (30, 15):
            res = pick_gap_sequence(mine, l, r, a, "exact")
            if res is not None:
                ci = int(res[0])
                rev = int(res[2] != lst[ci][3])
                best[g] = (a << 56) | (len(res[1]) << 32) | ((0x7FFFFFFF - ci) << 1) | rev
                break
    return best


@pytest.mark.parametrize("mode", ["exact", "align"])
@pytest.mark.parametrize("from_", [False, True])
def test_picks_read_only_the_valid_records_below_the_cap(gf, mode, from_):
    import torch
    from gappadder_amd import _lib as B
    from test_gpu_pick_align import _host_expect
    rng = np.random.default_rng(41 + from_)
    cases = PK.picker_cases(40 + from_, 160)
    _gaps(gf, cases)
    lst, cap = _dirty_list(cases, rng, [(31, 29)], 40 if from_ else 0, 40)
    first = 40 if from_ else 0
    n = len(lst)
    assert n > cap > first
    d_ctg, d_seq = _upload(lst)
    d_n = torch.tensor([n, first], dtype=torch.int32, device="cuda")
    d_best = torch.zeros(len(cases), dtype=torch.int64, device="cuda")
    d_closed = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = B.lib()
    fp = d_n.data_ptr() + 4
    if mode == "exact":
        want = _exact_twin(cases, lst, first)
        if from_:
            rc = lib.gf_pick_anchored2_from_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), cap, d_seq.data_ptr(), 30, 15, fp, d_best.data_ptr(),
                                                d_closed.data_ptr())
        else:
            rc = lib.gf_pick_anchored2_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), cap, d_seq.data_ptr(), 30, 15, d_best.data_ptr(),
                                           d_closed.data_ptr())
        assert rc == 0
    else:
        valid = [(x[0], x[3]) if x[4] == "ok" else (-1, "") for x in lst]
        want, picks_w, _ = _host_expect(cases, valid, first, (30, 15))
        d_pick = torch.zeros(cap * B.CTG_PICK.itemsize, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(2, dtype=torch.int32, device="cuda")
        args = (d_best.data_ptr(), d_closed.data_ptr(), d_pick.data_ptr(), d_st.data_ptr())
        if from_:
            rc = lib.gf_pick_aligned_from_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), cap, d_seq.data_ptr(), 30, 15, fp, *args)
        else:
            rc = lib.gf_pick_aligned_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), cap, d_seq.data_ptr(), 30, 15, *args)
        assert rc == 0
    gf.sync()
    best = d_best.cpu().numpy().view(np.uint64)
    n_want = int((want != 0).sum())
    assert 30 < n_want < len(cases)
    assert any(want[int(x[0])] == 0 for x in lst if x[4] == "decoy")     # a decoy, if it were read, would close an open gap
    bad = [g for g in range(len(cases)) if int(best[g]) != int(want[g])]
    assert not bad, (mode, from_, [(g, hex(int(best[g])), hex(int(want[g]))) for g in bad[:5]])
    assert int(d_closed[0]) == n_want
    if mode == "align":
        pk = np.frombuffer(d_pick.cpu().numpy().tobytes(), dtype=B.CTG_PICK)
        got = {i: (int(p["lp"]), int(p["rp"]), int(p["lm"]), int(p["rm"]), int(p["reverse"]), int(p["threshold"])) for i, p in enumerate(pk)
               if p["threshold"]}
        assert got == picks_w


@pytest.mark.parametrize("mode", ["exact", "align"])
def test_extended_fill_reads_only_the_valid_records_below_the_cap(gf, mode):
    import torch
    from gappadder_amd import _lib as B
    from test_gpu_extended_fill import _decode_all, _hand_cases, _random_cases, twin_expect
    rng = np.random.default_rng(43)
    cases = PK.picker_cases(44, 120) + _hand_cases() + _random_cases(45, 200)
    _gaps(gf, cases)
    lst, cap = _dirty_list(cases, rng, KK + [(0, 0)], 30, 30)
    first = 30
    n = len(lst)
    d_ctg, d_seq = _upload(lst)
    d_n = torch.tensor([n, first], dtype=torch.int32, device="cuda")
    best = np.zeros(len(cases), dtype=np.uint64)
    best[rng.choice(len(cases), len(cases) // 10, replace=False)] = 1 << 56
    d_best = _dev(best.view(np.int64))
    open_gaps = [g for g in range(len(cases)) if not best[g]]
    twin = [(x[0], x[1], x[2], x[3]) if x[4] == "ok" else (-1, x[1], x[2], x[3]) for x in lst]
    want = twin_expect([(l, r) for l, r, _ in cases], twin, KK, mode, open_gaps, first)
    assert sum(w[2] is not None for w in want.values()) > 100
    total = sum(len(w[2]) for w in want.values() if w[2] is not None)
    d_ext = torch.full((len(cases) * B.EXT_PICK.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    d_bases = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(B.EXT_WORDS, dtype=torch.int32, device="cuda")
    k_arr, kv_arr = np.array([a for a, _ in KK], dtype=np.int32), np.array([b for _, b in KK], dtype=np.int32)
    fn = B.lib().gf_pick_extended_aligned_dev if mode == "align" else B.lib().gf_pick_extended_dev
    assert fn(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), cap, d_seq.data_ptr(), 15, B._p(k_arr), B._p(kv_arr), len(KK), d_n.data_ptr() + 4,
              d_best.data_ptr(), d_ext.data_ptr(), d_bases.data_ptr(), total + 64, d_st.data_ptr()) == 0
    gf.sync()
    ext = np.frombuffer(d_ext.cpu().numpy().tobytes(), dtype=B.EXT_PICK)
    got = _decode_all(ext, d_bases.cpu().numpy().tobytes(), twin)
    bad = sorted(g for g in set(got) | set(want) if got.get(g) != want.get(g))
    assert not bad, (mode, [(g, got.get(g), want.get(g)) for g in bad[:3]])
    st = d_st.cpu().numpy().view(np.uint32)
    assert int(st[B.EXT_BASES]) + (int(st[B.EXT_BASES + 1]) << 32) == total and int(st[B.EXT_OVERFLOW]) == 0


# ---- the merge round --------------------------------------------------------------------------------------------------------------

def _merge_sets(rng, n_sets):
    lut = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda n: lut[rng.integers(0, 4, n)].tobytes().decode()
    sets = []
    for s in range(n_sets):
        g = rnd(int(rng.integers(600, 2500)))
        cs, at = [], 0
        while at < len(g) - 80:
            ln = int(rng.integers(80, 600))
            c = g[at:at + ln]
            cs.append(PK._rc(c) if rng.integers(0, 2) else c)
            at += max(20, ln - int(rng.integers(15, 120)))
        if rng.integers(0, 3) == 0:
            cs.append(rnd(200))
        sets.append([cs[i] for i in rng.permutation(len(cs))])
    return sets


def _merge_call(gf, recs, seq, n_gaps, n, contig_cap, seq_len, seq_cap, open_gaps, extra=2048):
    """gf_merge_open_gaps_dev on a hand-built list (buffers `extra` records / bases beyond the caps, canaries there); returns the stats,
    the counters and the whole buffers."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    ctg = _canary_records(contig_cap + extra)
    ctg[:len(recs)] = recs
    d_ctg = _dev(ctg.view(np.uint8))
    buf = np.full(seq_cap + 4096, 0x5A, dtype=np.uint8)
    buf[:len(seq)] = np.frombuffer(seq, dtype=np.uint8)
    d_seq = _dev(buf)
    cnt = np.zeros(4, dtype=np.uint32)
    cnt[0] = n
    cnt[2:4] = np.array([seq_len], dtype=np.uint64).view(np.uint32)
    d_cnt = _dev(cnt.view(np.int32))
    best = np.array([0 if o else 1 for o in open_gaps], dtype=np.uint64)
    d_best = _dev(best.view(np.int64))
    d_st = torch.full((B.MG_WORDS,), 7, dtype=torch.int32, device="cuda")
    pr = np.zeros(1, dtype=B.OVL_PARAMS)
    pr[0] = tuple(GapFill.MERGER_PARAMS)[:7] + (0.0,)
    assert B.lib().gf_merge_open_gaps_dev(gf.handle, d_ctg.data_ptr(), d_cnt.data_ptr(), contig_cap, d_seq.data_ptr(), d_cnt.data_ptr() + 8,
                                          seq_cap, d_best.data_ptr(), n_gaps, B._p(pr), 10, 128, None, None, 0, d_st.data_ptr()) == 0
    gf.sync()
    c = d_cnt.cpu().numpy().view(np.uint32)
    return (d_st.cpu().numpy().view(np.uint32), int(c[0]), int(c[2:4].view(np.uint64)[0]),
            np.frombuffer(d_ctg.cpu().numpy().tobytes(), dtype=B.CONTIG), d_seq.cpu().numpy().tobytes())


def _records(sets, tombs, rng):
    """Records of the sets in set order, with `tombs` tombstones of random gaps mixed in (their relative order kept)."""
    from gappadder_amd import _lib as B
    out = [(g, c) for g, cs in enumerate(sets) for c in cs]
    for _ in range(tombs):
        out.insert(int(rng.integers(0, len(out) + 1)), (int(rng.integers(0, len(sets))), None))
    recs = np.zeros(len(out), dtype=B.CONTIG)
    o = 0
    for i, (g, c) in enumerate(out):
        if c is None:
            recs[i] = (g, 31, 29, 5, 0, 9, 0, 0)
        else:
            recs[i] = (g, 31, 29, max(1, len(c) - 28), len(c), 0, 0, o)
            o += len(c)
    return recs, "".join(c for _, c in out if c is not None).encode()


def _merged(st, n1, ctg, seq, n_sets):
    n0 = int(st[7])
    out = [[] for _ in range(n_sets)]
    for i in range(n0, n1):
        out[int(ctg[i]["gap"])].append(_text(ctg, seq, i))
    return out


def test_merge_round_skips_tombstones(gf):
    from test_gpu_merge import _oracle_round
    from gappadder_amd import _lib as B
    rng = np.random.default_rng(51)
    sets = _merge_sets(rng, 40)
    open_gaps = [s % 9 != 4 for s in range(len(sets))]
    res = {}
    for tombs in (0, 60):
        recs, seq = _records(sets, tombs, rng)
        cap, scap = len(recs) + 4096, len(seq) + (1 << 20)
        st, n1, s1, ctg, sq = _merge_call(gf, recs, seq, len(sets), len(recs), cap, len(seq), scap, open_gaps)
        assert int(st[B.MG_ERR]) == 0 and int(st[B.MG_N0]) == len(recs)
        assert ctg[:len(recs)].tobytes() == recs.tobytes()                  # the list before the round is left as it was
        assert (ctg[n1:]["gap"] == CANARY_GAP).all() and sq[scap:] == b"\x5a" * (len(sq) - scap)
        res[tombs] = (st, _merged(st, n1, ctg, sq, len(sets)))
    (st0, m0), (st1, m1) = res[0], res[60]
    assert m1 == m0
    skip = {B.MG_N0, 10, 11, 13, 14}          # the first merged index, and the workgroups' queue cursors
    assert [int(x) for i, x in enumerate(st1) if i not in skip] == [int(x) for i, x in enumerate(st0) if i not in skip]
    want = _oracle_round(sets)
    n_new = 0
    for g in range(len(sets)):
        assert m0[g] == (want[g] if open_gaps[g] else []), g
        n_new += len(m0[g])
    assert n_new > 20


@pytest.mark.parametrize("over", ["contigs", "bases"])
def test_merge_round_handed_an_overflowed_list_is_a_no_op_that_keeps_it_visible(gf, over):
    from gappadder_amd import _lib as B
    rng = np.random.default_rng(52)
    sets = _merge_sets(rng, 30)
    recs, seq = _records(sets, 10, rng)
    cap, scap = len(recs) + 4096, len(seq) + (1 << 20)
    st_ok, n_ok, _, _, _ = _merge_call(gf, recs, seq, len(sets), len(recs), cap, len(seq), scap, [True] * len(sets))
    assert n_ok > len(recs) and int(st_ok[B.MG_ERR]) == 0                  # the same list within its caps: merged contigs appended
    if over == "contigs":
        cap = len(recs) - 5                        # the assembly counted 5 records beyond the cap (its last ones, not written)
        n_in, s_in, flag = len(recs), len(seq), 32
    else:
        scap = len(seq) - 1
        n_in, s_in, flag = len(recs), len(seq) + 300, 64       # bases beyond the cap (tombstones in the list)
    st, n1, s1, ctg, sq = _merge_call(gf, recs, seq, len(sets), n_in, cap, s_in, scap, [True] * len(sets))
    assert int(st[B.MG_ERR]) & flag, hex(int(st[B.MG_ERR]))
    assert (n1, s1) == (n_in, s_in)                                         # the overflow stays visible to fetch()
    assert int(st[B.MG_N_JOBS]) == 0 and int(st[B.MG_N_SETS]) == 0
    assert ctg[:len(recs)].tobytes() == recs[:len(recs)].tobytes()         # nothing appended, nothing rewritten
    assert (ctg[len(recs):]["gap"] == CANARY_GAP).all()
    assert sq[len(seq):] == b"\x5a" * (len(sq) - len(seq))


# ---- round 2: the contig k-mer table and the recruitment at the 32 / 64 boundaries --------------------------------------------------

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _canon(s):
    """Left-aligned 128-bit canonical k-mer (A0 C1 G2 T3) as (hi, lo)."""
    c = min(s, PK._rc(s))
    v = 0
    for j, ch in enumerate(c):
        v |= _CODE[ch] << (126 - 2 * j)
    return v >> 64, v & ((1 << 64) - 1)


def _kmers(s, k):
    for p in range(len(s) - k + 1):
        w = s[p:p + k]
        if all(ch in _CODE for ch in w):
            yield _canon(w)


def _r2_list(rng, n_gaps):
    """Per gap 1-3 contigs of 40-300 bases with the odd N; their texts; a list with tombstones, and decoys beyond the cap."""
    contigs = []
    for g in range(n_gaps):
        for _ in range(int(rng.integers(1, 4))):
            s = PK.rand_seq(rng, int(rng.integers(40, 300)))
            if rng.integers(0, 4) == 0:
                q = int(rng.integers(0, len(s)))
                s = s[:q] + "N" + s[q + 1:]
            contigs.append((g, 31, 29, s, "ok"))
    contigs += [(int(rng.integers(0, n_gaps)), 31, 29, "", "tomb") for _ in range(len(contigs) // 4)]
    contigs = [contigs[i] for i in rng.permutation(len(contigs))]
    cap = len(contigs)
    contigs += [(int(rng.integers(0, n_gaps)), 31, 29, PK.rand_seq(rng, 200), "decoy") for _ in range(20)]
    return contigs, cap


def _r2_table(gf, lst, cap, best, n_gaps, k, log2):
    import torch
    from gappadder_amd import _lib as B
    d_ctg, d_seq = _upload(lst)
    d_n = torch.tensor([len(lst)], dtype=torch.int32, device="cuda")
    d_best = _dev(best.view(np.int64))
    d_tab = torch.empty((24 << log2,), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(B.R2_WORDS, dtype=torch.int32, device="cuda")
    assert B.lib().gf_contig_kmer_table_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), cap, d_seq.data_ptr(), d_best.data_ptr(), n_gaps, k,
                                            d_tab.data_ptr(), log2, d_st.data_ptr()) == 0
    gf.sync()
    return d_tab, d_st


def _table_entries(d_tab):
    slot = np.dtype([("hi", "<u8"), ("lo", "<u8"), ("gap", "<u4"), ("state", "<u4")])
    t = np.frombuffer(d_tab.cpu().numpy().tobytes(), dtype=slot)
    t = t[t["state"] == 2]
    return [(int(a), int(b), int(g)) for a, b, g in zip(t["hi"], t["lo"], t["gap"])]


@pytest.mark.parametrize("k", [16, 31, 32, 33, 63, 64])
def test_contig_kmer_table_and_recruitment_against_a_plain_reference(gf, k):
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    rng = np.random.default_rng(60 + k)
    n_gaps, log2 = 48, 16
    lst, cap = _r2_list(rng, n_gaps)
    best = np.zeros(n_gaps, dtype=np.uint64)
    best[::5] = 1 << 56                                                   # closed gaps: not in the table
    d_tab, d_st = _r2_table(gf, lst, cap, best, n_gaps, k, log2)
    want = collections.defaultdict(set)
    for g, _, _, s, kind in lst[:cap]:
        if kind == "ok" and not best[g]:
            for km in _kmers(s, k):
                want[km].add(g)
    got = _table_entries(d_tab)
    assert len(got) == len(set(got))
    assert set(got) == {(hi, lo, g) for (hi, lo), gs in want.items() for g in gs}
    st = d_st.cpu().numpy().view(np.uint32)
    assert int(st[B.R2_TAB_FULL]) == 0 and len(got) > 1000
    # reads: pieces of the contigs (every gap, either strand, shifted) and strangers, with N-masked runs
    L = 100
    texts = [x for x in lst if x[4] != "tomb"]
    reads = []
    for i in range(1200):
        if i % 4 == 3:
            r = PK.rand_seq(rng, L)
        else:
            g, _, _, s, _ = texts[int(rng.integers(0, len(texts)))]
            a = int(rng.integers(0, max(1, len(s) - k)))
            r = (s[a:] + PK.rand_seq(rng, L))[:L]
            if rng.integers(0, 2):
                r = PK._rc(r)
        for _ in range(int(rng.integers(0, 3))):                          # an N-masked run
            p, w = int(rng.integers(0, L)), int(rng.integers(1, 6))
            r = (r[:p] + "N" * w + r[p + w:])[:L]
        reads.append(r)
    packed, nm = GapFill.pack_reads("".join(reads).encode(), L, with_mask=True)
    n_pairs = len(reads) // 2
    pairs = np.arange(n_pairs, dtype=np.uint32)[::-1].copy()
    d_reads, d_nm = _dev(packed.reshape(-1)), _dev(nm.reshape(-1).view(np.int32))
    d_pairs, d_np = _dev(pairs.view(np.int32)), torch.tensor([n_pairs], dtype=torch.int32, device="cuda")
    key_cap = 1 << 16
    d_keys = torch.full((key_cap,), -1, dtype=torch.int64, device="cuda")
    assert B.lib().gf_recruit_by_contigs_dev(gf.handle, d_reads.data_ptr(), d_nm.data_ptr(), len(reads), L, d_pairs.data_ptr(), d_np.data_ptr(),
                                             n_pairs, 3, k, d_tab.data_ptr(), log2, d_keys.data_ptr(), key_cap, d_st.data_ptr()) == 0
    gf.sync()
    st = d_st.cpu().numpy().view(np.uint32)
    assert int(st[B.R2_HITS]) <= key_cap
    keys = d_keys.cpu().numpy().view(np.uint64)
    keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    assert ((keys >> np.uint64(36)) & np.uint64(15) == 3).all()
    got_r = {(int(x) >> 40, int(x) & ((1 << 36) - 1)) for x in keys}
    want_r = set()
    for i, r in enumerate(reads):
        for km in _kmers(r, k):
            for g in want.get(km, ()):
                want_r.add((g, i // 2))
    assert got_r == want_r
    assert len(want_r) > 150


# ---- C. the pipeline: an overflowing step raises, and the next one is clean ---------------------------------------------------------

LAYOUTS = {"mixed550_k31": (550, [(31, 29)]), "mixed450_k51_61": (450, [(51, 49), (61, 59)])}
FEATURES = {"default": {}, "merge_in_step": {"merge_in_step": True}, "second_round": {"second_round": True},
            "extended_fill": {"extended_fill": True}}


@pytest.fixture(scope="module", params=sorted(LAYOUTS))
def layout(request):
    return _setup(*LAYOUTS[request.param])


def _summary(pipe, res):
    per_gap = collections.Counter((int(c["gap"]), int(c["k"]), int(c["kv"]), _text(res.contigs, res.seq, i)) for i, c in enumerate(res.contigs))
    out = {"n": (res.n_contigs, res.n_seq, res.n_closed), "contigs": per_gap, "picks": _picks(res), "merge": res.merge, "round2": res.round2}
    if res.ext is not None:
        out["ext"] = {g: (_text(res.contigs, res.seq, v[0]) if v[0] >= 0 else None, _text(res.contigs, res.seq, v[1]) if v[1] >= 0 else None,
                          v[2], v[3]) for g, v in pipe.extended_sequences(res).items()}
    return out


@pytest.mark.parametrize("mode", ["exact", "align"])
@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_a_step_beyond_its_caps_raises_and_the_next_is_clean(layout, feature, mode):
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    gf, cfg, gaps, flanks, d_reads, d_recs, kk = layout
    pipe = Pipeline(gf, len(gaps), L, kk, anchor_mode=mode, **FEATURES[feature])
    pipe.add_library(DeviceLibrary("x", 300, 30, 2 * N_PAIRS, d_reads, d_recs))
    pipe.prepare()
    caps = (pipe.contig_cap, pipe.seq_cap)
    pipe.step()
    want = _summary(pipe, pipe.fetch())
    n, bases = want["n"][:2]
    assert n > 0 and bases > 0 and n < caps[0] and bases < caps[1]
    if feature == "merge_in_step":
        assert want["merge"]["gaps_tried"] > 0
    for cc, sc, what in ((n, caps[1], "contig_cap exact"), (caps[0], bases, "seq_cap exact"), (n, bases, "both exact")):
        pipe.contig_cap, pipe.seq_cap = cc, sc
        pipe.step()
        assert _summary(pipe, pipe.fetch()) == want, what
    for cc, sc, what in ((n - 1, caps[1], "contig_cap - 1"), (caps[0], bases - 1, "seq_cap - 1"), (n - 1, bases - 1, "both - 1")):
        pipe.contig_cap, pipe.seq_cap = cc, sc
        pipe.step()
        with pytest.raises(RuntimeError):
            pipe.fetch()
        pipe.contig_cap, pipe.seq_cap = caps
        pipe.step()
        assert _summary(pipe, pipe.fetch()) == want, what
