"""The anchored pair span (gf_fill_pairs_anchored_dev, csrc/fill_anchor.hip) behind gf_fill_pairs_dev through the C ABI against its host
twin (gappadder_amd/pair_anchors.py) — records and statistics equal — on the hand-built contig lists and per-library pools of
test_gpu_pair_span.py (pool slices of 256, 257 and about 700 rows, contigs of 8 192 and 8 193 bases and one with an N, an open gap, a
mismatch gap, tombstones; L = 150, and L = 100 with N masks; exact anchors and the pick table; two libraries into two planes, sharing the
scratch and the anchor arrays), with alignment records and tagger hits built on top: for about three rows in four the mate is anchored in
a flank, where the row's placement allows it at a draft coordinate that gives an insert of the (mate-pair) library, otherwise anywhere within 700
bases of the gap; duplicates, clipped, secondary, supplementary and unmapped records, records without a read, anchors inside the gap,
to_mate = 0, other kinds, targets that are in no slice, hits of the open and the mismatch gap; the hit list shuffled twice; a hit counter
above the capacity; no hits; no closed gap; the parameter refusals."""
import numpy as np
import pytest

import test_gpu_pair_span as T

pytestmark = pytest.mark.gpu

MIN_PAIRS = (3, 8)          # per library
# (is_mean, is_sd, z) of the anchored calls: mate-pair inserts, longer than most of the contigs — gf_fill_pairs_dev keeps T.LIBS, its own
ALIBS = [(1500, 100, 3), (2500, 200, 2)]
_HITS = {}


def _gap_table(n_gaps):
    from gappadder_amd import _lib as B
    gp = np.zeros(n_gaps, dtype=B.GAP)
    for g in range(n_gaps):
        gp[g] = (0, 20000 * (g + 1), 20000 * (g + 1) + 100, g + 1)
    return gp


def _body_of(case, g, style):
    """(b0, b1) of gap g or None (open, mismatch): what locate answers, checked by test_gpu_pair_span's twin."""
    e = case["expect"][g]
    return None if e in (None, "mismatch") else e


def _hits(case, L, masked, style):
    """Per library (records, hits) (cached): see the module docstring.  The rows' placements — from the pair-span twin — only steer where
    the anchors are planted."""
    key = (id(case), L)
    if key in _HITS:
        return _HITS[key]
    from gappadder_amd import _lib as B
    _, _, where = T._twin(case, L, masked, style, 16)
    gaps = case["gaps"]
    gp = _gap_table(len(gaps))
    rng = np.random.default_rng(77 + L)
    out = []
    for l, (mean, sd, _) in enumerate(ALIBS):
        recs, hits = [], []

        def add(g, pos, flag, clip, read, kind=None, to_mate=1):
            recs.append((pos, 0, 0, 0, 0, flag, 60, clip, read))
            hits.append((len(recs) - 1, g, int(rng.integers(1, 3)) if kind is None else kind, to_mate))

        for g, G in enumerate(gaps):
            start, end = int(gp[g]["start"]), int(gp[g]["end"])
            body, rev = _body_of(case, g, style), int(G["rev"])
            ids = G["pools"][l][0]
            for i, r in enumerate(ids):
                if rng.random() < 0.25:
                    continue
                rows = where.get((l, g), []) if body is not None else []        # (empty for a contig the rounds skip)
                w = rows[i] if rows else None
                A0 = sA = None
                if w not in (None, "ambiguous") and rng.random() < 0.85:
                    ins = int(np.rint(rng.normal(mean, sd)))
                    str_a = 1 - w[0]
                    col = w[1] + L - ins if w[0] else w[1] + ins - L           # the anchor's column for an insert of `ins`
                    sA = 1 - str_a if rev else str_a
                    for A0 in ((start - (body[0] - col), end + (col - body[1])) if not rev else
                               (start - (col + L - body[1]), end + (body[0] - col - L))):
                        if 0 <= A0 < start or A0 >= end:
                            break
                    else:
                        A0 = None
                if A0 is None:
                    A0, sA = int(rng.choice([start - int(rng.integers(1, 700)), end + int(rng.integers(0, 700))])), int(rng.integers(0, 2))
                add(g, A0 + 1, 0x10 * sA | 0x1, 0, r ^ 1)
                x = rng.integers(0, 40)
                if x == 0:
                    add(g, A0 + 1 - int(rng.integers(1, 50)), 0x10 * int(rng.integers(0, 2)), 0, r ^ 1)       # a second record of the read: the smaller wins
                elif x == 1:
                    add(g, A0 + 1, 0x10 * (1 - sA), 0, r ^ 1)                                                 # the same base, the other strand
                elif x == 2:
                    add(g, max(1, A0 - 3), 0, int(rng.integers(1, 4)), r ^ 1)                                 # clipped
                elif x == 3:
                    add(g, max(1, A0 - 3), int(rng.choice([0x100, 0x800, 0x900])), 0, r ^ 1)                  # secondary / supplementary
                elif x == 4:
                    add(g, max(1, A0 - 3), 0x4, 0, r ^ 1)                                                     # unmapped
                elif x == 5:
                    add(g, start + 1 + int(rng.integers(0, 100)), 0, 0, r ^ 1)                                # inside the gap
                elif x == 6:
                    add(g, max(1, A0 - 3), 0, 0, r ^ 1, to_mate=0)
                elif x == 7:
                    add(g, max(1, A0 - 3), 0, 0, r ^ 1, kind=int(rng.choice([B.KIND_CLIP, B.KIND_LOWMAPQ])))
                elif x == 8:
                    add(g, max(1, A0 - 3), 0, 0, 0xFFFFFFFF)                                                  # no read
                elif x == 9:
                    add(g, max(1, A0 - 3), 0, 0, 2 * 30000 + int(rng.integers(0, 1000)))                      # a target in no slice
                elif x == 10:
                    add((g + 1) % len(gaps), 20000 * ((g + 1) % len(gaps) + 1) - 5, 0, 0, r ^ 1)              # ... or in another gap's
            add(g, start, 0, 0, 2 * 40000 + 1)                                                                # A0 = start - 1: left; absent
        out.append((np.array(recs, dtype=B.ALNREC), np.array(hits, dtype=B.TAGHIT)))
    _HITS[key] = out
    return out


def _twin(case, L, masked, style, hits, caps):
    from gappadder_amd import _lib as B
    from gappadder_amd import pair_anchors as PA
    _, _, where = T._twin(case, L, masked, style, 16)
    gaps = case["gaps"]
    gp = _gap_table(len(gaps))
    want = np.zeros((len(T.LIBS), len(gaps)), dtype=B.FILL_ANCHORS)
    stats = [dict.fromkeys(PA.STAT_KEYS, 0) for _ in T.LIBS]
    for l, (mean, sd, z) in enumerate(ALIBS):
        off = np.cumsum([0] + [len(G["pools"][l][0]) for G in gaps])
        ids = np.array([r for G in gaps for r in G["pools"][l][0]], dtype=np.uint32)
        at, hs = PA.scatter_host(hits[l][1], hits[l][0], gp, off, ids, caps[l])
        stats[l].update(hs)
        for g, G in enumerate(gaps):
            if not case["words"][g]:
                continue
            body = _body_of(case, g, style)
            if body is None:
                stats[l]["mismatches"] += 1
                continue
            pids, reads = G["pools"][l]
            reads = reads if masked else [r.replace("N", "A") for r in reads]
            want[l, g] = PA.anchors_host(reads, pids, [at.get(i) for i in range(off[g], off[g + 1])], G["stored"], body[0], body[1], int(G["rev"]),
                                         (int(gp[g]["start"]), int(gp[g]["end"])), mean, sd, *T._params(16, L), z=z, min_pairs=MIN_PAIRS[l], L=L,
                                         where=where[l, g])
            PA.add_to_stats(stats[l], want[l, g])
    return want, stats


def _run_device(case, L, masked, style, hits, caps, counts, words=None):
    """gf_fill_pairs_dev, then gf_fill_pairs_anchored_dev, per library; the scratch and the anchor array are shared.  caps, counts: per
    library the capacity of the hit list and what the counter says."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    gaps, recs = case["gaps"], case["recs"]
    n_gaps, n = len(gaps), len(recs)
    gf = GapFill(0)
    gf.set_gaps(_gap_table(n_gaps), 1, [G["flanks"] for G in gaps])
    ctg = np.zeros(n, dtype=B.CONTIG)
    o = 0
    for i, (g, s) in enumerate(recs):
        ctg[i] = (g, 31, 29, 1, len(s), 0, 0, o) if s is not None else (g, 31, 29, 3, 0, 5, 0, 0)
        o += len(s or "")
    seq = "".join(s or "" for _, s in recs).encode()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_ctg, d_seq = dev(ctg.view(np.uint8)), dev(np.frombuffer(seq, dtype=np.uint8))
    d_n = torch.tensor([n + 3], dtype=torch.int32, device="cuda")
    d_best = dev(np.array(case["words"] if words is None else words, dtype=np.uint64).view(np.int64))
    d_pick = None
    if style == "pick":
        pk = np.zeros(n, dtype=B.CTG_PICK)
        for ci, p in case["picks"].items():
            pk[ci] = p
        d_pick = dev(pk.view(np.uint8))
    shared = (d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), d_best.data_ptr(), d_pick.data_ptr() if d_pick is not None else None,
              T.A_LONG, T.A_SHORT)
    plane = n_gaps * B.FILL_ANCHORS.itemsize
    most = max(sum(len(G["pools"][l][0]) for G in gaps) for l in range(len(T.LIBS)))
    d_out = torch.full((len(T.LIBS) * plane,), 0x55, dtype=torch.uint8, device="cuda")
    d_pairs = torch.zeros(n_gaps * B.FILL_PAIRS.itemsize, dtype=torch.uint8, device="cuda")
    d_scr = torch.full((most + 4,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    d_anc = torch.full((most + 4,), 0x1234, dtype=torch.int64, device="cuda")
    stats = []
    for l, (mean, sd, z) in enumerate(T.LIBS):
        reads = [r for G in gaps for r in G["pools"][l][1]]
        ids = np.array([r for G in gaps for r in G["pools"][l][0]], dtype=np.uint32)
        off = np.cumsum([0] + [len(G["pools"][l][0]) for G in gaps]).astype(np.uint64)
        packed, nm = GapFill.pack_reads(reads, L, with_mask=True)
        d_pool = dev(np.concatenate([packed.reshape(-1), np.zeros(64, dtype=np.uint8)]))
        d_nm = dev(nm.view(np.int32)) if masked else None
        d_off, d_ids = dev(off.view(np.int64)), dev(np.concatenate([ids, np.zeros(4, dtype=np.uint32)]).view(np.int32))
        rc_, hh = hits[l]
        d_recs = dev(np.concatenate([rc_, np.zeros(1, dtype=B.ALNREC)]).view(np.uint8))
        d_hits = dev(np.concatenate([hh[:caps[l]], np.zeros(1, dtype=B.TAGHIT)]).view(np.uint8))       # nothing beyond the capacity exists
        d_cnt = torch.tensor([counts[l]], dtype=torch.int32, device="cuda")
        d_ps = torch.zeros(B.PS_WORDS, dtype=torch.int32, device="cuda")
        d_st = torch.full((B.PA_WORDS,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = B.lib().gf_fill_pairs_dev(gf.handle, d_pool.data_ptr(), d_nm.data_ptr() if masked else None, d_off.data_ptr(), d_ids.data_ptr(),
                                       len(reads), L, *shared, *T._params(16, L), mean, sd, z, d_scr.data_ptr(), d_pairs.data_ptr(), d_ps.data_ptr())
        assert rc == 0, (rc, B.lib().gf_last_error(gf.handle))
        rc = B.lib().gf_fill_pairs_anchored_dev(gf.handle, d_off.data_ptr(), d_ids.data_ptr(), len(reads), L, *shared, d_scr.data_ptr(),
                                                d_recs.data_ptr(), len(rc_), d_hits.data_ptr(), d_cnt.data_ptr(), caps[l], *ALIBS[l], MIN_PAIRS[l],
                                                d_anc.data_ptr(), d_out.data_ptr() + l * plane, d_st.data_ptr())
        assert rc == 0, (rc, B.lib().gf_last_error(gf.handle))
        gf.sync()
        assert int(d_anc[len(reads)]) == 0x1234 or len(reads) < most              # nothing beyond the pool's rows
        stats.append(d_st.cpu().numpy())
    assert int(d_anc[most]) == 0x1234 and int(d_scr[most]) == 0x7F7F7F7F
    return np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.FILL_ANCHORS).reshape(len(T.LIBS), n_gaps), stats


def _same(got, st, want, stats, case):
    from gappadder_amd import pair_anchors as PA
    for l in range(len(T.LIBS)):
        print("library %d: %s" % (l, PA.stats_of(st[l])))
        assert PA.stats_of(st[l]) == stats[l]
    bad = [(l, g) for l in range(len(T.LIBS)) for g in range(want.shape[1]) if got[l, g].tobytes() != want[l, g].tobytes()]
    assert not bad, [(l, g, case["gaps"][g]["kind"], got[l, g], want[l, g]) for l, g in bad[:4]]


def _cases_are_there(case, want, stats, hits, style):
    """What the cases are there for, from the twin alone."""
    from gappadder_amd import _lib as B
    by_kind = {}
    for g, G in enumerate(case["gaps"]):
        by_kind.setdefault(G["kind"], []).append(g)
    for f in ("n_placed", "n_misoriented", "n_in_range", "n_short", "n_long", "n_left", "n_span", "n_eval", "n_unspanned", "min_cover"):
        assert int(want[f].sum()) > 0, f
    for l in range(len(T.LIBS)):
        assert (want[l]["n_eval"] > 0).any() and (want[l]["n_anchored"] > want[l]["n_placed"]).any()
        assert (want[l]["n_in_range"] > want[l]["n_left"]).any() and (want[l]["n_left"] > 0).any()        # right and left anchors
        assert (want[l]["dev_min_sum"] < 0).any() and (want[l]["dev_max_sum"] > 0).any()
        for k in ("kept", "dropped_clipped", "dropped_in_gap", "dropped_secondary", "absent", "dropped_other"):
            assert stats[l][k] > 0, k
        assert stats[l]["mismatches"] == (1 if style == "exact" else 0)
    for kind, rows in (("rows256", 256), ("rows257", 257)):
        (g,) = by_kind[kind]
        assert int(want[0, g]["rows"]) == rows and int(want[0, g]["n_placed"]) > 100
    (g,) = by_kind["rows700"]
    assert int(want[0, g]["rows"]) > 612 and int(want[0, g]["n_in_range"]) > 200
    (g,) = by_kind["at_max"]
    assert int(want[0, g]["flags"]) == 0 and int(want[0, g]["n_placed"]) > 0
    (g,) = by_kind["over_max"]
    assert want[0, g].tobytes() == np.array((B.PS_F_LONG, int(want[0, g]["rows"])) + (0,) * 22, dtype=B.FILL_ANCHORS).tobytes() and int(want[0, g]["rows"]) > 0
    (g,) = by_kind["non_acgt"]
    assert int(want[1, g]["flags"]) == B.PS_F_NON_ACGT and int(want[1, g]["rows"]) > 0 and int(want[1, g]["n_anchored"]) == 0
    (g,) = by_kind["open"]
    assert not want[:, g].tobytes().strip(b"\0") and (hits[0][1]["gap"] == g).sum() > 5                    # an open gap that has hits


@pytest.mark.parametrize("style", ["exact", "pick"])
@pytest.mark.parametrize("L,masked", [(150, False), (100, True)])
def test_kernels_equal_the_twin(L, masked, style):
    case = T._build(L, masked, style, 9000 + L)
    hits = _hits(case, L, masked, style)
    caps = [len(h) for _, h in hits]
    want, stats = _twin(case, L, masked, style, hits, caps)
    _cases_are_there(case, want, stats, hits, style)
    got, st = _run_device(case, L, masked, style, hits, caps, caps)
    _same(got, st, want, stats, case)
    # two shuffles of the hit lists: the same bytes
    rng = np.random.default_rng(3)
    for _ in range(2):
        shuffled = [(r, h[rng.permutation(len(h))]) for r, h in hits]
        got2, st2 = _run_device(case, L, masked, style, shuffled, caps, caps)
        assert got2.tobytes() == got.tobytes() and all((a == b).all() for a, b in zip(st, st2))


def test_counter_above_the_capacity_no_hits_and_no_closed_gap():
    L, masked, style = 150, False, "exact"
    case = T._build(L, masked, style, 9000 + L)
    hits = _hits(case, L, masked, style)
    caps = [len(h) - 37 for _, h in hits]
    want, stats = _twin(case, L, masked, style, hits, caps)
    full, _ = _twin(case, L, masked, style, hits, [len(h) for _, h in hits])
    assert want.tobytes() != full.tobytes()
    got, st = _run_device(case, L, masked, style, hits, caps, [len(h) + 1000 for _, h in hits])
    _same(got, st, want, stats, case)
    # no hits: the counter says 0
    want, stats = _twin(case, L, masked, style, hits, [0, 0])
    assert int(want["n_anchored"].sum()) == 0 and int(want["rows"].sum()) > 0 and all(s["kept"] == 0 for s in stats)
    got, st = _run_device(case, L, masked, style, hits, [len(h) for _, h in hits], [0, 0])
    _same(got, st, want, stats, case)
    # no closed gap: every record is zero, only the hits are counted
    from gappadder_amd import pair_anchors as PA
    caps = [len(h) for _, h in hits]
    got, st = _run_device(case, L, masked, style, hits, caps, caps, words=[0] * len(case["gaps"]))
    assert not got.tobytes().strip(b"\0")
    _, stats = _twin(case, L, masked, style, hits, caps)
    for l in range(len(T.LIBS)):
        s = PA.stats_of(st[l])
        assert s["gaps"] == s["mismatches"] == s["anchored"] == 0 and {k: s[k] for k in PA.HIT_KEYS} == {k: stats[l][k] for k in PA.HIT_KEYS}


def test_arguments():
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    import torch
    gf = GapFill(0)
    gf.set_gaps(_gap_table(1), 1, [("A" * 100, "C" * 100)])
    lib = B.lib()
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = z.data_ptr()

    def args(sd=30, zz=3, mp=8, rows=0, ids=p, scr=p, anc=p, a_long=30, a_short=15, cap=0, hits=p):
        return (gf.handle, p, ids, rows, 150, p, p, 0, p, p, None, a_long, a_short, scr, p, 0, hits, p, cap, 400, sd, zz, mp, anc, p, p)

    assert lib.gf_fill_pairs_anchored_dev(*args()) == 0
    gf.sync()
    for kw in (dict(mp=0), dict(mp=-3), dict(zz=0), dict(sd=-1), dict(zz=3, sd=349526), dict(zz=1, sd=1 << 20), dict(zz=1 << 10, sd=1 << 10)):
        assert lib.gf_fill_pairs_anchored_dev(*args(**kw)) == B.GF_E_UNSUPPORTED, kw
    assert lib.gf_fill_pairs_anchored_dev(*args(zz=3, sd=349525)) == 0
    gf.sync()
    for kw in (dict(rows=8, ids=None), dict(rows=8, scr=None), dict(rows=8, anc=None), dict(cap=8, hits=None), dict(a_long=40),
               dict(a_long=30, a_short=30)):
        assert lib.gf_fill_pairs_anchored_dev(*args(**kw)) == B.GF_E_INVAL, kw
