"""The read-support kernel (gf_fill_support_dev, csrc/fill_support.hip) against its host twin (gappadder_amd/read_support.py) through the
C ABI, bit for bit, on hand-built pools and contig lists: pools of 0 / 1 / 64 / 300 rows; bodies of 0, 1, k - 1, k and 500 bases and
two long ones — three table chunks (1 024 windows each) with the longest zero run planted across the second chunk boundary of a
reverse pick, two chunks with it across the first of a forward pick; open gaps; a contig shorter
than k; a contig list at contig_cap with tombstones before winners; pick tables (the align and gapped modes) and re-located exact
anchors, both orientations, long and short anchor, repeated anchors, and a word whose span the contig does not carry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [16, 31, 32, 33, 51, 64]
POOLS = [0, 1, 64, 300]
A_LONG, A_SHORT, MIN_COUNT = 30, 15, 2
CHUNK = 1024        # fill_support.hip FS_CHUNK
INSERT = 40
# gap -> (body length, chunk boundary its planted zero run crosses): a foreign insert of INSERT bases that starts, in the STORED
# orientation of the contig, 18 body bases before window index boundary * CHUNK — its zero windows (insert + k - 1 of them: its end bases differ from
# the bases they replace) lie on both sides of the boundary, so the kernel's carry of the open run from one chunk
# into the next decides `zero_run`.  Gap 5 is a reverse pick (the insert position is mirrored), gap 20 a forward one.
LONG = {5: (2 * CHUNK + 150, 2), 20: (CHUNK + 150, 1)}


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4]


def _word(a, span, ci, rev):
    return (a << 56) | (min(span + 1, 0xFFFFFF) << 32) | ((0x7FFFFFFF - ci) << 1) | int(rev)


def _build(k, L, masked, style, seed):
    """One run's input.  Returns a dict: flanks, contig records [(gap, bases or None for a tombstone)], words, pick entries {contig: tuple},
    reads per gap, the constructed body per gap (None: open, "mismatch": the word lies)."""
    from gappadder_amd.pick_contigs import revcomp
    rng = np.random.default_rng(seed)
    bodies = [0, 1, k - 1, k, 500, 37, 200]
    gaps = []
    for g in range(40):
        kind = "plain"
        body_len = bodies[g % len(bodies)]
        if g in LONG:
            kind, body_len = "long", LONG[g][0]               # body + k - 1 windows (fewer where a flank part is shorter than k - 1)
        elif g in (9, 23):
            kind = "open"
        elif g == 12:
            kind = "short"
        elif g == 17 and style == "exact":
            kind = "repeat"
        elif g == 30 and style == "exact":
            kind = "mismatch"
        lf, rf, body = _seq(rng, 100), _seq(rng, 100), _seq(rng, body_len)
        truth = lf + body + rf
        rev, a = bool(g % 2), (A_LONG if g % 4 < 2 else A_SHORT)
        fill = body
        if kind == "long":
            at = LONG[g][1] * CHUNK - 18                      # in the stored orientation; window index = body position where the part
            at = body_len - at - INSERT if rev else at        # of the contig before the body has k - 1 bases, a few less otherwise
            fill = body[:at] + _other(body[at]) + _seq(rng, INSERT - 2) + _other(body[at + INSERT - 1]) + body[at + INSERT:]
        elif body_len >= 200 and g % 3 == 0:                  # one wrong base: a zero run of k
            fill = body[:90] + _other(body[90]) + body[91:]
        left_part, right_part = lf[-(60 + g % 7):], rf[:55 + g % 5]
        if kind == "repeat":                                  # the anchors once more outside: the leftmost / rightmost occurrences count
            left_part, right_part = lf[-a:] + _seq(rng, 20) + left_part, right_part + _seq(rng, 11) + rf[:a]
            b0, b1 = a, len(left_part) + len(fill) + len(right_part) - a
        else:
            b0, b1 = len(left_part), len(left_part) + len(fill)
        contig = left_part + fill + right_part
        if kind == "short":
            if style == "pick" or k >= 36:
                contig = lf[-15:] + "ACGTA" + rf[:15] if style == "exact" else "ACGTACGTACGT"
                b0, b1, a = (15, 20, A_SHORT) if style == "exact" else (5, 7, a)
            else:
                kind = "open"
        n = len(contig)
        stored = revcomp(contig) if rev else contig
        sb0, sb1 = (n - b1, n - b0) if rev else (b0, b1)
        n_rows = POOLS[(g // 2) % 4] if kind != "long" else 300
        reads = []
        for _ in range(n_rows):
            o = int(rng.integers(0, len(truth) - L + 1))
            r = truth[o:o + L]
            if masked and rng.integers(0, 4) == 0:
                p = int(rng.integers(0, L))
                r = r[:p] + "N" + r[p + 1:]
            reads.append(revcomp(r) if rng.integers(0, 2) else r)
        gaps.append({"kind": kind, "flanks": (lf, rf), "stored": stored, "body": (sb0, sb1), "rev": rev, "a": a, "reads": reads,
                     "decoys": [_seq(rng, int(rng.integers(20, 120))) for _ in range(int(rng.integers(0, 3)))]})
    # the contig list: decoys and tombstones mixed in, the list exactly at its capacity, the counter beyond it
    recs, words, picks, expect = [], [0] * len(gaps), {}, [None] * len(gaps)
    order = rng.permutation(len(gaps))
    for g in order.tolist():
        G = gaps[g]
        for d in G["decoys"]:
            recs.append((g, d))
        if g % 3 == 0:
            recs.append((g, None))                            # a tombstone before the winner
        ci = len(recs)
        recs.append((g, G["stored"]))
        if G["kind"] == "open":
            continue
        sb0, sb1 = G["body"]
        span = sb1 - sb0 + (7 if G["kind"] == "mismatch" else 0)
        words[g] = _word(G["a"], span, ci, G["rev"])
        expect[g] = "mismatch" if G["kind"] == "mismatch" else (sb0, sb1)
        if style == "pick":      # (lp, rp, lm, rm, reverse, threshold, reserved): 1-based positions of the two alignments around the body
            lm, rm = min(40, sb0), min(35, len(G["stored"]) - sb1)
            picks[ci] = (sb1 + 1, sb0 - lm + 1, rm, lm, 1, G["a"], 0) if G["rev"] else (sb0 - lm + 1, sb1 + 1, lm, rm, 0, G["a"], 0)
    return {"gaps": gaps, "recs": recs, "words": words, "picks": picks, "expect": expect}


def _run_device(case, k, L, masked, style):
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd.hip_api import GapFill
    gaps, recs = case["gaps"], case["recs"]
    n_gaps, n = len(gaps), len(recs)
    gp = np.zeros(n_gaps, dtype=B.GAP)
    for g in range(n_gaps):
        gp[g] = (0, 2000 * (g + 1), 2000 * (g + 1) + 100, g + 1)
    gf = GapFill(0)
    gf.set_gaps(gp, 1, [G["flanks"] for G in gaps])
    ctg = np.zeros(n, dtype=B.CONTIG)
    o = 0
    for i, (g, s) in enumerate(recs):
        ctg[i] = (g, 31, 29, 1, len(s), 0, 0, o) if s is not None else (g, 31, 29, 3, 0, 5, 0, 0)
        o += len(s or "")
    seq = "".join(s or "" for _, s in recs).encode()
    reads = [r for G in gaps for r in G["reads"]]
    off = np.cumsum([0] + [len(G["reads"]) for G in gaps]).astype(np.uint64)
    packed, nm = GapFill.pack_reads(reads, L, with_mask=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_pool = dev(np.concatenate([packed.reshape(-1), np.zeros(64, dtype=np.uint8)]))
    d_nm = dev(nm.view(np.int32)) if masked else None
    d_off, d_ctg, d_seq = dev(off.view(np.int64)), dev(ctg.view(np.uint8)), dev(np.frombuffer(seq, dtype=np.uint8))
    d_n = torch.tensor([n + 3], dtype=torch.int32, device="cuda")             # the counter counts records beyond the capacity
    d_best = dev(np.array(case["words"], dtype=np.uint64).view(np.int64))
    d_pick = None
    if style == "pick":
        pk = np.zeros(n, dtype=B.CTG_PICK)
        for ci, p in case["picks"].items():
            pk[ci] = p
        d_pick = dev(pk.view(np.uint8))
    d_out = torch.full((n_gaps * 32,), 0x55, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B.FS_WORDS,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = B.lib().gf_fill_support_dev(gf.handle, d_pool.data_ptr(), d_nm.data_ptr() if masked else None, d_off.data_ptr(), len(reads), L,
                                     d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), d_best.data_ptr(),
                                     d_pick.data_ptr() if d_pick is not None else None, A_LONG, A_SHORT, k, MIN_COUNT, d_out.data_ptr(),
                                     d_st.data_ptr())
    assert rc == 0, (rc, B.lib().gf_last_error(gf.handle))
    gf.sync()
    return np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.FILL_SUPPORT), d_st.cpu().numpy().view(np.uint32), gf


@pytest.mark.parametrize("style", ["exact", "pick"])
@pytest.mark.parametrize("L,masked", [(150, False), (100, True)])
@pytest.mark.parametrize("k", KS)
def test_kernel_records_equal_the_twin(k, L, masked, style):
    from gappadder_amd import _lib as B
    case = _build(k, L, masked, style, 1000 * k + L)
    want, n_eval, n_mis, n_win = _twin(case, k, L, masked, style)
    _cases_are_there(case, want, k, L, masked)
    got, st, _ = _run_device(case, k, L, masked, style)
    bad = [g for g in range(len(want)) if got[g].tobytes() != want[g].tobytes()]
    assert not bad, [(g, case["gaps"][g]["kind"], got[g], want[g]) for g in bad[:4]]
    assert int(st[B.FS_GAPS]) == n_eval and int(st[B.FS_MISMATCH]) == n_mis == (1 if style == "exact" else 0)
    assert int(st[B.FS_WINDOWS]) + (int(st[B.FS_WINDOWS + 1]) << 32) == n_win


def _twin(case, k, L, masked, style):
    """The records the twin gives for a run's input, with the stats words: (records, gaps evaluated, mismatches, windows)."""
    from gappadder_amd import _lib as B
    from gappadder_amd import read_support as RS
    want = np.zeros(len(case["gaps"]), dtype=B.FILL_SUPPORT)
    n_eval = n_mis = n_win = 0
    recs = case["recs"]
    for g, G in enumerate(case["gaps"]):
        w = case["words"][g]
        if not w:
            continue
        ci = 0x7FFFFFFF - ((w >> 1) & 0x7FFFFFFF)
        assert recs[ci] == (g, G["stored"])
        entry = None
        if style == "pick":
            entry = np.zeros((), dtype=B.CTG_PICK)
            entry[()] = case["picks"][ci]
        body = RS.locate(w, G["stored"], G["flanks"], entry)
        assert body == (None if case["expect"][g] == "mismatch" else case["expect"][g]), (g, G["kind"], body, case["expect"][g])
        if body is None:
            n_mis += 1
            continue
        # the twin reads what the device reads: without the mask words an N of a read is the base A
        reads = G["reads"] if masked else [r.replace("N", "A") for r in G["reads"]]
        want[g] = RS.support_host(reads, G["stored"], body[0], body[1], k, MIN_COUNT)
        n_eval += 1
        n_win += int(want[g]["n_windows"])
    return want, n_eval, n_mis, n_win


def _cases_are_there(case, want, k, L, masked):
    """What the cases are there for, from the twin alone."""
    from gappadder_amd import read_support as RS
    kinds = {G["kind"]: g for g, G in enumerate(case["gaps"])}
    for g, (body_len, boundary) in LONG.items():
        G = case["gaps"][g]
        assert G["kind"] == "long" and G["rev"] == bool(g % 2)
        n_win = int(want[g]["n_windows"])
        assert boundary * CHUNK < n_win <= body_len + k - 1 and (n_win + CHUNK - 1) // CHUNK == boundary + 1
        # the longest zero run of the gap, from the window supports: it is the planted one and has windows in both chunks
        reads = G["reads"] if masked else [r.replace("N", "A") for r in G["reads"]]
        sup = RS.window_supports(reads, G["stored"], G["body"][0], G["body"][1], k)
        runs, start = [], None
        for i, s_ in enumerate(sup + [1]):
            if s_ == 0 and start is None:
                start = i
            elif s_ != 0 and start is not None:
                runs.append((i - start, start, i - 1))
                start = None
        length, first, last = max(runs)
        assert length == int(want[g]["zero_run"]) >= INSERT + k - 1, (g, length, first, last)
        assert first < boundary * CHUNK <= last, (g, length, first, last)
        assert sum(r[0] == length for r in runs) == 1, (g, runs)              # no other run as long: this one decides the field
    assert not want[kinds["open"]].tobytes().strip(b"\0") and case["words"][kinds["open"]] == 0
    if "short" in kinds:
        assert case["words"][kinds["short"]] and int(want[kinds["short"]]["n_windows"]) == 0
    assert sum(int(r["n_windows"]) > 0 for r in want) >= 30 and sum(int(r["n_zero"]) == 0 and int(r["n_windows"]) > 0 for r in want) >= 3
    assert sum(int(r["zero_run"]) == k for r in want) >= 1


def test_arguments_are_checked():
    from gappadder_amd import _lib as B
    case = _build(31, 150, False, "exact", 5)
    _, _, gf = _run_device(case, 31, 150, False, "exact")
    lib = B.lib()
    import torch
    z = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = z.data_ptr()
    args = lambda k, a_long=30, a_short=15: (gf.handle, p, None, p, 0, 150, p, p, 0, p, p, None, a_long, a_short, k, 2, p, p)
    assert lib.gf_fill_support_dev(*args(15)) == B.GF_E_UNSUPPORTED and lib.gf_fill_support_dev(*args(65)) == B.GF_E_UNSUPPORTED
    assert lib.gf_fill_support_dev(*args(31, 40)) == B.GF_E_INVAL and lib.gf_fill_support_dev(*args(31, 30, 30)) == B.GF_E_INVAL
