"""gf_fill_adjudicate_dev (csrc/fill_adj.hip) called directly on hand-built contig lists and pools: the cases of
tests/fill_adj_cases.py — whose records are derived by hand — and, beside them, the cases that are the device's own, with the twin
(fill_adjudication.adjudicate_gaps) as their reference: pools of 0, 1, 255, 256, 257 and 513 rows around the kernel's batch of 256; fills
that start at contig offsets 63 and 64 on either strand; fills that differ in length by 1 and by 300 bases (the diagonals right of the
window); 2 400 small gaps in one call — more than twice the workgroups the entry launches, so that every workgroup takes several
gaps in turn — of kinds that leave the kernel's loop at different places (votes, an empty pool, a flank with an N, a locus too long,
an uncontested gap, and in a second call an altered record), mixed so that the gaps of one workgroup differ; open, uncontested and
LOST gaps in between; a gf_fill_alt record altered by the test (a mismatch); the refused arguments.  L = 150, and L = 100 with N masks; seeds of 12,
16 and 32 bases.  The alternatives' records come from gf_fill_alts_dev on the same list.  Records, statistics and the guard bytes around
d_adj must be equal (tobytes())."""
import random

import numpy as np
import pytest

import fill_adj_cases as JC

pytestmark = pytest.mark.gpu

GUARD = 64
WGS_PER_CU = 3      # fill_adj.hip AJ_WGS_PER_CU: the entry launches min(n_gaps, CUs * 3) workgroups
N_SMALL = 2400
# seed -> (max_mismatch at L = 150, at L = 100, min_overlap): floor(L / seed) > max_mismatch
PARAMS = {12: (4, 4, 40), 16: (4, 4, 48), 32: (3, 2, 48)}
_WORLDS = {}


def sampled(rng, Gs, L, n, masked):
    """n rows of the haplotypes Gs in turn: anywhere, either strand, 1 % substitutions, with `masked` one in four with an N."""
    out = []
    for x in range(n):
        G = Gs[x % len(Gs)]
        o = rng.randrange(0, len(G) - L + 1)
        r = [JC.flip(c, 0) if rng.random() < 0.01 else c for c in G[o:o + L]]
        if masked and rng.random() < 0.25:
            r[rng.randrange(L)] = "N"
        r = "".join(r)
        out.append(JC.rc(r) if rng.random() < 0.5 else r)
    return out


def device_cases(L, masked, big, seed=26):
    """(cases without hand-derived answers: the twin is their reference)"""
    rng = random.Random(seed + L)
    out = []

    def add(name, Fw, Fr, n_rows, turn_w=False, turn_r=False, cl=40, flank=400, n_at=None):
        lf, rf = JC.rnd(rng, flank), JC.rnd(rng, flank)
        if n_at is not None:                                                  # an N in the left flank, n_at bases before the gap
            lf = lf[:flank - n_at] + "N" + lf[flank - n_at + 1:]
        cut = lambda G: G[len(lf) - min(len(lf), 2 * L):]                     # (rows from around the fill, not from the far flanks)
        reads = sampled(rng, [cut(lf + Fw + rf)[:len(Fw) + 4 * L], cut(lf + Fr + rf)[:len(Fr) + 4 * L]], L, n_rows, masked)
        out.append(dict(name=name, L=L, lf=lf, rf=rf, fill_w=Fw, fill_r=Fr, reads=reads, want=None, turn_w=turn_w, turn_r=turn_r, rival_far=None, cl=cl))

    for n_rows in ((0, 1, 255, 256, 257, 513) if big else (257,)):
        F = JC.rnd(rng, 200)
        add("pool of %d rows" % n_rows, F, JC.flip(F, 70, 130), n_rows, turn_r=bool(n_rows & 1))
    for cl in (63, 64):
        for turn in (False, True):
            F = JC.rnd(rng, 130)
            add("fill at contig offset %d, strand %d" % (cl, turn), F, F[:64] + F[65:], 40, turn_w=turn, turn_r=not turn, cl=cl)
    F = JC.rnd(rng, 500)
    add("a length difference of 1", F, F[:100] + "A" + F[100:], 120)
    add("a length difference of 300", F, F[:100] + F[400:], 120, turn_w=True)
    if big:
        # (the kind follows x % 7, and the workgroups stride by a number that is no multiple of 7: the gaps of one workgroup differ)
        for x in range(N_SMALL):
            kind = x % 7
            F = JC.rnd(rng, 8192 - 2 * L + 1 if x % 400 == 13 else 40)      # (six of them: a locus of 8 193 bases)
            Fr = F if kind == 5 else F[:x % 30] + F[x % 30 + 2:] if kind == 0 else JC.flip(F, x % 40)
            add("small gap %d" % x, F, Fr, 0 if kind == 3 else 4 + x % 3, turn_w=bool(x & 1), turn_r=bool(x & 2), flank=200, n_at=50 if kind == 4 else None)
    return out


def assemble(cs):
    """fill_adj_cases.assemble for cases with a left context of their own, plus a LOST gap behind every 50th case."""
    contigs, flanks, best, reads, gap_of = [], [], [], [], {}
    ctg = lambda c, F, turn: JC.rc(c["lf"][-c["cl"]:] + F + c["rf"][:40]) if turn else c["lf"][-c["cl"]:] + F + c["rf"][:40]
    for x, c in enumerate(cs):
        g = len(flanks)
        gap_of[x] = g
        flanks.append((c["lf"], c["rf"]))
        best.append(JC.word(30, len(c["fill_w"]), len(contigs), int(c["turn_w"])))
        contigs += [(g, ctg(c, c["fill_w"], c["turn_w"])), (g, ctg(c, c["fill_r"], c["turn_r"]))]
        reads.append(c["reads"])
        if x % 50 == 7:                                               # LOST: the word states a span the contig does not carry
            g = len(flanks)
            flanks.append((c["lf"], c["rf"]))
            best.append(JC.word(30, len(c["fill_w"]) + 3, len(contigs), int(c["turn_w"])))
            contigs += [(g, ctg(c, c["fill_w"], c["turn_w"])), (g, ctg(c, c["fill_r"], c["turn_r"]))]
            reads.append(c["reads"][:2])
    return contigs, flanks, best, reads, gap_of


def world(L, masked, big):
    """One contig list, pool and context on the device (cached): the shared cases of this read length, then the device's own."""
    key = (L, masked, big)
    if key in _WORLDS:
        return _WORLDS[key]
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_alternatives as FA
    from gappadder_amd.hip_api import GapFill
    shared = [c for c in JC.cases() if c["L"] == L]
    c1, f1, b1, r1, gap_shared = JC.assemble(shared)
    own = device_cases(L, masked, big)
    c2, f2, b2, r2, gap_own = assemble(own)
    ng1, nc1 = len(f1), len(c1)
    contigs = c1 + [(g + ng1, s) for g, s in c2]
    flanks, reads = f1 + f2, r1 + r2
    best = b1 + [w - (nc1 << 1) if w else 0 for w in b2]              # (the contig field is 0x7FFFFFFF - index)
    if not masked:
        reads = [[r.replace("N", "A") for r in rs] for rs in reads]   # without the mask words an N of a read is the base A
    n, n_gaps = len(contigs), len(flanks)
    ctg = np.zeros(n, dtype=B.CONTIG)
    o = 0
    for i, (g, s) in enumerate(contigs):
        ctg[i] = (g, 31, 29, 1, len(s), 0, 0, o)
        o += len(s)
    gaps = np.zeros(n_gaps, dtype=B.GAP)
    for g in range(n_gaps):
        gaps[g] = (0, 20000 * (g + 1), 20000 * (g + 1) + 100, g + 1)
    gf = GapFill(0)
    gf.set_gaps(gaps, 1, flanks)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    flat = [r for rs in reads for r in rs]
    packed, nm = GapFill.pack_reads(flat, L, with_mask=True)
    w = dict(L=L, masked=masked, shared=shared, gap_shared=gap_shared, own=own, gap_own={x: g + ng1 for x, g in gap_own.items()}, contigs=contigs,
             flanks=flanks, best=best, reads=reads, n=n, n_gaps=n_gaps, n_rows=len(flat), gf=gf, lib=B.lib(), dev=dev,
             d_ctg=dev(ctg.view(np.uint8)), d_seq=dev(np.frombuffer("".join(s for _, s in contigs).encode(), dtype=np.uint8)),
             d_pool=dev(np.concatenate([packed.reshape(-1), np.zeros(64, dtype=np.uint8)])), d_nm=dev(nm.view(np.int32)) if masked else None,
             d_off=dev(np.cumsum([0] + [len(rs) for rs in reads]).astype(np.int64)), d_n=torch.tensor([n], dtype=torch.int32, device="cuda"),
             d_best=dev(np.array(best, dtype=np.uint64).view(np.int64)), twins={})
    # the alternatives' records of this list, from the device, equal to their own twin
    d_alt = torch.zeros(n_gaps * B.FILL_ALT.itemsize, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(B.FA_WORDS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = w["lib"].gf_fill_alts_dev(gf.handle, w["d_ctg"].data_ptr(), w["d_n"].data_ptr(), n, w["d_seq"].data_ptr(), 30, 15, 16, None, w["d_best"].data_ptr(),
                                   d_alt.data_ptr(), None, d_st.data_ptr())
    assert rc == 0, (rc, w["lib"].gf_last_error(gf.handle))
    gf.sync()
    w["alts"] = np.frombuffer(d_alt.cpu().numpy().tobytes(), dtype=B.FILL_ALT).copy()
    want_alts, _, ast = FA.alts_host(contigs, flanks, best)
    assert w["alts"].tobytes() == want_alts.tobytes()
    n_lost = sum(1 for x in range(len(own)) if x % 50 == 7)
    n_same = sum(1 for c in own if c["fill_w"] == c["fill_r"])              # (uncontested: two contigs of one fill)
    assert ast["lost"] == n_lost and ast["contested"] == len(shared) + len(own) - n_same, ast
    _WORLDS[key] = w
    return w


def params(w, s, context=None, min_votes=3, ratio=2):
    mm_150, mm_100, mo = PARAMS[s]
    return s, (mm_150 if w["L"] == 150 else mm_100), mo, (w["L"] if context is None else context), min_votes, ratio


def twin(w, prm, alts=None):
    from gappadder_amd import fill_adjudication as ADJ
    key = prm if alts is None else None
    if key is None or key not in w["twins"]:
        out = ADJ.adjudicate_gaps(w["alts"] if alts is None else alts, w["contigs"], w["flanks"], w["best"], lambda g: w["reads"][g], w["L"], (30, 15), *prm)
        if key is None:
            return out
        w["twins"][key] = out
    return w["twins"][key]


def call(w, prm, alts=None, expect=0, **over):
    """(records, statistics dictionary) of one call; the outputs and the scratch are pre-filled with junk; the guard bytes are checked."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import fill_adjudication as ADJ
    text, lens = ADJ.flank_context(w["flanks"], prm[3] if 1 <= prm[3] <= 1000 else 1)
    d_text, d_lens = w["dev"](text.reshape(-1)), w["dev"](lens.reshape(-1).view(np.int16))
    d_alt = w["dev"]((w["alts"] if alts is None else alts).view(np.uint8))
    d_scratch = torch.full((w["n_rows"] + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_rec = torch.full((w["n_gaps"] * B.FILL_ADJ.itemsize + 2 * GUARD,), 0x55, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B.AJ_WORDS + 4,), 7, dtype=torch.int32, device="cuda")          # (two guard words on either side: the u64 counters stay aligned)
    ptr = lambda t: t.data_ptr() if t is not None else None
    a = dict(pool=ptr(w["d_pool"]), nm=ptr(w["d_nm"]), off=ptr(w["d_off"]), rows=w["n_rows"], L=w["L"], ctg=ptr(w["d_ctg"]), n=ptr(w["d_n"]), cap=w["n"],
             seq=ptr(w["d_seq"]), best=ptr(w["d_best"]), a_l=30, a_s=15, alt=ptr(d_alt), text=ptr(d_text), lens=ptr(d_lens), scratch=ptr(d_scratch),
             rec=d_rec.data_ptr() + GUARD, st=d_st.data_ptr() + 8)
    a.update(over)
    torch.cuda.synchronize()
    rc = w["lib"].gf_fill_adjudicate_dev(w["gf"].handle, a["pool"], a["nm"], a["off"], a["rows"], a["L"], a["ctg"], a["n"], a["cap"], a["seq"], a["best"],
                                         a["a_l"], a["a_s"], a["alt"], a["text"], a["lens"], a["scratch"], *prm, a["rec"], a["st"])
    assert rc == expect, (rc, expect, over, prm, w["lib"].gf_last_error(w["gf"].handle))
    w["gf"].sync()
    raw, st = d_rec.cpu().numpy().tobytes(), d_st.cpu().numpy()
    if expect:
        return None
    assert raw[:GUARD] == raw[-GUARD:] == b"\x55" * GUARD and list(st[:2]) + list(st[-2:]) == [7] * 4
    assert int(d_scratch[-1]) == 0x5A5A5A5A
    return np.frombuffer(raw[GUARD:-GUARD], dtype=B.FILL_ADJ), ADJ.stats_dict(st[2:-2])


def same(w, got, want):
    names = {g: c["name"] for cs, gaps in ((w["shared"], w["gap_shared"]), (w["own"], w["gap_own"])) for x, c in enumerate(cs) for g in [gaps[x]]}
    bad = [g for g in range(w["n_gaps"]) if got[0][g].tobytes() != want[0][g].tobytes()]
    assert not bad, [(g, names.get(g), got[0][g], want[0][g]) for g in bad[:4]]
    assert got[1] == want[1]


def test_the_big_world_equals_the_twin_and_the_hand_derived_answers():
    """L = 150, seed 16: every pool size around the batch, 2 400 small gaps of mixed kinds in one call, LOST, open and uncontested gaps
    in between; every workgroup takes at least two gaps."""
    import torch
    from test_fill_adjudication_host import as_dict
    w = world(150, False, True)
    blocks = torch.cuda.get_device_properties(0).multi_processor_count * WGS_PER_CU
    print("gaps", w["n_gaps"], "workgroups", blocks)
    assert w["n_gaps"] > 2 * blocks                                   # (g += gridDim.x: a second and a third gap per workgroup)
    prm = params(w, 16)
    want = twin(w, prm)
    got = call(w, prm)
    print(got[1])
    same(w, got, want)
    for x, c in enumerate(w["shared"]):
        assert as_dict(got[0][w["gap_shared"][x]]) == c["want"], c["name"]
    st = want[1]
    small = [(x, c) for x, c in enumerate(w["own"]) if c["name"].startswith("small gap")]
    n_same = sum(1 for _, c in small if c["fill_w"] == c["fill_r"])
    n_long = sum(1 for _, c in small if len(c["fill_w"]) > 7000 and c["fill_w"] != c["fill_r"])
    n_n = sum(1 for _, c in small if "N" in c["lf"] and len(c["fill_w"]) < 7000 and c["fill_w"] != c["fill_r"])
    assert len(small) == N_SMALL and n_same > 300 and n_long >= 5 and n_n > 300
    assert st["contested"] == len(w["shared"]) + len(w["own"]) - n_same and st["mismatches"] == 0
    assert st["skipped_long"] == 1 + n_long and st["skipped_non_acgt"] == 1 + n_n
    assert sum(1 for x, c in small if int(got[0][w["gap_own"][x]]["flags"]) & JC.NO_ROWS) > 300
    assert st["keep"] >= 3 and st["switch"] >= 2 and st["undecided"] >= 5 and st["ties"] > 500
    zero = [g for g in range(w["n_gaps"]) if not int(w["alts"][g]["flags"]) & 4 or int(w["alts"][g]["flags"]) & 32]
    n_lost = sum(x % 50 == 7 for x in range(len(w["own"])))
    n_lost_same = sum(1 for x, c in enumerate(w["own"]) if x % 50 == 7 and c["fill_w"] == c["fill_r"])
    assert len(zero) == 2 * len(w["shared"]) + n_lost + n_same and not got[0][zero].tobytes().strip(b"\0"), (len(zero), n_lost, n_same, n_lost_same)
    by = {c["name"]: got[0][w["gap_own"][x]] for x, c in enumerate(w["own"])}
    for n_rows in (0, 1, 255, 256, 257, 513):
        r = by["pool of %d rows" % n_rows]
        assert int(r["votes_w"]) + int(r["votes_r"]) + int(r["ties"]) + int(r["unplaced"]) == n_rows and bool(int(r["flags"]) & JC.NO_ROWS) == (n_rows == 0)
    assert int(by["pool of 513 rows"]["votes_w"]) > 20 and int(by["pool of 513 rows"]["votes_r"]) > 20
    for name in ("a length difference of 1", "a length difference of 300"):
        r = by[name]
        assert int(r["votes_w"]) >= 5 and int(r["votes_r"]) >= 5 and int(r["ties"]) >= 20 and abs(int(r["locus_w"]) - int(r["locus_r"])) in (1, 300), (name, r)
    # a second call gives the same bytes (nothing of the first is left in the scratch the kernel reads)
    again = call(w, prm)
    assert again[0].tobytes() == got[0].tobytes() and again[1] == got[1]
    # a third call with every eleventh contested gap's record altered: mismatches in among the other exits.  By the definition such a
    # gap gets the zero record and is counted as a mismatch instead of what it was; every other record stays
    bad, exp_rec, exp_st = w["alts"].copy(), want[0].copy(), dict(want[1])
    hit = [g for g in range(w["n_gaps"]) if int(w["alts"][g]["flags"]) & 4 and not int(w["alts"][g]["flags"]) & 32][5::11]
    for g in hit:
        bad[g]["rival_len"] += 1
        r = exp_rec[g].copy()
        exp_rec[g] = np.zeros((), dtype=exp_rec.dtype)
        exp_st["mismatches"] += 1
        exp_st["skipped_long"] -= bool(int(r["flags"]) & JC.LONG)
        exp_st["skipped_non_acgt"] -= bool(int(r["flags"]) & JC.NON_ACGT)
        if int(r["verdict"]):
            exp_st["adjudicated"] -= 1
            exp_st[("keep", "switch", "undecided")[int(r["verdict"]) - 1]] -= 1
            for k in ("votes_w", "votes_r", "ties"):
                exp_st[k] -= int(r[k])
    assert len(hit) > 150
    same(w, call(w, prm, alts=bad), (exp_rec, exp_st))


@pytest.mark.parametrize("L, masked, s", [(150, False, 12), (150, False, 16), (150, False, 32), (100, True, 12), (100, True, 16), (100, True, 32), (100, False, 16)])
def test_seeds_read_lengths_and_masks(L, masked, s):
    from test_fill_adjudication_host import as_dict
    w = world(L, masked, False)
    prm = params(w, s, min_votes=2 if s == 32 else 3, ratio=3 if s == 12 else 2)
    want = twin(w, prm)
    got = call(w, prm)
    print(L, masked, s, got[1])
    same(w, got, want)
    assert want[1]["adjudicated"] >= len(w["own"]) and want[1]["votes_w"] > 30 and want[1]["votes_r"] > 30
    if s == 16 and (masked or L == 150):
        for x, c in enumerate(w["shared"]):
            assert as_dict(got[0][w["gap_shared"][x]]) == c["want"], c["name"]
    for x, c in enumerate(w["own"]):
        if c["name"].startswith("fill at contig offset"):
            r = got[0][w["gap_own"][x]]
            assert int(r["verdict"]) and int(r["votes_w"]) + int(r["votes_r"]) >= 3, (c["name"], r)


def test_a_shorter_context_and_other_thresholds():
    w = world(150, False, False)
    for kw in (dict(context=48), dict(context=1000), dict(min_votes=1, ratio=16), dict(min_votes=40, ratio=2)):
        prm = params(w, 16, **kw)
        got = call(w, prm)
        same(w, got, twin(w, prm))
        if "context" in kw:
            g = w["gap_own"][0]
            assert int(got[0][g]["locus_w"]) == 200 + 2 * min(kw["context"], 400)


def test_an_altered_record_is_a_mismatch():
    from gappadder_amd import _lib as B
    w = world(150, False, False)
    prm = params(w, 16)
    full = twin(w, prm)
    g = w["gap_own"][0]
    for field, value in (("rival_len", int(w["alts"][g]["rival_len"]) + 1), ("fill_len", int(w["alts"][g]["fill_len"]) - 1),
                         ("flags", int(w["alts"][g]["flags"]) ^ B.FA_F_REVERSE), ("flags", int(w["alts"][g]["flags"]) ^ B.FA_F_RIVAL_REVERSE),
                         ("rival", w["n"] + 5), ("rival", int(w["alts"][g]["rival"]) + 2), ("contig", int(w["alts"][g]["contig"]) + 1)):
        bad = w["alts"].copy()
        bad[g][field] = value
        want = twin(w, prm, bad)
        assert want[1]["mismatches"] == 1 and not want[0][g].tobytes().strip(b"\0")
        got = call(w, prm, alts=bad)
        same(w, got, want)
        assert np.delete(got[0], g).tobytes() == np.delete(full[0], g).tobytes()


def test_arguments_out_of_range_are_refused():
    from gappadder_amd import _lib as B
    w = world(150, False, False)
    ok = params(w, 16)
    U, I = B.GF_E_UNSUPPORTED, B.GF_E_INVAL
    for prm, code in (((11,) + ok[1:], U), ((33,) + ok[1:], U), ((16, 16, 48, 150, 3, 2), U), ((16, -1, 48, 150, 3, 2), U), ((16, 4, 15, 150, 3, 2), U),
                      ((16, 4, 151, 150, 3, 2), U), ((32, 4, 48, 150, 3, 2), U), ((16, 4, 48, 47, 3, 2), I), ((16, 4, 48, 1001, 3, 2), I),
                      ((16, 4, 48, 150, 0, 2), I), ((16, 4, 48, 150, 3, 1), I), ((16, 4, 48, 150, 3, 17), I), ((11, 4, 48, 150, 0, 2), U)):
        call(w, prm, expect=code)
    for over in (dict(alt=None), dict(text=None), dict(lens=None), dict(scratch=None), dict(rec=None), dict(st=None), dict(best=None), dict(off=None),
                 dict(pool=None), dict(ctg=None), dict(n=None), dict(seq=None), dict(a_l=33), dict(a_l=7, a_s=0), dict(a_s=30), dict(a_s=7),
                 dict(cap=0x80000000), dict(L=0), dict(L=1001)):
        call(w, ok, expect=I, **over)
    # the edges of the ranges are accepted
    for prm in ((12, 0, 12, 12, 1, 16), (32, 3, 150, 1000, 3, 2), (16, 4, 48, 48, 1, 2)):
        assert call(w, prm) is not None
    assert call(w, ok, a_s=0) is not None and call(w, ok, scratch=None, rows=0, pool=None) is not None
