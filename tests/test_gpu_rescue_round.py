"""Pipeline(rescue_round=True): the reference's rescue round (assemble_gaps.py:357-366, body :166-217) inside the device step, against the
CLI's definition (assemble_gaps.bridging_reads_batch = gf_bridging_reads on the HQ reads and the merged contigs), the oracle's merger and
the host picker: a hand-built gap that only its bridging read closes, and a thin-coverage synthetic step whose merge round leaves many
gaps open."""
import numpy as np
import pytest

import rescue_cases as RC
import sample_check as SC

pytestmark = pytest.mark.gpu

SEED, SLEN, NSCF, GPS, L = 20260021, 200_000, 4, 6, 150
# thin coverage: 30 000 pairs over 800 kb (about 11x of reads) with 550-bp gaps — the merge round leaves most gaps open
THIN_PAIRS, THIN_GAP = 30_000, 550


def _thin_env():
    import torch
    from gappadder_amd.hip_api import GapFill
    gf = GapFill(0)
    cfg = GapFill.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=THIN_GAP, read_len=L)
    gaps, flanks = GapFill.synth_layout(cfg)
    gf.set_gaps(gaps, NSCF, flanks)
    rb = (L + 3) // 4
    d_reads = torch.empty(2 * THIN_PAIRS * rb + 64, dtype=torch.uint8, device="cuda")
    d_recs = torch.empty(2 * THIN_PAIRS * 32, dtype=torch.uint8, device="cuda")
    gf.synth_pairs_dev(cfg, 0, THIN_PAIRS, d_reads.data_ptr(), d_recs.data_ptr())
    gf.sync()
    return {"gf": gf, "cfg": cfg, "gaps": gaps, "flanks": flanks, "d_reads": d_reads, "d_recs": d_recs, "n_reads": 2 * THIN_PAIRS,
            "n_scaffolds": NSCF}


def _hole_env():
    import torch
    from gappadder_amd.hip_api import GapFill
    c = RC.one_hole_case()
    gf = GapFill(0)
    gf.set_gaps(c["gaps"], 1, c["flanks"])
    packed, _ = GapFill.pack_reads(c["reads_blob"], L)
    d_reads = torch.from_numpy(np.concatenate([packed.reshape(-1), np.zeros(64, np.uint8)])).cuda()
    d_recs = torch.from_numpy(c["recs"].view(np.uint8).copy()).cuda()
    return {"gf": gf, "gaps": c["gaps"], "flanks": c["flanks"], "d_reads": d_reads, "d_recs": d_recs, "n_reads": c["n_reads"], "case": c,
            "n_scaffolds": 1}


def _run(env, steps=1, tag_ahead=False, kk=((31, 29),), contig_cap=None, **kw):
    from gappadder_amd.hip_api import GapFill
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    gf = env["gf"]
    tag_ctx = None
    if tag_ahead:        # (the tagger's context on the second stream knows the gaps too)
        tag_ctx = GapFill(0)
        tag_ctx.set_gaps(env["gaps"], env["n_scaffolds"], None)
    pipe = Pipeline(gf, len(env["gaps"]), L, list(kk), **kw)
    pipe.tag_ahead = tag_ahead
    pipe.add_library(DeviceLibrary("x", 300, 30, env["n_reads"], env["d_reads"], env["d_recs"], tag_ctx=tag_ctx))
    pipe.prepare()
    if contig_cap is not None:
        contig_cap(pipe)
    out = []
    for _ in range(steps):
        pipe.step()
        out.append(pipe.fetch())
    return pipe, out


@pytest.fixture(scope="module")
def hole():
    return _hole_env()


@pytest.fixture(scope="module")
def thin():
    return _thin_env()


@pytest.fixture(scope="module", params=["exact", "align"])
def thin_on(thin, request):
    pipe, (r1, r2) = _run(thin, steps=2, merge_in_step=True, rescue_round=True, anchor_mode=request.param)
    return request.param, pipe, r1, r2


@pytest.fixture(scope="module")
def thin_off(thin):
    return _run(thin, merge_in_step=True)[1][0]


def _bridge_rows(res):
    return [i for i in range(res.rescue_first, res.rescue_first + res.rescue["bridges"])]


def _own_rows(res, g, kk):
    pair = {(int(k), int(kv)): q for q, (k, kv) in enumerate(kk)}
    rows = [i for i in range(res.rescue_first) if int(res.contigs[i]["gap"]) == g and int(res.contigs[i]["length"])
            and (int(res.contigs[i]["k"]), int(res.contigs[i]["kv"])) in pair]
    rows.sort(key=lambda i: (pair[(int(res.contigs[i]["k"]), int(res.contigs[i]["kv"]))], -int(res.contigs[i]["length"]), RC.contig_text(res, i), i))
    return rows


def _unpack(rows):
    codes = np.stack([(rows >> s) & 3 for s in (6, 4, 2, 0)], axis=-1).reshape(len(rows), -1)[:, :L]
    return ["".join(r) for r in np.array(list("ACGT"))[codes]]


def _host_bridges(env, pipe, res):
    """Definition 2-4 on the host: per tried gap the bridges gf_bridging_reads finds among its HQ reads against its alignment set."""
    from gappadder_amd import _lib as B
    from gappadder_amd.assemble_gaps import bridging_reads_batch
    from gappadder_amd.pipeline import decode_best
    lb = pipe.libs[0]
    n_th = int(lb.d_cnt[4])
    th = np.frombuffer(lb.d_thits[:n_th * 12].cpu().numpy().tobytes(), dtype=B.TAGHIT)
    recs = np.frombuffer(env["d_recs"].cpu().numpy().tobytes(), dtype=B.ALNREC)
    rows = env["d_reads"][:env["n_reads"] * ((L + 3) // 4)].cpu().numpy().reshape(env["n_reads"], -1)
    hq = RC.hq_reads(recs, th, len(env["gaps"]), lambda r: _unpack(rows[r:r + 1])[0])
    tried = [g for g, w in enumerate(res.best.tolist()) if not w or decode_best(w)[2] >= res.rescue_first]
    merge_first = res.merge["contigs_before"]
    items = [(RC.alignment_set(res, g, merge_first, res.rescue_first), {"%d_%d" % (l, r): s for l, r, s in hq.get(g, [])}) for g in tried]
    got = bridging_reads_batch(items) if items else []
    return {g: [s for _, s in b] for g, b in zip(tried, got) if b}, sum(len(hq.get(g, [])) for g in tried), len(tried)


def test_one_gap_one_hole_is_closed_by_its_bridging_read(hole):
    """Coverage drops to one pair over 40 bases near the left flank: the merge round leaves the gap open, the rescue finds exactly the
    one bridge and the gap closes with the true sequence."""
    pipe_off, (off,) = _run(hole, merge_in_step=True)
    assert int(off.best[0]) == 0
    pipe, (res,) = _run(hole, merge_in_step=True, rescue_round=True)
    rs = res.rescue
    assert rs["gaps_tried"] == 1 and rs["bridges"] == 1 and rs["gaps_with_bridges"] == 1 and rs["closed"] == 1 and rs["dropped"] == 0, rs
    b = res.contigs[res.rescue_first]
    assert int(b["k"]) == int(b["kv"]) == 0xFFFF and RC.contig_text(res, res.rescue_first) == hole["case"]["bridge"]
    picked = pipe.picked_sequences(res)
    st, en = hole["case"]["gap"]
    truth = hole["case"]["truth"]
    body = picked[0][1]
    assert body in truth[st - 6:en + 6] and abs(len(body) - (en - st + 10)) <= 1, (len(body), en - st)


def test_bridges_equal_the_host_definition(thin, thin_on, thin_off):
    mode, pipe, res, _ = thin_on
    want, n_hq, n_tried = _host_bridges(thin, pipe, res)
    rs = res.rescue
    print("thin %s: tried %d (off: %d open), hq %d, bridges %d in %d gaps, merged %d, closed %d, dropped %d"
          % (mode, rs["gaps_tried"], int((thin_off.best == 0).sum()), rs["hq_reads"], rs["bridges"], rs["gaps_with_bridges"], rs["merged_contigs"],
             rs["closed"], rs["dropped"]))
    assert rs["dropped"] == 0 and rs["gaps_tried"] == n_tried == int((thin_off.best == 0).sum()) and rs["hq_reads"] == n_hq
    assert rs["gaps_tried"] >= 5 and rs["bridges"] > 0
    got = {}
    for i in _bridge_rows(res):
        assert int(res.contigs[i]["k"]) == int(res.contigs[i]["kv"]) == 0xFFFF
        got.setdefault(int(res.contigs[i]["gap"]), []).append(RC.contig_text(res, i))
    assert got == want


def test_rescue_merge_equals_the_oracle(thin_on):
    mode, pipe, res, _ = thin_on
    kk = pipe.kk
    n_merged = 0
    for g in sorted(set(int(res.contigs[i]["gap"]) for i in _bridge_rows(res))):
        own = [RC.contig_text(res, i) for i in _own_rows(res, g, kk)]
        br = [RC.contig_text(res, i) for i in _bridge_rows(res) if int(res.contigs[i]["gap"]) == g]
        lo = res.rescue_first + res.rescue["bridges"]
        got = [RC.contig_text(res, i) for i in range(lo, len(res.contigs)) if int(res.contigs[i]["gap"]) == g]
        assert got == SC.expected_merged_contigs(own + br), g
        n_merged += len(got)
    assert n_merged == res.rescue["merged_contigs"]


def test_rescue_picks_equal_the_host_twin(thin, thin_on):
    from gappadder_amd.pick_contigs import pick_gap_sequence
    from gappadder_amd.pipeline import decode_best
    mode, pipe, res, _ = thin_on
    flanks, a = thin["flanks"], pipe.anchors[-1]
    seqs = pipe.picked_sequences(res)
    n = 0
    for g, w in enumerate(res.best.tolist()):
        if w and decode_best(w)[2] < res.rescue_first:
            continue
        recs = [("c%d" % i, RC.contig_text(res, i)) for i in range(res.rescue_first, len(res.contigs)) if int(res.contigs[i]["gap"]) == g]
        want = pick_gap_sequence(recs, flanks[g][0], flanks[g][1], a, mode=mode) if recs else None
        if want is None:
            assert not w, g
        else:
            assert w and seqs[g][1] == want[1], g
            n += 1
    assert n == res.rescue["closed"]


def _contig_set(res, lo=0, hi=None):
    """The records of [lo, hi) as a multiset (the assembly lists a gap's contigs in no fixed order)."""
    hi = len(res.contigs) if hi is None else hi
    return sorted((int(c["gap"]), int(c["k"]), int(c["kv"]), int(c["n_nodes"]), int(c["cov_sum"]), RC.contig_text(res, i))
                  for i, c in enumerate(res.contigs[lo:hi], lo))


def _picks(res):
    """Pick words with the contig named by its bases."""
    from gappadder_amd.pipeline import decode_best
    return {g: decode_best(w)[:2] + (decode_best(w)[3], RC.contig_text(res, decode_best(w)[2])) for g, w in enumerate(res.best.tolist()) if w}


def _same(a, b):
    return _contig_set(a) == _contig_set(b) and _picks(a) == _picks(b) and a.rescue == b.rescue and a.rescue_first == b.rescue_first


def test_nothing_before_the_rescue_changes_and_steps_repeat(thin, thin_on, thin_off):
    mode, pipe, r1, r2 = thin_on
    off = thin_off if mode == "exact" else _run(thin, merge_in_step=True, anchor_mode=mode)[1][0]
    f = r1.rescue_first
    assert f == len(off.contigs) and _contig_set(r1, 0, f) == _contig_set(off)
    p1, p0 = _picks(r1), _picks(off)
    assert all(p1[g] == p0[g] for g in p0) and set(p0) <= set(p1)
    assert _same(r1, r2)


def test_tag_ahead_gives_the_same_results(thin):
    """The next step's tagger rewrites the hits on a second stream after the HQ keys are listed: the same results, step after step."""
    _, (r1,) = _run(thin, merge_in_step=True, rescue_round=True)
    _, (a, b) = _run(thin, steps=2, tag_ahead=True, merge_in_step=True, rescue_round=True)
    assert _same(a, r1) and _same(b, r1)


@pytest.mark.parametrize("where", ["merge", "bridges"])
def test_a_contig_list_the_rescue_overflows_raises_and_the_next_step_is_clean(hole, where):
    """contig_cap just past the bridge (the rescue's merge overflows) or at the first bridge (the bridge append overflows: no record at
    the cap, the counters count it): the step raises; restored, the next step equals a clean run."""
    pipe, (ref,) = _run(hole, merge_in_step=True, rescue_round=True)
    assert ref.rescue["bridges"] == 1 and ref.rescue["merged_contigs"] >= 1
    cap0, first = pipe.contig_cap, ref.rescue_first
    pipe.contig_cap = first + 1 if where == "merge" else first
    canary = pipe.d_ctg[first * 32:(first + 1) * 32].clone()
    if where == "bridges":
        pipe.d_ctg[first * 32:(first + 1) * 32].fill_(0xA5)
        canary.fill_(0xA5)
    pipe.step()
    with pytest.raises(RuntimeError):
        pipe.fetch()
    st = pipe.rescue.d_st.cpu().numpy()
    if where == "bridges":
        from gappadder_amd import _lib as B
        assert int(st[B.RS_APPEND_ERR]) == 2 and int(st[B.RS_BRIDGES]) == 1 and int(pipe.d_acnt[0]) >= first + 1
        assert bool((pipe.d_ctg[first * 32:(first + 1) * 32] == canary).all())       # nothing written at the cap
    pipe.contig_cap = cap0
    pipe.step()
    assert _same(pipe.fetch(), ref)


def test_cli_closes_the_gap_with_the_same_sequence(hole, tmp_path):
    """The one-hole case as files (builtin BAM, no both-unmapped pairs) through `python -m gappadder_amd.main -c All`: the CLI's host rounds
    (gap_reads_high_quality files, bridges appended to the restored contigs, merge, pick at 15) write the sequence the device rescue picked."""
    import os
    import subprocess
    import sys
    import pipeline_util as PU
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pipe, (res,) = _run(hole, merge_in_step=True, rescue_round=True)
    body = pipe.picked_sequences(res)[0][1]
    cfgp, wf, _ = PU.materialise(RC.one_hole_files(hole["case"]), str(tmp_path), kmers=((31, 29),), builtin_bam=True)
    r = subprocess.run([sys.executable, "-m", "gappadder_amd.main", "-c", "All", "-g", cfgp], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    picked = open(wf + "picked_seqs.fa").read().split("\n")
    assert len(picked) >= 2 and picked[0].startswith(">0_1"), picked[:2]
    assert picked[1] == body


def _two_lib_env(hole):
    """The one-hole case as library 0 and, as library 1, the bridge pair once more with an N-masked base in the gap read: the hole's
    k-mers that do not cover the N now count twice, those that do stay single, so the contigs still break there and both gap reads bridge."""
    import torch
    from gappadder_amd.hip_api import GapFill
    c = hole["case"]
    s, a, b = c["pairs"][-1]
    t = c["truth"]
    pos = next(x for x in range(1888, 1900) if t[x] not in "T")          # (the read base comp(t[x]) is not the 'A' a masked base packs as)
    gap_read = list(RC.revcomp(t[b:b + L]))
    gap_read[b + L - 1 - pos] = "N"
    blob = (t[a:a + L] + "".join(gap_read)).encode()
    recs1 = c["recs"][np.isin(c["recs"]["read"], [c["n_reads"] - 2, c["n_reads"] - 1])].copy()
    recs1["read"] -= c["n_reads"] - 2
    packed, nm = GapFill.pack_reads(blob, L, with_mask=True)
    d_reads1 = torch.from_numpy(np.concatenate([packed.reshape(-1), np.zeros(64, np.uint8)])).cuda()
    d_nm1 = torch.from_numpy(nm.reshape(-1).copy()).cuda()
    d_recs1 = torch.from_numpy(recs1.view(np.uint8).copy()).cuda()
    return {"d_reads": d_reads1, "d_recs": d_recs1, "d_nmask": d_nm1, "n_reads": 2, "text": blob.decode(), "n_at": b + L - 1 - pos}


def test_second_library_and_n_masked_read(hole):
    """Library order and N masks (definition 2 and 4): the bridges are library 0's gap read, then library 1's with its N — which never
    seeds, counts as a mismatch and is written as 'N' —, equal to gf_bridging_reads on the HQ reads of both libraries."""
    from gappadder_amd import _lib as B
    from gappadder_amd.assemble_gaps import bridging_reads_batch
    from gappadder_amd.pipeline import DeviceLibrary, Pipeline
    e1 = _two_lib_env(hole)
    pipe = Pipeline(hole["gf"], 1, L, [(31, 29)], merge_in_step=True, rescue_round=True)
    pipe.add_library(DeviceLibrary("a", 300, 30, hole["n_reads"], hole["d_reads"], hole["d_recs"]))
    pipe.add_library(DeviceLibrary("b", 300, 30, 2, e1["d_reads"], e1["d_recs"], d_nmask=e1["d_nmask"]))
    pipe.prepare()
    pipe.step()
    res = pipe.fetch()
    rs = res.rescue
    assert rs["gaps_tried"] == 1 and rs["bridges"] == 2 and rs["dropped"] == 0, rs
    got = [RC.contig_text(res, i) for i in _bridge_rows(res)]
    assert got == [hole["case"]["bridge"], e1["text"][L:]] and got[1][e1["n_at"]] == "N", (rs, got)
    # the host definition on both libraries' HQ reads, library 0 first
    rows0 = hole["d_reads"][:hole["n_reads"] * ((L + 3) // 4)].cpu().numpy().reshape(hole["n_reads"], -1)
    texts = [lambda r: _unpack(rows0[r:r + 1])[0], lambda r: e1["text"][r * L:(r + 1) * L]]
    reads = {}
    for l, (lb, recs_t) in enumerate(zip(pipe.libs, (hole["d_recs"], e1["d_recs"]))):
        th = np.frombuffer(lb.d_thits[:int(lb.d_cnt[4]) * 12].cpu().numpy().tobytes(), dtype=B.TAGHIT)
        recs = np.frombuffer(recs_t.cpu().numpy().tobytes(), dtype=B.ALNREC)
        for _, r, txt in RC.hq_reads(recs, th, 1, texts[l], lib=l).get(0, []):
            reads["%d_%d" % (l, r)] = txt
    assert rs["hq_reads"] == len(reads)
    want = bridging_reads_batch([(RC.alignment_set(res, 0, res.merge["contigs_before"], res.rescue_first), reads)])[0]
    assert [s_ for _, s_ in want] == got


@pytest.mark.parametrize("mode", ["exact", "align"])
def test_extended_fill_after_the_rescue_equals_the_host_twin(thin, mode):
    from gappadder_amd.pick_contigs import extension_order, pick_extended_sequence
    pipe, (res,) = _run(thin, merge_in_step=True, rescue_round=True, extended_fill=True, anchor_mode=mode)
    fills = pipe.extended_sequences(res)
    flanks, kk = thin["flanks"], pipe.kk
    want = {}
    for g in np.nonzero(res.best == 0)[0].tolist():
        rows = [i for i in range(len(res.contigs)) if int(res.contigs[i]["gap"]) == g and int(res.contigs[i]["length"])]
        cs = [(int(res.contigs[i]["k"]), int(res.contigs[i]["kv"]), RC.contig_text(res, i)) for i in rows]
        order = [rows[j] for j in extension_order(cs, kk)]
        r = pick_extended_sequence([("%d" % i, RC.contig_text(res, i)) for i in order], flanks[g][0], flanks[g][1], pipe.anchors[-1], mode)
        if r is not None:
            want[g] = (int(r[0]) if r[0] else -1, int(r[1]) if r[1] else -1, r[2], r[3])
    assert fills == want and len(want) == res.extended["gaps_extended"]


@pytest.mark.parametrize("kw, why", [(dict(), "rescue_round needs merge_in_step"), (dict(merge_in_step=True, world=2), "rescue_round runs on a single rank"),
                                     (dict(merge_in_step=True, force_exchange=True), "rescue_round runs on a single rank"),
                                     (dict(merge_in_step=True, second_round=True), "rescue_round with second_round")])
def test_refused_combinations(thin, kw, why):
    from gappadder_amd.pipeline import Pipeline
    with pytest.raises(ValueError, match=why):
        Pipeline(thin["gf"], len(thin["gaps"]), L, [(31, 29)], rescue_round=True, **kw)
