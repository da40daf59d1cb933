"""Pipeline(pileup=True) on the shared synthetic step (step_util): Results.pileup and the track against the host twin on the step's own
pools, contigs and picks — exact anchors, behind the merge round, and in align mode; nothing else of the step changes, the other rounds'
records included; fill_confidence against picked_sequences; a substitution planted in a fill shows as a minority column; the records-only
mode; what the constructor refuses."""
import numpy as np
import pytest

from step_util import L, contigs as _contigs, picks as _picks, run as _run, setup as _setup

pytestmark = pytest.mark.gpu

# name -> (gap length, k pairs, Pipeline options): 300-base gaps are closed by the first pick; of the 550-base gaps most stay open for the merge round
RUNS = {"exact": (300, [(31, 29), (41, 39)], {"anchor_mode": "exact"}),
        "align": (300, [(31, 29), (41, 39)], {"anchor_mode": "align"}),
        "merge": (550, [(31, 29)], {"merge_in_step": True})}
OTHERS = {"read_support": True, "polish": True, "pair_span": True}
_ENVS = {}


def _env(gap_len, kk):
    key = (gap_len, tuple(kk))
    if key not in _ENVS:
        _ENVS[key] = _setup(gap_len, kk)
    return _ENVS[key]


@pytest.fixture(scope="module", params=sorted(RUNS))
def pair(request):
    gap_len, kk, kw = RUNS[request.param]
    env = _env(gap_len, kk)
    on = _run(env, pools=True, pileup=True, **OTHERS, **kw)
    off = _run(env, pools=True, **OTHERS, **kw)
    return request.param, env, on, off


def test_pileup_equals_the_twin_on_the_steps_own_pools(pair):
    from gappadder_amd import pileup as PU
    name, env, (pipe, (res,)), _ = pair
    flanks = env[3]
    assert pipe.pileup.params == (16, 4, 48, 3, 80) and pipe.after_pick.index(pipe.pileup) == pipe.after_pick.index(pipe.polish) + 1
    assert pipe.after_pick.index(pipe.pairs) == pipe.after_pick.index(pipe.pileup) + 1
    want, tracks, stats = PU.pileup_of_results(res, flanks, L)
    closed = np.nonzero(res.best)[0]
    assert len(closed) and sorted(tracks) == closed.tolist() and stats["mismatches"] == 0
    assert res.pileup_track.shape == (stats["entries"], 8) and res.pileup_track.dtype == np.uint16
    bad, spans = [], []
    for g in range(len(want)):
        a = res.pileup[g].copy()
        o, n = int(a["off"]), int(a["len"])
        a["off"] = 0
        if a.tobytes() != want[g].tobytes() or (g in tracks and not (PU.track_of(res, g) == tracks[g]).all()) or (g not in tracks and (o or n)):
            bad.append(g)
        if g in tracks:
            spans.append((o, o + n))
    assert not bad, [(g, res.pileup[g], want[g]) for g in bad[:4]]
    assert res.pileup_stats == stats
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == len(res.pileup_track) and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    print("%s: %d of %d gaps closed, columns %d, low %d, minority %d, one strand %d, longest low run %d, rows placed %d, ambiguous %d"
          % (name, len(closed), len(res.best), int(res.pileup["n_cols"].sum()), stats["low"], int(res.pileup["n_minority"].sum()),
             int(res.pileup["n_one_strand"].sum()), int(res.pileup["low_run"].max()), stats["placed"], stats["ambiguous"]))
    assert stats["placed"] > 0
    # the polish places the same rows by the same rule
    assert (res.pileup["reads_placed"] == res.polish["reads_placed"]).all() and (res.pileup["reads_ambiguous"] == res.polish["reads_ambiguous"]).all()
    assert (res.pileup["n_uncovered"] == res.polish["n_uncovered"]).all()
    if name == "merge":
        assert res.merge is not None


def test_fill_confidence_has_an_entry_per_picked_base(pair):
    from gappadder_amd import pileup as PU
    from gappadder_amd.fill_rounds import _LUT
    _, _, (pipe, (res,)), _ = pair
    picked, conf = pipe.picked_sequences(res), pipe.fill_confidence(res)
    assert sorted(picked) == sorted(conf) == np.nonzero(res.best)[0].tolist()
    agree = total = 0
    for g, (ci, body, rev) in picked.items():
        cci, text, entries, crev = conf[g]
        assert (cci, text, crev) == (ci, body, rev) and entries.shape == (len(body), 8)
        codes = _LUT[np.frombuffer(body.encode(), dtype=np.uint8)].astype(np.int64)
        both = entries[:, :4].astype(np.int64) + entries[:, 4:]
        agree += int(both[np.arange(len(body)), codes].sum())                  # the entries are turned with the sequence: its own base leads
        total += int(both.sum())
        assert [PU.phred(e, b) for e, b in zip(entries[:3], body[:3])] == [min(40, 5 * max(0, 3 * int(x[c]) - 2 * int(x.sum()))) if x.sum() else 0
                                                                           for x, c in zip(both[:3], codes[:3])]
    assert total > 0 and agree > 0.98 * total


def _records(res):
    """Every contig record with its bases, order-free: two runs of the SAME step list the same records in different orders."""
    return sorted((int(c["gap"]), int(c["k"]), int(c["kv"]), int(c["n_nodes"]), int(c["length"]), int(c["cov_sum"]), s)
                  for c, (_, _, _, s) in zip(res.contigs, _contigs(res)))


def _by_bases(res, recs, strip=()):
    """Per closed gap the bytes of a round's record but for the fields `strip`, keyed by gap (a record names no contig index)."""
    out = {}
    for g in np.nonzero(res.best)[0]:
        a = recs[g].copy()
        for f in strip:
            a[f] = 0
        out[int(g)] = a.tobytes()
    return out


def _same_pool(off_a, rows_a, off_b, rows_b, ids_a=None, ids_b=None):
    """Two fetched pools: the offsets byte for byte; the rows (with their read ids) byte for byte where they come in one order, and as
    sorted rows per gap otherwise."""
    assert off_a.tobytes() == off_b.tobytes() and rows_a.shape == rows_b.shape and len(rows_a) == int(off_a[-1]) > 0
    if rows_a.tobytes() == rows_b.tobytes() and (ids_a is None or ids_a.tobytes() == ids_b.tobytes()):
        return
    for g in range(len(off_a) - 1):
        a, b = rows_a[int(off_a[g]):int(off_a[g + 1])], rows_b[int(off_b[g]):int(off_b[g + 1])]
        assert sorted(r.tobytes() for r in a) == sorted(r.tobytes() for r in b), g
        if ids_a is not None:
            assert sorted(ids_a[int(off_a[g]):int(off_a[g + 1])].tolist()) == sorted(ids_b[int(off_b[g]):int(off_b[g + 1])].tolist()), g


def test_the_round_changes_nothing_else(pair):
    """Contigs, picks, pools and the other rounds' records of the step with the round on against the step with it off: order-free
    where the step's contig order is unspecified, the bytes wherever the two lists do come in one order.  The pools are fetched AFTER
    the round read them, in every vote pass, from global memory."""
    from gappadder_amd import polish as PL
    _, _, (pipe, (res,)), (pipe_off, (ref,)) = pair
    assert ref.pileup is None and ref.pileup_track is None and ref.pileup_stats is None and pipe_off.pileup is None
    assert _records(res) == _records(ref) and len(res.seq) == len(ref.seq)
    assert _picks(res) == _picks(ref) and (res.best != 0).tobytes() == (ref.best != 0).tobytes()
    assert res.merge == ref.merge
    _same_pool(res.pool_off, res.pool_rows, ref.pool_off, ref.pool_rows)
    assert len(res.lib_pool_off) == len(ref.lib_pool_off) == 1
    for l in range(len(res.lib_pool_off)):
        _same_pool(res.lib_pool_off[l], res.lib_pool_rows[l], ref.lib_pool_off[l], ref.lib_pool_rows[l], res.lib_pool_ids[l], ref.lib_pool_ids[l])
    assert {g: v[1:] for g, v in pipe.picked_sequences(res).items()} == {g: v[1:] for g, v in pipe_off.picked_sequences(ref).items()}
    assert res.support.tobytes() == ref.support.tobytes() and res.support_stats == ref.support_stats
    assert _by_bases(res, res.polish, ("off",)) == _by_bases(ref, ref.polish, ("off",)) and res.polish_stats == ref.polish_stats
    assert {g: PL.polished_text(res, g) for g in np.nonzero(res.best)[0]} == {g: PL.polished_text(ref, g) for g in np.nonzero(ref.best)[0]}
    assert res.pairs.tobytes() == ref.pairs.tobytes() and res.pair_stats == ref.pair_stats
    if res.contigs.tobytes() == ref.contigs.tobytes():        # the same list order: then every byte is the same
        assert res.seq == ref.seq and res.best.tobytes() == ref.best.tobytes()


def test_a_planted_substitution_is_a_minority_column():
    """A base of the fill of every winning contig of the exact step replaced; the entry, on the step's pools and that list, has to mark the
    column — and no other column that was not marked before."""
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import pileup as PU
    from gappadder_amd import read_support as RS
    from gappadder_amd.pipeline import decode_best
    gap_len, kk, kw = RUNS["exact"]
    env = _env(gap_len, kk)
    pipe, (res,) = _run(env, pileup=True, **kw)
    seq, cols = bytearray(res.seq), {}
    for g in np.nonzero(res.best)[0]:
        ci = decode_best(res.best[g])[2]
        c = res.contigs[ci]
        text = res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])].decode()
        b0, b1 = RS.locate(res.best[g], text, env[3][g], None)
        j = (b0 + b1) // 2
        seq[int(c["seq_off"]) + j] = ord("ACGT"[("ACGT".index(text[j]) + 1 + g % 3) % 4])
        cols[int(g)] = (ci, j, b0)
    assert len(cols) == 24
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_ctg, d_seq = dev(res.contigs.view(np.uint8)), dev(np.frombuffer(bytes(seq), dtype=np.uint8))
    d_n, d_best = torch.tensor([len(res.contigs)], dtype=torch.int32, device="cuda"), dev(res.best.view(np.int64))
    d_rec = torch.zeros(len(res.best) * B.FILL_PILEUP.itemsize, dtype=torch.uint8, device="cuda")
    d_track = torch.zeros(len(seq) * 16, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(B.PU_WORDS, dtype=torch.int32, device="cuda")
    pipe._chk(pipe.lib.gf_fill_pileup_dev(pipe.h, pipe.asm_ptr, None, pipe.asm_off, pipe.asm_rows, L, d_ctg.data_ptr(), d_n.data_ptr(), len(res.contigs),
                                          d_seq.data_ptr(), d_best.data_ptr(), None, *pipe.anchor_pair, *pipe.pileup.params, d_rec.data_ptr(),
                                          d_track.data_ptr(), len(seq), d_st.data_ptr()), "gf_fill_pileup_dev")
    pipe.barrier()
    rec = np.frombuffer(d_rec.cpu().numpy().tobytes(), dtype=B.FILL_PILEUP)
    track = np.frombuffer(d_track.cpu().numpy().tobytes(), dtype="<u2").reshape(-1, 8)
    stats = PU.stats_of(d_st.cpu().numpy())
    assert stats["mismatches"] == 0 and stats["gaps"] == 24 and stats["overflow"] == 0
    marked = 0
    for g, (ci, j, b0) in cols.items():
        base = chr(seq[int(res.contigs[ci]["seq_off"]) + j])
        e = track[int(rec[g]["off"]) + j]
        before = PU.track_of(res, g)[j]
        assert int(rec[g]["len"]) == int(res.contigs[ci]["length"])
        if int(before.sum()) and not PU.is_minority(before, chr(res.seq[int(res.contigs[ci]["seq_off"]) + j])):
            assert PU.is_minority(e, base) and PU.phred(e, base) == 0, (g, j, e, before)
            assert int(rec[g]["n_minority"]) == int(res.pileup[g]["n_minority"]) + 1
            marked += 1
    assert marked > 12


def test_records_only_mode_and_what_the_constructor_refuses():
    from gappadder_amd.pipeline import Pipeline
    gap_len, kk, kw = RUNS["exact"]
    env = _env(gap_len, kk)
    pipe, (res,) = _run(env, pileup=True, pileup_track=False, **kw)
    full = _run(env, pileup=True, **kw)[1][0]
    assert res.pileup_track is None and pipe.pileup.d_track is None and res.pileup_stats == dict(full.pileup_stats, entries=0)
    want = full.pileup.copy()
    want["off"] = want["len"] = 0
    assert res.pileup.tobytes() == want.tobytes() and full.pileup["len"].sum() == full.pileup_stats["entries"] > 0
    with pytest.raises(ValueError, match="track"):
        pipe.fill_confidence(res)
    gf = env[0]
    with pytest.raises(ValueError, match="pileup with second_round"):
        Pipeline(gf, 24, L, [(31, 29)], pileup=True, second_round=True)
    with pytest.raises(ValueError, match="pileup runs on a single rank"):
        Pipeline(gf, 24, L, [(31, 29)], pileup=True, world=2)
    with pytest.raises(ValueError, match="pileup"):
        Pipeline(gf, 24, L, [(31, 29)], pileup=True, pileup_seed=40)
    with pytest.raises(ValueError, match="pileup"):
        Pipeline(gf, 24, L, [(31, 29)], pileup=True, pileup_min_agree=0)
