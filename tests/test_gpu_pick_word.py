"""The saturated span of the pick word (csrc/pick_word.hpp; the definition: csrc/pick.hip, the host's codec: pipeline.decode_best): a
fill of more than 0xFFFFFF - 1 bases leaves the span field at 0xFFFFFF, which still outranks every shorter span, and a reader of the word
takes a saturated field for "at least that long" instead of a mismatch.  Exact anchors, forward and reverse; the word through
gf_pick_anchored2_dev, through read_support.locate (the host twin of fill_body.hpp) and through the device's fill_body in
gf_fill_polish_dev with an empty pool."""
import numpy as np
import pytest

import pick_util as PK

pytestmark = pytest.mark.gpu

BODY = (1 << 24) + 5                       # span + 1 = 2^24 + 6 > 0xFFFFFF
SAT = 0xFFFFFF
L = 150


def _rand(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()


def _closing(rng, left, right, body):
    """50 random + the left flank's gap-side end + body + the right flank's start + 40 random: the body lies at [90, 90 + body)."""
    return _rand(rng, 50) + left[-40:] + _rand(rng, body) + right[:40] + _rand(rng, 40)


def test_a_saturated_span_wins_the_pick_and_is_no_mismatch_to_its_readers():
    import torch
    from gappadder_amd import _lib as B
    from gappadder_amd import pipeline as P
    from gappadder_amd import polish as PL
    from gappadder_amd import read_support as SUP
    from gappadder_amd.hip_api import GapFill
    rng = np.random.default_rng(2406)
    flanks = [(PK.rand_seq(rng, 120), PK.rand_seq(rng, 120)) for _ in range(2)]
    short0 = _closing(rng, *flanks[0], 300)
    long0 = _closing(rng, *flanks[0], BODY)
    long1 = PK._rc(_closing(rng, *flanks[1], BODY))
    recs = [(0, short0), (0, long0), (1, long1)]             # the short contig of gap 0 is listed first
    want = {0: (1, 0, (90, 90 + BODY)), 1: (2, 1, (80, 80 + BODY))}       # gap: contig, strand, body in the stored orientation
    n = len(recs)
    ctg = np.zeros(n, dtype=B.CONTIG)
    o = 0
    for i, (g, s) in enumerate(recs):
        ctg[i] = (g, 31, 29, 1, len(s), 0, 0, o)
        o += len(s)
    gaps = np.zeros(2, dtype=B.GAP)
    for g in range(2):
        gaps[g] = (0, 20000 * (g + 1), 20000 * (g + 1) + 100, g + 1)
    gf = GapFill(0)
    gf.set_gaps(gaps, 1, flanks)
    lib = B.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    d_ctg, d_seq = dev(ctg.view(np.uint8)), dev(np.frombuffer("".join(s for _, s in recs).encode(), dtype=np.uint8))
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    d_best = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_closed = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.gf_pick_anchored2_dev(gf.handle, d_ctg.data_ptr(), d_n.data_ptr(), n, d_seq.data_ptr(), 30, 15, d_best.data_ptr(),
                                     d_closed.data_ptr()) == 0
    gf.sync()
    best = d_best.cpu().numpy().view(np.uint64)
    print("words", [hex(int(b)) for b in best], "closed", int(d_closed.cpu()[0]))
    assert int(d_closed.cpu()[0]) == 2
    for g, (ci, rev, body) in want.items():
        assert P.decode_best(best[g]) == (30, SAT, ci, rev), (g, P.decode_best(best[g]))
        # the host twin of fill_body: its `span >= span1` branch
        assert SUP.locate(best[g], recs[ci][1], flanks[g], None) == body, g

    # the device's fill_body, through the polish with an empty pool: a long contig is copied out unpolished, not a mismatch
    base_cap = sum(len(recs[ci][1]) for ci, _, _ in want.values())
    d_off = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_pool = torch.zeros(256, dtype=torch.uint8, device="cuda")
    d_out = torch.full((2 * B.FILL_POLISH.itemsize,), 0x55, dtype=torch.uint8, device="cuda")
    d_bases = torch.full((base_cap + 256,), 0x2E, dtype=torch.uint8, device="cuda")
    d_st = torch.full((B.PL_WORDS,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.gf_fill_polish_dev(gf.handle, d_pool.data_ptr(), None, d_off.data_ptr(), 0, L, d_ctg.data_ptr(), d_n.data_ptr(), n,
                                d_seq.data_ptr(), d_best.data_ptr(), None, 30, 15, PL.SEED, PL.MAX_MISMATCH, PL.MIN_OVERLAP, PL.MIN_VOTES,
                                d_out.data_ptr(), d_bases.data_ptr(), base_cap, d_st.data_ptr())
    assert rc == 0, (rc, lib.gf_last_error(gf.handle))
    gf.sync()
    got = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=B.FILL_POLISH)
    st = PL.stats_of(d_st.cpu().numpy())
    bases = d_bases.cpu().numpy()
    print("polish", got, st)
    assert st == dict.fromkeys(PL.STAT_KEYS, 0) | {"skipped_long": 2, "bases": base_cap}
    spans = []
    for g, (ci, rev, body) in want.items():
        text, rec = PL.polish_host([], recs[ci][1], *body)
        assert int(rec["flags"]) == B.PL_F_LONG and int(rec["n_cols"]) == BODY and text == recs[ci][1]
        assert all(int(got[g][f]) == int(rec[f]) for f in B.FILL_POLISH.names if f != "off"), (g, got[g], rec)     # (off: in the order of arrival)
        off = int(got[g]["off"])
        assert bases[off:off + len(text)].tobytes() == text.encode(), g
        spans.append((off, off + len(text)))
    (lo0, hi0), (lo1, hi1) = sorted(spans)
    assert lo0 == 0 and hi0 == lo1 and hi1 == base_cap and set(bases[base_cap:].tolist()) == {0x2E}
    gf.close()
