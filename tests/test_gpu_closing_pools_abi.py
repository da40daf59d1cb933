"""gf_closing_pools_dev (csrc/closing_pools.hip) on hand-made device buffers against second_round.closing_pools_host gathered in numpy:
offsets, row bytes, masks, ids, libraries and statistics, exactly, with guard bytes around every output.  The sorted keys and the flag
scan are left by the existing pools calls (round 1's; a gated later round behind it), as they are in the step."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0x5A
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


def _guarded(n_bytes, fill=GUARD, guard=256):
    import torch
    t = torch.full((guard + n_bytes + guard,), GUARD, dtype=torch.uint8, device="cuda")
    if fill != GUARD:
        t[guard:guard + n_bytes] = fill
    return t, t.data_ptr() + guard


def _payload(t, guard=256):
    return t[guard:len(t) - guard].cpu().numpy()


def _guards_intact(t, guard=256):
    h = t.cpu().numpy()
    return bool((h[:guard] == GUARD).all() and (h[len(h) - guard:] == GUARD).all())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _key(g, l, p):
    return (np.asarray(g, dtype=np.uint64) << np.uint64(40)) | (np.asarray(l, dtype=np.uint64) << np.uint64(36)) | np.asarray(p, dtype=np.uint64)


class _Case:
    """Libraries, a source pool and a key list; the keys go through gf_round2_pools_dev, which leaves d_sorted and d_work."""

    def __init__(self, gf, seed, n_gaps, L, n_lib, src_mask, lib_mask, n_keys=300, n_pairs=500, pad=0, gated=False):
        import torch
        from gappadder_amd import _lib as B
        rng = np.random.default_rng(seed)
        self.gf, self.lib, self.B, self.n_gaps, self.L, self.n_lib = gf, B.lib(), B, n_gaps, L, n_lib
        self.rb, self.mw = int(self.lib.gf_packed_read_bytes(L)), (L + 31) // 32
        self.reads = [rng.integers(0, 256, size=(2 * n_pairs, self.rb), dtype=np.uint8) for _ in range(n_lib)]
        # lib_mask: "all", "some" (library 0 has none) or None
        self.masks = [rng.integers(0, 1 << 32, size=(2 * n_pairs, self.mw), dtype=np.uint32) if lib_mask == "all" or (lib_mask == "some" and l) else None
                      for l in range(n_lib)]
        self.d_reads = [_dev(r) for r in self.reads]
        self.d_masks = [_dev(m) if m is not None else None for m in self.masks]
        self.lib_ptrs = (C.c_void_p * n_lib)(*[t.data_ptr() for t in self.d_reads])
        self.mask_ptrs = (C.c_void_p * n_lib)(*[t.data_ptr() if t is not None else None for t in self.d_masks]) if lib_mask else None
        n_src = rng.integers(0, 9, size=n_gaps)
        if n_gaps > 2:
            n_src[1] = 0                     # a gap without step rows (closed below)
        else:
            n_src[-1] = max(n_src[-1], 3)    # (the one closed gap of the small shapes has step rows)
        self.src_off = np.concatenate([[0], np.cumsum(n_src)]).astype(np.int64)
        n = int(self.src_off[-1])
        self.src = rng.integers(0, 256, size=(n, self.rb), dtype=np.uint8)
        self.src_nm = rng.integers(0, 1 << 32, size=(n, self.mw), dtype=np.uint32) if src_mask else None
        self.src_ids = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        self.d_src, self.d_src_off, self.d_src_ids = _dev(np.concatenate([self.src.reshape(-1), np.zeros(8, np.uint8)])), _dev(self.src_off), _dev(self.src_ids) if n else _dev(np.zeros(1, np.uint32))
        self.d_src_nm = _dev(np.concatenate([self.src_nm.reshape(-1), np.zeros(1, np.uint32)])) if src_mask else None
        # keys over every gap and library with repeats, the same pair in two libraries, and two of gaps beyond n_gaps
        g, l, p = rng.integers(0, n_gaps, size=n_keys), rng.integers(0, n_lib, size=n_keys), rng.integers(0, min(n_pairs, 60), size=n_keys)
        k = _key(g, l, p)
        k = np.concatenate([k, k[:n_keys // 8], _key(g[:20], (l[:20] + 1) % n_lib, p[:20]), _key([n_gaps, n_gaps + 3], [0, n_lib - 1], [5, 6])])
        if n_gaps > 1:      # gap 0 (open below) and gap 1 (closed, no step rows) hold a key of every library
            k = np.concatenate([k, _key([0] * n_lib + [1] * n_lib, list(range(n_lib)) * 2, [7] * (2 * n_lib))])
        self.hits = k[rng.permutation(len(k))]
        self.key_cap = len(self.hits) + pad         # pad == 0: the keys end exactly at key_cap
        self.tuples = [(int(x) >> 40, (int(x) >> 36) & 15, int(x) & ((1 << 36) - 1)) for x in self.hits]
        keys = _dev(np.concatenate([self.hits, np.full(pad, EMPTY, dtype=np.uint64)]))
        self.sorted, self.p_sorted = _guarded(8 * self.key_cap)
        self.rwork, self.p_rwork = _guarded(4 * int(self.lib.gf_round2_work_words(self.key_cap, n_gaps)))
        rows = torch.zeros(2 * (n_gaps + 1), dtype=torch.int64, device="cuda")
        st = torch.zeros(2 * B.R2_WORDS, dtype=torch.int32, device="cuda")
        self.d_best = torch.zeros(n_gaps, dtype=torch.int64, device="cuda")        # (every gap open while the rounds run)
        assert self.lib.gf_round2_pools_dev(gf.handle, keys.data_ptr(), self.p_sorted, self.key_cap, self.lib_ptrs, n_lib, L, self.d_src.data_ptr(),
                                            self.d_src_off.data_ptr(), self.d_best.data_ptr(), n_gaps, self.p_rwork, rows.data_ptr(), None, 0,
                                            st.data_ptr()) == 0
        if gated:       # a later round that the round before's GROWN word gates: other keys in the key buffer, nothing carried out
            junk = _dev(_key(rng.integers(0, n_gaps, size=self.key_cap), 0, rng.integers(0, 50, size=self.key_cap)))
            dead = torch.zeros(1, dtype=torch.int32, device="cuda")
            prev = torch.zeros(n_gaps, dtype=torch.int32, device="cuda")
            assert self.lib.gf_round_pools_dev(gf.handle, junk.data_ptr(), self.p_sorted, self.key_cap, self.lib_ptrs, n_lib, L, self.d_src.data_ptr(),
                                               self.d_src_off.data_ptr(), self.d_best.data_ptr(), n_gaps, prev.data_ptr(), self.p_rwork,
                                               rows.data_ptr() , None, 0, st.data_ptr() + 4 * B.R2_WORDS, dead.data_ptr()) == 0
        gf.sync()

    def expected(self, best, filt, src_lib, with_ids):
        from gappadder_amd.second_round import closing_pools_host
        pools = closing_pools_host(np.diff(self.src_off).tolist(), best.tolist(), self.tuples, None if filt < 0 else filt)
        off = np.concatenate([[0], np.cumsum([len(p) for p in pools])]).astype(np.int64)
        n = int(off[-1])
        rows, nm = np.zeros((n, self.rb), np.uint8), np.zeros((n, self.mw), np.uint32)
        ids, libs = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        i = 0
        for g, p in enumerate(pools):
            for l, x in p:
                if l < 0:
                    s = int(self.src_off[g]) + x
                    rows[i], ids[i], libs[i] = self.src[s], self.src_ids[s] if with_ids else 0xFFFFFFFF, src_lib & 0xFF
                    if self.src_nm is not None:
                        nm[i] = self.src_nm[s]
                else:
                    rows[i], ids[i], libs[i] = self.reads[l][x], x, l
                    if self.masks[l] is not None:
                        nm[i] = self.masks[l][x]
                i += 1
        recruited = sum(1 for p in pools for l, _ in p if l >= 0)
        return {"off": off, "rows": rows, "nm": nm, "ids": ids, "libs": libs, "n": n, "gaps": sum(1 for p in pools if p), "recruited": recruited}

    def run(self, best, filt, pool_cap, want_masks, want_ids, src_ids=True, src_lib=0):
        """-> (offsets, rows, masks, ids, libraries, statistics, all guards intact?) of one call."""
        B, n_gaps = self.B, self.n_gaps
        self.d_best.copy_(_dev(best))
        room = max(1, pool_cap)
        off, p_off = _guarded(8 * (n_gaps + 1))
        pool, p_pool = _guarded(room * self.rb)
        nm, p_nm = _guarded(room * self.mw * 4)
        ids, p_ids = _guarded(room * 4)
        libs, p_libs = _guarded(room)
        st, p_st = _guarded(4 * B.CP_WORDS)
        work, p_work = _guarded(4 * int(self.lib.gf_closing_pools_work_words(n_gaps)))
        rc = self.lib.gf_closing_pools_dev(self.gf.handle, self.p_sorted, self.p_rwork, self.key_cap, self.lib_ptrs, self.mask_ptrs, self.n_lib, filt, self.L,
                                           self.d_src.data_ptr(), self.d_src_off.data_ptr(), self.d_src_nm.data_ptr() if self.d_src_nm is not None else None,
                                           self.d_src_ids.data_ptr() if src_ids else None, src_lib, self.d_best.data_ptr(), n_gaps, p_work, p_off,
                                           p_pool, pool_cap, p_nm if want_masks else None, p_ids if want_ids else None, p_libs if want_ids else None, p_st)
        assert rc == 0
        self.gf.sync()
        ok = all(_guards_intact(t) for t in (off, pool, nm, ids, libs, st, work, self.sorted, self.rwork))
        return (_payload(off).view(np.int64), _payload(pool), _payload(nm).view(np.uint32), _payload(ids).view(np.uint32), _payload(libs),
                _payload(st).view(np.uint32), ok)

    def check(self, best, filt, want_masks=True, want_ids=True, src_ids=True, src_lib=0):
        """The call with exactly the rows it needs, then with one row less."""
        B = self.B
        w = self.expected(best, filt, src_lib, src_ids)
        n = w["n"]
        off, pool, nm, ids, libs, st, ok = self.run(best, filt, n, want_masks, want_ids, src_ids, src_lib)
        assert ok
        assert off.tolist() == w["off"].tolist()
        assert pool[:n * self.rb].tobytes() == w["rows"].tobytes() and (pool[n * self.rb:] == GUARD).all()
        if want_masks:
            assert nm[:n * self.mw].tolist() == w["nm"].reshape(-1).tolist()
        else:
            assert (nm.view(np.uint8) == GUARD).all()
        if want_ids:
            assert ids[:n].tolist() == w["ids"].tolist() and libs[:n].tolist() == w["libs"].tolist()
        else:
            assert (ids.view(np.uint8) == GUARD).all() and (libs == GUARD).all()
        assert (int(st[B.CP_ROWS]) | int(st[B.CP_ROWS + 1]) << 32, int(st[B.CP_GAPS]), int(st[B.CP_RECRUITED]), int(st[B.CP_OVF])) == \
            (n, w["gaps"], w["recruited"], 0)
        assert not st[5:].any()
        if n:       # one row short: the flag, every pool empty, nothing written anywhere
            off, pool, nm, ids, libs, st, ok = self.run(best, filt, n - 1, want_masks, want_ids, src_ids, src_lib)
            assert ok and not off.any()
            assert all((a.view(np.uint8) == GUARD).all() for a in (pool, nm, ids, libs))
            assert (int(st[B.CP_ROWS]) | int(st[B.CP_ROWS + 1]) << 32, int(st[B.CP_GAPS]), int(st[B.CP_RECRUITED]), int(st[B.CP_OVF])) == (n, 0, 0, 1)
        return w


def _best(n_gaps, seed, closed=0.6):
    """Pick words: nonzero for the closed gaps — gap 1 (no step rows) among them, gap 0 open when there is more than one gap."""
    rng = np.random.default_rng(seed)
    b = np.where(rng.random(n_gaps) < closed, np.int64(1) << 56 | 5, 0).astype(np.int64)
    if n_gaps > 1:
        b[0], b[1] = 0, 1 << 56
    else:
        b[0] = 1 << 56
    return b


# (n_gaps, read length, libraries, library filter, source masks, library masks, ids, gated)
SHAPES = [(1, 150, 1, -1, False, None, True, False),
          (2, 150, 3, -1, True, "all", True, False),
          (257, 150, 3, -1, False, "some", True, False),
          (257, 150, 3, 1, True, None, True, False),
          (257, 150, 3, 1, False, "all", False, True),
          (257, 33, 3, -1, True, "some", True, True),
          (2, 33, 1, -1, False, None, False, False),
          (257, 4, 3, 1, True, "all", True, False),
          (1, 4, 1, -1, False, "all", True, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "g%d-L%d-n%d-f%d-%s-%s-%s-%s" % s)
def test_the_call_equals_the_twin(gf, shape):
    n_gaps, L, n_lib, filt, src_mask, lib_mask, with_ids, gated = shape
    # pad 0: the keys end exactly at key_cap (every other shape leaves empty keys behind them)
    c = _Case(gf, 100 + n_gaps + L, n_gaps, L, n_lib, src_mask, lib_mask, pad=0 if n_gaps != 2 else 37, gated=gated)
    best = _best(n_gaps, 7 + L)
    want_masks = bool(src_mask or lib_mask)
    w = c.check(best, filt, want_masks=want_masks, want_ids=with_ids, src_ids=with_ids, src_lib=max(filt, 0))
    assert 0 < w["recruited"] < w["n"]
    if n_gaps > 2:
        # the closed gap without step rows holds recruits alone; the open gap 0 has keys and no pool
        assert w["off"][1] == w["off"][0] == 0 and any(t[0] == 0 for t in c.tuples)
        assert w["off"][2] - w["off"][1] == 2 * len({t[1:] for t in c.tuples if t[0] == 1 and (filt < 0 or t[1] == filt)}) > 0


def test_masks_asked_for_where_no_source_has_one_are_zero_and_ids_without_source_ids(gf):
    c = _Case(gf, 5, 64, 150, 2, False, None, pad=11)
    w = c.check(_best(64, 3), -1, want_masks=True, want_ids=True, src_ids=False, src_lib=-1)
    assert not w["nm"].any() and (w["libs"] == 0xFF).any() and (w["ids"] == 0xFFFFFFFF).any()


def test_no_closed_gap_and_every_gap_closed(gf):
    c = _Case(gf, 9, 33, 150, 3, True, "all", pad=5)
    w = c.check(np.zeros(33, dtype=np.int64), -1)
    assert w["n"] == 0 and w["gaps"] == 0 and not w["off"].any()
    w = c.check(np.full(33, 1 << 56, dtype=np.int64), 2)
    assert w["gaps"] > 0 and w["recruited"] == 2 * len({t for t in c.tuples if t[0] < 33 and t[1] == 2})
