"""The entry points of recruitment rounds 2 and later (csrc/round_n.hip) on their own, against numpy / Python definitions written here:
the k-mer table of the contigs from an index on (through the table's entries and the recruitment's keys), the key carry and the round's
pools on synthetic key lists, and the gate.  Guard bytes surround every output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0x5A
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
PAIR_MASK = np.uint64((1 << 36) - 1)
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_RC = str.maketrans("ACGT", "TGCA")


@pytest.fixture(scope="module")
def gf():
    from gappadder_amd.hip_api import GapFill
    g = GapFill(0)
    yield g
    g.close()


def _guarded(n_bytes, fill=GUARD, guard=256):
    """A device byte buffer of n_bytes between two guards (-> whole tensor, address of the payload)."""
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


def _put(ptr_tensor, a, guard=256):
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    ptr_tensor[guard:guard + len(b)] = torch.from_numpy(b.copy()).cuda()


def _rand_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def _canon(w):
    c = min(w, w[::-1].translate(_RC))
    v = 0
    for j, ch in enumerate(c):
        v |= _CODE[ch] << (126 - 2 * j)
    return v >> 64, v & ((1 << 64) - 1)


def _kmers(s, k):
    for p in range(len(s) - k + 1):
        w = s[p:p + k]
        if all(ch in _CODE for ch in w):
            yield _canon(w)


# ---- the table from an index on ----------------------------------------------------------------------------------------------------

N_GAPS_T, CLOSED_T, LOG2_T, L_T = 5, 4, 17, 100


def _contig_list(rng, k):
    """[(gap, text)] over the gaps 0-3 (open) and 4 (closed): a dozen contigs of 200-400 bases, a tombstone, one shorter than k, one of
    exactly k bases, two with an N, two of the closed gap, and one of 9 000 bases: a lane rolls runs of 8 positions and a wave covers 512
    per trip, so every contig here crosses run boundaries and the long one many trip boundaries."""
    lst = [(int(rng.integers(0, 4)), _rand_seq(rng, int(rng.integers(200, 401)))) for _ in range(12)]
    lst += [(1, ""), (2, _rand_seq(rng, k - 1)), (3, _rand_seq(rng, k)), (CLOSED_T, _rand_seq(rng, 300)), (CLOSED_T, _rand_seq(rng, 250))]
    for g in (0, 2):
        s = _rand_seq(rng, 300)
        q = int(rng.integers(k, 300 - k))
        lst.append((g, s[:q] + "N" + s[q + 1:]))
    lst.append((1, _rand_seq(rng, 9000)))
    return [lst[i] for i in rng.permutation(len(lst))]


def _upload_contigs(lst):
    import torch
    from gappadder_amd import _lib as B
    ctg = np.zeros(len(lst), dtype=B.CONTIG)
    o = 0
    for i, (g, s) in enumerate(lst):
        ctg[i]["gap"], ctg[i]["k"], ctg[i]["kv"], ctg[i]["n_nodes"], ctg[i]["length"] = g, 31, 29, max(1, len(s) - 28), len(s)
        ctg[i]["seq_off"] = o if s else 0
        o += len(s)
    blob = np.frombuffer("".join(s for _, s in lst).encode() + b"\0" * 64, dtype=np.uint8)
    return torch.from_numpy(ctg.view(np.uint8).copy()).cuda(), torch.from_numpy(blob.copy()).cuda()


def _reads_for(rng, lst, k, n):
    """Reads cut from the contigs (either strand, some running off the end into noise, some with an N-masked run) and strangers."""
    texts = [s for _, s in lst if len(s) >= k]
    reads = []
    for i in range(n):
        if i % 4 == 3:
            r = _rand_seq(rng, L_T)
        else:
            s = texts[int(rng.integers(0, len(texts)))]
            a = int(rng.integers(0, max(1, len(s) - k)))
            r = (s[a:a + L_T].replace("N", "A") + _rand_seq(rng, L_T))[:L_T]
            if rng.integers(0, 2):
                r = r[::-1].translate(_RC)
        if rng.integers(0, 3) == 0:
            p, w = int(rng.integers(0, L_T)), int(rng.integers(1, 6))
            r = (r[:p] + "N" * w + r[p + w:])[:L_T]
        reads.append(r)
    return reads


@pytest.fixture(scope="module", params=[31, 51])
def table_case(request, gf):
    """Contigs, reads, and per read the canonical k-mers — computed once per k."""
    import torch
    from gappadder_amd.hip_api import GapFill
    k = request.param
    rng = np.random.default_rng(700 + k)
    lst = _contig_list(rng, k)
    reads = _reads_for(rng, lst, k, 600)
    packed, nm = GapFill.pack_reads("".join(reads).encode(), L_T, with_mask=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    n_pairs = len(reads) // 2
    d = {"k": k, "lst": lst, "reads": reads, "read_kmers": [set(_kmers(r, k)) for r in reads],
         "contig_kmers": [set(_kmers(s, k)) if len(s) >= k else set() for _, s in lst], "d_reads": dev(packed.reshape(-1)),
         "d_nm": dev(nm.reshape(-1).view(np.int32)), "d_pairs": dev(np.arange(n_pairs, dtype=np.int32)[::-1]),
         "d_np": torch.tensor([n_pairs], dtype=torch.int32, device="cuda"), "n_pairs": n_pairs}
    d["d_ctg"], d["d_seq"] = _upload_contigs(lst)
    best = np.zeros(N_GAPS_T, dtype=np.int64)
    best[CLOSED_T] = 1 << 56
    d["best"], d["d_best"] = best, dev(best)
    return d


def _table_and_keys(gf, c, first, cap, existing=False):
    """-> (table entries {(hi, lo, gap)}, recruited {(gap, pair)}, statistics) of one table build and one recruitment."""
    import torch
    from gappadder_amd import _lib as B
    lib, k = B.lib(), c["k"]
    tab, p_tab = _guarded(24 << LOG2_T)
    st, p_st = _guarded(4 * B.R2_WORDS, fill=0)
    d_n = torch.tensor([len(c["lst"])], dtype=torch.int32, device="cuda")
    d_first = torch.tensor([first], dtype=torch.int32, device="cuda")
    if existing:
        assert lib.gf_contig_kmer_table_dev(gf.handle, c["d_ctg"].data_ptr(), d_n.data_ptr(), cap, c["d_seq"].data_ptr(), c["d_best"].data_ptr(),
                                            N_GAPS_T, k, p_tab, LOG2_T, p_st) == 0
    else:
        assert lib.gf_contig_kmer_table_from_dev(gf.handle, c["d_ctg"].data_ptr(), d_n.data_ptr(), cap, c["d_seq"].data_ptr(), c["d_best"].data_ptr(),
                                                 N_GAPS_T, k, d_first.data_ptr(), p_tab, LOG2_T, p_st, None) == 0
    key_cap = 1 << 15
    keys, p_keys = _guarded(8 * key_cap, fill=0xFF)
    assert lib.gf_recruit_by_contigs_dev(gf.handle, c["d_reads"].data_ptr(), c["d_nm"].data_ptr(), len(c["reads"]), L_T, c["d_pairs"].data_ptr(),
                                         c["d_np"].data_ptr(), c["n_pairs"], 2, k, p_tab, LOG2_T, p_keys, key_cap, p_st) == 0
    gf.sync()
    assert _guards_intact(tab) and _guards_intact(st) and _guards_intact(keys)
    slot = np.dtype([("hi", "<u8"), ("lo", "<u8"), ("gap", "<u4"), ("state", "<u4")])
    t = np.frombuffer(_payload(tab).tobytes(), dtype=slot)
    assert set(np.unique(t["state"]).tolist()) <= {0, 2}
    t = t[t["state"] == 2]
    entries = [(int(a), int(b), int(g)) for a, b, g in zip(t["hi"], t["lo"], t["gap"])]
    assert len(entries) == len(set(entries))
    kk = _payload(keys).view(np.uint64)
    kk = kk[kk != EMPTY]
    assert (((kk >> np.uint64(36)) & np.uint64(15)) == 2).all()
    stats = _payload(st).view(np.uint32)
    assert int(stats[B.R2_HITS]) == len(kk) <= key_cap and int(stats[B.R2_TAB_FULL]) == 0
    return set(entries), {(int(x) >> 40, int(x) & ((1 << 36) - 1)) for x in kk}, stats


def _expected(c, first, cap):
    table = {}
    n_pos = 0
    for i in range(first, min(len(c["lst"]), cap)):
        g = c["lst"][i][0]
        if c["best"][g] == 0:
            s = c["lst"][i][1]
            n_pos += sum(1 for p in range(len(s) - c["k"] + 1) if all(ch in _CODE for ch in s[p:p + c["k"]]))
            for km in c["contig_kmers"][i]:
                table.setdefault(km, set()).add(g)
    entries = {(hi, lo, g) for (hi, lo), gs in table.items() for g in gs}
    keys = {(g, i // 2) for i, ks in enumerate(c["read_kmers"]) for km in ks & table.keys() for g in table[km]}
    return entries, keys, n_pos


def test_table_from_an_index_equals_the_definition_and_the_existing_entry(gf, table_case):
    from gappadder_amd import _lib as B
    c = table_case
    n = len(c["lst"])
    long_at = next(i for i, (_, s) in enumerate(c["lst"]) if len(s) == 9000)
    exact_at = next(i for i, (_, s) in enumerate(c["lst"]) if len(s) == c["k"])
    seen_nonempty = 0
    for first, cap in ((0, n), (n // 2, n), (long_at, n), (exact_at, n), (n - 1, n), (n, n), (n + 7, n), (0, n - 3), (n - 5, n - 3), (n - 2, n - 3)):
        ent, keys, st = _table_and_keys(gf, c, first, cap)
        want_ent, want_keys, n_pos = _expected(c, first, cap)
        assert ent == want_ent, (first, cap, len(ent), len(want_ent))
        assert keys == want_keys, (first, cap, len(keys), len(want_keys))
        assert int(st[B.R2_KMERS]) == n_pos, (first, cap)
        seen_nonempty += bool(want_keys)
        if first >= min(n, cap):
            assert not ent and not keys
        if first == 0:          # the whole list: the existing entry's table, keys and count
            ent0, keys0, st0 = _table_and_keys(gf, c, 0, cap, existing=True)
            assert ent0 == ent and keys0 == keys and int(st0[B.R2_KMERS]) == n_pos
    assert seen_nonempty >= 5
    # the closed gap, the tombstone, the short contig and the k-mers over an N are what the definition leaves out: they are in the list
    ent, keys, _ = _table_and_keys(gf, c, 0, n)
    assert CLOSED_T not in {g for _, _, g in ent} and {g for g, _ in keys} == {0, 1, 2, 3}
    exact = c["lst"][exact_at]
    assert _canon(exact[1]) + (exact[0],) in ent


# ---- carry + pools on synthetic key lists ------------------------------------------------------------------------------------------

N_GAPS, L_P, N_LIB = 6, 50, 2
CLOSED, STALE, BY_ONE = 1, 2, 3           # closed with keys; open, no new pair; open, exactly one new pair


def _key(g, lib, pair):
    return (np.asarray(g, dtype=np.uint64) << np.uint64(40)) | (np.asarray(lib, dtype=np.uint64) << np.uint64(36)) | np.asarray(pair, dtype=np.uint64)


def _gap(keys):
    return (keys >> np.uint64(40)).astype(np.int64)


class _Rig:
    """The buffers of a round, each between guards, and the numpy definition of what a round leaves in them."""

    def __init__(self, gf, rng, n_pairs, key_cap, pool_cap):
        import ctypes as C
        import torch
        from gappadder_amd import _lib as B
        self.gf, self.lib, self.B = gf, B.lib(), B
        self.rb = int(self.lib.gf_packed_read_bytes(L_P))
        self.key_cap, self.pool_cap, self.n_pairs = key_cap, pool_cap, n_pairs
        self.reads = [rng.integers(0, 256, size=(2 * n_pairs, self.rb), dtype=np.uint8) for _ in range(N_LIB)]
        self.d_reads = [torch.from_numpy(r.copy()).cuda() for r in self.reads]
        self.lib_ptrs = (C.c_void_p * N_LIB)(*[t.data_ptr() for t in self.d_reads])
        r1 = rng.integers(1, 9, size=N_GAPS)
        self.asm_off = np.concatenate([[0], np.cumsum(r1)]).astype(np.int64)
        self.asm_pool = rng.integers(0, 256, size=(int(self.asm_off[-1]), self.rb), dtype=np.uint8)
        self.d_asm_pool, self.d_asm_off = torch.from_numpy(self.asm_pool.copy()).cuda(), torch.from_numpy(self.asm_off.copy()).cuda()
        self.words = int(self.lib.gf_round2_work_words(key_cap, N_GAPS))
        self.keys, self.p_keys = _guarded(8 * key_cap, fill=0xFF)
        self.sorted, self.p_sorted = _guarded(8 * key_cap)
        self.work, self.p_work = _guarded(4 * self.words)
        self.rows, self.p_rows = _guarded(16 * (N_GAPS + 1))
        self.pool, self.p_pool = _guarded(max(1, pool_cap) * self.rb)
        self.prev, self.p_prev = _guarded(4 * N_GAPS)
        self.st, self.p_st = _guarded(4 * B.R2_WORDS * 3, fill=0)          # three rounds' blocks
        self.np_live, self.p_np_live = _guarded(4 * N_LIB)
        self.snap, self.p_snap = _guarded(8 * key_cap)
        self.d_np = torch.tensor([n_pairs, n_pairs - 1], dtype=torch.int32, device="cuda")
        self.d_n = torch.tensor([1234], dtype=torch.int32, device="cuda")
        self.d_best = torch.zeros(N_GAPS, dtype=torch.int64, device="cuda")

    def all_guards_intact(self):
        return all(_guards_intact(t) for t in (self.keys, self.sorted, self.work, self.rows, self.pool, self.prev, self.np_live, self.snap, self.st))

    def block(self, r):
        return self.p_st + 4 * self.B.R2_WORDS * r

    def stats(self, r):
        return _payload(self.st).view(np.uint32).reshape(3, self.B.R2_WORDS)[r]

    def round1(self, hits):
        """The existing round-1 pools call over `hits` (what leaves sorted keys, flags, scan and counts for the first carry)."""
        import torch
        _put(self.keys, np.concatenate([hits, np.full(self.key_cap - len(hits), EMPTY, dtype=np.uint64)]))
        scratch = torch.empty((self.asm_pool.shape[0] + 2 * len(hits) + 8) * self.rb, dtype=torch.uint8, device="cuda")
        assert self.lib.gf_round2_pools_dev(self.gf.handle, self.p_keys, self.p_sorted, self.key_cap, self.lib_ptrs, N_LIB, L_P,
                                            self.d_asm_pool.data_ptr(), self.d_asm_off.data_ptr(), self.d_best.data_ptr(), N_GAPS, self.p_work,
                                            self.p_rows, scratch.data_ptr(), self.asm_pool.shape[0] + 2 * len(hits) + 8, self.block(0)) == 0
        self.gf.sync()

    def carry(self, r, live, snapshot=True):
        assert self.lib.gf_round_carry_dev(self.gf.handle, self.p_keys, self.p_sorted, self.key_cap, N_GAPS, self.p_work, self.p_prev, self.block(r - 1),
                                           self.block(r), self.d_n.data_ptr(), self.d_np.data_ptr(), self.p_np_live, N_LIB,
                                           self.p_snap if snapshot else None, live) == 0
        self.gf.sync()

    def append(self, r, hits, emitted=None):
        """What the recruitment does: the hits behind the keys already there, up to the capacity; HITS counts them all."""
        import torch
        st = self.stats(r)
        at = int(st[self.B.R2_HITS])
        room = hits[:max(0, self.key_cap - at)]
        if len(room):
            self.keys[256 + 8 * at:256 + 8 * (at + len(room))] = torch.from_numpy(room.view(np.uint8).copy()).cuda()
        total = np.array([at + (len(hits) if emitted is None else emitted)], dtype=np.uint32)
        off = 256 + 4 * (self.B.R2_WORDS * r + self.B.R2_HITS)
        self.st[off:off + 4] = torch.from_numpy(total.view(np.uint8).copy()).cuda()

    def pools(self, r, live=None, pool_cap=None):
        assert self.lib.gf_round_pools_dev(self.gf.handle, self.p_keys, self.p_sorted, self.key_cap, self.lib_ptrs, N_LIB, L_P,
                                           self.d_asm_pool.data_ptr(), self.d_asm_off.data_ptr(), self.d_best.data_ptr(), N_GAPS, self.p_prev,
                                           self.p_work, self.p_rows, self.p_pool, self.pool_cap if pool_cap is None else pool_cap, self.block(r),
                                           live) == 0
        self.gf.sync()

    def expected_pools(self, uniq, prev_cnt, best, pool_cap):
        cnt = np.bincount(_gap(uniq), minlength=N_GAPS)
        r1 = np.diff(self.asm_off)
        grew = (best == 0) & (cnt > prev_cnt)
        rows = np.where(grew, r1 + 2 * cnt, 0)
        off = np.concatenate([[0], np.cumsum(rows)])
        tot = int(off[-1])
        ovf = tot > pool_cap
        parts = []
        for g in np.nonzero(grew)[0]:
            mine = uniq[_gap(uniq) == g]
            li, pr = ((mine >> np.uint64(36)) & np.uint64(15)).astype(np.int64), (mine & PAIR_MASK).astype(np.int64)
            rec = np.zeros((2 * len(mine), self.rb), dtype=np.uint8)
            for l in range(N_LIB):
                m = li == l
                rec[0::2][m], rec[1::2][m] = self.reads[l][2 * pr[m]], self.reads[l][2 * pr[m] + 1]
            parts += [self.asm_pool[self.asm_off[g]:self.asm_off[g + 1]], rec]
        pool = np.concatenate(parts).reshape(-1) if parts and not ovf else np.zeros(0, dtype=np.uint8)
        return {"cnt": cnt, "rows": rows, "off": np.zeros_like(off) if ovf else off, "tot": tot, "ovf": ovf, "pool": pool,
                "new": int((cnt - prev_cnt)[best == 0].clip(min=0).sum()), "grown": int(grew.sum()), "with": int((cnt != 0).sum()),
                "tried": int((best == 0).sum())}

    def check_pools(self, r, want, uniq):
        B = self.B
        st = self.stats(r)
        rows = _payload(self.rows).view(np.int64)
        assert rows[:N_GAPS].tolist() == want["rows"].tolist() and rows[N_GAPS] == 0
        assert rows[N_GAPS + 1:].tolist() == want["off"].tolist()
        assert (int(st[B.R2_UNIQUE]), int(st[B.R2_NEW]), int(st[B.R2_GROWN]), int(st[B.R2_WITH]), int(st[B.R2_TRIED])) == \
            (len(uniq), want["new"], want["grown"], want["with"], want["tried"])
        assert int(st[B.R2_ROWS]) | (int(st[B.R2_ROWS + 1]) << 32) == want["tot"] and int(st[B.R2_POOL_OVF]) == int(want["ovf"])
        assert int(st[B.R2_GATED]) == 0
        pool = _payload(self.pool)
        assert pool[:len(want["pool"])].tobytes() == want["pool"].tobytes()
        assert (pool[len(want["pool"]):] == GUARD).all()                     # nothing behind the last pool, nothing at all on overflow
        work = _payload(self.work).view(np.uint32)
        assert work[2 * self.key_cap:2 * self.key_cap + N_GAPS].tolist() == want["cnt"].tolist()
        s = _payload(self.sorted).view(np.uint64)
        assert (s[1:] >= s[:-1]).all()
        assert self.all_guards_intact()


def _round1_hits(rng, n_pairs):
    """Round 1's hits: ~300 keys over every gap and both libraries with duplicates, and a few of gaps beyond n_gaps."""
    g = rng.integers(0, N_GAPS, size=300)
    k = _key(g, rng.integers(0, N_LIB, size=300), rng.integers(0, min(n_pairs - 1, 400), size=300))
    k = np.concatenate([k, k[:40], _key([N_GAPS, N_GAPS + 3], [0, 1], [5, 6])])
    return k[rng.permutation(len(k))]


def _new_hits(rng, m, prev_unique, n_pairs):
    """m hits of a later round: one fresh pair for BY_ONE, repeats of carried keys (STALE gets nothing else), fresh and repeated keys for
    the gaps 0, CLOSED, 4, 5, and the odd key of a gap beyond n_gaps."""
    if m == 0:
        return np.zeros(0, dtype=np.uint64)
    out = [_key([BY_ONE], [1], [n_pairs - 2])]              # (pairs of round 1 lie below n_pairs - 2 in library 1: fresh)
    rest = m - 1
    n_old, n_bad = rest // 5, min(rest // 50, 3)
    n_fresh = rest - n_old - n_bad
    if n_old:
        out.append(prev_unique[rng.integers(0, len(prev_unique), size=n_old)])
    if n_bad:
        out.append(_key(rng.integers(N_GAPS, N_GAPS + 4, size=n_bad), 0, rng.integers(0, n_pairs - 2, size=n_bad)))
    if n_fresh:
        g = np.array([0, CLOSED, 4, 5])[rng.integers(0, 4, size=n_fresh)]
        out.append(_key(g, rng.integers(0, N_LIB, size=n_fresh), rng.integers(0, n_pairs - 2, size=n_fresh)))
    k = np.concatenate(out)
    return k[rng.permutation(len(k))]


def _valid_unique(keys):
    keys = keys[(keys != EMPTY) & (_gap(keys) < N_GAPS)]
    return np.unique(keys)


def _one_trip():
    """Keys one grid-stride trip of the key kernels covers: 16 workgroups of 256 threads per CU at the most."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256


@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, "trip", "over"])
def test_carry_and_pools_equal_the_definition(gf, m):
    import torch
    over = m == "over"
    big = m == "trip"
    m = 257 if over else (_one_trip() + 257 if big else m)
    rng = np.random.default_rng(900 + (m % 1000))
    n_pairs = 200_000 if big else 500
    hits1 = _round1_hits(rng, n_pairs)
    u1 = _valid_unique(hits1)
    new = _new_hits(rng, m, u1, n_pairs)
    key_cap = max(len(hits1), len(u1) + m)              # m >= 255: exactly full after the round's hits
    u2 = _valid_unique(np.concatenate([u1, new]))
    rig = _Rig(gf, rng, n_pairs, key_cap, pool_cap=0)
    best = np.zeros(N_GAPS, dtype=np.int64)
    rig.round1(hits1)
    assert int(rig.stats(0)[rig.B.R2_UNIQUE]) == len(u1)
    # the first pick of round 1 closed CLOSED
    best[CLOSED] = 1 << 56
    rig.d_best.copy_(torch.from_numpy(best))
    live = torch.tensor([3], dtype=torch.int32, device="cuda")
    # ---- round 2: carry
    rig.carry(1, live.data_ptr())
    keys = _payload(rig.keys).view(np.uint64)
    assert keys[:len(u1)].tolist() == u1.tolist() and (keys[len(u1):] == EMPTY).all()
    assert _payload(rig.snap).view(np.uint64)[:len(u1)].tolist() == u1.tolist()
    assert (_payload(rig.snap)[8 * len(u1):] == GUARD).all()
    prev_cnt = np.bincount(_gap(u1), minlength=N_GAPS)
    assert _payload(rig.prev).view(np.uint32).tolist() == prev_cnt.tolist()
    st = rig.stats(1)
    assert int(st[rig.B.R2_HITS]) == len(u1) and [int(x) for i, x in enumerate(st) if i != rig.B.R2_HITS] == [0] * 15
    assert _payload(rig.np_live).view(np.uint32).tolist() == [n_pairs, n_pairs - 1]
    assert rig.all_guards_intact()
    # ---- round 2: the recruitment's hits behind the carried keys ("over": one more emitted than there is room for), then the pools
    rig.append(1, new, emitted=len(new) + 1 if over else None)
    want = rig.expected_pools(u2, prev_cnt, best, 1 << 40)
    tot = want["tot"]
    # first with room for one row less than the pools need: every pool empty, the flag set, nothing written ...
    if tot:
        short = _Rig.__new__(_Rig)
        short.__dict__.update(rig.__dict__)
        short.pool, short.p_pool = _guarded(max(1, tot - 1) * rig.rb)
        short.pools(1, pool_cap=tot - 1)
        w = rig.expected_pools(u2, prev_cnt, best, tot - 1)
        assert w["ovf"] and len(w["pool"]) == 0
        short.check_pools(1, w, u2)
        # (the statistics are sums: zero the block's pool words before the call that counts)
        z = torch.zeros(4 * rig.B.R2_WORDS, dtype=torch.uint8, device="cuda")
        hits_word = rig.stats(1)[rig.B.R2_HITS].copy()
        rig.st[256 + 4 * rig.B.R2_WORDS:256 + 8 * rig.B.R2_WORDS] = z
        off = 256 + 4 * (rig.B.R2_WORDS + rig.B.R2_HITS)
        rig.st[off:off + 4] = torch.from_numpy(np.array([hits_word], dtype=np.uint32).view(np.uint8).copy()).cuda()
    # ... then with exactly the room they need
    rig.pool, rig.p_pool = _guarded(max(1, tot) * rig.rb)
    rig.pool_cap = tot
    rig.pools(1)
    rig.check_pools(1, want, u2)
    if m:
        assert want["rows"][CLOSED] == 0 and want["cnt"][CLOSED] > 0                          # closed, with keys: no pool
        assert want["rows"][STALE] == 0 and want["cnt"][STALE] == prev_cnt[STALE] > 0         # open, not grown: no pool
        assert want["cnt"][BY_ONE] == prev_cnt[BY_ONE] + 1 and want["rows"][BY_ONE] > 0       # grown by one pair
    else:
        assert want["grown"] == 0 and tot == 0
    if m >= 255:
        assert want["rows"][0] > 0 and want["rows"][4] > 0 and len(u1) + m == key_cap
    # ---- round 3's carry reads what round 2's pools left: every distinct valid key so far, closed gaps' included
    rig.carry(2, rig.block(1) + 4 * rig.B.R2_GROWN)
    keys = _payload(rig.keys).view(np.uint64)
    st3 = rig.stats(2)
    if want["grown"]:
        assert (keys[:len(u2)] == u2).all() and (keys[len(u2):] == EMPTY).all()
        assert _payload(rig.prev).view(np.uint32).tolist() == want["cnt"].tolist()
        assert int(st3[rig.B.R2_HITS]) == len(u2) and int(st3[rig.B.R2_GATED]) == 0
    else:               # round 2 grew nothing: round 3 is gated
        assert int(st3[rig.B.R2_GATED]) == 1 and int(st3[rig.B.R2_FIRST]) == 1234 and int(st3[rig.B.R2_HITS]) == 0
        assert _payload(rig.np_live).view(np.uint32).tolist() == [0, 0]
    assert rig.all_guards_intact()


def test_a_gated_round_writes_nothing_but_first_and_gated(gf, table_case):
    """d_live == 0: carry, table and pools leave every buffer as it was (filled with the guard pattern here); the round's block gets
    FIRST = n and GATED = 1, the candidate counts the recruitment reads are zeroed."""
    import torch
    from gappadder_amd import _lib as B
    rng = np.random.default_rng(77)
    rig = _Rig(gf, rng, 500, 777, pool_cap=64)
    rig.keys.fill_(GUARD)
    dead = torch.zeros(1, dtype=torch.int32, device="cuda")
    rig.carry(1, dead.data_ptr())
    c = table_case
    tab, p_tab = _guarded(24 << LOG2_T)
    d_n = torch.tensor([len(c["lst"])], dtype=torch.int32, device="cuda")
    d_first = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert B.lib().gf_contig_kmer_table_from_dev(gf.handle, c["d_ctg"].data_ptr(), d_n.data_ptr(), len(c["lst"]), c["d_seq"].data_ptr(),
                                                 c["d_best"].data_ptr(), N_GAPS_T, c["k"], d_first.data_ptr(), p_tab, LOG2_T, rig.block(1),
                                                 dead.data_ptr()) == 0
    rig.pools(1, live=dead.data_ptr())
    gf.sync()
    for t in (rig.keys, rig.sorted, rig.work, rig.rows, rig.pool, rig.prev, rig.snap, tab):
        assert (t.cpu().numpy() == GUARD).all()
    st = rig.stats(1)
    assert int(st[B.R2_FIRST]) == 1234 and int(st[B.R2_GATED]) == 1
    assert [int(x) for i, x in enumerate(st) if i not in (B.R2_FIRST, B.R2_GATED)] == [0] * 14
    assert not rig.stats(0).any() and not rig.stats(2).any()
    assert _payload(rig.np_live).view(np.uint32).tolist() == [0, 0] and _guards_intact(rig.np_live) and _guards_intact(rig.st)
    # the same calls with a live word do write: the gate, not the inputs, kept them still
    alive = torch.ones(1, dtype=torch.int32, device="cuda")
    assert B.lib().gf_contig_kmer_table_from_dev(gf.handle, c["d_ctg"].data_ptr(), d_n.data_ptr(), len(c["lst"]), c["d_seq"].data_ptr(),
                                                 c["d_best"].data_ptr(), N_GAPS_T, c["k"], d_first.data_ptr(), p_tab, LOG2_T, rig.block(2),
                                                 alive.data_ptr()) == 0
    gf.sync()
    assert not (_payload(tab) == GUARD).all() and _guards_intact(tab)
