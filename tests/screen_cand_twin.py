"""numpy twins of the partitioned screen filter (gappadder_amd/csrc/screen_pf4.hip), written from the definitions and independent of the
library: the flanks' canonical 16-mers with the masks of their neighbouring bases (index.hip `extract`, index_dev.hip
`idx_sgrp_build_kernel`), the candidate reads of the filter (`pf4_ext_ok`, `pf4_resolve_kernel`), and the state pass A leaves behind — every
part's pairs by group, its fill history and its count.  Also the inputs of the GPU tests that compare the device with these: random reads
of which a part carries exactly one planted seed, so that a pair lost anywhere in the filter loses a candidate."""
import math
import re

import numpy as np

import probe_column_twin as T

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = str.maketrans("ACGT", "TGCA")
_ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)
NB = 256            # buckets: the top eight bits of a scrambled key
GROUP = 4           # probes of a read sorted per group, at most


def word16(s):
    w = 0
    for c in s:
        w = (w << 2) | _CODE[c]
    return w


def acgt_runs(s, k):
    """The maximal runs [i, j) of A, C, G, T (upper case) of at least k bases."""
    return [(m.start(), m.end()) for m in re.finditer("[ACGT]+", s) if m.end() - m.start() >= k]


def _mask(nearest, nxt):
    """Mask over the codes nearest << 2 | next of the two bases beside an occurrence; None = the run ends before that base."""
    if nearest is None:
        return 0
    if nxt is None:
        return 0xF << (4 * _CODE[nearest])
    return 1 << (4 * _CODE[nearest] + _CODE[nxt])


def _comp(c):
    return None if c is None else c.translate(_COMP)


def flank_seed_set(flanks, k):
    """(keys, left, right): the canonical 16-mers of every 16-mer inside a maximal ACGT run of >= k bases of a flank, sorted, and per key
    the masks of what stands left / right of it in the orientation of the canonical form."""
    masks = {}
    for pair in flanks:
        for s in pair:
            for i, j in acgt_runs(s, k):
                for pos in range(i, j - 15):
                    text = s[pos:pos + 16]
                    w, wr = word16(text), word16(text.translate(_COMP)[::-1])
                    r1, r2 = (s[pos + 16] if pos + 16 < j else None), (s[pos + 17] if pos + 17 < j else None)
                    l1, l2 = (s[pos - 1] if pos - 1 >= i else None), (s[pos - 2] if pos - 2 >= i else None)
                    m = masks.setdefault(min(w, wr), [0, 0])
                    if w <= wr:     # the text is the canonical form (a palindrome takes this reading and the next)
                        m[0] |= _mask(l1, l2)
                        m[1] |= _mask(r1, r2)
                    if wr <= w:     # the text is its reverse complement: the sides swap, the bases are complemented
                        m[0] |= _mask(_comp(r1), _comp(r2))
                        m[1] |= _mask(_comp(l1), _comp(l2))
    keys = np.array(sorted(masks), dtype=np.uint32)
    left = np.array([masks[int(x)][0] for x in keys], dtype=np.uint32)
    right = np.array([masks[int(x)][1] for x in keys], dtype=np.uint32)
    return keys, left, right


def pack(codes):
    """(n, L) base codes 0..3 -> (n, ceil(L / 4)) packed rows, first base in the top bits, the pad zero."""
    n, L = codes.shape
    rb = (L + 3) // 4
    c = np.zeros((n, 4 * rb), dtype=np.uint8)
    c[:, :L] = codes
    return (c[:, 0::4] << 6) | (c[:, 1::4] << 4) | (c[:, 2::4] << 2) | c[:, 3::4]


def pack_ascii(blob, L):
    """ASCII reads (bytes, n * L) -> packed rows; what is not A, C, G, T packs as A."""
    a = np.frombuffer(blob, dtype=np.uint8).reshape(-1, L)
    codes = np.zeros(a.shape, dtype=np.uint8)
    for c, ch in enumerate(b"ACGT"):
        codes[a == ch] = c
    return pack(codes)


def unpack(packed):
    """(n, 4 * rb + 4) base codes, four spare zero columns behind."""
    n, rb = packed.shape
    b = np.zeros((n, 4 * rb + 4), dtype=np.uint8)
    for q in range(4):
        b[:, q:4 * rb:4] = (packed >> (6 - 2 * q)) & 3
    return b


def _words(bases, off):
    w = np.zeros(bases.shape[0], dtype=np.uint64)
    for i in range(16):
        w = (w << np.uint64(2)) | bases[:, off + i].astype(np.uint64)
    return w


def candidates(packed, L, k, flanks, ext_allowed=True, check_ext=True, seeds=None):
    """(reads, qualifies): the reads with at least one probe whose canonical 16-mer is a flank's and, where the geometry checks `ext`
    bases behind a seed, whose next `ext` bases some flank has beside that 16-mer; qualifies[r, j] = probe j of read r does.
    check_ext=False: the same probes without the neighbour check (the filter's serial path).  seeds: flank_seed_set(flanks, k), if at hand."""
    first, stride, n_probes, ext = T.geometry(L, k, ext_allowed)
    keys, left, right = seeds if seeds is not None else flank_seed_set(flanks, k)
    bases = unpack(packed)
    qual = np.zeros((packed.shape[0], n_probes), dtype=bool)
    for j in range(n_probes):
        off = first + j * stride
        w = _words(bases, off)
        key = T.canon16(w)
        at = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
        ok = keys[at] == key
        if ext and check_ext:
            code = (bases[:, off + 16].astype(np.uint32) << 2) | bases[:, off + 17]
            rev = key != w          # the read shows the reverse complement of the canonical form: its right side is the canonical left side
            code = np.where(rev, code ^ 15, code)
            mask = np.where(rev, left[at], right[at])
            ok &= ((mask >> code) & 1) != 0 if ext >= 2 else ((mask >> (code & 12)) & 15) != 0
        qual[:, j] = ok
    return np.nonzero(qual.any(axis=1))[0].astype(np.uint32), qual


def plan(n_reads, L, k, n_cu, writers=0, ext_allowed=True, tiles_wg=32):
    """The partitioned filter's plan (screen.hip `plan_screen`): n_writers, n_iter, cap, n_grp, n_groups, gs."""
    n_probes = T.geometry(L, k, ext_allowed)[2]
    tiles = (n_reads + 63) // 64
    nw = max(min((tiles + tiles_wg - 1) // tiles_wg, n_cu, 256), 1)
    if writers > 0:
        nw = min(nw, writers)
    n_iter = (tiles + nw * tiles_wg - 1) // (nw * tiles_wg)
    expect = float(n_iter) * tiles_wg * 64.0 * n_probes / NB
    cap = (int(expect * 1.05 + 6.0 * math.sqrt(expect + 1.0) + 128.0) + 63) & ~63
    n_grp = (n_probes + min(n_probes, GROUP) - 1) // min(n_probes, GROUP)
    n_groups = n_iter * n_grp
    return {"n_writers": nw, "n_iter": n_iter, "cap": cap, "n_grp": n_grp, "n_groups": n_groups, "gs": (n_groups + 1 + 15) & ~15}


def pass_a_state(packed, L, k, n_writers, tiles_wg=32, ext_allowed=True):
    """Pass A's state from its definition.  Writer w takes, in iteration `it`, the tiles_wg 64-read tiles from (it * n_writers + w) * tiles_wg
    (its batch); probe j of read r is a pair of group it * n_grp + j // grp in the part (bucket = top 8 bits of the scrambled key, writer),
    with the entry (key bits & 0xFFFFFF) << 8 | the read's octet inside the batch.  Returns count (per part), fills (per part the position
    at which every group starts, and the count), and pairs / runs: the entries sorted inside every (part, group) run, and the run's number
    part * n_groups + group of each — the arrays that screen_state_util.filter_state reads from the device.  (A part that overflows its
    capacity is cut short there; here it is not.)  pair_part / pair_group: where the pair of (probe j, read r) lies."""
    n = packed.shape[0]
    n_probes = T.geometry(L, k, ext_allowed)[2]
    pk = T.column(packed, L, k, ext_allowed).reshape(n_probes, -1)[:, :n].astype(np.int64)
    r = np.arange(n, dtype=np.int64)
    tile = r >> 6
    it, w = tile // (n_writers * tiles_wg), (tile // tiles_wg) % n_writers
    octet = ((tile % tiles_wg) << 3) | ((r & 63) >> 3)
    grp = min(n_probes, GROUP)
    n_grp = (n_probes + grp - 1) // grp
    n_iter = ((n + 63) // 64 + n_writers * tiles_wg - 1) // (n_writers * tiles_wg)
    n_groups = n_iter * n_grp
    parts = NB * n_writers
    part = (pk >> 24) * n_writers + w[None, :]
    group = np.broadcast_to(it[None, :] * n_grp + (np.arange(n_probes, dtype=np.int64) // grp)[:, None], pk.shape)
    entry = ((pk & 0xFFFFFF) << 8) | octet[None, :]
    run = (part * n_groups + group).ravel()
    order = np.lexsort((entry.ravel(), run))
    per_run = np.bincount(run, minlength=parts * n_groups).reshape(parts, n_groups)
    fills = np.zeros((parts, n_groups + 1), dtype=np.uint32)
    fills[:, 1:] = np.cumsum(per_run, axis=1)
    return {"count": fills[:, -1].copy(), "fills": fills, "pairs": entry.ravel()[order].astype(np.uint32), "runs": run[order],
            "n_groups": n_groups, "n_grp": n_grp, "n_iter": n_iter, "pair_part": part, "pair_group": np.array(group)}


def tail_facts(count, fills):
    """What the parts of a run offer pass B: the tail classes ((count - 1) % 1024) // 256 among the parts of more than one trip (1 024
    entries), the residues count % 4, the largest count, and every part's last group that holds pairs (-1: an empty part)."""
    count = np.asarray(count).astype(np.int64)
    long = count[count > 1024]
    per = np.diff(np.asarray(fills).astype(np.int64), axis=1)
    last = np.where(per.any(axis=1), per.shape[1] - 1 - np.argmax(per[:, ::-1] > 0, axis=1), -1)
    return {"tails": set(((long - 1) % 1024 // 256).tolist()), "mod4": set((count % 4).tolist()), "max": int(count.max()), "min": int(count.min()),
            "last_group": last}


def planted_in_last_group(state, count, fills, reads, qual):
    """The fraction of the parts (count, fills: as dumped) whose last group with pairs starts inside the part's tail trip of pass B and holds
    a pair of one of `reads` (planted: qual says through which probe; where that pair lies: state, the twin's)."""
    count, fills = np.asarray(count).astype(np.int64), np.asarray(fills).astype(np.int64)
    last = tail_facts(count, fills)["last_group"]
    j = np.argmax(qual[reads], axis=1)
    part, group = state["pair_part"][j, reads], state["pair_group"][j, reads]
    has = np.zeros(len(last), dtype=bool)
    has[part[group == last[part]]] = True
    in_tail = (last >= 0) & (fills[np.arange(len(last)), np.maximum(last, 0)] >= (count - 1) // 1024 * 1024)
    return (has & in_tail).mean()


def homes(state, qual, reads):
    """(read, part, group) of every qualifying pair of `reads`: where a lost candidate's pairs lie."""
    return [(int(r), int(state["pair_part"][j, r]), int(state["pair_group"][j, r])) for r in reads for j in np.nonzero(qual[r])[0]]


def scrambled_set(keys):
    """The flank 16-mers as pass A's scrambled keys, sorted."""
    return np.sort((keys.astype(np.uint64) * np.uint64(T.S16_MUL)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def exact_set_pairs(pairs, runs, n_writers, n_groups, keys):
    """How many of the dumped pairs (entries and their runs) have a key of the exact set: what pass B puts on its pair list."""
    bucket = (np.asarray(runs, dtype=np.int64) // n_groups) // n_writers
    pk = ((bucket << 24) | (pairs.astype(np.int64) >> 8)).astype(np.uint32)
    return int(np.isin(pk, scrambled_set(keys)).sum())


# ---- the grouped exact set (index_dev.hip): a key's home is the group of four slots hash_s16_set(key) >> 2 of 2^s_log2 slots

def hash_s16_set(keys, s_log2):
    m = np.uint64(0xFFFFFFFF)
    x = (keys.astype(np.uint64) * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0xC2B2AE35)) & m
    return (x >> np.uint64(32 - s_log2)).astype(np.uint32)


def crowded_keys(keys):
    """The keys whose home group is the home of more than four keys: one of them at least lies in a later group (which one, an atomic decides)."""
    s_log2 = max(8, int(2 * len(keys) + 2 - 1).bit_length())
    home = hash_s16_set(keys, s_log2) >> 2
    per = np.bincount(home, minlength=1 << (s_log2 - 2))
    return keys[per[home] > 4]


# ---- inputs

def planted_case(n, L, k, flanks, seed, ext_allowed=True, frac=0.25, decoys=0.05, hits=0.01, only_keys=None):
    """n random reads.  A fraction `frac` carries one planted seed: a (16 + ext)-mer cut from inside a qualifying flank run, as it stands
    or reverse-complemented, at one of the read's probe offsets; a fraction `decoys` carries a flank 16-mer alone (what follows it is
    random: with ext > 0 most of them are no candidates); a fraction `hits` carries k to k + 29 bases of a flank run, either strand, anywhere
    in the read: the reads the screen has to return.  only_keys: plant the 16-mers of these canonical keys only, every one of them.
    Returns the reads as base codes, ASCII and packed rows, and the rows planted / decoyed."""
    first, stride, n_probes, ext = T.geometry(L, k, ext_allowed)
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
    # every 16-mer position q inside a qualifying run, in one concatenated text; lo / hi: the run's bounds
    cat, q_all, lo_all, hi_all, runs = [], [], [], [], []
    at = 0
    for pair in flanks:
        for s in pair:
            for i, j in acgt_runs(s, k):
                cat.append(np.array([_CODE[c] for c in s[i:j]], dtype=np.uint8))
                q = np.arange(at, at + (j - i) - 15)
                q_all.append(q)
                lo_all.append(np.full(len(q), at))
                hi_all.append(np.full(len(q), at + (j - i)))
                runs.append((at, at + (j - i)))
                at += j - i
    cat, q_all, lo_all, hi_all = np.concatenate(cat), np.concatenate(q_all), np.concatenate(lo_all), np.concatenate(hi_all)
    if only_keys is not None:
        w = np.zeros(len(q_all), dtype=np.uint64)
        for i in range(16):
            w = (w << np.uint64(2)) | cat[q_all + i].astype(np.uint64)
        sel = np.isin(T.canon16(w).astype(np.uint32), only_keys)
        q_all, lo_all, hi_all = q_all[sel], lo_all[sel], hi_all[sel]

    def plant(rows, e, cover):
        # forward: text[q, q + 16 + e); reverse: the reverse complement of text[q - e, q + 16) — both inside the run
        opt_q = np.concatenate([q_all[q_all + 16 + e <= hi_all], q_all[q_all - e >= lo_all] - e])
        opt_rc = np.concatenate([np.zeros((q_all + 16 + e <= hi_all).sum(), dtype=bool), np.ones((q_all - e >= lo_all).sum(), dtype=bool)])
        pick = rng.permutation(len(opt_q))[np.arange(len(rows)) % len(opt_q)] if cover else rng.integers(0, len(opt_q), len(rows))
        seg = cat[opt_q[pick][:, None] + np.arange(16 + e)[None, :]]
        seg = np.where(opt_rc[pick][:, None], 3 - seg[:, ::-1], seg)
        off = first + rng.integers(0, n_probes, len(rows)) * stride
        codes[rows[:, None], off[:, None] + np.arange(16 + e)[None, :]] = seg

    rows = rng.permutation(n)
    n_pl, n_de, n_hit = int(round(frac * n)), int(round(decoys * n)), int(round(hits * n))
    planted, decoy = np.sort(rows[:n_pl]), np.sort(rows[n_pl:n_pl + n_de])
    for r in rows[n_pl + n_de:n_pl + n_de + n_hit]:
        lo, hi = runs[rng.integers(len(runs))]
        m = min(k + int(rng.integers(0, 30)), hi - lo, L)
        a = lo + int(rng.integers(0, hi - lo - m + 1))
        seg = cat[a:a + m]
        off = int(rng.integers(0, L - m + 1))
        codes[r, off:off + m] = 3 - seg[::-1] if rng.integers(2) else seg
    plant(planted, ext, only_keys is not None)
    if n_de:
        plant(decoy, 0, False)
    return {"codes": codes, "blob": _ASCII[codes].tobytes(), "packed": pack(codes), "planted": planted, "decoy": decoy}


def confirmed(planted, qual):
    """The planted reads that qualify through exactly one probe."""
    return planted[qual[planted].sum(axis=1) == 1]
