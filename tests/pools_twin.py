"""Plain definition of the per-gap read pools (gappadder_amd/csrc/pools.hip, include/gapfill_hip.h "a-4 / a-5 on the device"),
numpy and Python sets only, no device.

A key is uint64 (gap << 32 | read), read = 2 * pair + mate.  The pools are the SET of (gap, read) keys with gap < n_gaps; inside a gap
the reads are ordered by (mate, pair) — the left FASTQ file's stream order, then the right file's.  Nothing here follows the kernels:
no histogram, no sort network, only sets and `sorted`."""
import numpy as np

NO_GAP = 0xFFFFFFFF
POOL_OVERFLOW = 0x80000000


def make_keys(gap, read):
    """uint64 keys of equally long gap / read arrays (or scalars)."""
    return (np.asarray(gap, dtype=np.uint64) << np.uint64(32)) | np.asarray(read, dtype=np.uint64)


def build_pools(keys_u64, n_gaps, reads, pool_cap):
    """-> (pool_off u64[n_gaps + 1], ids u32[min(total, pool_cap)], rows u8[len(ids), rb], overflow_flag).

    pool_off is exact whatever pool_cap is; ids and rows exist only below pool_cap; the flag is pool_off[-1] > pool_cap.  The row of a
    read >= len(reads) is not defined here (the read is counted and listed all the same): it comes back as zeros."""
    reads = np.asarray(reads, dtype=np.uint8)
    pairs = {(k >> 32, k & 0xFFFFFFFF) for k in np.asarray(keys_u64, dtype=np.uint64).tolist()}
    per_gap = {}
    for g, r in pairs:
        if g < n_gaps:
            per_gap.setdefault(g, []).append(r)
    cnt = np.zeros(n_gaps, dtype=np.uint64)
    ids = []
    for g in sorted(per_gap):
        cnt[g] = len(per_gap[g])
        ids.extend(sorted(per_gap[g], key=lambda r: (r & 1, r >> 1)))
    pool_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(cnt, dtype=np.uint64)])
    total = int(pool_off[-1])
    ids = np.asarray(ids[:pool_cap], dtype=np.uint32)
    rows = np.zeros((len(ids), reads.shape[1]), dtype=np.uint8)
    known = ids < len(reads)
    rows[known] = reads[ids[known].astype(np.int64)]
    return pool_off, ids, rows, total > pool_cap


def keys_from_screen(hits, pairs):
    """Screen hits (gap, read) -> keys; with `pairs` every hit is followed by its mate's key.  (The device producer reserves places with
    atomics: the same keys as a multiset.)"""
    g, r = hits["gap"].astype(np.uint64), hits["read"].astype(np.uint64)
    if not pairs:
        return make_keys(g, r)
    out = np.empty(2 * len(hits), dtype=np.uint64)
    out[0::2] = make_keys(g, r)
    out[1::2] = make_keys(g, r ^ np.uint64(1))
    return out


def keys_from_tags(recs, taghits, row_gap_or_None):
    """Tagger / second-hop hits -> keys: the read is the record's (low 32 bits), or its mate when to_mate is set; the gap is hit.gap, or
    row_gap[hit.gap] for second-hop hits.  A record without a read (read == 0xFFFFFFFF) names no gap: gap 0xFFFFFFFF."""
    own = (recs["read"][taghits["rec"].astype(np.int64)] & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    read = own ^ (taghits["to_mate"] != 0).astype(np.uint64)
    gap = taghits["gap"].astype(np.int64)
    if row_gap_or_None is not None:
        gap = np.asarray(row_gap_or_None)[gap]
    gap = np.where(own == NO_GAP, NO_GAP, gap).astype(np.uint64)
    return make_keys(gap, read)


def keys_all(hits, pairs, recs, taghits_or_None, hophits_or_None, row_gap):
    """The three lists in fixed places: screen hits (with mates), then the tagger's, then the second hop's."""
    parts = [keys_from_screen(hits, pairs)]
    if taghits_or_None is not None:
        parts.append(keys_from_tags(recs, taghits_or_None, None))
    if hophits_or_None is not None:
        parts.append(keys_from_tags(recs, hophits_or_None, row_gap))
    return np.concatenate(parts)
