"""A numpy twin of the tagger's linear layout (gf_tag_layout, include/gapfill_hip.h): the scaffolds laid end to end on granule boundaries,
the 4-byte key of a record on that line, the MAPQ-0 bit plane and the parts of the column's buffer.  Written from the header's words, not
from the kernels; shared by test_tag_linear_layout_host.py and test_gpu_tag_linear_keys.py."""
import numpy as np

GRANULE_MAX, GRANULE_MIN, LDS_BITS_LOG2 = 20, 6, 17
SENTINEL = 0xFFFFFFFF


def fnv1a64(words):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(words, dtype="<u4").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def layout(ends, n_recs):
    """The layout of scaffolds with these exclusive ends: the largest granule 2^A, A in 20 .. 6, for which the line stays below 2^32 - 2^A and a
    map of 2^17 bins over it has bins no wider than the granule; use = 0 when there is none."""
    ends = [int(e) for e in ends]
    for a in range(GRANULE_MAX, GRANULE_MIN - 1, -1):
        gr = 1 << a
        sizes = [(e + gr - 1) // gr * gr for e in ends]
        total = sum(sizes)
        if total >= (1 << 32) - gr:
            continue
        need = GRANULE_MIN
        while (total >> need) + 1 > (1 << LDS_BITS_LOG2):
            need += 1
        if need > a:
            continue
        base = np.zeros(len(ends) + 1, dtype=np.uint64)
        base[1:] = np.cumsum(np.asarray(sizes, dtype=np.uint64))
        base = base.astype(np.uint32)
        return dict(use=1, granule_log2=a, span=total, base=base, checksum=fnv1a64(base), n_recs=int(n_recs), n_scaffolds=len(ends))
    return dict(use=0, granule_log2=0, span=0, base=None, checksum=0, n_recs=int(n_recs), n_scaffolds=len(ends))


def ends_of(recs, n_scaffolds):
    """max(pos) + 1 per scaffold over the placed records (ref < n_scaffolds); 0 for a scaffold without one."""
    ends = np.zeros(n_scaffolds, dtype=np.uint64)
    ok = recs["ref"] < n_scaffolds
    np.maximum.at(ends, recs["ref"][ok].astype(np.int64), recs["pos"][ok].astype(np.uint64) + 1)
    return ends


def parts(n, n_scaffolds):
    """(key words, first plane word, plane words, first base word, words in all) of a column of n records."""
    key_words = (n + 3) // 4 * 4 + 4                 # the next multiple of 4 keys plus one 16-byte load
    plane_at = (key_words * 4 + 31) // 32 * 8        # from a 32-byte boundary
    plane_words = (n + 255) // 256 * 8               # a whole 32-byte piece per 256 records
    return key_words, plane_at, plane_words, plane_at + plane_words, plane_at + plane_words + n_scaffolds + 1


def column(recs, n_scaffolds, base):
    """(keys, plane) of the records under a layout's base[]: base[ref] + pos, the sentinel for unplaced records, unknown scaffolds and the pad;
    bit i of the plane set where record i is placed on a known scaffold with MAPQ 0."""
    n = len(recs)
    key_words, _, plane_words, _, _ = parts(n, n_scaffolds)
    keys = np.full(key_words, SENTINEL, dtype=np.uint32)
    ok = recs["ref"] < n_scaffolds
    ref = np.where(ok, recs["ref"], 0).astype(np.int64)
    lin = base.astype(np.uint64)[ref] + recs["pos"].astype(np.uint64)
    assert not ok.any() or int(lin[ok].max()) < SENTINEL
    keys[:n][ok] = lin[ok].astype(np.uint32)
    bits = np.zeros(plane_words * 32, dtype=np.uint8)
    bits[:n] = ok & (recs["mapq"] == 0)
    plane = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return keys, plane
