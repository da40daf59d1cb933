"""Pipeline(read_support=True): how the reads of a closed gap's own pool back the k-mers of its fill — one fixed-size record per gap
(gf_fill_support, _lib.FILL_SUPPORT) after the last pick of the step (gf_fill_support_dev, csrc/fill_support.hip).  The reference has
no such check.  Results.support (the records) and .support_stats; single rank; not with second_round, whose pool is not the step's.

The definition is the host twin below (support_host).  For a closed gap with winning contig c (stored orientation):
  body      [b0, b1) = the bases of c strictly between the two flank hits of the pick.  "exact": the hits re-located by pick.hip's
            rule at the anchor length a of the pick word (locate_exact) — forward: b0 = leftmost left anchor + a, b1 = rightmost right
            anchor; reverse word: b0 = leftmost revcomp(right anchor) + a, b1 = rightmost revcomp(left anchor); a span that is not the
            word's (unsaturated) span field is a MISMATCH: zero record, counted, fetch() raises.  "align" / "gapped": from the contig's
            gf_ctg_pick (locate_pick): between the last base of the one alignment and the first of the other; alignments that touch or
            overlap give the empty body at b0;
  windows   starts s in [max(0, b0 - k + 1), min(len(c) - k, max(b1, b0) - 1)]: every k-window of c with a body base, the junction
            windows of an empty body; none when c is shorter than k.  A window with a byte other than A, C, G, T has support 0;
  support   the number of windows of the pool's reads (offsets 0 .. L - k of every row, windows over a masked base skipped — the
            assembly's count phase) whose canonical k-mer (kmer_dev.hpp: the smaller of the left-aligned 2-bit word and its reverse
            complement's, one 64-bit word for k <= 32, two above) is the window's;
  record    n_windows, n_zero (support 0), n_below (support < min_count), min, max, zero_run (longest run of consecutive zero-support
            windows: one wrong base gives about k, a foreign insert its length + k - 1), sum; all zero for an open gap.
The record does not depend on the orientation of the pick."""
import numpy as np
import torch

from . import _lib as B
from . import fill_rounds as FR
from . import pipeline as P
from .fill_rounds import _LUT
from .pick_contigs import revcomp

K_MIN, K_MAX = 16, 64


def check_k(k):
    if not K_MIN <= int(k) <= K_MAX:
        raise ValueError("support_k %r: %d..%d" % (k, K_MIN, K_MAX))
    return int(k)


def codes_of(reads):
    """Equal-length texts -> (2-bit codes, valid): a byte other than A, C, G, T is invalid (a masked base of a packed row)."""
    n = len(reads)
    L = len(reads[0]) if n else 0
    a = np.frombuffer("".join(reads).encode(), dtype=np.uint8).reshape(n, L) if n else np.zeros((0, 0), dtype=np.uint8)
    c = _LUT[a]
    return (c & 3).astype(np.uint8), c < 4


def codes_of_rows(rows, L, nmask=None):
    """Packed rows (gf_pack_reads: base i in byte i / 4, first base in the top bits) with their N-mask words (bit i % 32 of word i / 32),
    or None -> (codes, valid)."""
    if not len(rows):
        return np.zeros((0, L), dtype=np.uint8), np.ones((0, L), dtype=bool)
    rows = np.asarray(rows, dtype=np.uint8).reshape(len(rows), -1)
    i = np.arange(L)
    codes = (rows[:, i // 4] >> (6 - 2 * (i % 4)).astype(np.uint8)) & 3
    if nmask is None:
        return codes, np.ones(codes.shape, dtype=bool)
    m = np.asarray(nmask, dtype=np.uint32).reshape(len(rows), -1)
    return codes, ((m[:, i // 32] >> (i % 32).astype(np.uint32)) & 1) == 0


def _pack(win):
    """Left-aligned 64-bit words of windows of at most 32 codes (last axis)."""
    w = win.shape[-1]
    if w == 0:
        return np.zeros(win.shape[:-1], dtype=np.uint64)
    sh = (62 - 2 * np.arange(w)).astype(np.uint64)
    return np.bitwise_or.reduce(win.astype(np.uint64) << sh, axis=-1)


def canonical_keys(codes, valid, k):
    """Canonical k-mers of every window of every row: (keys, ok).  k <= 32: keys[r, p] is the one 64-bit word; k > 32: keys[r, p] =
    (hi, lo).  ok[r, p]: the window holds no invalid base."""
    n, L = codes.shape
    if L < k:
        return np.zeros((n, 0) + ((2,) if k > 32 else ()), dtype=np.uint64), np.zeros((n, 0), dtype=bool)
    win = np.lib.stride_tricks.sliding_window_view(codes, k, axis=1)
    ok = np.lib.stride_tricks.sliding_window_view(valid, k, axis=1).all(axis=-1)
    rc = 3 - win[..., ::-1]
    if k <= 32:
        f, r = _pack(win), _pack(rc)
        return np.minimum(f, r), ok
    fh, fl, rh, rl = _pack(win[..., :32]), _pack(win[..., 32:]), _pack(rc[..., :32]), _pack(rc[..., 32:])
    less = (rh < fh) | ((rh == fh) & (rl < fl))
    return np.stack([np.where(less, rh, fh), np.where(less, rl, fl)], axis=-1), ok


def _as_items(keys, k):
    return [int(x) for x in keys] if k <= 32 else [(int(h), int(l)) for h, l in keys]


def kmer_counts(codes, valid, k):
    """{canonical key: occurrences} over the valid windows of the rows."""
    keys, ok = canonical_keys(codes, valid, k)
    out = {}
    for key in _as_items(keys[ok], k):
        out[key] = out.get(key, 0) + 1
    return out


def window_range(n, b0, b1, k):
    """First and last evaluated window start of a contig of n bases with body [b0, b1) (last < first: none)."""
    return max(0, b0 - k + 1), min(n - k, max(b1, b0) - 1)


def window_supports(reads, contig, b0, b1, k):
    """The supports of the evaluated windows of `contig`, in window order.  reads: texts of one length (a byte other than A, C, G, T
    is a masked base) or (codes, valid) arrays."""
    k = check_k(k)
    lo, hi = window_range(len(contig), int(b0), int(b1), k)
    if hi < lo:
        return []
    codes, valid = codes_of(reads) if isinstance(reads, (list, tuple)) and (not reads or isinstance(reads[0], str)) else reads
    cnt = kmer_counts(codes, valid, k) if len(codes) else {}
    cc, cv = codes_of([contig[lo:hi + k]])
    keys, ok = canonical_keys(cc, cv, k)
    return [cnt.get(key, 0) if good else 0 for key, good in zip(_as_items(keys[0], k), ok[0])]


def record_of(sup, min_count):
    """gf_fill_support of a list of window supports."""
    rec = np.zeros((), dtype=B.FILL_SUPPORT)
    if not sup:
        return rec
    run = best = 0
    for s in sup:
        run = run + 1 if s == 0 else 0
        best = max(best, run)
    rec["n_windows"], rec["n_zero"], rec["n_below"] = len(sup), sum(s == 0 for s in sup), sum(s < min_count for s in sup)
    rec["min"], rec["max"], rec["zero_run"], rec["sum"] = min(sup), max(sup), best, sum(sup)
    return rec


def support_host(reads, contig, b0, b1, k, min_count=2):
    """The record of one closed gap: the pool's reads, the winning contig as stored, its body [b0, b1)."""
    return record_of(window_supports(reads, contig, b0, b1, k), int(min_count))


def locate_exact(contig, left_flank, right_flank, a, reverse):
    """The body of an exact pick at anchor length a, or None when an anchor is not there (pick.hip's hits; module docstring)."""
    a = int(a)
    if len(left_flank) < a or len(right_flank) < a:
        return None
    la, ra = left_flank[len(left_flank) - a:], right_flank[:a]
    if any(c not in "ACGT" for c in la + ra):
        return None
    first, last = (revcomp(ra), revcomp(la)) if reverse else (la, ra)
    i, j = contig.find(first), contig.rfind(last)
    if i < 0 or j < 0 or j < i + a:
        return None
    return i + a, j


def locate_pick(p, reverse):
    """The body between the two alignments of a gf_ctg_pick (1-based positions, aligned lengths)."""
    lp, rp, lm, rm = int(p["lp"]), int(p["rp"]), int(p["lm"]), int(p["rm"])
    b0, b1 = (rp - 1 + rm, lp - 1) if reverse else (lp - 1 + lm, rp - 1)
    return b0, max(b0, b1)


def locate(word, contig, flanks_of_gap, ctg_pick_entry):
    """(b0, b1) of a pick word on its winning contig, or None: a mismatch."""
    a_len, span1, _, rev = P.decode_best(word)
    if ctg_pick_entry is not None:
        return locate_pick(ctg_pick_entry, rev) if int(ctg_pick_entry["threshold"]) else None
    body = locate_exact(contig, flanks_of_gap[0], flanks_of_gap[1], a_len, rev)
    if body is None:
        return None
    span = body[1] - body[0] + 1
    return body if (span == span1 if span1 < 0xFFFFFF else span >= span1) else None


def support_of_results(res, flanks, L, k, min_count=2, nmask=None):
    """The twin over a whole step: (records, stats) from fetch(pools=True)'s pools and the fetched contigs and picks."""
    out = np.zeros(len(res.best), dtype=B.FILL_SUPPORT)
    stats = {"gaps": 0, "mismatches": 0, "windows": 0}
    for g, contig, body in FR.closed_fills(res, flanks):
        if body is None:
            stats["mismatches"] += 1
            continue
        reads = FR.fill_reads(res, g, L, nmask)
        out[g] = support_host(reads, contig, body[0], body[1], k, min_count)
        stats["gaps"] += 1
        stats["windows"] += int(out[g]["n_windows"])
    return out, stats


class ReadSupport(FR.FillRound):
    WHAT, RECORD = "read support", B.FILL_SUPPORT

    def __init__(self, pipe, k):
        super().__init__(pipe)
        self.k = check_k(k)

    def prepare(self):
        p = self.p
        self.d_rec = p._u8(max(1, p.n_gaps) * B.FILL_SUPPORT.itemsize)
        self.d_stats = torch.zeros(B.FS_WORDS, dtype=torch.int32, device=p.dev)

    def _launch(self, d_nmask):
        """On the pool the step assembled."""
        p = self.p
        p._chk(p.lib.gf_fill_support_dev(p.h, *self.pool_args(d_nmask), p.L, *self.shared_args(), self.k, p.min_count,
                                         self.d_rec.data_ptr(), self.d_stats.data_ptr()), "gf_fill_support_dev")

    def fetch(self, r):
        st = self.d_stats.cpu().numpy().view(np.uint32)
        r.support_stats = {"gaps": int(st[B.FS_GAPS]), "mismatches": int(st[B.FS_MISMATCH]), "windows": P.counter_u64(st, B.FS_WINDOWS), "k": self.k}
        self.check_mismatches(r.support_stats["mismatches"])
        r.support = self.records()[0]
