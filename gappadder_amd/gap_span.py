"""Pipeline(gap_span=True): the size of every gap of the draft, open or closed, measured from the read pairs that span it — per library,
the pairs whose two mates map cleanly to the draft on either side of a gap are gathered from the library's alignment records, and one
64-byte record per (library, gap) holds their number, the sum and the sum of squares of their observed template lengths and the pairs
that were looked at and dropped (gf_gap_span, _lib.GAP_SPAN; gf_gap_span_dev, csrc/gap_span.hip), once per step on the context and
stream of the library's tagger.  It reads the library's records and the gap table and nothing else: neither the recruitment nor a contig.
Results.gap_span ([n_lib, n_gaps]) and .gap_span_stats (a dictionary per library); single rank — the sums are additive over ranks, and
that reduction is left out.  Nothing else of the step changes.  DESIGN.md §21.

The definition is the host twin below (gap_span_host).  Parameters: the library's is_mean mu and is_sd sigma, the read length L, an
integer z >= 1, an integer shift D >= 0 (how far off the draft's N-run may be) and q = the pipeline's anchor_mapq.
  derived      dist2 = mu + 3 sigma (the tagger's own window: its bin map for the library serves unchanged), lo = mu - z sigma - D,
               hi = mu + z sigma + D; hi < 2^20 is required, so the sum of tlen^2 stays inside 64 bits for any record count below 2^32;
  gaps         gap g lies on scaffold s at [start, end), G0 = end - start; gaps are grouped by scaffold and ascend inside a scaffold;
  candidates   record A is a candidate of gap g iff flag & 1, flag & (4 | 8 | 0x100 | 0x800) == 0, A is forward (flag & 0x10 == 0) and
               its mate reverse (flag & 0x20), ref == mate_ref == s < n_scaffolds, pos >= 1, mate_pos >= 1, tlen > 0, with A0 = pos - 1:
               A0 + L <= start and start - A0 <= dist2 (the tagger's left window with the read clear of the N-run), and with
               M0 = mate_pos - 1, M1 = A0 + tlen: end <= M0 < M1.  Every pair is seen once, through its leftmost forward record.  THE
               MATE'S OWN MAPQ AND CLIP FLAG ARE NOT IN A's RECORD AND ARE NOT CONSULTED;
  classes      a candidate lands in exactly one counter, the tests applied in this order: n_multi — another gap of the scaffold meets
               [A0, M1): end[g - 1] > A0 or start[g + 1] < M1, each only when that gap exists on scaffold s; n_clipped — clipflag != 0;
               n_lowq — mapq < q; n_low — tlen < lo; n_high — tlen > hi; accepted otherwise: n, sum (i64, of tlen), sum_sq (u64, of
               tlen^2), tlen_min, tlen_max (both 0 when n == 0);
  record       flags (GS_F_PAIRS iff n >= 1), n_cand (all of the above together), n, n_multi, n_clipped, n_lowq, n_low, n_high,
               tlen_min, tlen_max, sum, sum_sq.  Order-free integers: the device equals the twin byte for byte;
  statistics   candidates, accepted, multi, clipped, lowq, low, high over the gaps, and the gaps with n >= 1.

The estimate (estimate(); floating point on the exact integers, host only).  naive = G0 + mu - sum / n.  It is biased: only pairs that
CAN span are seen.  The model: inserts x follow the discrete normal (mu, sigma) over |x - mu| <= 6 sigma.  A pair of insert x over a gap
of true size G is seen with weight w(x; G) = max(0, min(dist2, x - G - L) - L + 1) — the places of A0 with the read clear of the gap, inside
the window, and the mate beyond the gap — at the observed t = x - G + G0, when lo <= t <= hi.  m(G) is the expected accepted t
(expected_mean); est is the G in [0, hi - 2 L] where m(G) meets sum / n, found by bisection (m does not increase with G; where it is
undefined because every spanning insert would be seen beyond hi it counts as +inf, where none spans or all fall below lo as -inf); se =
sd(t) / sqrt(n) / max(m(est) - m(est + 1), eps).  Where the model degenerates: G + 2 L far above mu — only the upper tail of the inserts
spans, their mean grows almost as fast as G, the slope of m goes to 0 and with it the information in the mean (se grows without bound;
where no insert of the support spans at all, m is undefined and est stops below that)."""
import collections
import math

import numpy as np

from . import _lib as B

Z, SHIFT, MIN_PAIRS = 3, 1000, 8
HI_LIMIT = 1 << 20
STAT_KEYS = ("candidates", "accepted", "multi", "clipped", "lowq", "low", "high", "gaps_with_pairs")
COUNTERS = ("n_multi", "n_clipped", "n_lowq", "n_low", "n_high")
Estimate = collections.namedtuple("Estimate", "naive est se")


def check_params(z=Z, shift=SHIFT, min_pairs=MIN_PAIRS):
    """(z, shift, min_pairs) as integers; ValueError for a value out of range (the ABI answers GF_E_UNSUPPORTED)."""
    out = []
    for name, v, lo in (("span_z", z, 1), ("span_shift", shift, 0), ("span_min_pairs", min_pairs, 1)):
        try:
            iv = int(v)
        except (TypeError, ValueError):
            iv = None
        if iv is None or isinstance(v, bool) or iv != v or iv < lo:
            raise ValueError("gap_span %s %r: an integer, at least %d" % (name, v, lo))
        out.append(iv)
    return tuple(out)


def window(is_mean, is_sd, z=Z, shift=SHIFT):
    """(dist2, lo, hi) of a library; ValueError when the library is out of the range the sums are defined for."""
    mu, sd = int(is_mean), int(is_sd)
    if mu < 0 or sd < 0:
        raise ValueError("gap_span: is_mean %r and is_sd %r must not be negative" % (is_mean, is_sd))
    hi = mu + int(z) * sd + int(shift)
    if hi >= HI_LIMIT:
        raise ValueError("gap_span: is_mean + span_z * is_sd + span_shift = %d: below 2^20 (the sum of squares is kept in 64 bits)" % hi)
    return mu + 3 * sd, mu - int(z) * sd - int(shift), hi


def gap_span_host(recs, gaps, n_scaffolds, L, is_mean, is_sd, z=Z, shift=SHIFT, min_mapq=30):
    """The records of one library against the gap table: (gf_gap_span per gap, the statistics dictionary).  recs: _lib.ALNREC; gaps:
    _lib.GAP, grouped by scaffold, ascending inside a scaffold."""
    z, shift, _ = check_params(z, shift)
    dist2, lo, hi = window(is_mean, is_sd, z, shift)
    L, q = int(L), int(min_mapq)
    gaps = np.asarray(gaps)
    out = np.zeros(len(gaps), dtype=B.GAP_SPAN)
    flag = recs["flag"].astype(np.int64)
    ok = ((flag & 1) != 0) & ((flag & (4 | 8 | 0x100 | 0x800)) == 0) & ((flag & 0x10) == 0) & ((flag & 0x20) != 0)
    ok &= (recs["ref"] == recs["mate_ref"]) & (recs["ref"] < int(n_scaffolds)) & (recs["pos"] >= 1) & (recs["mate_pos"] >= 1) & (recs["tlen"] > 0)
    r = recs[ok]
    order = np.lexsort((r["pos"], r["ref"]))
    r = r[order]
    ref, a0 = r["ref"].astype(np.int64), r["pos"].astype(np.int64) - 1
    m0, tlen = r["mate_pos"].astype(np.int64) - 1, r["tlen"].astype(np.int64)
    m1 = a0 + tlen
    key = (ref << 32) | a0                              # ascending: one searchsorted per gap
    scaf, start, end = gaps["scaffold"].astype(np.int64), gaps["start"].astype(np.int64), gaps["end"].astype(np.int64)
    for g in range(len(gaps)):
        s, st, en = int(scaf[g]), int(start[g]), int(end[g])
        if st - L < 0:
            continue
        i0 = np.searchsorted(key, (s << 32) | max(0, st - dist2), side="left")        # st - dist2 <= A0 <= st - L
        i1 = np.searchsorted(key, (s << 32) | (st - L), side="right")
        if i1 <= i0:
            continue
        sl = slice(i0, i1)
        c = (m0[sl] >= en) & (m0[sl] < m1[sl])
        if not c.any():
            continue
        ca0, cm1, ct = a0[sl][c], m1[sl][c], tlen[sl][c]
        cclip, cq = r["clipflag"][sl][c], r["mapq"][sl][c].astype(np.int64)
        multi = np.zeros(len(ct), dtype=bool)
        if g > 0 and scaf[g - 1] == s:
            multi |= end[g - 1] > ca0
        if g + 1 < len(gaps) and scaf[g + 1] == s:
            multi |= start[g + 1] < cm1
        rest = ~multi
        clipped = rest & (cclip != 0)
        rest &= ~clipped
        lowq = rest & (cq < q)
        rest &= ~lowq
        low = rest & (ct < lo)
        rest &= ~low
        high = rest & (ct > hi)
        rest &= ~high
        rec = out[g]
        rec["n_cand"] = len(ct)
        for f, m in zip(COUNTERS, (multi, clipped, lowq, low, high)):
            rec[f] = int(m.sum())
        n = int(rest.sum())
        if n:
            t = ct[rest]
            rec["flags"], rec["n"], rec["sum"], rec["sum_sq"] = B.GS_F_PAIRS, n, int(t.sum()), int((t.astype(np.uint64) ** 2).sum())
            rec["tlen_min"], rec["tlen_max"] = int(t.min()), int(t.max())
    return out, stats_of_records(out)


def stats_of_records(rec):
    """The statistics dictionary (STAT_KEYS) of a plane of records."""
    tot = {k: int(rec[f].astype(np.uint64).sum()) for k, f in (("candidates", "n_cand"), ("accepted", "n"), ("multi", "n_multi"),
                                                              ("clipped", "n_clipped"), ("lowq", "n_lowq"), ("low", "n_low"), ("high", "n_high"))}
    tot["gaps_with_pairs"] = int((rec["n"] >= 1).sum())
    return tot


def stats_of(words):
    """The statistics words of gf_gap_span_dev (u32[GS_WORDS]) as the twin's dictionary."""
    st = np.ascontiguousarray(words).view(np.uint32)
    d = {k: int(st[2 * i:2 * i + 2].view(np.uint64)[0]) for i, k in enumerate(STAT_KEYS[:7])}
    d["gaps_with_pairs"] = int(st[B.GS_GAPS_WITH_PAIRS])
    return d


def _model(G, G0, L, mu, sigma, z, D):
    """(sum of weights, sum of weights * t) of the model of the module docstring at true gap size G."""
    mu, sigma, L = float(mu), float(sigma), int(L)
    dist2, lo, hi = mu + 3 * sigma, mu - z * sigma - D, mu + z * sigma + D
    x = np.arange(math.ceil(mu - 6 * sigma), math.floor(mu + 6 * sigma) + 1, dtype=np.float64)
    p = np.exp(-0.5 * ((x - mu) / sigma) ** 2) if sigma > 0 else np.ones_like(x)
    w = np.maximum(0.0, np.minimum(dist2, x - G - L) - L + 1)
    t = x - G + G0
    w = np.where((t >= lo) & (t <= hi), w * p, 0.0)
    return float(w.sum()), float((w * t).sum())


def expected_mean(G, G0, L, mu, sigma, z=Z, D=SHIFT):
    """m(G): the expected accepted template length over a gap of true size G that the draft states as G0; None where no pair is seen."""
    sw, swt = _model(G, G0, L, mu, sigma, z, D)
    return swt / sw if sw > 0 else None


def estimate(rec, G0, L, mu, sigma, z=Z, D=SHIFT, min_pairs=MIN_PAIRS):
    """Estimate(naive, est, se) of a gf_gap_span record, or None when it has fewer than min_pairs accepted pairs (module docstring)."""
    n = int(rec["n"])
    if n < int(min_pairs) or n < 1:
        return None
    mean = int(rec["sum"]) / n
    naive = G0 + mu - mean
    hi = mu + z * sigma + D

    lo, x_max = mu - z * sigma - D, math.floor(mu + 6 * sigma)

    def m(G):
        """m(G), continued where it is undefined: +inf where every spanning insert is seen beyond hi (G far below G0), -inf where none
        spans or all are seen below lo (G too large)."""
        v = expected_mean(G, G0, L, mu, sigma, z, D)
        if v is not None:
            return v
        return -math.inf if x_max - G < 2 * L or x_max - G + G0 < lo else math.inf
    a, b = 0, max(0, int(hi) - 2 * int(L))              # bisection: m(a) >= mean > m(b)
    va, vb = m(a), m(b)
    if va <= mean:
        est = float(a)
    elif vb >= mean:
        est = float(b)
    else:
        while b - a > 1:
            mid = (a + b) // 2
            v = m(mid)
            if v >= mean:
                a, va = mid, v
            else:
                b, vb = mid, v
        est = float(b) if math.isinf(va) else float(a) if math.isinf(vb) or va <= vb else a + (va - mean) / (va - vb)
    var = max(0.0, int(rec["sum_sq"]) / n - mean * mean)
    m0, m1 = m(est), m(est + 1)
    slope = (m0 - m1) if math.isfinite(m0) and math.isfinite(m1) else 0.0
    return Estimate(naive, est, math.sqrt(var) / math.sqrt(n) / max(slope, 1e-6))


def gap_span_of_results(libs_recs, libs, gaps, n_scaffolds, L, z=Z, shift=SHIFT, min_mapq=30):
    """The twin over a step's libraries: (records [n_lib, n_gaps], a statistics dictionary per library).  libs_recs: the fetched records of
    every library; libs: (is_mean, is_sd) per library."""
    out = np.zeros((len(libs), len(gaps)), dtype=B.GAP_SPAN)
    stats = []
    for l, ((mu, sd), recs) in enumerate(zip(libs, libs_recs)):
        out[l], st = gap_span_host(recs, gaps, n_scaffolds, L, mu, sd, z, shift, min_mapq)
        stats.append(st)
    return out, stats


class GapSpan:
    """The round object the Pipeline holds: prepare() allocates a record plane and a block of statistics words per library, enqueue(lb)
    launches one library's pass behind its tagger (same context, same stream), fetch(r) fills Results.gap_span and .gap_span_stats."""

    def __init__(self, pipe, z=Z, shift=SHIFT, min_pairs=MIN_PAIRS):
        self.p = pipe
        self.z, self.shift, self.min_pairs = check_params(z, shift, min_pairs)
        self.d_rec = None

    def check_library(self, lb):
        window(lb.is_mean, lb.is_sd, self.z, self.shift)

    def prepare(self):
        import torch
        p = self.p
        for lb in p.libs:
            self.check_library(lb)
        self.plane = max(1, p.n_gaps) * B.GAP_SPAN.itemsize
        self.d_rec = torch.zeros(len(p.libs) * self.plane, dtype=torch.uint8, device=p.dev)
        self.d_stats = torch.zeros(len(p.libs) * B.GS_WORDS, dtype=torch.int32, device=p.dev)
        torch.cuda.synchronize()

    def enqueue(self, lb):
        """One launch sequence for library lb, on the context its tagger runs on.  Before prepare() (no buffers yet): nothing."""
        if self.d_rec is None:
            return
        p, l = self.p, self.p.libs.index(lb)
        keys = lb.d_rec_keys.data_ptr() if (p.key_column and lb.d_rec_keys is not None) else None
        p._chk(p.lib.gf_gap_span_dev(lb.h2, lb.d_recs.data_ptr(), keys, lb.n_recs, p.L, lb.is_mean, lb.is_sd, self.z, self.shift, p.anchor_mapq,
                                     self.d_rec.data_ptr() + l * self.plane, self.d_stats.data_ptr() + 4 * l * B.GS_WORDS), "gf_gap_span_dev")

    def fetch(self, r):
        p = self.p
        st = self.d_stats.cpu().numpy().reshape(len(p.libs), B.GS_WORDS)
        r.gap_span_stats = [stats_of(st[l]) for l in range(len(p.libs))]
        n = p.n_gaps * B.GAP_SPAN.itemsize
        raw = np.ascontiguousarray(self.d_rec.cpu().numpy().reshape(len(p.libs), -1)[:, :n])
        r.gap_span = np.frombuffer(raw.tobytes(), dtype=B.GAP_SPAN).reshape(len(p.libs), p.n_gaps)
