"""Pipeline(pair_span=True, pair_anchors=True): the anchored pair span — the pair-span round (pair_span.py) needs BOTH
mates of a pair on the winning contig, which is shorter than a mate-pair insert; this extension pairs a mate the tagger found ANCHORED in
a flank of the gap, at its draft coordinate, with the placement of the other mate on the contig, and so measures the length of the fill
against the library's insert size (gf_fill_anchors, _lib.FILL_ANCHORS; gf_fill_pairs_anchored_dev, csrc/fill_anchor.hip).
Results.pair_anchors ([n_lib, n_gaps]) and .pair_anchor_stats (a dictionary per library).  The reference has no such stage.

The definition is the host twin below.  Per library and closed gap g; the contig c of n bases, the strand bit rev, the body [b0, b1) and
the MISMATCH, LONG and NON_ACGT rules are pair_span.py's:
  anchors     a tagger hit h (of the library's hits [0, min(count, hit_cap))) with to_mate == 1 and kind DISCORDANT or UNMAP says: record
              A = recs[h.rec] lies in a flank of gap h.gap and A's mate B = A.read ^ 1 was recruited for it.  Kept when A has clipflag == 0
              (the record carries no CIGAR: a clipped record's leftmost base is unknown), flag & (0x100 | 0x800) == 0, flag & 4 == 0, a
              read, A0 = A.pos - 1 < gap.start (a LEFT anchor) or >= gap.end (a RIGHT one), and B has a row in the gap's id slice.  Every
              other hit is dropped and counted (scatter_host).  Several kept hits of one (g, B): the smallest (A0 << 1 | sA) counts,
              sA = (flag >> 4) & 1;
  placement   of A on the stored contig, virtual, signed and unbounded (L: the read length):
                  rev = 0, strand sA:      col = b0 - (start - A0) (left),      b1 + (A0 - end) (right)
                  rev = 1, strand 1 - sA:  col = b1 + (start - A0) - L (left),  b0 - (A0 - end) - L (right)
  pairs       a row B with an anchor: n_anchored; B PLACED at (strand, d) by pair_span.py's placement: a placed pair of A and B, and
              pair_span.py's rules word for word: proper (opposite strands, d_f <= d_r) or misoriented, insert = d_r + L - d_f, in range
              iff lo < insert < hi (lo, hi = is_mean -/+ z * is_sd), short, long, spanning iff d_f <= b0 and b1 <= d_r + L;
  coverage    every in-range pair covers the columns [max(0, d_f), min(n, d_r + L)) and carries dev = insert - is_mean.  Over the body:
              min_cover, min_col, n_unspanned as in pair_span.py; among the columns covered by at least min_pairs pairs (n_eval) the one
              with the smallest mean dev (dev_min_col, dev_min_n, dev_min_sum) and the one with the largest (dev_max_*); means compared
              exactly (cross-multiplied integers), a tie goes to the smaller column.  A fill with D bases missing at column p lowers the
              insert of every pair over p: dev_min_sum / dev_min_n is about -D there; z_score() is dev_sum / (is_sd * sqrt(n));
  record      FILL_ANCHORS; all zero for an open gap or a mismatch, flags and rows for a skipped contig.  z * is_sd < 2^20.
Order-free integers: the device equals the twin."""
import math

import numpy as np
import torch

from . import _lib as B
from . import fill_rounds as FR
from . import pair_span as PSP
from . import pipeline as P
from . import polish as POL

SEED, MAX_MISMATCH, MIN_OVERLAP, Z = 16, 4, 48, 3       # (pair_span's defaults; its names are not there yet when the package is imported through it)
MIN_PAIRS = 8
NO_READ = 0xFFFFFFFF
COUNT_FIELDS = ("n_anchored", "n_placed", "n_proper", "n_misoriented", "n_in_range", "n_short", "n_long", "n_left", "n_span")
HIT_KEYS = ("kept", "dropped_clipped", "dropped_in_gap", "dropped_secondary", "absent", "dropped_other")        # (the words PA_KEPT ...)
STAT_KEYS = ("gaps", "mismatches", "skipped_long", "skipped_non_acgt") + HIT_KEYS + ("anchored", "placed", "proper", "in_range", "span")
FIELDS = tuple(B.FILL_ANCHORS.names)



def check_params(L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, z=Z, is_sd=0, min_pairs=MIN_PAIRS):
    """pair_span.check_params' four parameters and min_pairs as integers; ValueError for a value out of range (the ABI answers
    GF_E_UNSUPPORTED)."""
    out = PSP.check_params(L, seed, max_mismatch, min_overlap, z, is_sd)
    mp = int(min_pairs)
    if mp < 1 or mp != min_pairs:
        raise ValueError("pair_anchors min_pairs %r: an integer, at least 1" % (min_pairs,))
    if out[3] * int(is_sd) >= 1 << 20:
        raise ValueError("pair_anchors z %d with is_sd %d: z * is_sd below 2^20" % (out[3], int(is_sd)))
    return out + (mp,)


def scatter_host(hits, recs, gaps, off, ids, hit_cap=None):
    """The anchors of one library: ({pool row: (A0, sA)}, a dictionary of HIT_KEYS) from its tagger hits (TAGHIT; the first hit_cap of
    them), its records (ALNREC), the gap table (GAP) and the library's pool offsets and read ids."""
    st = dict.fromkeys(HIT_KEYS, 0)
    best = {}
    n_gaps = len(off) - 1
    row_of = [None] * n_gaps
    for h in hits[:len(hits) if hit_cap is None else int(hit_cap)]:
        g, k = int(h["gap"]), int(h["rec"])
        if int(h["to_mate"]) != 1 or int(h["kind"]) not in (B.KIND_DISCORDANT, B.KIND_UNMAP) or k >= len(recs) or g >= n_gaps:
            st["dropped_other"] += 1
            continue
        A = recs[k]
        flag, own = int(A["flag"]), int(A["read"]) & 0xFFFFFFFF
        if int(A["clipflag"]):
            st["dropped_clipped"] += 1
            continue
        if flag & (0x100 | 0x800):
            st["dropped_secondary"] += 1
            continue
        if flag & 4 or own == NO_READ or int(A["pos"]) == 0:
            st["dropped_other"] += 1
            continue
        A0 = int(A["pos"]) - 1
        if int(gaps[g]["start"]) <= A0 < int(gaps[g]["end"]):
            st["dropped_in_gap"] += 1
            continue
        if row_of[g] is None:
            r0 = int(off[g])
            row_of[g] = {int(r): r0 + i for i, r in enumerate(ids[r0:int(off[g + 1])])}
        row = row_of[g].get(own ^ 1)
        if row is None:
            st["absent"] += 1
            continue
        st["kept"] += 1
        key = (A0 << 1) | ((flag >> 4) & 1)
        if row not in best or key < best[row]:
            best[row] = key
    return {row: (key >> 1, key & 1) for row, key in best.items()}, st


def virtual_placement(A0, sA, rev, b0, b1, start, end, L):
    """(strand, column, left?) of an anchor on the stored contig (module docstring)."""
    left = A0 < start
    if not rev:
        return sA, (b0 - (start - A0) if left else b1 + (A0 - end)), left
    return 1 - sA, (b1 + (start - A0) - L if left else b0 - (A0 - end) - L), left


def anchors_host(reads, ids, anchors, contig, b0, b1, rev, gap, is_mean, is_sd, seed=SEED, max_mismatch=MAX_MISMATCH,
                 min_overlap=MIN_OVERLAP, z=Z, min_pairs=MIN_PAIRS, L=None, where=None):
    """gf_fill_anchors of one closed gap and one library: the library's pool rows for the gap (as pair_span_host takes them) with their
    read ids, per row None or the anchor (A0, sA) of its mate, the winning contig as stored, its body [b0, b1), the word's strand bit and
    the gap's (start, end) on the draft.  L: the read length, for an empty pool; where: the rows' placements (polish.placements with the
    same parameters) when the caller has them already."""
    codes, valid = POL._reads(reads)
    L = codes.shape[1] if len(codes) else L
    s, mm_max, mo, zz, mp = check_params(L if L is not None else 1 << 20, seed, max_mismatch, min_overlap, z, is_sd, min_pairs)
    assert len(ids) == len(codes) == len(anchors), "one id and one anchor entry per row"
    b0, b1 = int(b0), max(int(b0), int(b1))
    start, end = int(gap[0]), int(gap[1])
    n = len(contig)
    rec = np.zeros((), dtype=B.FILL_ANCHORS)
    rec["rows"] = len(ids)
    flag = FR.skip_flag(contig, B.PS_F_LONG, B.PS_F_NON_ACGT)
    if flag:
        rec["flags"] = flag
        return rec
    rec["n_cols"] = b1 - b0
    if where is None:
        where = POL.placements((codes, valid), contig, s, mm_max, mo) if len(codes) else []
    is_mean = int(is_mean)
    lo, hi = is_mean - zz * int(is_sd), is_mean + zz * int(is_sd)
    cnt = dict.fromkeys(COUNT_FIELDS, 0)
    span_sum = dev_sum = 0
    cov, dev = [0] * (n + 1), [0] * (n + 1)
    for i, a in enumerate(anchors):
        if a is None:
            continue
        cnt["n_anchored"] += 1
        w = where[i]
        if w is None or w == "ambiguous":
            continue
        cnt["n_placed"] += 1
        str_a, col, left = virtual_placement(int(a[0]), int(a[1]), rev, b0, b1, start, end, L)
        d_f, d_r = (w[1], col) if str_a else (col, w[1])
        if str_a == w[0] or d_f > d_r:
            cnt["n_misoriented"] += 1
            continue
        cnt["n_proper"] += 1
        insert = d_r + L - d_f
        in_range = lo < insert < hi
        cnt["n_in_range" if in_range else "n_short" if insert <= lo else "n_long"] += 1
        if d_f <= b0 and b1 <= d_r + L:
            cnt["n_span"] += 1
            span_sum += insert
        if in_range:
            cnt["n_left"] += bool(left)
            dev_sum += insert - is_mean
            x0, x1 = min(n, max(0, d_f)), min(n, max(0, d_r + L))
            cov[x0] += 1
            cov[x1] -= 1
            dev[x0] += insert - is_mean
            dev[x1] -= insert - is_mean
    for f in COUNT_FIELDS:
        rec[f] = cnt[f]
    rec["span_insert_sum"], rec["dev_sum"] = span_sum, dev_sum
    if b1 > b0:
        c_run = s_run = 0
        cover, sums = [], []
        for c in range(b1):
            c_run += cov[c]
            s_run += dev[c]
            if c >= b0:
                cover.append(c_run)
                sums.append(s_run)
        rec["min_cover"], rec["min_col"], rec["n_unspanned"] = min(cover), b0 + cover.index(min(cover)), sum(1 for v in cover if v == 0)
        mn = mx = None                           # (column, pairs, sum)
        for c, (k, v) in enumerate(zip(cover, sums), b0):
            if k < mp:
                continue
            rec["n_eval"] += 1
            if mn is None or v * mn[1] < mn[2] * k:             # v / k < mn.sum / mn.n, exactly; an equal mean keeps the smaller column
                mn = (c, k, v)
            if mx is None or v * mx[1] > mx[2] * k:
                mx = (c, k, v)
        if mn is not None:
            rec["dev_min_col"], rec["dev_min_n"], rec["dev_min_sum"] = mn
            rec["dev_max_col"], rec["dev_max_n"], rec["dev_max_sum"] = mx
    return rec


def add_to_stats(stats, rec):
    """One examined or skipped gap's record into a statistics dictionary (STAT_KEYS)."""
    f = int(rec["flags"])
    stats["skipped_long"] += bool(f & B.PS_F_LONG)
    stats["skipped_non_acgt"] += bool(f & B.PS_F_NON_ACGT)
    stats["gaps"] += not f
    for key, field in (("anchored", "n_anchored"), ("placed", "n_placed"), ("proper", "n_proper"), ("in_range", "n_in_range"), ("span", "n_span")):
        stats[key] += int(rec[field])


def anchors_of_results(res, flanks, L, libs, gaps, recs, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, z=Z,
                       min_pairs=MIN_PAIRS, nmasks=None, hit_caps=None):
    """The twin over a whole step: (records [n_lib, n_gaps], a statistics dictionary per library) from fetch(pools=True)'s per-library
    pools, read ids and tagger hits (lib_pool_off, lib_pool_rows, lib_pool_ids, lib_taghits) and the fetched contigs and picks.  libs:
    (is_mean, is_sd) per library; gaps: the gap table (GAP); recs: per library its records (ALNREC); nmasks: as pair_span_of_results."""
    out = np.zeros((len(libs), len(res.best)), dtype=B.FILL_ANCHORS)
    stats = [dict.fromkeys(STAT_KEYS, 0) for _ in libs]
    for l, (is_mean, is_sd) in enumerate(libs):
        check_params(L, seed, max_mismatch, min_overlap, z, is_sd, min_pairs)
        off, rows, ids = res.lib_pool_off[l], res.lib_pool_rows[l], res.lib_pool_ids[l]
        at, hit_stats = scatter_host(res.lib_taghits[l], recs[l], gaps, off, ids, None if hit_caps is None else hit_caps[l])
        stats[l].update(hit_stats)
        nm = None if nmasks is None else nmasks[l]
        for g, contig, body in FR.closed_fills(res, flanks):
            if body is None:
                stats[l]["mismatches"] += 1
                continue
            r0, r1, reads = FR.pool_reads(off, rows, g, L, nm)
            out[l, g] = anchors_host(reads, ids[r0:r1], [at.get(i) for i in range(r0, r1)], contig, body[0], body[1], P.decode_best(res.best[g])[3],
                                     (int(gaps[g]["start"]), int(gaps[g]["end"])), is_mean, is_sd, seed, max_mismatch, min_overlap, z, min_pairs, L)
            add_to_stats(stats[l], out[l, g])
    return out, stats


def stats_of(words):
    """The statistics words of gf_fill_pairs_anchored_dev (u32[PA_WORDS]) as anchors_of_results' dictionary."""
    st = np.asarray(words).view(np.uint32)
    out = {"gaps": int(st[B.PA_GAPS]), "mismatches": int(st[B.PA_MISMATCH]), "skipped_long": int(st[B.PA_SKIPPED_LONG]),
           "skipped_non_acgt": int(st[B.PA_SKIPPED_NON_ACGT])}
    out.update({k: int(st[B.PA_KEPT + i]) for i, k in enumerate(HIT_KEYS)})
    out.update({k: P.counter_u64(st, w) for k, w in (("anchored", B.PA_ANCHORED), ("placed", B.PA_PLACED), ("proper", B.PA_PROPER),
                                                     ("in_range", B.PA_IN_RANGE), ("span", B.PA_SPAN))})
    return out


def dev_means(rec):
    """(dev_min_sum // dev_min_n, dev_max_sum // dev_max_n) of a record, or (None, None) without an evaluated column."""
    if not int(rec["n_eval"]):
        return None, None
    return int(rec["dev_min_sum"]) // int(rec["dev_min_n"]), int(rec["dev_max_sum"]) // int(rec["dev_max_n"])


def z_score(dev_sum, n, is_sd):
    """dev_sum / (is_sd * sqrt(n)): the deviation of n pairs' mean insert from is_mean in standard errors; None without pairs or spread."""
    return int(dev_sum) / (int(is_sd) * math.sqrt(int(n))) if int(n) and int(is_sd) else None


class PairAnchors(FR.FillRound):
    WHAT, RECORD = "pair anchors", B.FILL_ANCHORS

    def __init__(self, pipe, min_pairs=MIN_PAIRS, read_len=None):
        super().__init__(pipe)
        self.min_pairs = check_params(read_len, *pipe.pairs.params, min_pairs=min_pairs)[4]

    def prepare(self):
        """A record plane and a block of statistics words per library; one anchor word per row of a library's pool array, shared by the
        libraries' launches like the pair span's placement words."""
        p = self.p
        if p.tag_ahead:
            raise ValueError("pair_anchors with tag_ahead: the next step's tagger rewrites the hits this round reads")
        for lb in p.libs:
            check_params(p.L, *p.pairs.params, is_sd=lb.is_sd, min_pairs=self.min_pairs)
        self.plane = max(1, p.n_gaps) * B.FILL_ANCHORS.itemsize
        self.d_rec = p._u8(len(p.libs) * self.plane)
        self.d_stats = torch.zeros(len(p.libs) * B.PA_WORDS, dtype=torch.int32, device=p.dev)
        self.d_anchor = torch.zeros(p.lib_cap, dtype=torch.int64, device=p.dev)

    def launch_library(self, l):
        """Library l's call: directly behind its gf_fill_pairs_dev (PairSpan._launch), whose placement words it reads."""
        if self.d_rec is None:
            return
        p, lb = self.p, self.p.libs[l]
        p._chk(p.lib.gf_fill_pairs_anchored_dev(p.h, lb.d_pool_off.data_ptr(), lb.d_ids.data_ptr(), p.lib_cap, p.L, *self.shared_args(),
                                                p.pairs.d_scratch.data_ptr(), lb.d_recs.data_ptr(), lb.n_recs, lb.d_thits.data_ptr(),
                                                lb.cp + 4 * P.CNT_TAG, lb.hit_cap, lb.is_mean, lb.is_sd, p.pairs.params[3], self.min_pairs,
                                                self.d_anchor.data_ptr(), self.d_rec.data_ptr() + l * self.plane,
                                                self.d_stats.data_ptr() + 4 * l * B.PA_WORDS), "gf_fill_pairs_anchored_dev")

    def _launch(self, d_nmask):
        """Nothing of its own: the pair span's launch loop calls launch_library per library."""

    def fetch(self, r):
        p = self.p
        st = self.d_stats.cpu().numpy().reshape(len(p.libs), B.PA_WORDS)
        r.pair_anchor_stats = [stats_of(st[l]) for l in range(len(p.libs))]
        bad = [s["mismatches"] for s in r.pair_anchor_stats]
        self.check_mismatches(max(bad, default=0), " (per library: %s)" % bad)
        r.pair_anchors = self.records(len(p.libs))
