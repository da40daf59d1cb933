"""Pipeline(pileup=True): the per-base confidence of the fills the step closed — the reads of a gap's own pool are placed, without gaps in
the alignment, on the gap's winning contig (the polish's placement, polish.placements), every column of the CONTIG keeps its pile-up
counts per base and read strand in a track, and one record per gap sums up the weak columns of the fill (gf_fill_pileup,
_lib.FILL_PILEUP; gf_fill_pileup_dev, csrc/fill_pileup.hip) after the polish and before the pair span.  The reference has nothing like
it.  Results.pileup (the records), .pileup_track ([entries, 8] u16, rec["off"] / rec["len"]) and .pileup_stats; single rank; not with
second_round, whose pool is not the step's.  The step's contigs, bases and pick words do not change, and neither does the polish.

The definition is the host twin below (pileup_host).  For a closed gap with winning contig c of n bases (stored orientation):
  body       [b0, b1) exactly as the read-support round locates it (read_support.locate); a contig that does not carry the word's pick is
             the same MISMATCH: zero record, counted, fetch() raises;
  placement  exactly polish.placements with seed, max_mismatch, min_overlap (the same ranges, fill_rounds.check_placement): a row is
             PLACED at one (strand, diagonal), AMBIGUOUS (no vote) or ignored;
  votes      a placed row votes its unmasked bases on EVERY column of the contig it overlaps, not only the body — any cut of the contig
             is served (Pipeline._pick_cut is not always [b0, b1)), and the flank columns show how the fill joins the draft: counter
             fwd[b] when the row lies on the contig as stored (strand 0), rev[b] when its reverse complement does (strand 1); b is the
             base as it reads on the stored contig;
  entry      of a column: 16 bytes, u16 fwd[4], rev[4], each min(count, 65535);
  classes    over the BODY columns, from the unsaturated counts, with cur = c[j]: depth = the sum of all eight, agree = fwd[cur] +
             rev[cur], alt = the largest fwd[b] + rev[b] over b != cur.  uncovered: depth == 0.  thin: 0 < depth < min_depth.
             contested: depth >= min_depth and 100 * agree < min_agree * depth.  minority: alt > agree, at any depth above 0.
             one_strand: depth >= min_depth and one strand's four counters are all zero.  A column is LOW when it is uncovered, thin or
             contested — three disjoint classes.  min_depth >= 1 and 1 <= min_agree <= 100 are integers;
  record     off, len (the contig's entries in the track; len = n, 0 when no track was written), flags, n_cols (body columns),
             n_uncovered, n_thin, n_contested, n_minority, n_one_strand, low_run (the longest run of consecutive low body columns),
             low_run_col (its first column, body-relative; the smallest on ties; 0 without a run), min_depth_seen, min_depth_col
             (body-relative, smallest on ties; 0, 0 for an empty body), depth_sum (u64, unsaturated, body), reads_placed,
             reads_ambiguous (rows, wherever on the contig); all zero for an open gap;
  skipped    a contig longer than MAX_CONTIG bases or with a byte other than A, C, G, T is flagged (n_cols set, the other counts zero, no
             track) and counted;
  capacity   a track that does not fit the track buffer sets OVERFLOW: off = len = 0, nothing is written, the summary is still
             computed, and fetch() raises.  Without a track buffer (pileup_track=False) only the records are written: off = len = 0, no flag.

phred() turns a column's counters into a MONOTONE score for the FASTQ the CLI writes; it is not a calibrated error probability."""
import numpy as np
import torch

from . import _lib as B
from . import fill_rounds as FR
from . import pipeline as P
from . import polish as POL
from .fill_rounds import _LUT

SEED, MAX_MISMATCH, MIN_OVERLAP, MIN_DEPTH, MIN_AGREE = 16, 4, 48, 3, 80
Q_MAX = 40


def check_params(L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_depth=MIN_DEPTH, min_agree=MIN_AGREE):
    """The five parameters as integers; ValueError for a value out of range (module docstring; the ABI answers GF_E_UNSUPPORTED)."""
    md, ma = int(min_depth), int(min_agree)
    return FR.check_placement("pileup", L, seed, max_mismatch, min_overlap,
                              [(md < 1, "min_depth %r: at least 1" % (min_depth,)), (not 1 <= ma <= 100, "min_agree %r: 1..100" % (min_agree,))]) + (md, ma)


def _classes(counts, cur, min_depth, min_agree):
    """(uncovered, thin, contested, minority, one_strand, depth) of columns: counts [m, 8] unsaturated integers, cur [m] the contig's codes."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 8)
    cur = np.asarray(cur, dtype=np.int64).reshape(-1)
    both = c[:, :4] + c[:, 4:]
    depth = both.sum(axis=1)
    agree = both[np.arange(len(c)), cur]
    rest = both.copy()
    rest[np.arange(len(c)), cur] = -1
    alt = np.maximum(rest.max(axis=1), 0) if len(c) else depth
    deep = depth >= min_depth
    return (depth == 0, (depth > 0) & ~deep, deep & (100 * agree < min_agree * depth), alt > agree,
            deep & ((c[:, :4].sum(axis=1) == 0) | (c[:, 4:].sum(axis=1) == 0)), depth)


def _code(base):
    c = int(_LUT[ord(base)]) if isinstance(base, str) else int(base)
    if not 0 <= c <= 3:
        raise ValueError("base %r: A, C, G or T" % (base,))
    return c


def is_low(entry, base, min_depth=MIN_DEPTH, min_agree=MIN_AGREE):
    """Is the column with the track entry `entry` (8 counters) and the base `base` (a letter or a code) low: uncovered, thin or contested?"""
    unc, thin, con = _classes(entry, [_code(base)], int(min_depth), int(min_agree))[:3]
    return bool(unc[0] or thin[0] or con[0])


def is_minority(entry, base):
    """Does another base have more votes than `base` in the column with the track entry `entry`?"""
    return bool(_classes(entry, [_code(base)], 1, 1)[3][0])


def phred(entry, base):
    """The score of `base` in a column with the track entry `entry`: 0 for depth 0, else min(40, 5 * max(0, agree - 2 * other)) with agree
    = the base's two counters and other = depth - agree.  Monotone in agree, anti-monotone in other; NOT a calibrated probability."""
    e = np.asarray(entry, dtype=np.int64).reshape(8)
    b = _code(base)
    depth, agree = int(e.sum()), int(e[b] + e[4 + b])
    return 0 if depth == 0 else min(Q_MAX, 5 * max(0, agree - 2 * (depth - agree)))


def _codes(text):
    c = _LUT[np.frombuffer(text.encode(), dtype=np.uint8)].astype(np.int64)
    if (c > 3).any():
        raise ValueError("a sequence with a track has bases A, C, G, T only")
    return c


def phred_of(entries, text):
    """phred() of every base of `text` in its column of `entries` [len(text), 8], as an array; zeros without entries."""
    if entries is None:
        return np.zeros(len(text), dtype=np.int64)
    e, c = np.asarray(entries, dtype=np.int64).reshape(len(text), 8), _codes(text)
    depth = e.sum(axis=1)
    agree = (e[:, :4] + e[:, 4:])[np.arange(len(c)), c]
    return np.where(depth == 0, 0, np.minimum(Q_MAX, 5 * np.maximum(0, agree - 2 * (depth - agree))))


def quality_string(entries, text):
    """The FASTQ quality line of `text` on its entries: chr(33 + phred) per base."""
    return (phred_of(entries, text) + 33).astype(np.uint8).tobytes().decode()


def low_of(entries, text, min_depth=MIN_DEPTH, min_agree=MIN_AGREE):
    """is_low() of every base of `text` in its column of `entries`, as an array; all low without entries."""
    if entries is None:
        return np.ones(len(text), dtype=bool)
    unc, thin, con = _classes(np.asarray(entries).reshape(len(text), 8), _codes(text), int(min_depth), int(min_agree))[:3]
    return unc | thin | con


def oriented(entries, flip):
    """The track of a cut in the orientation picked_sequences writes it: as it is, or (flip) entry i = entry len - 1 - i with b -> 3 - b
    and fwd <-> rev swapped.  An involution; a reverse-strand read's votes become forward votes on the flipped cut."""
    e = np.asarray(entries).reshape(-1, 8)
    return e[::-1, ::-1].copy() if flip else e.copy()       # (column 4 s + b -> 4 (1 - s) + 3 - b = 7 - (4 s + b))


def pileup_host(reads, contig, b0, b1, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_depth=MIN_DEPTH, min_agree=MIN_AGREE,
                detail=False, track=True):
    """(track entries [n, 8] u16 or None, gf_fill_pileup with off = 0) of one closed gap: the pool's reads (texts of one length, a byte
    other than A, C, G, T a masked base; or (codes, valid) arrays), the winning contig as stored, its body [b0, b1).  detail: the rows'
    placements and the unsaturated counts as well.  track=False: the records-only mode (len = 0, no entries)."""
    codes, valid = POL._reads(reads)
    L = codes.shape[1] if len(codes) else None
    s, mm_max, mo, md, ma = check_params(L if L is not None else 1 << 20, seed, max_mismatch, min_overlap, min_depth, min_agree)
    b0, b1 = int(b0), max(int(b0), int(b1))
    rec = np.zeros((), dtype=B.FILL_PILEUP)
    rec["n_cols"] = b1 - b0
    flag = FR.skip_flag(contig, B.PU_F_LONG, B.PU_F_NON_ACGT)
    if flag:
        rec["flags"] = flag
        return (None, rec, [], None) if detail else (None, rec)
    cc = _LUT[np.frombuffer(contig.encode(), dtype=np.uint8)]
    n = len(cc)
    where = POL.placements((codes, valid), contig, s, mm_max, mo) if len(codes) else []
    counts = np.zeros((n, 8), dtype=np.int64)
    for r, w in enumerate(where):
        if w is None or w == "ambiguous":
            continue
        strand, d = w[0], w[1]
        q, v = (codes[r], valid[r]) if strand == 0 else (3 - codes[r][::-1], valid[r][::-1])
        i = np.arange(max(0, -d), min(L, n - d))
        i = i[v[i]]
        np.add.at(counts, (d + i, 4 * strand + q[i].astype(np.int64)), 1)
    unc, thin, con, mino, one, depth = _classes(counts[b0:b1], cc[b0:b1], md, ma)
    rec["len"] = n if track else 0
    rec["n_uncovered"], rec["n_thin"], rec["n_contested"] = int(unc.sum()), int(thin.sum()), int(con.sum())
    rec["n_minority"], rec["n_one_strand"] = int(mino.sum()), int(one.sum())
    low = unc | thin | con
    run = start = 0
    for j in range(b1 - b0):                     # (ascending: a later run of the same length does not replace the first)
        if low[j]:
            start = j if not run else start
            run += 1
            if run > int(rec["low_run"]):
                rec["low_run"], rec["low_run_col"] = run, start
        else:
            run = 0
    if b1 > b0:
        rec["min_depth_seen"], rec["min_depth_col"] = int(depth.min()), int(np.argmin(depth))       # (the first of equal depths)
    rec["depth_sum"] = int(depth.sum())
    rec["reads_placed"] = sum(w is not None and w != "ambiguous" for w in where)
    rec["reads_ambiguous"] = sum(w == "ambiguous" for w in where)
    entries = np.minimum(counts, 65535).astype(np.uint16) if track else None
    return (entries, rec, where, counts) if detail else (entries, rec)


STAT_KEYS = ("gaps", "mismatches", "skipped_long", "skipped_non_acgt", "placed", "ambiguous", "entries", "low", "overflow")


def add_stats(stats, rec, n):
    """One closed, located gap's record (contig of n bases) added to a STAT_KEYS dictionary, as the kernel counts it."""
    f = int(rec["flags"])
    stats["skipped_long"] += bool(f & B.PU_F_LONG)
    stats["skipped_non_acgt"] += bool(f & B.PU_F_NON_ACGT)
    if f & (B.PU_F_LONG | B.PU_F_NON_ACGT):
        return
    stats["gaps"] += 1
    stats["placed"] += int(rec["reads_placed"])
    stats["ambiguous"] += int(rec["reads_ambiguous"])
    stats["entries"] += n if int(rec["len"]) else 0
    stats["low"] += int(rec["n_uncovered"]) + int(rec["n_thin"]) + int(rec["n_contested"])


def pileup_of_results(res, flanks, L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_depth=MIN_DEPTH, min_agree=MIN_AGREE,
                      nmask=None, track=True):
    """The twin over a whole step: (records with off = 0, {gap: entries [n, 8] u16}, stats) from fetch(pools=True)'s pools and the
    fetched contigs and picks."""
    check_params(L, seed, max_mismatch, min_overlap, min_depth, min_agree)
    out, tracks = np.zeros(len(res.best), dtype=B.FILL_PILEUP), {}
    stats = dict.fromkeys(STAT_KEYS, 0)
    for g, contig, body in FR.closed_fills(res, flanks):
        if body is None:
            stats["mismatches"] += 1
            continue
        reads = FR.fill_reads(res, g, L, nmask)
        entries, out[g] = pileup_host(reads, contig, body[0], body[1], seed, max_mismatch, min_overlap, min_depth, min_agree, track=track)
        if entries is not None:
            tracks[int(g)] = entries
        add_stats(stats, out[g], len(contig))
    return out, tracks, stats


def stats_of(words):
    """The statistics words of gf_fill_pileup_dev (u32[PU_WORDS]) as pileup_of_results' dictionary."""
    st = np.asarray(words).view(np.uint32)
    return {"gaps": int(st[B.PU_GAPS]), "mismatches": int(st[B.PU_MISMATCH]), "skipped_long": int(st[B.PU_SKIPPED_LONG]),
            "skipped_non_acgt": int(st[B.PU_SKIPPED_NON_ACGT]), "placed": P.counter_u64(st, B.PU_PLACED),
            "ambiguous": P.counter_u64(st, B.PU_AMBIGUOUS), "entries": P.counter_u64(st, B.PU_ENTRIES), "low": P.counter_u64(st, B.PU_LOW),
            "overflow": int(st[B.PU_OVERFLOW])}


class FillPileup(FR.FillRound):
    WHAT, RECORD = "pileup", B.FILL_PILEUP

    def __init__(self, pipe, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_depth=MIN_DEPTH, min_agree=MIN_AGREE, track=True,
                 read_len=None):
        super().__init__(pipe)
        self.params = check_params(read_len, seed, max_mismatch, min_overlap, min_depth, min_agree)
        self.track = bool(track)

    def prepare(self):
        """The track takes an entry per contig base: no set of winners is longer (the bound of the polish's base buffer).  Without
        a track the pointer is null and the capacity 0: records only."""
        p = self.p
        self.track_cap = p.seq_cap if self.track else 0
        self.d_rec = p._u8(max(1, p.n_gaps) * B.FILL_PILEUP.itemsize)
        self.d_track = p._u8(max(1, self.track_cap) * B.PU_ENTRY_BYTES) if self.track else None
        self.d_stats = torch.zeros(B.PU_WORDS, dtype=torch.int32, device=p.dev)

    def _launch(self, d_nmask):
        """On the pool the step assembled (after the polish)."""
        p = self.p
        p._chk(p.lib.gf_fill_pileup_dev(p.h, *self.pool_args(d_nmask), p.L, *self.shared_args(), *self.params,
                                        self.d_rec.data_ptr(), self.d_track.data_ptr() if self.track else None, self.track_cap,
                                        self.d_stats.data_ptr()), "gf_fill_pileup_dev")

    def fetch(self, r):
        r.pileup_stats = stats_of(self.d_stats.cpu().numpy())
        self.check_mismatches(r.pileup_stats["mismatches"])
        if r.pileup_stats["overflow"] or r.pileup_stats["entries"] > self.track_cap:
            raise RuntimeError("pileup: %d track entries (cap %d)" % (r.pileup_stats["entries"], self.track_cap))
        r.pileup = self.records()[0]
        r.pileup_track = (np.frombuffer(self.d_track[:r.pileup_stats["entries"] * B.PU_ENTRY_BYTES].cpu().numpy().tobytes(), dtype="<u2").reshape(-1, 8)
                          if self.track else None)


def track_of(res, g):
    """The track entries [n, 8] of gap g's winning contig (stored orientation) of a Results, or None: an open gap, a skipped contig, no track."""
    rec = res.pileup[g]
    if res.pileup_track is None or not int(rec["len"]):
        return None
    return res.pileup_track[int(rec["off"]):int(rec["off"]) + int(rec["len"])]
