"""Pipeline(pair_span=True): a pair-span check of the fills the step closed — per library, the rows of the library's own pool are
placed, without gaps in the alignment, on the gap's winning contig, the two mates of every read pair are put together, and one record
per (library, gap) says how the pairs' inserts and their physical coverage of the fill fit the library's insert size (gf_fill_pairs,
_lib.FILL_PAIRS; gf_fill_pairs_dev, csrc/fill_pairs.hip) at the end of the step.  The reference collects reads by this very statistic
(collect_reads_for_gaps.py:5-6: mean -/+ 3 sd) and never applies it to its result.  Results.pairs ([n_lib, n_gaps]) and .pair_stats (a
dictionary per library); single rank; with second_round only on the closing pools (closing_pools: each library's closing pool).  Nothing else of the step changes.

The definition is the host twin below (pair_span_host).  For a closed gap, one library, the winning contig c of n bases
(stored orientation; always the UNPOLISHED one):
  body        [b0, b1) exactly as the read-support and polish rounds locate it (read_support.locate); a contig that does not carry the
              word's pick is the same MISMATCH: zero record, counted, fetch() raises;
  placement   of a row: the polish's rule word for word (polish.placements: seed, max_mismatch, min_overlap, L // seed > max_mismatch):
              PLACED at (strand, diagonal d), AMBIGUOUS or unplaced;
  pairs       over the rows of the LIBRARY's pool for the gap (read id = 2 * pair + mate; a read with two rows — a closing pool may hold one among the step's rows and among the recruits — counts at its first): ids r and r ^ 1
              both present: a complete pair; both rows PLACED: a placed pair; the mates on opposite strands and the strand-0 mate's
              diagonal d_f <= the strand-1 mate's d_r: proper (FR), insert = d_r + L - d_f; every other placed pair: misoriented;
  classes     lo = is_mean - z * is_sd, hi = is_mean + z * is_sd: in range iff lo < insert < hi (strict, collect_reads_for_gaps.py:243),
              short iff insert <= lo, long iff insert >= hi;
  spanning    a proper pair of any class with d_f <= b0 and b1 <= d_r + L: n_span and span_insert_sum — span_insert_sum / n_span is an
              insert-size sample of the library for a fill of the right length, and D lower for a fill with D bases missing;
  coverage    every in-range pair covers the columns [max(0, d_f), min(n, d_r + L)); over the body: min_cover, min_col (the smallest
              column that attains it), n_unspanned (columns no such pair covers); all 0 for an empty body;
  skipped     a contig longer than MAX_CONTIG bases or with a byte other than A, C, G, T: a flag and `rows` in the record, every count
              zero, the gap counted — never a failure;
  record      flags, rows, pairs_complete, pairs_placed, n_proper, n_misoriented, n_in_range, n_short, n_long, n_span, span_insert_sum,
              n_cols, min_cover, min_col, n_unspanned; all zero for an open gap.  Order-free integers: the device equals the twin."""
import numpy as np
import torch

from . import _lib as B
from . import fill_rounds as FR
from . import pipeline as P
from . import polish as POL
from .fill_rounds import MAX_CONTIG

SEED, MAX_MISMATCH, MIN_OVERLAP, Z = 16, 4, 48, 3       # (the first three: the polish's defaults)
COUNT_FIELDS = ("pairs_complete", "pairs_placed", "n_proper", "n_misoriented", "n_in_range", "n_short", "n_long", "n_span")
STAT_KEYS = ("gaps", "mismatches", "skipped_long", "skipped_non_acgt", "unspanned", "complete", "placed", "proper", "in_range", "span")


def check_params(L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, z=Z, is_sd=0):
    """The four parameters as integers; ValueError for a value out of range (module docstring; the ABI answers GF_E_UNSUPPORTED)."""
    zz = int(z)
    return FR.check_placement("pair_span", L, seed, max_mismatch, min_overlap, [(zz < 1 or zz != z, "z %r: an integer, at least 1" % (z,)),
                                                                               (int(is_sd) < 0, "is_sd %r: at least 0" % (is_sd,))]) + (zz,)


def pair_span_host(reads, ids, contig, b0, b1, is_mean, is_sd, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, z=Z, detail=False):
    """gf_fill_pairs of one closed gap and one library: the library's pool rows for the gap (texts of one length, a byte other than A, C,
    G, T a masked base; or (codes, valid) arrays) with their read ids, the winning contig as stored, its body [b0, b1).  detail: the
    rows' placements as well."""
    codes, valid = POL._reads(reads)
    L = codes.shape[1] if len(codes) else None
    s, mm_max, mo, zz = check_params(L if L is not None else 1 << 20, seed, max_mismatch, min_overlap, z, is_sd)
    ids = [int(r) for r in ids]
    row_of = {}
    for i, r in enumerate(ids):         # (a library's closing pool may hold a read twice, among the step's rows and among the recruits: its first row)
        row_of.setdefault(r, i)
    assert len(ids) == len(codes), "one id per row"
    b0, b1 = int(b0), max(int(b0), int(b1))
    n = len(contig)
    rec = np.zeros((), dtype=B.FILL_PAIRS)
    rec["rows"] = len(ids)
    flag = FR.skip_flag(contig, B.PS_F_LONG, B.PS_F_NON_ACGT)
    if flag:
        rec["flags"] = flag
        return (rec, []) if detail else rec
    rec["n_cols"] = b1 - b0
    where = POL.placements((codes, valid), contig, s, mm_max, mo) if len(codes) else []
    lo, hi = int(is_mean) - zz * int(is_sd), int(is_mean) + zz * int(is_sd)
    cnt = dict.fromkeys(COUNT_FIELDS, 0)
    span_sum = 0
    diff = np.zeros(n + 1, dtype=np.int64)
    for r, i in row_of.items():
        if r & 1 or (r ^ 1) not in row_of:
            continue
        cnt["pairs_complete"] += 1
        w0, w1 = where[i], where[row_of[r ^ 1]]
        if w0 is None or w1 is None or w0 == "ambiguous" or w1 == "ambiguous":
            continue
        cnt["pairs_placed"] += 1
        (d_f, d_r) = (w0[1], w1[1]) if w0[0] == 0 else (w1[1], w0[1])
        if w0[0] == w1[0] or d_f > d_r:
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
            diff[max(0, d_f)] += 1
            diff[min(n, d_r + L)] -= 1
    for f in COUNT_FIELDS:
        rec[f] = cnt[f]
    rec["span_insert_sum"] = span_sum
    if b1 > b0:
        cover = np.cumsum(diff)[b0:b1]
        rec["min_cover"], rec["min_col"], rec["n_unspanned"] = int(cover.min()), b0 + int(np.argmin(cover)), int((cover == 0).sum())
    return (rec, where) if detail else rec


def add_to_stats(stats, rec):
    """One examined or skipped gap's record into a statistics dictionary (STAT_KEYS)."""
    f = int(rec["flags"])
    stats["skipped_long"] += bool(f & B.PS_F_LONG)
    stats["skipped_non_acgt"] += bool(f & B.PS_F_NON_ACGT)
    stats["gaps"] += not f
    stats["unspanned"] += int(rec["n_unspanned"]) > 0
    for key, field in (("complete", "pairs_complete"), ("placed", "pairs_placed"), ("proper", "n_proper"), ("in_range", "n_in_range"), ("span", "n_span")):
        stats[key] += int(rec[field])


def pair_span_of_results(res, flanks, L, libs, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, z=Z, nmasks=None):
    """The twin over a whole step: (records [n_lib, n_gaps], a statistics dictionary per library) from fetch(pools=True)'s per-library
    pools and read ids (lib_pool_off, lib_pool_rows, lib_pool_ids) and the fetched contigs and picks.  libs: (is_mean, is_sd) per library;
    nmasks: per library the N-mask rows aligned with its pool rows, or None."""
    out = np.zeros((len(libs), len(res.best)), dtype=B.FILL_PAIRS)
    stats = [dict.fromkeys(STAT_KEYS, 0) for _ in libs]
    for l, (is_mean, is_sd) in enumerate(libs):
        check_params(L, seed, max_mismatch, min_overlap, z, is_sd)
        off, rows, ids, nm = FR.fill_lib_pool(res, l, None if nmasks is None else nmasks[l])
        for g, contig, body in FR.closed_fills(res, flanks):
            if body is None:
                stats[l]["mismatches"] += 1
                continue
            r0, r1, reads = FR.pool_reads(off, rows, g, L, nm)
            out[l, g] = pair_span_host(reads, ids[r0:r1], contig, body[0], body[1], is_mean, is_sd, seed, max_mismatch, min_overlap, z)
            add_to_stats(stats[l], out[l, g])
    return out, stats


def stats_of(words):
    """The statistics words of gf_fill_pairs_dev (u32[PS_WORDS]) as pair_span_of_results' dictionary."""
    st = np.asarray(words).view(np.uint32)
    return {"gaps": int(st[B.PS_GAPS]), "mismatches": int(st[B.PS_MISMATCH]), "skipped_long": int(st[B.PS_SKIPPED_LONG]),
            "skipped_non_acgt": int(st[B.PS_SKIPPED_NON_ACGT]), "unspanned": int(st[B.PS_UNSPANNED]),
            "complete": P.counter_u64(st, B.PS_COMPLETE), "placed": P.counter_u64(st, B.PS_PLACED), "proper": P.counter_u64(st, B.PS_PROPER),
            "in_range": P.counter_u64(st, B.PS_IN_RANGE), "span": P.counter_u64(st, B.PS_SPAN)}


def span_mean_minus_is(rec, is_mean):
    """span_insert_sum // n_span - is_mean of a record, or None without a spanning pair."""
    return int(rec["span_insert_sum"]) // int(rec["n_span"]) - int(is_mean) if int(rec["n_span"]) else None


class PairSpan(FR.FillRound):
    WHAT, RECORD = "pair span", B.FILL_PAIRS

    def __init__(self, pipe, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, z=Z, read_len=None):
        super().__init__(pipe)
        self.params = check_params(read_len, seed, max_mismatch, min_overlap, z)

    def prepare(self):
        """A record plane and a block of statistics words per library; one placement word per row of a library's pool array and — when a
        library has N masks — one mask row, both shared by the libraries' launches (they follow each other on the step's stream)."""
        p = self.p
        for lb in p.libs:
            check_params(p.L, *self.params, is_sd=lb.is_sd)
        self.nmw = (p.L + 31) // 32
        self.plane = max(1, p.n_gaps) * B.FILL_PAIRS.itemsize
        self.d_rec = p._u8(len(p.libs) * self.plane)
        self.d_stats = torch.zeros(len(p.libs) * B.PS_WORDS, dtype=torch.int32, device=p.dev)
        self.d_scratch = torch.zeros(self.lib_pool_cap(), dtype=torch.int32, device=p.dev)
        self.d_nm = torch.zeros(p.lib_cap * self.nmw, dtype=torch.int32, device=p.dev) if any(lb.d_nmask is not None for lb in p.libs) else None

    def masks_of(self, l):
        """The address of library l's N masks in pool-row order — gathered through the pool's read ids into the buffer the libraries
        share, so valid until the next call — or None for a library without masks."""
        p, lb = self.p, self.p.libs[l]
        if lb.d_nmask is None:
            return None
        p._chk(p.lib.gf_gather_rows_dev(p.h, lb.d_nmask.data_ptr(), lb.n_reads, 4 * self.nmw, lb.d_ids.data_ptr(),
                                        lb.d_pool_off.data_ptr() + 8 * p.n_gaps, p.lib_cap, self.d_nm.data_ptr()), "gf_gather_rows_dev")
        return self.d_nm.data_ptr()

    def lib_pool_args(self, l):
        """(pool, N masks or None, offsets, read ids, capacity in rows, head offsets or None) of library l's pool as gf_fill_pairs_split_dev
        takes them: the library's closing pool where the step builds one (second_round.ClosingPools; its head: the library's own pool), else
        the library's own pool of the step, ordered by (mate side, pair) throughout."""
        p, lb = self.p, self.p.libs[l]
        if p.closing is not None:
            return p.closing.lib_pool_args(l)
        return (p.pool_ptr[l], self.masks_of(l), lb.d_pool_off.data_ptr(), lb.d_ids.data_ptr(), p.lib_cap, None)

    def lib_pool_cap(self):
        p = self.p
        return p.closing.lib_cap if p.closing is not None else p.lib_cap

    def _launch(self, d_nmask):
        """One launch per library (after the read-support and polish rounds), on that library's pool, read ids and — gathered by the
        ids, so d_nmask, the masks of the step's merged pool, is not used — N masks."""
        p = self.p
        for l, lb in enumerate(p.libs):
            p._chk(p.lib.gf_fill_pairs_split_dev(p.h, *self.lib_pool_args(l), p.L,
                                           *self.shared_args(), *self.params[:3], lb.is_mean, lb.is_sd, self.params[3], self.d_scratch.data_ptr(),
                                           self.d_rec.data_ptr() + l * self.plane, self.d_stats.data_ptr() + 4 * l * B.PS_WORDS), "gf_fill_pairs_split_dev")
            if p.anchored is not None:        # (pair_anchors.py: it reads this library's placement words before the next library's replace them)
                p.anchored.launch_library(l)

    def fetch(self, r):
        p = self.p
        st = self.d_stats.cpu().numpy().reshape(len(p.libs), B.PS_WORDS)
        r.pair_stats = [stats_of(st[l]) for l in range(len(p.libs))]
        bad = [s["mismatches"] for s in r.pair_stats]
        self.check_mismatches(max(bad, default=0), " (per library: %s)" % bad)      # (every library's launch meets the same contigs)
        r.pairs = self.records(len(p.libs))
