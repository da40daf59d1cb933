"""Pipeline(alternatives=True, adjudicate=True): the READ ADJUDICATION of the contested fills.  The alternatives round
(fill_alternatives.py) names, for a closed gap, a rival: a contig of the winner's level that carries both anchors and spells another
fill.  This round places the gap's own pool — the reads the step just assembled — on both fills and lets every row vote for the one it
fits strictly better (gf_fill_adjudicate_dev, csrc/fill_adj.hip; exact anchors; single rank; not with second_round).  It writes buffers
of its own: Results.adjudication (gf_fill_adj per gap, _lib.FILL_ADJ) and .adj_stats; Pipeline.adjudicated_sequences gives every closed
gap's sequence with the rival's in place of the winner's where the verdict is SWITCH.  The verdict is advice: `best`, the contigs and
picked_sequences do not change.  DESIGN.md §26.

The definition is the host twin below (adjudicate_host), which the device equals byte for byte.  Placement rule (seed s, max_mismatch,
min_overlap: polish.py's, word for word), context C (default: the read length), min_votes v, ratio q; per gap g with flanks LF, RF:
  contested   the gap's gf_fill_alt has HAS_RIVAL and not LOST; every other gap gets the all-zero record;
  fills       the oriented fills F_w of `contig` and F_r of `rival` by the alternatives' rule (fill_alternatives.candidate).  MISMATCH
              (zero record, counted, fetch() raises): best[g] does not name `contig`; either index is no contig of g in the list or no
              candidate; a fill's strand or length is not what the record states (REVERSE, RIVAL_REVERSE, fill_len, rival_len);
  locus       locus(F) = LF[-C:] + F + RF[:C], a flank shorter than C whole: T_w = locus(F_w), T_r = locus(F_r).  Both share their flank
              text, so a row's keys can differ only where the fills differ;
  skipped     either locus longer than MAX_CONTIG bases: LONG; else a locus byte other than A, C, G, T: NON_ACGT.  The lengths are set,
              votes and verdict zero, the gap is counted; never truncated;
  key         of a row on a locus: over its accepted (strand, diagonal) pairs (polish.placements' `accepted`, the locus as the contig)
              the smallest (mm, -ov), whatever its multiplicity — a read inside a repeat both fills contain fits both equally and
              ties; no accepted pair: NONE.  The row's strand there: 0 when any pair with that key lies on strand 0, else 1;
  vote        W when key_w < key_r (NONE is larger than every key), R when key_r < key_w, a tie when both exist and are equal,
              unplaced when both are NONE; `only`: votes of rows that are NONE on the other locus; votes_w_s0 / votes_r_s0: votes of
              rows whose strand on the locus they vote for is 0;
  verdict     KEEP (1) when votes_w >= v and votes_w >= q * votes_r; SWITCH (2) when votes_r >= v and votes_r >= q * votes_w;
              UNDECIDED (3) otherwise (q >= 2 and v >= 1: never both);
  record      contig, rival, locus_w, locus_r (bases), the seven counters (u32), verdict, flags LONG, NON_ACGT, RIVAL_FAR (the rival's
              dist is 0xFFFF), NO_ROWS (an empty pool).
The defaults of v and q are parameters, not measured thresholds.
Limits: seed 12..32, max_mismatch 0..15, seed <= min_overlap <= L, L // seed > max_mismatch; min_overlap <= C <= 1000; v >= 1; 2 <= q <= 16."""
import numpy as np
import torch

from . import _lib as B
from . import fill_alternatives as FA
from . import fill_rounds as FR
from .fill_rounds import MAX_CONTIG, _LUT

SEED, MAX_MISMATCH, MIN_OVERLAP, MIN_VOTES, RATIO = 16, 4, 48, 3, 2
WHAT = "adjudicate"
VERDICTS = ("none", "keep", "switch", "undecided")
STAT_KEYS = ("contested", "adjudicated", "keep", "switch", "undecided", "skipped_long", "skipped_non_acgt", "mismatches", "votes_w", "votes_r", "ties")
COUNTERS = ("votes_w", "votes_r", "votes_w_s0", "votes_r_s0", "ties", "unplaced", "only")


def _int(name, v, lo, hi):
    try:
        iv = int(v)
    except (TypeError, ValueError):
        iv = None
    if iv is None or isinstance(v, bool) or iv != v or not lo <= iv <= (iv if hi is None else hi):
        raise ValueError("%s %s %r: an integer %s" % (WHAT, name, v, ("in %d..%d" % (lo, hi)) if hi is not None else "of at least %d" % lo))
    return iv


def check_params(L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, context=None, min_votes=MIN_VOTES, ratio=RATIO):
    """(seed, max_mismatch, min_overlap, context, min_votes, ratio) as integers; ValueError for a value out of range (the ABI answers
    GF_E_UNSUPPORTED for the placement rule, GF_E_INVAL for the other three).  context None: the read length."""
    s, mm, mo = FR.check_placement(WHAT, L, seed, max_mismatch, min_overlap)
    c = _int("context", int(L) if context is None else context, mo, B.AJ_MAX_CONTEXT)
    return s, mm, mo, c, _int("min_votes", min_votes, 1, None), _int("ratio", ratio, 2, B.AJ_MAX_RATIO)


def _text(s):
    return s.decode() if isinstance(s, (bytes, bytearray)) else str(s)


def locus(lf, fill, rf, C):
    """LF[-C:] + F + RF[:C] (texts); a flank shorter than C is used whole."""
    lf, rf, C = _text(lf), _text(rf), int(C)
    return lf[max(0, len(lf) - C):] + _text(fill) + rf[:C]


def _reads(reads):
    from .read_support import codes_of
    return codes_of(reads) if isinstance(reads, (list, tuple)) and (not reads or isinstance(reads[0], str)) else reads


def best_keys(reads, locus_text, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP):
    """Per row None (no accepted pair) or (mm, ov, strand): the smallest (mm, -ov) over the row's accepted (strand, diagonal) pairs on
    the locus (A, C, G, T only), whatever its multiplicity, and 0 when a pair with that key lies on strand 0, else 1.  The placement
    definition of polish.py restated: a diagonal d places q[i] on c[d + i], is accepted when the overlap has at least min_overlap
    positions, at most max_mismatch unmasked mismatches and a seed window [j s, j s + s), j < L // s, wholly inside it, without a
    masked base and equal to the locus there."""
    codes, valid = _reads(reads)
    s, mm_max, mo = int(seed), int(max_mismatch), int(min_overlap)
    cc = _LUT[np.frombuffer(locus_text.encode(), dtype=np.uint8)]
    assert (cc < 4).all()
    n, L = len(cc), codes.shape[1] if len(codes) else 0
    index = {}
    for p in range(n - s + 1):
        index.setdefault(cc[p:p + s].tobytes(), []).append(p)
    out = []
    for r in range(len(codes)):
        best = None
        for strand in (0, 1):
            q, v = (codes[r], valid[r]) if strand == 0 else ((3 - codes[r][::-1]).astype(np.uint8), valid[r][::-1])
            diagonals = set()
            for j in range(L // s):
                if v[j * s:j * s + s].all():
                    diagonals.update(p - j * s for p in index.get(np.ascontiguousarray(q[j * s:j * s + s]).tobytes(), ()))
            for d in diagonals:
                i0, i1 = max(0, -d), min(L, n - d)
                if i1 - i0 < mo:
                    continue
                mm = int(((q[i0:i1] != cc[d + i0:d + i1]) & v[i0:i1]).sum())
                if mm <= mm_max and (best is None or (mm, -(i1 - i0), strand) < best):
                    best = (mm, -(i1 - i0), strand)
        out.append(None if best is None else (best[0], -best[1], best[2]))
    return out


def verdict_of(votes_w, votes_r, min_votes=MIN_VOTES, ratio=RATIO):
    return (B.AJ_KEEP if votes_w >= min_votes and votes_w >= ratio * votes_r else
            B.AJ_SWITCH if votes_r >= min_votes and votes_r >= ratio * votes_w else B.AJ_UNDECIDED)


def adjudicate_host(reads, lf, rf, fill_w, fill_r, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, context=None,
                    min_votes=MIN_VOTES, ratio=RATIO, contig=0, rival=0, rival_far=False, detail=False, read_len=None):
    """The gf_fill_adj (_lib.FILL_ADJ) of one contested gap: the pool's reads (texts of one length, a byte other than A, C, G, T a masked
    base; or (codes, valid) arrays), the flanks, the two oriented fills.  contig, rival, rival_far: what the record copies from the
    gap's gf_fill_alt.  detail: (record, [(key on T_w, key on T_r)] per row) instead.  read_len: the read length of an EMPTY pool (the
    parameters are checked against it, and it is the default context); required with an empty pool."""
    codes, valid = _reads(reads)
    if not len(codes) and read_len is None:
        raise ValueError("%s: an empty pool needs read_len" % WHAT)
    L = codes.shape[1] if len(codes) else int(read_len)
    s, mm, mo, C, v, q = check_params(L, seed, max_mismatch, min_overlap, context, min_votes, ratio)
    t_w, t_r = locus(lf, fill_w, rf, C), locus(lf, fill_r, rf, C)
    rec = np.zeros((), dtype=B.FILL_ADJ)
    rec["contig"], rec["rival"], rec["locus_w"], rec["locus_r"] = contig, rival, len(t_w), len(t_r)
    flags = (B.AJ_F_RIVAL_FAR if rival_far else 0) | (0 if len(codes) else B.AJ_F_NO_ROWS)
    skip = B.AJ_F_LONG if max(len(t_w), len(t_r)) > MAX_CONTIG else B.AJ_F_NON_ACGT if (_LUT[np.frombuffer((t_w + t_r).encode(), dtype=np.uint8)] > 3).any() else 0
    rec["flags"] = flags | skip
    if skip:
        return (rec, []) if detail else rec
    k_w = best_keys((codes, valid), t_w, s, mm, mo) if len(codes) else []
    k_r = best_keys((codes, valid), t_r, s, mm, mo) if len(codes) else []
    n = dict.fromkeys(COUNTERS, 0)
    none = (16, 0)                                # (above every key: mm <= 15)
    for a, b in zip(k_w, k_r):
        ka, kb = (none if a is None else (a[0], -a[1])), (none if b is None else (b[0], -b[1]))
        if a is None and b is None:
            n["unplaced"] += 1
        elif ka == kb:
            n["ties"] += 1
        elif ka < kb:
            n["votes_w"] += 1
            n["votes_w_s0"] += a[2] == 0
            n["only"] += b is None
        else:
            n["votes_r"] += 1
            n["votes_r_s0"] += b[2] == 0
            n["only"] += a is None
    for k in COUNTERS:
        rec[k] = n[k]
    rec["verdict"] = verdict_of(n["votes_w"], n["votes_r"], v, q)
    return (rec, list(zip(k_w, k_r))) if detail else rec


def adjudicate_gaps(alts, contigs, flanks, best, reads_of, L, anchors=(30, 15), seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP,
                    context=None, min_votes=MIN_VOTES, ratio=RATIO):
    """The twin over a list: alts (_lib.FILL_ALT per gap), contigs [(gap, text)] in list order, flanks [(left, right)], best (the pick
    words), reads_of(g) -> the gap's rows (texts or (codes, valid)), L: the read length.  Returns (records: _lib.FILL_ADJ per gap, statistics {STAT_KEYS})."""
    params = check_params(L, seed, max_mismatch, min_overlap, context, min_votes, ratio)
    a_l, a_s = FA.check_anchors(anchors)
    out = np.zeros(len(flanks), dtype=B.FILL_ADJ)
    st = dict.fromkeys(STAT_KEYS, 0)
    for g in range(len(flanks)):
        a = alts[g]
        fl = int(a["flags"])
        if not fl & B.FA_F_HAS_RIVAL or fl & B.FA_F_LOST:
            continue
        st["contested"] += 1
        lf, rf = FA._bytes(flanks[g][0]), FA._bytes(flanks[g][1])
        ci, ri, word = int(a["contig"]), int(a["rival"]), int(best[g])
        fills = []
        ok = word != 0 and FA.CONTIG_MAX - ((word >> 1) & FA.CONTIG_MAX) == ci
        for idx, rev, ln in ((ci, bool(fl & B.FA_F_REVERSE), int(a["fill_len"])), (ri, bool(fl & B.FA_F_RIVAL_REVERSE), int(a["rival_len"]))):
            c = FA.candidate(FA._bytes(contigs[idx][1]), lf, rf, a_l, a_s) if ok and idx < len(contigs) and int(contigs[idx][0]) == g else None
            ok = c is not None and bool(c[2]) == rev and c[1] == ln
            fills.append(c[3].decode() if ok else None)
        if not ok:
            st["mismatches"] += 1
            continue
        rec = adjudicate_host(reads_of(g), lf, rf, fills[0], fills[1], *params, contig=ci, rival=ri, rival_far=int(a["dist"]) == B.FA_DIST_FAR,
                              read_len=L)
        out[g] = rec
        f = int(rec["flags"])
        st["skipped_long"] += bool(f & B.AJ_F_LONG)
        st["skipped_non_acgt"] += bool(f & B.AJ_F_NON_ACGT)
        if int(rec["verdict"]):
            st["adjudicated"] += 1
            st[VERDICTS[int(rec["verdict"])]] += 1
            for k in ("votes_w", "votes_r", "ties"):
                st[k] += int(rec[k])
    return out, st


def adjudication_of_results(pipe, res, nmask=None):
    """The twin on a step's Results (fetch(pools=True)): what Results.adjudication and .adj_stats must equal."""
    reads_of = lambda g: FR.fill_reads(res, g, pipe.L, nmask)
    return adjudicate_gaps(res.alts, FA.contigs_of_results(res), pipe.gf.flanks, res.best, reads_of, pipe.L, pipe.anchors, *pipe.adj.params)


def stats_dict(words):
    """The statistics words of gf_fill_adjudicate_dev (u32[AJ_WORDS]) as adjudicate_gaps' dictionary."""
    st = np.ascontiguousarray(words).view(np.uint32)
    u64 = lambda w: int(st[w:w + 2].view(np.uint64)[0])
    return {"contested": int(st[B.AJ_SEEN]), "adjudicated": int(st[B.AJ_ADJUDICATED]), "keep": int(st[B.AJ_N_KEEP]), "switch": int(st[B.AJ_N_SWITCH]),
            "undecided": int(st[B.AJ_N_UNDECIDED]), "skipped_long": int(st[B.AJ_SKIPPED_LONG]), "skipped_non_acgt": int(st[B.AJ_SKIPPED_NON_ACGT]),
            "mismatches": int(st[B.AJ_MISMATCH]), "votes_w": u64(B.AJ_VOTES_W), "votes_r": u64(B.AJ_VOTES_R), "ties": u64(B.AJ_TIES)}


def flank_context(flanks, C):
    """(text u8 [n_gaps, 2, C], lengths u16 [n_gaps, 2]) as gf_fill_adjudicate_dev reads them: LF[-C:] and RF[:C], each from the start of
    its C bytes."""
    text, lens = np.zeros((max(1, len(flanks)), 2, C), dtype=np.uint8), np.zeros((max(1, len(flanks)), 2), dtype=np.uint16)
    for g, (l, r) in enumerate(flanks):
        for side, t in enumerate((FA._bytes(l)[max(0, len(l) - C):], FA._bytes(r)[:C])):
            text[g, side, :len(t)] = np.frombuffer(t, dtype=np.uint8)
            lens[g, side] = len(t)
    return text, lens


class FillAdjudication(FR.FillRound):
    """The round object the Pipeline holds: an after-pick round (it reads the step's pool and d_nmask) that also reads the alternatives'
    records."""
    WHAT, RECORD = WHAT, B.FILL_ADJ

    def __init__(self, pipe, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, context=None, min_votes=MIN_VOTES, ratio=RATIO, read_len=None):
        super().__init__(pipe)
        self.params = check_params(read_len, seed, max_mismatch, min_overlap, context, min_votes, ratio)

    def prepare(self):
        """The flank context is uploaded once, from the flanks the GapFill holds; the scratch word per row of the assembled pool."""
        p = self.p
        if p.gf.flanks is None:
            raise ValueError("adjudicate needs the flanks given to gf_set_gaps")
        text, lens = flank_context(p.gf.flanks, self.params[3])
        self.d_text = torch.from_numpy(text.reshape(-1)).to(p.dev)
        self.d_lens = torch.from_numpy(lens.reshape(-1).view(np.int16)).to(p.dev)
        self.d_scratch = torch.zeros(max(1, self.pool_cap()), dtype=torch.int32, device=p.dev)
        self.d_rec = p._u8(max(1, p.n_gaps) * B.FILL_ADJ.itemsize)
        self.d_stats = torch.zeros(B.AJ_WORDS, dtype=torch.int32, device=p.dev)

    def _launch(self, d_nmask):
        """On the pool the step assembled, behind the alternatives round (whose records it reads) and the other after-pick rounds."""
        p = self.p
        if p.alts.d_rec is None or self.pool_cap() > self.d_scratch.numel():
            raise RuntimeError("adjudicate: the alternatives round has no records, or the pool outgrew the scratch")
        p._chk(p.lib.gf_fill_adjudicate_dev(p.h, *self.pool_args(d_nmask), p.L, p.d_ctg.data_ptr(), p.ap, p.contig_cap,
                                            p.d_seq.data_ptr(), p.d_best.data_ptr(), *p.anchor_pair, p.alts.d_rec.data_ptr(), self.d_text.data_ptr(),
                                            self.d_lens.data_ptr(), self.d_scratch.data_ptr(), *self.params, self.d_rec.data_ptr(),
                                            self.d_stats.data_ptr()), "gf_fill_adjudicate_dev")

    def fetch(self, r):
        r.adj_stats = stats_dict(self.d_stats.cpu().numpy())
        self.check_mismatches(r.adj_stats["mismatches"], " or the alternatives' record")
        r.adjudication = self.records()[0]
