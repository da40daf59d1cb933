"""Pipeline(flank_joins=True): the gaps whose FLANKS OVERLAP.  A scaffolder may put an N-run between two contig ends that share o bases:
nothing is missing there, the draft repeats o bases on both sides of the run.  The assembly builds the right contig — it runs straight
through the junction — but on it the right anchor starts before the left anchor ends, so the pick (span >= 0, pick_contigs.select_full)
drops it and the gap stays open in every round.  This round looks, after the last pick of the step, at every gap still open and at
exactly that case (gf_pick_joins_dev, csrc/pick_join.hip; exact anchors only; single rank).  It reads the step's contigs and the flanks
and writes buffers of its own: Results.joins (gf_flank_join per gap, _lib.FLANK_JOIN) and .join_stats; Pipeline.joined_gaps gives
{gap: overlap} of the usable ones.  Nothing else of the step changes.  DESIGN.md §24.

The definition is the host twin below (joins_host), which the device equals byte for byte.  Per open gap g (best[g] == 0) with flanks LF,
RF of n_l, n_r bytes, anchor lengths long then short (the step's anchor_pair), X = max_overlap, C = min_context, M = max_mismatch; for
every contig of g in list order and for strand 0 (S = the contig) and 1 (S = its reverse complement: A<->T, C<->G, every other byte as
it is):
  level       a = the long length when the gap has anchors of it (both flanks at least a bytes, the anchors' bytes all in ACGT) and S
              carries both; else the short length under the same conditions; else the strand gives nothing;
  positions   i = S.find(LF[-a:]), j = S.rfind(RF[:a]); j >= i + a is the pick's pair and skipped; otherwise o = i + a - j >= 1 is a
              CANDIDATE;
  rejections  counted apart, tested in this order: far (o > X); short flank (o + C > n_l or o + C > n_r); no context (j < C or
              i + a + C > len(S): a contig inside the shared sequence proves nothing);
  agreement   m_l = #{x < o + C: S[j - C + x] != LF[n_l - o - C + x]}, m_r = #{y < o + C: S[j + y] != RF[y]}, bytes as stored;
              m_l > M or m_r > M: mismatch, counted;
  winner      of the accepted candidates the largest word level << 56 | (255 - min(255, m_l + m_r)) << 48 | (0xFFFF - o) << 32 |
              (0x7FFFFFFF - contig) << 1 | strand: the longer anchor, fewer mismatches, the smaller overlap, the earlier contig, the
              forward strand;
  record      of the winner: contig, overlap, level, left_pos = i, right_pos = j, m_left, m_right, m_flanks = #{x < o: LF[n_l - o + x]
              != RF[x]}; of the gap: n_candidates, n_accepted (saturating at 65 535), o_min, o_max over the accepted; flags REVERSE
              (strand 1), AMBIGUOUS (o_min != o_max), MULTI (on the winner's strand an anchor of its level occurs at more than one
              position).  All zero: the gap is closed or has no accepted candidate;
  usable      overlap > 0 and neither AMBIGUOUS nor MULTI.
Limits: 1 <= X <= 1024, 0 <= C <= 255, 0 <= M <= 15, anchors 8 <= short < long <= 32 (or one length), flanks below 65 536 bytes, the
contig index below 2^31 - 1."""
import numpy as np
import torch

from . import _lib as B

MAX_OVERLAP, MIN_CONTEXT, MAX_MISMATCH = 256, 30, 2
STAT_KEYS = ("open_gaps", "joined", "usable", "candidates", "far", "short_flank", "no_context", "mismatch", "no_anchors")
_WORDS = (B.FJ_OPEN, B.FJ_JOINED, B.FJ_USABLE, B.FJ_CANDIDATES, B.FJ_FAR, B.FJ_SHORT_FLANK, B.FJ_NO_CONTEXT, B.FJ_MISMATCH, B.FJ_NO_ANCHORS)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")       # (the device's base_comp: upper case, any other byte as it is)
CONTIG_MAX = 0x7FFFFFFF


def check_params(max_overlap=MAX_OVERLAP, min_context=MIN_CONTEXT, max_mismatch=MAX_MISMATCH):
    """(X, C, M) as integers; ValueError for a value out of range (the ABI answers GF_E_INVAL)."""
    out = []
    for name, v, lo, hi in (("join_max_overlap", max_overlap, 1, B.FJ_MAX_OVERLAP), ("join_min_context", min_context, 0, B.FJ_MAX_CONTEXT),
                            ("join_max_mismatch", max_mismatch, 0, B.FJ_MAX_MISMATCH)):
        try:
            iv = int(v)
        except (TypeError, ValueError):
            iv = None
        if iv is None or isinstance(v, bool) or iv != v or not lo <= iv <= hi:
            raise ValueError("flank_joins %s %r: an integer in %d..%d" % (name, v, lo, hi))
        out.append(iv)
    return tuple(out)


def check_anchors(anchors):
    """(long, short or 0) of the step's anchor lengths; ValueError outside 8 <= short < long <= 32."""
    a = tuple(int(x) for x in anchors)
    a_l, a_s = a[0], (a[1] if len(a) > 1 else 0)
    if not 8 <= a_l <= 32 or (a_s and not 8 <= a_s < a_l):
        raise ValueError("flank_joins: anchor lengths %r: 8 <= short < long <= 32" % (anchors,))
    return a_l, a_s


def usable(rec):
    """Is the record a join the write-back may apply?"""
    return int(rec["overlap"]) > 0 and not int(rec["flags"]) & (B.FJ_F_AMBIGUOUS | B.FJ_F_MULTI)


def _bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def _has_anchors(lf, rf, a):
    return len(lf) >= a and len(rf) >= a and all(c in b"ACGT" for c in lf[len(lf) - a:] + rf[:a])


def _differences(a, b):
    return sum(x != y for x, y in zip(a, b))


def contigs_of_results(res):
    """[(gap, text)] of a step's Results, in list order: what joins_host takes."""
    return [(int(c["gap"]), res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])]) for c in res.contigs]


def joins_host(contigs, flanks, best, anchors=(30, 15), X=MAX_OVERLAP, C=MIN_CONTEXT, M=MAX_MISMATCH, first=0):
    """The twin.  contigs: [(gap, text)] in list order (the position is the contig index; a gap outside 0 .. n_gaps - 1 is a tombstone),
    of which those from index `first` on are looked at; flanks: [(left, right)] per gap; best: the pick words per gap (0: open).
    Returns (records: _lib.FLANK_JOIN per gap, statistics: {STAT_KEYS})."""
    X, C, M = check_params(X, C, M)
    a_l, a_s = check_anchors(anchors)
    levels = (a_l, a_s) if a_s else (a_l,)
    n_gaps = len(flanks)
    fl = [(_bytes(l), _bytes(r)) for l, r in flanks]
    if any(len(l) >= B.FJ_FLANK_LIMIT or len(r) >= B.FJ_FLANK_LIMIT for l, r in fl):
        raise ValueError("flank_joins: a flank of %d bases or more" % B.FJ_FLANK_LIMIT)
    rec = np.zeros(n_gaps, dtype=B.FLANK_JOIN)
    st = dict.fromkeys(STAT_KEYS, 0)
    accepted = [[] for _ in range(n_gaps)]        # per gap: (word, level, i, j, o, m_l, m_r, contig, strand, multi)
    n_cand = [0] * n_gaps
    for g in range(n_gaps):
        if int(best[g]) == 0:
            st["open_gaps"] += 1
            st["no_anchors"] += not _has_anchors(fl[g][0], fl[g][1], levels[-1])
    for ci, (g, text) in enumerate(contigs):
        g = int(g)
        if ci < first or not 0 <= g < n_gaps or int(best[g]) != 0 or len(text) < levels[-1]:
            continue
        lf, rf = fl[g]
        if not _has_anchors(lf, rf, levels[-1]):
            continue
        text = _bytes(text)
        for strand, S in ((0, text), (1, text.translate(_COMP)[::-1])):
            for a in levels:
                if not _has_anchors(lf, rf, a):
                    continue
                la, ra = lf[len(lf) - a:], rf[:a]
                i, j = S.find(la), S.rfind(ra)
                if i >= 0 and j >= 0:
                    break
            else:
                continue
            if j >= i + a:
                continue
            o = i + a - j
            st["candidates"] += 1
            n_cand[g] += 1
            if o > X:
                st["far"] += 1
            elif o + C > len(lf) or o + C > len(rf):
                st["short_flank"] += 1
            elif j < C or i + a + C > len(S):
                st["no_context"] += 1
            else:
                m_l = _differences(S[j - C:j + o], lf[len(lf) - o - C:])
                m_r = _differences(S[j:j + o + C], rf[:o + C])
                if m_l > M or m_r > M:
                    st["mismatch"] += 1
                    continue
                word = a << 56 | (255 - min(255, m_l + m_r)) << 48 | (0xFFFF - o) << 32 | (CONTIG_MAX - ci) << 1 | strand
                multi = S.rfind(la) != i or S.find(ra) != j
                accepted[g].append((word, a, i, j, o, m_l, m_r, ci, strand, multi))
    for g, acc in enumerate(accepted):
        if not acc:
            continue
        _, a, i, j, o, m_l, m_r, ci, strand, multi = max(acc)
        lf, rf = fl[g]
        os_ = [x[4] for x in acc]
        flags = (B.FJ_F_REVERSE if strand else 0) | (B.FJ_F_AMBIGUOUS if min(os_) != max(os_) else 0) | (B.FJ_F_MULTI if multi else 0)
        rec[g] = (ci, i, j, o, m_l, m_r, _differences(lf[len(lf) - o:], rf[:o]), min(n_cand[g], 0xFFFF), min(len(acc), 0xFFFF), min(os_), max(os_),
                  a, flags, 0)
        st["joined"] += 1
        st["usable"] += bool(usable(rec[g]))
    return rec, st


def stats_dict(words):
    """The statistics words of gf_pick_joins_dev as joins_host's dictionary."""
    return {k: int(words[w]) for k, w in zip(STAT_KEYS, _WORDS)}


class FlankJoins:
    """The round object the Pipeline holds (the shape of extended_fill.ExtendedFill)."""

    def __init__(self, pipe, max_overlap=MAX_OVERLAP, min_context=MIN_CONTEXT, max_mismatch=MAX_MISMATCH):
        self.p, self.params = pipe, check_params(max_overlap, min_context, max_mismatch)
        self.d_rec = None

    def prepare(self):
        """Called once, after the rounds have settled the capacities of the step's contig list."""
        p = self.p
        self.anchor_pair = check_anchors(p.anchors)
        self.d_rec = p._u8(p.n_gaps * B.FLANK_JOIN.itemsize)
        self.d_stats = torch.zeros(B.FJ_WORDS, dtype=torch.int32, device=p.dev)

    def enqueue(self):
        """After the last pick of the step, before the extended fill: the joins of the gaps d_best leaves open, over all of the step's contigs."""
        p = self.p
        if self.d_rec is None:        # a sizing run of one of the rounds: nobody reads its records
            return
        p._chk(p.lib.gf_pick_joins_dev(p.h, p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), *self.anchor_pair, *self.params, None,
                                       p.d_best.data_ptr(), self.d_rec.data_ptr(), self.d_stats.data_ptr()), "gf_pick_joins_dev")

    def fetch(self, r):
        p = self.p
        r.joins = np.frombuffer(self.d_rec[:p.n_gaps * B.FLANK_JOIN.itemsize].cpu().numpy().tobytes(), dtype=B.FLANK_JOIN)
        r.join_stats = stats_dict(self.d_stats.cpu().numpy().view(np.uint32))


def joins_of_results(pipe, res):
    """The twin on a step's Results: what Results.joins and .join_stats must equal."""
    return joins_host(contigs_of_results(res), pipe.gf.flanks, res.best, pipe.anchors, *pipe.joins.params)
