"""Pipeline(alternatives=True): the RIVAL FILLS of the closed gaps.  The pick closes a gap with the contig that carries both anchors at the
highest level and has the longest span (pick_contigs.select_full; csrc/pick.hip); every other contig of the gap that carries both anchors
is dropped.  With several (k, kv) pairs, the merge and the rescue round a closed gap usually has several.  Mostly they agree; where they
do not — a collapsed or expanded repeat, a heterozygous site, an assembly error at one k — the gap has more than one path between its
flanks, the classical warning sign of a gap closer.  This round looks, after the last pick of the step, at every closed gap and at all
of its contigs again (gf_fill_alts_dev, csrc/fill_alt.hip; exact anchors only; single rank) and writes buffers of its own: Results.alts
(gf_fill_alt per gap, _lib.FILL_ALT), .alt_contigs (gf_fill_alt_contig per contig, _lib.FILL_ALT_CONTIG) and .alt_stats;
Pipeline.alternative_sequences gives the rival's gap sequence of every contested gap.  Nothing else of the step changes.  DESIGN.md §25.

The definition is the host twin below (alts_host), which the device equals byte for byte.  Anchor lengths long then short (the step's
anchor_pair), B = max_dist; per gap g with flanks LF, RF:
  candidate   a contig of g at an index in [first, n) to which the pick's own rule gives a word.  Skipped: a contig shorter than twice
              the short anchor; a gap without short anchors (both flanks at least that long, the anchors' bytes all in ACGT).  Level: the
              long length when the gap has anchors of it, the contig has twice its bytes and the pair below exists at it; else the short
              one.  The pair of a level a, with L = LF[-a:], R = RF[:a], on the contig s as stored: forward when s holds L and R,
              i = s.find(L), j = s.rfind(R), a pair when j >= i + a; only when the forward strand lacks one of them, reverse, when s
              holds rc(R) and rc(L) (a flank of exactly a bases: its reverse hit does not count when s holds its forward one),
              i = s.find(rc(R)), j = s.rfind(rc(L)), a pair when j >= i + a.  span = j - i - a, strand 0 / 1, word = level << 56 |
              min(span + 1, 0xFFFFFF) << 32 | (0x7FFFFFFF - contig) << 1 | strand;
  fill        the span bytes between the anchors, oriented: s[i + a:j], reverse-complemented on strand 1 (A<->T, C<->G, every other byte
              as it is);
  winner      the contig best[g] names, at its index whatever `first` is: it must be a contig of g below n, and a candidate of the
              word's level and strand whose span matches the word's field (a saturated field: any span at least that long).  Otherwise
              the gap is LOST: level and the flag, nothing else; its contigs are not looked at;
  classes     of every other candidate: LOWER (level below the winner's); above it: the flag OUTRANKED, counted as a candidate and
              otherwise ignored (its per-contig record stays zero); the winner's level: a PEER, and OUTRANKED when its word is greater than
              best[g].  A peer with fill P against the winner's W: IDENTICAL (equal), NEAR (Levenshtein distance <= B, unit costs, bytes as
              oriented) or FAR (a length difference beyond B included);
  rival       of the NEAR and FAR peers the one with the largest word: the contig the pick would have taken without the winner;
              lcp = the common prefix of W and P, lcs = the common suffix of W[lcp:] and P[lcp:], dist = its distance or 0xFFFF;
  record      contig, rival, fill_len, rival_len, lcp, lcs, len_min / len_max over the winner and its peers, the class counters
              (saturating at 65 535; n_candidates counts the winner and the outranking candidates too), dist, level, flags REVERSE,
              RIVAL_REVERSE, HAS_RIVAL (the gap is CONTESTED), LENGTH_VARIES, OUTRANKED, LOST.  All zero: the gap is open;
  per contig  length (the span), dist (a NEAR peer's, else 0xFFFF), cls 0 none / 1 WINNER / 2 IDENTICAL / 3 NEAR / 4 FAR / 5 LOWER, strand.
Limits: 1 <= B <= 31, anchors 8 <= short < long <= 32 (or one length), the contig index below 2^31 - 1."""
import functools

import numpy as np
import torch

from . import _lib as B
from .flank_joins import CONTIG_MAX, _COMP, _bytes, _has_anchors, check_anchors, contigs_of_results

MAX_DIST = 16
SPAN_SAT = 0xFFFFFF
STAT_KEYS = ("closed_gaps", "contested", "length_varies", "candidates", "lower", "identical", "near", "far", "outranked", "lost")
_WORDS = (B.FA_CLOSED, B.FA_CONTESTED, B.FA_LENGTH_VARIES, B.FA_CANDIDATES, B.FA_LOWER, B.FA_IDENTICAL, B.FA_NEAR, B.FA_FAR, B.FA_OUTRANKED, B.FA_LOST)
CLASS_NAMES = ("none", "winner", "identical", "near", "far", "lower")


def check_params(max_dist=MAX_DIST):
    """B as an integer; ValueError for a value out of range (the ABI answers GF_E_INVAL)."""
    try:
        iv = int(max_dist)
    except (TypeError, ValueError):
        iv = None
    if iv is None or isinstance(max_dist, bool) or iv != max_dist or not 1 <= iv <= B.FA_MAX_DIST:
        raise ValueError("alternatives alt_max_dist %r: an integer in 1..%d" % (max_dist, B.FA_MAX_DIST))
    return iv


def contested(rec):
    """Does the gap have a rival: a contig of the winner's level whose fill is not the winner's?"""
    return bool(int(rec["flags"]) & B.FA_F_HAS_RIVAL)


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _pair(s, lf, rf, a):
    """The pick's pair of level a on the contig s: (i, j, strand) with j >= i + a, or None."""
    l, r = lf[len(lf) - a:], rf[:a]
    has_l, has_r = l in s, r in s
    if has_l and has_r:
        i, j, strand = s.find(l), s.rfind(r), 0
    else:
        rl, rr = revcomp(l), revcomp(r)
        if not (rl in s and not (len(lf) == a and has_l) and rr in s and not (len(rf) == a and has_r)):
            return None
        i, j, strand = s.find(rr), s.rfind(rl), 1
    return (i, j, strand) if j >= i + a else None


def candidate(s, lf, rf, a_l, a_s):
    """(level, span, strand, oriented fill) of the contig s (bytes) for a gap with the flanks lf, rf, or None: no word."""
    short = a_s or a_l
    if len(s) < 2 * short or not _has_anchors(lf, rf, short):
        return None
    for a in ((a_l, short) if a_s else (a_l,)):
        if a != short and not (_has_anchors(lf, rf, a) and len(s) >= 2 * a):
            continue
        p = _pair(s, lf, rf, a)
        if p is not None:
            i, j, strand = p
            body = s[i + a:j]
            return a, j - i - a, strand, revcomp(body) if strand else body
    return None


def pick_word(level, span, contig, strand):
    return level << 56 | min(span + 1, SPAN_SAT) << 32 | (CONTIG_MAX - contig) << 1 | strand


@functools.lru_cache(maxsize=4096)
def levenshtein(a, b):
    """The full-matrix distance of two byte strings, unit costs, a row at a time: t = min(diagonal + (x != y), above + 1), then the cells
    to the left, row[j] = min over k <= j of t[k] + (j - k), as a running minimum of t[k] - k."""
    if not a or not b:
        return len(a) + len(b)
    x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
    at = np.arange(len(y) + 1, dtype=np.int64)
    row, t = at.copy(), np.empty(len(y) + 1, dtype=np.int64)
    for i in range(1, len(x) + 1):
        t[0] = i
        np.minimum(row[:-1] + (y != x[i - 1]), row[1:] + 1, out=t[1:])
        row = np.minimum.accumulate(t - at) + at
    return int(row[-1])


def distance(w, p, max_dist):
    """(lcp, lcs, dist) of two fills: dist is the Levenshtein distance when it is at most max_dist, else 0xFFFF (a length difference beyond
    max_dist decides that without a DP).  Prefix and suffix are stripped first, which changes no distance."""
    m = min(len(w), len(p))
    lcp = next((x for x in range(m) if w[x] != p[x]), m)
    lcs = next((x for x in range(m - lcp) if w[len(w) - 1 - x] != p[len(p) - 1 - x]), m - lcp)
    if abs(len(w) - len(p)) > max_dist:
        return lcp, lcs, B.FA_DIST_FAR
    d = levenshtein(w[lcp:len(w) - lcs], p[lcp:len(p) - lcs])
    return lcp, lcs, d if d <= max_dist else B.FA_DIST_FAR


def alts_host(contigs, flanks, best, anchors=(30, 15), max_dist=MAX_DIST, first=0):
    """The twin.  contigs: [(gap, text)] in list order (the position is the contig index; a gap outside 0 .. n_gaps - 1 is a tombstone),
    of which those from index `first` on are candidates (the winner is found at any index); flanks: [(left, right)] per gap; best: the
    pick words per gap (0: open).  Returns (records: _lib.FILL_ALT per gap, per-contig records: _lib.FILL_ALT_CONTIG, statistics:
    {STAT_KEYS})."""
    max_dist = check_params(max_dist)
    a_l, a_s = check_anchors(anchors)
    n_gaps, n = len(flanks), len(contigs)
    fl = [(_bytes(l), _bytes(r)) for l, r in flanks]
    rec = np.zeros(n_gaps, dtype=B.FILL_ALT)
    per = np.zeros(n, dtype=B.FILL_ALT_CONTIG)
    st = dict.fromkeys(STAT_KEYS, 0)
    winners = {}                                 # gap: (word, level, contig, fill, strand)
    for g in range(n_gaps):
        word = int(best[g])
        if not word:
            continue
        st["closed_gaps"] += 1
        level, field, ci, strand = word >> 56, (word >> 32) & SPAN_SAT, CONTIG_MAX - ((word >> 1) & CONTIG_MAX), word & 1
        c = candidate(_bytes(contigs[ci][1]), *fl[g], a_l, a_s) if ci < n and int(contigs[ci][0]) == g else None
        if c is None or c[0] != level or c[2] != strand or not (c[1] + 1 == field if field < SPAN_SAT else c[1] + 1 >= field):
            rec[g]["level"], rec[g]["flags"] = level, B.FA_F_LOST
            st["lost"] += 1
            continue
        winners[g] = (word, level, ci, c[3], strand)
        per[ci] = (len(c[3]), B.FA_DIST_FAR, B.FA_C_WINNER, strand)
        st["candidates"] += 1
    tally = {g: dict(n=1, lower=0, identical=0, near=0, far=0, lens=[len(w[3])], outranked=False, rivals=[]) for g, w in winners.items()}
    for ci, (g, text) in enumerate(contigs):
        g = int(g)
        if ci < first or g not in winners or ci == winners[g][2]:
            continue
        c = candidate(_bytes(text), *fl[g], a_l, a_s)
        if c is None:
            continue
        word, level, _, W, _ = winners[g]
        lvl, span, strand, P = c
        t = tally[g]
        t["n"] += 1
        st["candidates"] += 1
        if lvl < level:
            t["lower"] += 1
            st["lower"] += 1
            per[ci] = (span, B.FA_DIST_FAR, B.FA_C_LOWER, strand)
            continue
        if lvl > level:
            t["outranked"] = True
            continue
        own = pick_word(lvl, span, ci, strand)
        t["outranked"] |= own > word
        t["lens"].append(span)
        lcp, lcs, d = distance(W, P, max_dist)
        name, cls = ("identical", B.FA_C_IDENTICAL) if W == P else ("near", B.FA_C_NEAR) if d != B.FA_DIST_FAR else ("far", B.FA_C_FAR)
        t[name] += 1
        st[name] += 1
        per[ci] = (span, d if cls == B.FA_C_NEAR else B.FA_DIST_FAR, cls, strand)
        if cls != B.FA_C_IDENTICAL:
            t["rivals"].append((own, ci, span, lcp, lcs, d, strand))
    for g, (word, level, ci, W, strand) in winners.items():
        t = tally[g]
        flags = (B.FA_F_REVERSE if strand else 0) | (B.FA_F_OUTRANKED if t["outranked"] else 0) | (B.FA_F_LENGTH_VARIES if min(t["lens"]) != max(t["lens"]) else 0)
        rival = (0, 0, 0, 0, 0, 0, 0)
        if t["rivals"]:
            rival = max(t["rivals"])
            flags |= B.FA_F_HAS_RIVAL | (B.FA_F_RIVAL_REVERSE if rival[6] else 0)
        _, rci, rlen, lcp, lcs, d, _ = rival
        rec[g] = (ci, rci, len(W), rlen, lcp, lcs, min(t["lens"]), max(t["lens"]), min(t["n"], 0xFFFF), min(t["lower"], 0xFFFF),
                  min(t["identical"], 0xFFFF), min(t["near"], 0xFFFF), min(t["far"], 0xFFFF), d, level, flags, 0)
        st["contested"] += bool(t["rivals"])
        st["length_varies"] += bool(flags & B.FA_F_LENGTH_VARIES)
        st["outranked"] += t["outranked"]
    return rec, per, st


def stats_dict(words):
    """The statistics words of gf_fill_alts_dev as alts_host's dictionary."""
    return {k: int(words[w]) for k, w in zip(STAT_KEYS, _WORDS)}


class FillAlternatives:
    """The round object the Pipeline holds (the shape of flank_joins.FlankJoins)."""

    def __init__(self, pipe, max_dist=MAX_DIST):
        self.p, self.max_dist = pipe, check_params(max_dist)
        self.d_rec = None

    def prepare(self):
        """Called once, after the rounds have settled the capacities of the step's contig list."""
        p = self.p
        self.anchor_pair = check_anchors(p.anchors)
        self.d_rec = p._u8(p.n_gaps * B.FILL_ALT.itemsize)
        self.d_per = p._u8(p.contig_cap * B.FILL_ALT_CONTIG.itemsize)
        self.d_stats = torch.zeros(B.FA_WORDS, dtype=torch.int32, device=p.dev)

    def enqueue(self):
        """After the last pick of the step, beside the joins and before the extended fill: the alternatives of the gaps d_best closes, over all of the step's contigs."""
        p = self.p
        if self.d_rec is None:        # a sizing run of one of the rounds: nobody reads its records
            return
        p._chk(p.lib.gf_fill_alts_dev(p.h, p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), *self.anchor_pair, self.max_dist, None,
                                      p.d_best.data_ptr(), self.d_rec.data_ptr(), self.d_per.data_ptr(), self.d_stats.data_ptr()), "gf_fill_alts_dev")

    def fetch(self, r):
        p = self.p
        r.alts = np.frombuffer(self.d_rec[:p.n_gaps * B.FILL_ALT.itemsize].cpu().numpy().tobytes(), dtype=B.FILL_ALT)
        r.alt_contigs = np.frombuffer(self.d_per[:len(r.contigs) * B.FILL_ALT_CONTIG.itemsize].cpu().numpy().tobytes(), dtype=B.FILL_ALT_CONTIG)
        r.alt_stats = stats_dict(self.d_stats.cpu().numpy().view(np.uint32))
        if r.alt_stats["lost"]:
            lost = [int(g) for g in np.nonzero(r.alts["flags"] & B.FA_F_LOST)[0]]
            raise RuntimeError("fill alternatives: the pick words of %d gaps (%s) do not lead back to their contigs" % (len(lost), lost[:8]))


def alts_of_results(pipe, res):
    """The twin on a step's Results: what Results.alts, .alt_contigs and .alt_stats must equal."""
    return alts_host(contigs_of_results(res), pipe.gf.flanks, res.best, pipe.anchors, pipe.alts.max_dist)
