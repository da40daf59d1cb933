"""Flank anchoring -> gap sequence selection (SURVEY.md §8f "next" rank 1; mirrors ContigsSelection, pick_contigs.py:64-358,
361-539, 542-603).  The reference aligns the two flanks to the gap's contigs with `bwa mem -T {score} -a`, and everything after
that is its own code: per contig and side the longest hit of each clip type (:97-146), the best same-strand pair of a left and a
right hit (:149-297), over the contigs the longest span (:300-321), the slice (:341-349) and the header (:352).  bwa is out of scope
here; its place is taken by EXACT anchors (`anchor_hits`): the last `score` bases of the left flank and the first `score` bases of
the right flank (score = the reference's bwa_min_score: 30, later 15).  The selection itself follows the reference hit for hit —
including what its coordinates do on the reverse strand (the slice then keeps the last base of the LEFT anchor instead of the
first base of the right one) — and is pinned on the reference's own answers (tests/golden/pick_kat.json.gz through
oracle/gp_oracle.py).  The same rule runs on the device as gf_pick_anchored_dev (csrc/pick.hip).  A gap with a picked sequence
is what this build reports as "closed".

A second, opt-in stand-in (`mode="align"`, `align_hits`) is closer to what bwa does: ungapped seed-and-extend of the WHOLE flanks.
Exact anchors lose a gap to one draft base that differs from the reads within `score` bases of the flank's gap-side end; bwa aligns
through such a base.  bwa is absent here, so this definition is this build's own, modelled on bwa mem's defaults and pinned on
hand-derived answers (tests/test_pick_align_host.py), not on bwa's output.  For every contig, side and strand:
  query      Q = the flank (forward strand) or revcomp(flank) (reverse strand), aligned to the FORWARD contig, so positions and clip
             types come out in SAM's frame, as in the reference's flanks.sam;
  seeds      on each diagonal d (contig index = query index + d) a seed is a maximal run of >= SEED_LEN (19, `-k`) consecutive
             identical ACGT bases; diagonals ascending, seeds left to right; a seed that lies inside an alignment already produced on
             its diagonal is skipped (every produced alignment counts, whatever its score);
  extension  left first, then right, ungapped, from the seed's length as score: match +1, mismatch -4, a non-ACGT base on either
             side -1; each side keeps the FIRST maximum of the running score and stops when the running score falls more than
             ZDROP (100) below it;
  end rule   when the contig reaches the query's end on that side and the extension got there without stopping, g = the running
             score at that end: the alignment goes to the end when g > 0 and g > best - CLIP_PEN (5), else it is clipped at the
             maximum (bwa's `gscore <= 0 || gscore <= score - pen_clip`);
  hit        reported when its score >= T (the round's score, 30 or 15): pos = contig index of the first aligned query base + 1,
             M = aligned length, clip type from (query start > 0, query end < |Q|): BOTH, LEFT, RIGHT or NONE;
  cap        at most ALIGN_CAP (64) alignments per (contig, side, strand), in the order they were produced; later ones are dropped
             and counted; a contig with more than SEED_MAX (1024) seeds over both flanks and strands gives no hits and is counted;
  order      within a (contig, side) hits are ordered by score descending, forward before reverse, then pos ascending — so
             select_full's "first on ties" and pick_extended_sequence's "first contig" mean something definite.
Flanks are limited to FLANK_MAX (1 024) bases.  Indels between flank and contig are out of scope in this mode.  The device runs the
same rule as gf_pick_aligned_dev (csrc/pick_align.hip).

A third, opt-in stand-in (`mode="gapped"`, `gapped_hits`) aligns THROUGH an indel between flank and contig: a draft base inserted or
deleted within `score` bases of a flank's gap-side end breaks the exact anchors, and leaves an `align` hit clipped on the gap side.
Again the definition is this build's own, on bwa mem's defaults (`-O 6 -E 1`), pinned on hand-derived answers
(tests/test_pick_gapped_host.py).  Queries, seeds, production order (query, diagonal, query start), thresholds, ALIGN_CAP, SEED_MAX,
FLANK_MAX, the hit order and the clip types are those of `align`; what differs:
  extension  from each end of the seed run (left end first, then right) a banded affine-gap DP over cells (i, j) = (contig bases, query
             bases) taken beyond the seed in the direction of extension: H(0, 0) = the score so far (the seed length on the left, the
             left result on the right); H(i, j) = max(H(i-1, j-1) + s, E, F) with s = match +1, mismatch -4, non-ACGT on either side -1,
             E(i, j) = max(H(i, j-1) - 7, E(i, j-1) - 1), F(i, j) = max(H(i-1, j) - 7, F(i-1, j) - 1): a gap of g bases costs
             GAP_OPEN + g * GAP_EXT = 6 + g; only cells with |i - j| <= GAP_BAND (31) exist; a value <= 0 is dead and propagates
             nothing; there is NO z-drop, so the values do not depend on the order the cells are evaluated in;
  results    best = the maximum live H, at the first such cell in (i ascending, j ascending) order; g = the maximum live H in the
             query's last column on that side, first by i; the side runs to the query's end at g's cell when g > 0 and
             g > best - CLIP_PEN, else it stops at best's cell.  No traceback: the scores and the two end cells are all there is;
  hit        pos = contig index of the first aligned CONTIG base + 1; M = the number of CONTIG bases the alignment covers (contig
             end - contig begin).  A stated departure from the reference, whose map_length sums the CIGAR's M columns only
             (pick_contigs.py:35-62): every consumer (the slices of pick_gap_sequence and pick_extended_sequence, the span of
             select_per_contig) uses pos + M - 1 as the alignment's last contig base, and with the M-sum an alignment through a
             deletion would cut the gap sequence at the wrong base.  Ungapped hits are the same under both readings;
  skip       a seed is skipped when an alignment kept for the same query contains it: the seed run's query interval lies inside the
             alignment's query interval and the seed's first contig base inside its contig interval (whatever the alignment's score);
  cap        a seed that is not skipped produces an alignment; the first ALIGN_CAP per (contig, side, strand) are extended and kept
             (for the hits and for the skip rule), later ones are counted as dropped and neither extended nor kept.
The device runs the same rule as gf_pick_gapped_dev (the gapped instantiation of csrc/pick_align.hip)."""
import os

import numpy as np

_COMP = str.maketrans("ACGTacgt", "TGCATGCA")            # gnrt_reverse_complementary, pick_contigs.py:19-33: upper-case output
_BOTH, _LEFT, _RIGHT, _NONE = 1, 2, 3, 4                 # clip types (pick_contigs.py:9-12)


def revcomp(s):
    return s.translate(_COMP)[::-1]


# The reference's rounds read a gap's small FASTA files again and again (flanks: twice per pick and round; contigs.fa: every merge, pick
# and recruit step — 23 000 parses for 1 000 gaps).  A parse is kept per path and handed out again while the file's (mtime, size, inode) stay
# what they were: one stat instead of open + read + split.  Files beyond 1 MB (a draft) are never kept.
_FASTA_CACHE, _FASTA_CACHE_BYTES = {}, [0]


def _cached_fasta(path, parse):
    st = os.stat(path)
    key = (st.st_mtime_ns, st.st_size, st.st_ino)
    hit = _FASTA_CACHE.get(path)
    if hit is not None and hit[0] == key:
        return list(hit[1])
    recs = parse(path)
    if st.st_size <= (1 << 20):
        if _FASTA_CACHE_BYTES[0] > (1 << 30):      # (a human-scale run: 20 000 gaps x a few files x tens of kB stay far below)
            _FASTA_CACHE.clear()
            _FASTA_CACHE_BYTES[0] = 0
        _FASTA_CACHE[path] = (key, recs)
        _FASTA_CACHE_BYTES[0] += st.st_size
    return list(recs)


def read_fasta(path):
    return _cached_fasta(path, _parse_fasta)


def _parse_fasta(path):
    out, name, chunks = [], None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(chunks)))
                name, chunks = line[1:].split()[0], []
            elif line:
                chunks.append(line)
    if name is not None:
        out.append((name, "".join(chunks)))
    return out


def anchor_hits(contigs, left_flank, right_flank, score):
    """The stand-in for `bwa mem -T {score} -a` (pick_contigs.py:79-86): [(side, reverse?, contig index, 1-based position in the
    contig, clip type, matched bases)], per contig forward left / forward right / reverse left / reverse right.  Forward: the
    LEFTMOST occurrence of the left anchor, the RIGHTMOST of the right anchor; reverse: the same in the reverse-complemented
    contig, reported in the contig's own coordinates with the clip on the other end, as SAM does."""
    a = int(score)
    if len(left_flank) < a or len(right_flank) < a:
        return []
    la, ra = left_flank[len(left_flank) - a:], right_flank[:a]
    if any(c not in "ACGT" for c in la + ra):
        return []
    l_clipped, r_clipped = len(left_flank) > a, len(right_flank) > a
    out = []
    for ci, (_, seq) in enumerate(contigs):
        n = len(seq)
        for rev, s in ((False, seq), (True, revcomp(seq))):
            i, j = s.find(la), s.rfind(ra)
            if i >= 0:       # left flank = [clipped part][anchor]: clip in front on the forward strand, behind on the reverse strand
                out.append(("left", rev, ci, n - i - a + 1 if rev else i + 1, _NONE if not l_clipped else _RIGHT if rev else _LEFT, a))
            if j >= 0:
                out.append(("right", rev, ci, n - j - a + 1 if rev else j + 1, _NONE if not r_clipped else _LEFT if rev else _RIGHT, a))
    return out


SEED_LEN, MATCH, MISMATCH, N_SCORE, ZDROP, CLIP_PEN = 19, 1, -4, -1, 100, 5     # bwa mem: -k, -A, -B, N penalty, -d, -L
ALIGN_CAP, SEED_MAX, FLANK_MAX = 64, 1024, 1024
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _seeds(qs, c, index):
    """Seeds of the four queries in one contig: [(query id, diagonal, query start)] (run starts of >= SEED_LEN identical ACGT bases)."""
    out = []
    for p in range(len(c) - SEED_LEN + 1):
        for qi, q in index.get(c[p:p + SEED_LEN], ()):
            Q = qs[qi]
            if p == 0 or q == 0 or Q[q - 1] != c[p - 1] or Q[q - 1] not in _CODE:
                out.append((qi, p - q, q))
    return out


def _sc(a, b):
    if a not in _CODE or b not in _CODE:
        return N_SCORE
    return MATCH if a == b else MISMATCH


def _extend(Q, c, d, qs):
    """One seed -> (query begin, query end, score, seed end)."""
    n, m = len(Q), len(c)
    se = qs
    while se < n and se + d < m and Q[se] == c[se + d] and Q[se] in _CODE:
        se += 1
    run = best = se - qs
    qb, i, stopped = qs, qs - 1, False
    while i >= 0 and i + d >= 0:
        run += _sc(Q[i], c[i + d])
        if run > best:
            best, qb = run, i
        elif best - run > ZDROP:
            stopped = True
            break
        i -= 1
    score = best
    if not stopped and i < 0 and run > 0 and run > best - CLIP_PEN:
        qb, score = 0, run
    run = best = score
    qe, j, stopped = se, se, False
    while j < n and j + d < m:
        run += _sc(Q[j], c[j + d])
        if run > best:
            best, qe = run, j + 1
        elif best - run > ZDROP:
            stopped = True
            break
        j += 1
    score = best
    if not stopped and j == n and run > 0 and run > best - CLIP_PEN:
        qe, score = n, run
    return qb, qe, score, se


def _alignments(contig, queries, index, cap, stats):
    """Per query id (0 left, 1 revcomp(left), 2 right, 3 revcomp(right)) the alignments that survive the cap, in production order:
    [(diagonal, query begin, query end, score)]."""
    seeds = _seeds(queries, contig, index)
    out = [[], [], [], []]
    if len(seeds) > SEED_MAX:
        stats["seed_overflow"] = stats.get("seed_overflow", 0) + 1
        return out
    produced = [0, 0, 0, 0]
    last, max_qe = None, -1
    for qi, d, q in sorted(seeds):
        if (qi, d) != last:
            last, max_qe = (qi, d), -1
        qb, qe, score, se = _extend(queries[qi], contig, d, q)
        if se <= max_qe:                     # inside an alignment already produced on this diagonal
            continue
        max_qe = max(max_qe, qe)
        produced[qi] += 1
        if produced[qi] > cap:
            stats["dropped"] = stats.get("dropped", 0) + 1
            continue
        out[qi].append((d, qb, qe, score))
    return out


def _queries(left_flank, right_flank):
    if len(left_flank) > FLANK_MAX or len(right_flank) > FLANK_MAX:
        raise ValueError("align mode: flanks are limited to %d bases" % FLANK_MAX)
    strict = lambda f: "".join(x if x in _CODE else "N" for x in f)      # (a non-ACGT base stays one on the other strand)
    qs = (left_flank, revcomp(strict(left_flank)), right_flank, revcomp(strict(right_flank)))
    index = {}
    for qi, Q in enumerate(qs):
        for q in range(len(Q) - SEED_LEN + 1):
            k = Q[q:q + SEED_LEN]
            if all(x in _CODE for x in k):
                index.setdefault(k, []).append((qi, q))
    return qs, index


def align_hits(contigs, left_flank, right_flank, score, cap=ALIGN_CAP, stats=None):
    """The `align` stand-in for `bwa mem -T {score} -a` (the definition: this module's docstring): the same hit tuples as
    anchor_hits, [(side, reverse?, contig index, 1-based position in the contig, clip type, matched bases)], per contig the left
    hits, then the right hits, each in the documented order.  stats (a dict or None) counts "dropped" alignments beyond the cap and
    contigs skipped for "seed_overflow"."""
    stats = {} if stats is None else stats
    qs, index = _queries(left_flank, right_flank)
    out = []
    for ci, (_, seq) in enumerate(contigs):
        per_q = _alignments(seq, qs, index, int(cap), stats)
        for side, q0 in (("left", 0), ("right", 2)):
            hits = []
            for rev in (False, True):
                n = len(qs[q0 + rev])
                for d, qb, qe, sc in per_q[q0 + rev]:
                    if sc < score:
                        continue
                    ct = _BOTH if qb > 0 and qe < n else _LEFT if qb > 0 else _RIGHT if qe < n else _NONE
                    hits.append((-sc, rev, d + qb + 1, ct, qe - qb))
            hits.sort(key=lambda h: h[:3])
            out += [(side, rev, ci, pos, ct, m) for _, rev, pos, ct, m in hits]
    return out


GAP_OPEN, GAP_EXT, GAP_BAND = 6, 1, 31                   # bwa mem: -O, -E; the band is this build's: 63 diagonals, one wavefront
_DEAD = -(1 << 20)
_SUB = np.array([[MATCH if a == b else MISMATCH for b in range(4)] + [N_SCORE] for a in range(4)] + [[N_SCORE] * 5], dtype=np.int64)


def _codes(s):
    return np.array([_CODE.get(x, 4) for x in s], dtype=np.int64)


def _gapped_side(qc, cc, h0):
    """One side of the gapped extension.  qc, cc: the codes of the query / the contig beyond the seed, in the direction of extension;
    h0: the score so far.  Returns (score, contig bases taken, query bases taken).  Row by row (i = contig bases); in a row the band's
    cells are indexed by b = j - i + GAP_BAND, so (i-1, j-1) is the previous row's b and (i-1, j) its b + 1; the in-row gap state E is
    a running maximum: E(i, j) = max over j' < j of max(M, F)(i, j') - GAP_OPEN - (j - j') * GAP_EXT (opening from an E costs more than
    extending it, and a positive end of such a chain has positive links)."""
    J, W = len(qc), 2 * GAP_BAND + 1
    I = min(len(cc), J + GAP_BAND)
    # column j of the query at index j + GAP_BAND: the substitution scores against each contig code, dead outside 1..J / 0..J
    prof = np.full((5, J + 3 * GAP_BAND + 2), _DEAD, dtype=np.int64)
    prof[:, GAP_BAND + 1:GAP_BAND + 1 + J] = _SUB[:, qc] if J else 0
    col = np.full(J + 3 * GAP_BAND + 2, _DEAD, dtype=np.int64)
    col[GAP_BAND:GAP_BAND + J + 1] = 0
    ar = np.arange(W, dtype=np.int64)
    H, F = np.full(W + 1, _DEAD, dtype=np.int64), np.full(W + 1, _DEAD, dtype=np.int64)
    H[GAP_BAND] = h0
    for j in range(1, min(J, GAP_BAND) + 1):                     # row 0: a gap of j query bases
        if h0 - GAP_OPEN - j * GAP_EXT > 0:
            H[GAP_BAND + j] = h0 - GAP_OPEN - j * GAP_EXT
    best, bi, bj = h0, 0, 0
    g, gi = 0, 0
    if J <= GAP_BAND and H[GAP_BAND + J] > 0:
        g = int(H[GAP_BAND + J])
    for i in range(1, I + 1):
        Fn = np.maximum(H[1:] - (GAP_OPEN + GAP_EXT), F[1:] - GAP_EXT)
        Hq = np.maximum(H[:W] + prof[cc[i - 1], i:i + W], Fn)
        acc = np.maximum.accumulate(Hq + ar * GAP_EXT)
        Hn = Hq.copy()
        np.maximum(Hn[1:], acc[:-1] - GAP_OPEN - ar[1:] * GAP_EXT, out=Hn[1:])
        Hn += col[i:i + W]
        Hn[Hn <= 0] = _DEAD
        mx = int(Hn.max())
        if mx <= 0:                                              # a dead row: no F below it, nothing lives on
            break
        if mx > best:
            best, bi, bj = mx, i, i - GAP_BAND + int(Hn.argmax())
        b = J - i + GAP_BAND
        if 0 <= b < W and Hn[b] > g:
            g, gi = int(Hn[b]), i
        H[:W], F[:W] = Hn, Fn
    if g > 0 and g > best - CLIP_PEN:
        return g, gi, J
    return best, bi, bj


def _gapped_extend(Qc, Cc, d, qs):
    """One seed -> (query begin, query end, contig begin, contig end, score); Qc, Cc: the codes of the query and the contig."""
    n, m = len(Qc), len(Cc)
    se = qs
    while se < n and se + d < m and Qc[se] == Cc[se + d] and Qc[se] < 4:
        se += 1
    score, ci, qj = _gapped_side(Qc[:qs][::-1], Cc[:qs + d][::-1], se - qs)
    qb, cb = qs - qj, qs + d - ci
    score, ci, qj = _gapped_side(Qc[se:], Cc[se + d:], score)
    return qb, se + qj, cb, se + d + ci, score


_GAPPED_CACHE = {}       # the rounds ask for one gap's contigs at score 30, then 15: the alignments do not depend on the score


def _gapped_alignments(contig, queries, index, cap, stats):
    """Per query id the alignments kept, in production order: [(query begin, query end, contig begin, contig end, score)]."""
    key = (contig, queries, cap)
    if key not in _GAPPED_CACHE:
        if len(_GAPPED_CACHE) >= 4096:
            _GAPPED_CACHE.clear()
        own = {}
        _GAPPED_CACHE[key] = (_gapped_alignments_of(contig, queries, index, cap, own), own)
    out, own = _GAPPED_CACHE[key]
    for k, v in own.items():
        stats[k] = stats.get(k, 0) + v
    return out


def _gapped_alignments_of(contig, queries, index, cap, stats):
    seeds = _seeds(queries, contig, index)
    out = [[], [], [], []]
    if len(seeds) > SEED_MAX:
        stats["seed_overflow"] = stats.get("seed_overflow", 0) + 1
        return out
    Cc, Qc = _codes(contig), [_codes(q) for q in queries]
    produced = [0, 0, 0, 0]
    for qi, d, q in sorted(seeds):
        Q, se = Qc[qi], q
        while se < len(Q) and se + d < len(Cc) and Q[se] == Cc[se + d] and Q[se] < 4:
            se += 1
        if any(qb <= q and se <= qe and cb <= q + d < ce for qb, qe, cb, ce, _ in out[qi]):
            continue
        produced[qi] += 1
        if produced[qi] > cap:
            stats["dropped"] = stats.get("dropped", 0) + 1
            continue
        out[qi].append(_gapped_extend(Q, Cc, d, q))
    return out


def gapped_hits(contigs, left_flank, right_flank, score, cap=ALIGN_CAP, stats=None):
    """The `gapped` stand-in for `bwa mem -T {score} -a` (the definition: this module's docstring): align_hits' hit tuples in
    align_hits' order, from alignments that may run through an indel; the matched bases are the CONTIG bases covered.  stats as for
    align_hits."""
    stats = {} if stats is None else stats
    qs, index = _queries(left_flank, right_flank)
    out = []
    for ci, (_, seq) in enumerate(contigs):
        per_q = _gapped_alignments(seq, qs, index, int(cap), stats)
        for side, q0 in (("left", 0), ("right", 2)):
            hits = []
            for rev in (False, True):
                n = len(qs[q0 + rev])
                for qb, qe, cb, ce, sc in per_q[q0 + rev]:
                    if sc < score:
                        continue
                    ct = _BOTH if qb > 0 and qe < n else _LEFT if qb > 0 else _RIGHT if qe < n else _NONE
                    hits.append((-sc, rev, cb + 1, ct, ce - cb))
            hits.sort(key=lambda h: h[:3])
            out += [(side, rev, ci, pos, ct, m) for _, rev, pos, ct, m in hits]
    return out


ANCHOR_MODES = ("exact", "align", "gapped")


def stand_in_hits(mode, contigs, left_flank, right_flank, score):
    if mode == "exact":
        return anchor_hits(contigs, left_flank, right_flank, score)
    if mode == "align":
        return align_hits(contigs, left_flank, right_flank, score)
    if mode == "gapped":
        return gapped_hits(contigs, left_flank, right_flank, score)
    raise ValueError("flank anchor mode %r: 'exact', 'align' or 'gapped'" % (mode,))


_PAIRS = ((_NONE, _NONE), (_NONE, _LEFT), (_NONE, _RIGHT), (_LEFT, _NONE), (_LEFT, _RIGHT), (_RIGHT, _NONE), (_RIGHT, _LEFT))


def select_full(hits):
    """pick_contigs.py:97-321 on hit tuples: (contig index, left pos, right pos, left match, right match, reverse?) or None."""
    best = None
    for ci, (span, lp, rp, lm, rm, rc) in select_per_contig(hits).items():
        if span > (-1 if best is None else best[0]):     # longest span, the earlier contig on ties (:313-321)
            best = (span, ci, lp, rp, lm, rm, rc)
    return None if best is None else best[1:]


def select_per_contig(hits):
    """pick_contigs.py:97-297 per contig: {contig index: (span, left pos, right pos, left match, right match, reverse?)}, in the
    order the contigs first appear among the hits; only contigs with a same-strand pair."""
    table = {}                                           # contig -> side -> clip type -> (reverse?, match, pos)
    for side, rev, ci, pos, ct, m in hits:
        if ct == _BOTH:
            continue
        slot = table.setdefault(ci, {}).setdefault(side, {})
        if ct not in slot or m > slot[ct][1]:
            slot[ct] = (rev, m, pos)
    out = {}
    for ci, sides in table.items():
        if len(sides) != 2:
            continue
        top, sel, rc = -1, None, False
        for lt, rt in _PAIRS:                            # the reference's seven pairs in its order (:173-291)
            l, r = sides["left"].get(lt), sides["right"].get(rt)
            if l is None or r is None or l[0] != r[0] or not top < l[1] + r[1]:
                continue
            top, sel = l[1] + r[1], (l[2], r[2], l[1], r[1])
            rc = rc or l[0]                              # (:176-177: set by any winning reverse pair, never cleared)
        if sel is None:
            continue
        lp, rp, lm, rm = sel
        out[ci] = ((lp - (rp + rm)) if rc else (rp - (lp + lm)), lp, rp, lm, rm, rc)
    return out


def pick_gap_sequence(contigs, left_flank, right_flank, anchor_len, mode="exact"):
    """contigs: [(name, seq)].  Returns (name, gap_seq, contig as written to picked_contigs.fa) or None (pick_contigs.py:331-358).
    mode: the stand-in for bwa's hits, "exact" (anchor_hits), "align" (align_hits; anchor_len is then the score threshold) or "gapped"
    (gapped_hits, likewise)."""
    sel = select_full(stand_in_hits(mode, contigs, left_flank, right_flank, anchor_len))
    if sel is None:
        return None
    ci, lp, rp, lm, rm, rc = sel
    name, seq = contigs[ci]
    if rc:
        return name, revcomp(seq[rp + rm - 1:lp]), revcomp(seq)
    return name, seq[lp + lm - 1:rp], seq


def pick_extended_sequence(contigs, left_flank, right_flank, anchor_len, mode="exact"):
    """The fallback of the last round (run_pick_extended_contig, pick_contigs.py:361-539): no contig carries both anchors in
    order, so the gap is filled from each side as far as a contig reaches and the parts are joined by 'NN' (:517-525).  Hit for
    hit the reference's rule on the stand-in's hits: clipped hits only (:388-389), per side the contig with the longest match —
    the anchors all match `anchor_len` bases and the reference's tie test is constant (int > str, :444, :457), so the FIRST contig
    with a hit; when both sides pick the same contig only the right side is used, and its slice then keeps the first anchor base
    (:480-486 vs :509-512); reverse-strand slices keep one anchor base as well (:496, :474).  In "align" mode the hits carry real
    match lengths, but the tie test stays constant, so it is still the first hit in align_hits' order ("gapped": the same order).  Returns (left_name,
    right_name, sequence or None, picked_contigs text or None)."""
    first = {"left": None, "right": None}
    for side, rev, ci, pos, ct, m in stand_in_hits(mode, contigs, left_flank, right_flank, anchor_len):
        want = (_RIGHT if rev else _LEFT) if side == "left" else (_LEFT if rev else _RIGHT)
        if ct == want and first[side] is None:
            first[side] = (ci, pos, m, rev)
    l, r = first["left"], first["right"]
    if l is None and r is None:
        return None
    l_seq = r_seq = text = ""
    rc_l = rc_r = True
    if l is not None and r is not None and l[0] == r[0]:
        l = None
        ci, pos, m, rc_r = r
        seq = contigs[ci][1]
        r_seq, text = (seq[pos + m - 1:] if rc_r else seq[:pos]), seq
        rc_l = first["left"][3]
    else:
        if l is not None:
            ci, pos, m, rc_l = l
            seq = contigs[ci][1]
            l_seq, text = (seq[:pos] if rc_l else seq[pos + m - 1:]), seq
        if r is not None:
            ci, pos, m, rc_r = r
            seq = contigs[ci][1]
            r_seq, text = (seq[pos + m - 1:] if rc_r else seq[:pos - 1]), text + "NN" + seq
    out = (revcomp(l_seq) if rc_l else l_seq) + "NN" + (revcomp(r_seq) if rc_r else r_seq)
    names = tuple(contigs[x[0]][0] if x is not None else "" for x in (first["left"], first["right"]))
    return names[0], names[1], (out if out != "NN" else None), (text if text not in ("", "NN") else None)


def extension_order(contigs, k_pairs):
    """The contig order of the device step's extended fill (gf_pick_extended_dev): pick_extended_sequence takes the FIRST contig with
    a hit per side, and the device lists a gap's contigs in no fixed order.  contigs: [(k, kv, bases)]; k_pairs: the pipeline's
    [(k, kv)].  Returns the contig indices sorted by (position of (k, kv) in k_pairs — the merged contigs' (0, 0) and any pair not in
    the list after every pair, as contigs.fa concatenates the per-pair files, and the rescue round's bridges (RESCUE_MARK, RESCUE_MARK)
    after those —, length descending, bases ascending, index)."""
    from ._lib import RESCUE_MARK
    rank = {(RESCUE_MARK, RESCUE_MARK): len(k_pairs) + 1}
    for i, (k, kv) in enumerate(k_pairs):
        rank.setdefault((int(k), int(kv)), i)
    n = len(k_pairs)
    return sorted(range(len(contigs)), key=lambda i: (rank.get((int(contigs[i][0]), int(contigs[i][1])), n), -len(contigs[i][2]),
                                                      contigs[i][2], i))


def decode_extended(rec, contig_seq):
    """One gf_ext_pick record (fields left, right, l_beg, l_len, l_rev, r_beg, r_len, r_rev; 0xFFFFFFFF = no contig) -> the fields of
    pick_extended_sequence with contig indices for names: (left contig or -1, right contig or -1, fill or None, picked_contigs text or
    None), or None when neither side has a contig.  contig_seq(i) = the bases of contig i."""
    none = 0xFFFFFFFF
    left, right = int(rec["left"]), int(rec["right"])
    if left == none and right == none:
        return None
    parts = []
    for ci, beg, n, rev in ((left, rec["l_beg"], rec["l_len"], rec["l_rev"]), (right, rec["r_beg"], rec["r_len"], rec["r_rev"])):
        s = contig_seq(ci)[int(beg):int(beg) + int(n)] if int(n) else ""
        parts.append(revcomp(s) if int(rev) else s)
    fill = parts[0] + "NN" + parts[1]
    if left != none and left == right:
        text = contig_seq(right)
    else:
        text = (contig_seq(left) if left != none else "") + ("NN" + contig_seq(right) if right != none else "")
    return (left if left != none else -1, right if right != none else -1, fill if fill != "NN" else None,
            text if text not in ("", "NN") else None)


class ContigsSelection:
    def __init__(self, working_space, mode="exact"):
        """mode: how the flanks are anchored on the contigs, "exact" (anchor_hits), "align" (align_hits) or "gapped" (gapped_hits)."""
        if mode not in ANCHOR_MODES:
            raise ValueError("flank anchor mode %r: 'exact', 'align' or 'gapped'" % (mode,))
        self.working_folder, self.mode = working_space, mode

    def _pick_one(self, gid, anchor_len):
        wf = self.working_folder
        sf_flank = wf + "../flank_regions/%s.fa" % gid
        sf_contig = wf + "velvet_temp/%s/contigs.fa" % gid
        for p in (wf + "velvet_temp/%s/picked_seqs.fa" % gid, wf + "velvet_temp/%s/picked_contigs.fa" % gid):
            if os.path.exists(p):
                os.remove(p)
        if not (os.path.exists(sf_flank) and os.path.exists(sf_contig)):
            return False
        fl = dict(read_fasta(sf_flank))
        res = pick_gap_sequence(read_fasta(sf_contig), fl.get(gid + "_left", ""), fl.get(gid + "_right", ""), anchor_len, self.mode)
        if res is None:
            return False
        name, gap_seq, oriented = res
        if gap_seq:
            with open(wf + "velvet_temp/%s/picked_seqs.fa" % gid, "w") as f:
                f.write(">%s_%s\n%s\n" % (gid, name, gap_seq))
        with open(wf + "velvet_temp/%s/picked_contigs.fa" % gid, "w") as f:
            f.write(">%s_%s\n%s\n" % (gid, name, oriented))
        return bool(gap_seq)

    def pick_full_constructed_contigs(self, bwa_score, fa_list, sf_picked):
        n = 0
        for gid in fa_list:
            if self._pick_one(gid, int(bwa_score)):
                n += 1
            for src, dst in (("picked_seqs.fa", sf_picked), ("picked_contigs.fa", sf_picked + "_ori.txt")):
                p = self.working_folder + "velvet_temp/%s/%s" % (gid, src)
                if os.path.exists(p):
                    with open(dst, "a") as out, open(p) as f:   # the reference appends with `cat >>` (:564-572)
                        out.write(f.read())
        return n

    def pick_extended_contigs(self, bwa_score, fa_list, sf_picked):
        """pick_contigs.py:583-603: per gap velvet_temp/{id}/picked_seqs.fa + picked_contigs.fa with header
        '>{id}_{left contig}_{right contig}_extended', appended to the ledger like the full picks."""
        n = 0
        for gid in fa_list:
            wf = self.working_folder
            sf_flank = wf + "../flank_regions/%s.fa" % gid
            sf_contig = wf + "velvet_temp/%s/contigs.fa" % gid
            if not (os.path.exists(sf_flank) and os.path.exists(sf_contig)):
                continue
            fl = dict(read_fasta(sf_flank))
            res = pick_extended_sequence(read_fasta(sf_contig), fl.get(gid + "_left", ""), fl.get(gid + "_right", ""), int(bwa_score),
                                         self.mode)
            if res is None:
                continue
            left_name, right_name, seq, contig_text = res
            hdr = ">%s_%s_%s_extended\n" % (gid, left_name, right_name)
            for fn, body, dst in (("picked_seqs.fa", seq, sf_picked), ("picked_contigs.fa", contig_text, sf_picked + "_ori.txt")):
                if body is None:                          # nothing but 'NN' to report: the file is not written (:527-537)
                    continue
                with open(wf + "velvet_temp/%s/%s" % (gid, fn), "w") as f:
                    f.write(hdr + body + "\n")
                with open(dst, "a") as out:
                    out.write(hdr + body + "\n")
            n += seq is not None
        return n

    def get_already_picked(self, sf_picked):
        picked = {}
        if os.path.exists(sf_picked):
            with open(sf_picked) as f:
                for line in f:
                    if line[0] == ">":
                        fl = line[1:].split("_")
                        picked[fl[0] + "_" + fl[1]] = 1
        return picked
