"""Pipeline(polish=True, polish_indels=True): the consensus polish of the closed fills (polish.py) with rows that may be placed with ONE
indel, votes on indel events as well as on columns, and a polished contig that may change length (gf_fill_polish_gapped,
_lib.FILL_POLISH_GAPPED; gf_fill_polish_gapped_dev, csrc/fill_polish_gapped.hip).  It replaces the plain polish launch of the step; with
the option off nothing changes.  Body location, skip flags, parameter check and the column decision are polish.py's and fill_rounds.py's.

The definition is the host twin below (polish_gapped_host).  Parameters: polish.py's seed s, max_mismatch, min_overlap,
min_votes, plus max_indel G (1..16).  As there, every row gives two sequences q of L bases (the row; its reverse complement with the mask
reversed), both placed on the contig c AS STORED (n bases); every coordinate is a column of c as stored.
  diagonals   of q: every d = p - j * s of a clean (unmasked) seed window j < L // s of q that equals c at p; first(d) / last(d) are the
              smallest / largest such j
  ungapped    polish.py's accepted (strand, d): cost = mm, ov as there
  split       an ordered pair of seeded diagonals (d1, d2) of one q with 0 < |d2 - d1| <= G.  DEL (c has bases the read lacks):
              g = d2 - d1 > 0, gi = 0; INS (the read has bases c lacks): gi = d1 - d2 > 0.  The breakpoint x ranges over
              [(first(d1) + 1) * s, last(d2) * s - gi] — a clean seed of d1 left of it, a clean seed of d2 right of the inserted bases —,
              an INS needs q[x, x + gi) unmasked.  Left part q[i0, x) on d1, i0 = max(0, -d1); right part q[x + gi, i1) on d2,
              i1 = min(L, n - d2); mm(x) the unmasked differing bases of both parts; the candidate's x has the smallest mm(x), on a tie
              the SMALLEST x (the leftmost column of c for both strands); ov = (x - i0) + (i1 - x - gi); accepted when ov >= min_overlap
              and cost = mm + 2 <= max_mismatch.  Its event: (DEL, p = d1 + x, g) — columns [p, p + g) go away — or
              (INS, p = d1 + x, gi, q[x, x + gi)) — inserted before column p
  placement   all accepted candidates of a row by (cost ascending, ov descending): one best: PLACED there (reads_split counts the rows
              placed split); several: AMBIGUOUS, no vote of any kind; none: ignored
  votes       a placed row votes q[i] on its column for every unmasked aligned i whose column lies in the body [b0, b1) (both parts of
              a split row; inserted bases vote nowhere).  A split row gives one vote to its event when the event lies in the body — DEL:
              b0 <= p and p + g <= b1; INS: b0 <= p <= b1 —, else the event is dropped and counted (events_outside); the row stays placed
  against     of an event e (gd = g for a DEL, 0 for an INS; site [max(0, p - s), min(n, p + gd + s))): the placed rows that do not vote e
              and have one aligned part (one diagonal, contiguous columns) covering the whole site
  decision    columns: polish.py's rule on these votes.  Events: e passes when votes(e) >= min_votes and votes(e) > against(e); the
              passing events by (votes descending, p, DEL before INS, length, inserted bases as a base-4 number) are accepted greedily,
              unless the closed interval [p, p + gd] meets an accepted one's; an INS that would take the inserted total beyond
              MAX_INSERTED (64) bases is dropped and PL_F_INS_CAP set.  More than MAX_EVENTS (64) distinct in-body events on one contig:
              PL_F_EVENTS, no event applied (columns still decided), events_seen = MAX_EVENTS + 1
  output      walk j = 0 .. n: an accepted INS at j, then — unless an accepted DEL covers j — the decided base.  Nothing outside the
              body changes
  record      gf_fill_polish's 40 bytes with their meaning (len: the OUTPUT length; n_changed: substituted columns, deleted ones
              included; reads_placed includes split rows), then n_events (accepted), n_inserted, n_deleted (bases), reads_split,
              events_seen (distinct in-body events), events_outside."""
import numpy as np
import torch

from . import _lib as B
from . import fill_rounds as FR
from . import pipeline as P
from . import polish as POL
from .fill_rounds import _LUT
from .polish import SEED, MAX_MISMATCH, MIN_OVERLAP, MIN_VOTES

MAX_INDEL = 8
MAX_EVENTS, MAX_INSERTED = B.PLG_MAX_EVENTS, B.PLG_MAX_INSERTED
DEL, INS = 0, 1


def check_params(L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES, max_indel=MAX_INDEL):
    """The five parameters as integers; ValueError for a value out of range (the ABI answers GF_E_UNSUPPORTED)."""
    G = int(max_indel)
    if not 1 <= G <= 16:
        raise ValueError("polish max_indel %r: 1..16" % (max_indel,))
    return POL.check_params(L, seed, max_mismatch, min_overlap, min_votes) + (G,)


def _strand(codes, valid, r, strand):
    return (codes[r], valid[r]) if strand == 0 else ((3 - codes[r][::-1]).astype(np.uint8), valid[r][::-1])


def seeded_diagonals(q, v, index, s):
    """{d: (first, last)} of one sequence: the clean seed windows that equal the contig (index: s-mer bytes -> positions)."""
    out = {}
    for j in range(len(q) // s):
        if v[j * s:j * s + s].all():
            for p in index.get(np.ascontiguousarray(q[j * s:j * s + s]).tobytes(), ()):
                f, l = out.get(p - j * s, (j, j))
                out[p - j * s] = (min(f, j), max(l, j))
    return out


def split_candidate(q, v, cc, s, d1, d2, first1, last2):
    """(mm, ov, x) of the split candidate (d1, d2) of q, or None when no breakpoint is allowed."""
    n, L = len(cc), len(q)
    gi = max(0, d1 - d2)
    x_lo, x_hi = (first1 + 1) * s, last2 * s - gi
    if x_lo > x_hi:
        return None
    i0, i1 = max(0, -d1), min(L, n - d2)
    diff = lambda d, a, b: ((q[a:b] != cc[d + a:d + b]) & v[a:b]).astype(np.int64)
    left = np.concatenate([[0], np.cumsum(diff(d1, i0, x_hi))])                      # left[k]: the differing bases of q[i0, i0 + k) on d1
    right = np.concatenate([np.cumsum(diff(d2, x_lo + gi, i1)[::-1])[::-1], [0]])   # right[k]: of q[x_lo + gi + k, i1) on d2
    best = None
    for x in range(x_lo, x_hi + 1):
        if gi and not v[x:x + gi].all():
            continue
        mm = int(left[x - i0] + right[x - x_lo])
        if best is None or mm < best[0]:
            best = (mm, (x - i0) + (i1 - x - gi), x)
    return best


def placements_gapped(reads, contig, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, max_indel=MAX_INDEL):
    """Per row None (no accepted candidate), "ambiguous", (strand, d, mm, ov) — placed without a gap, polish.placements' tuple — or
    (strand, d1, mm, ov, d2, x) — placed split; mm without the indel's cost.  contig: A, C, G, T only."""
    codes, valid = POL._reads(reads)
    s, mm_max, mo, G = int(seed), int(max_mismatch), int(min_overlap), int(max_indel)
    cc = _LUT[np.frombuffer(contig.encode(), dtype=np.uint8)]
    assert (cc < 4).all()
    n, L = len(cc), codes.shape[1] if len(codes) else 0
    index = {}
    for p in range(n - s + 1):
        index.setdefault(cc[p:p + s].tobytes(), []).append(p)
    out = []
    for r in range(len(codes)):
        accepted = []                                  # (cost, -ov, placement)
        for strand in (0, 1):
            q, v = _strand(codes, valid, r, strand)
            diagonals = seeded_diagonals(q, v, index, s)
            for d in diagonals:
                i0, i1 = max(0, -d), min(L, n - d)
                if i1 - i0 < mo:
                    continue
                mm = int(((q[i0:i1] != cc[d + i0:d + i1]) & v[i0:i1]).sum())
                if mm <= mm_max:
                    accepted.append((mm, -(i1 - i0), (strand, d, mm, i1 - i0)))
            for d1, (first1, _) in diagonals.items():
                for d2, (_, last2) in diagonals.items():
                    if d1 == d2 or abs(d2 - d1) > G:
                        continue
                    c = split_candidate(q, v, cc, s, d1, d2, first1, last2)
                    if c is not None and c[1] >= mo and c[0] + 2 <= mm_max:
                        accepted.append((c[0] + 2, -c[1], (strand, d1, c[0], c[1], d2, c[2])))
        if not accepted:
            out.append(None)
            continue
        key = min(a[:2] for a in accepted)
        best = [a for a in accepted if a[:2] == key]
        out.append(best[0][2] if len(best) == 1 else "ambiguous")
    return out


def parts_of(w, q, n):
    """The aligned parts of a placement of sequence q: [(first read position, end read position, diagonal)]."""
    L = len(q)
    if len(w) == 4:
        return [(max(0, -w[1]), min(L, n - w[1]), w[1])]
    d1, d2, x = w[1], w[4], w[5]
    return [(max(0, -d1), x, d1), (x + max(0, d1 - d2), min(L, n - d2), d2)]


def event_of(w, q):
    """(kind, p, length, inserted bases as a base-4 number) of a split placement."""
    d1, d2, x = w[1], w[4], w[5]
    if d2 > d1:
        return (DEL, d1 + x, d2 - d1, 0)
    num = 0
    for b in q[x:x + d1 - d2]:
        num = num * 4 + int(b)
    return (INS, d1 + x, d1 - d2, num)


def in_body(e, b0, b1):
    return b0 <= e[1] and e[1] + e[2] <= b1 if e[0] == DEL else b0 <= e[1] <= b1


def decide_events(votes, against, min_votes):
    """(accepted events, INS cap met?) of {event: votes} and {event: against}: the passing events in the definition's order, accepted
    greedily."""
    passing = sorted((e for e in votes if votes[e] >= min_votes and votes[e] > against.get(e, 0)), key=lambda e: (-votes[e], e[1], e[0], e[2], e[3]))
    taken, inserted, capped = [], 0, False
    for e in passing:
        lo, hi = e[1], e[1] + (e[2] if e[0] == DEL else 0)
        if any(not (hi < a[1] or a[1] + (a[2] if a[0] == DEL else 0) < lo) for a in taken):
            continue
        if e[0] == INS:
            if inserted + e[2] > MAX_INSERTED:
                capped = True
                continue
            inserted += e[2]
        taken.append(e)
    return taken, capped


def polish_gapped_host(reads, contig, b0, b1, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES,
                       max_indel=MAX_INDEL, detail=False):
    """(polished contig, gf_fill_polish_gapped with off = 0) of one closed gap; arguments as polish.polish_host.  detail: the rows'
    placements and {event: (votes, against)} as well."""
    codes, valid = POL._reads(reads)
    L = codes.shape[1] if len(codes) else None
    s, mm_max, mo, mv, G = check_params(L if L is not None else 1 << 20, seed, max_mismatch, min_overlap, min_votes, max_indel)
    b0, b1 = int(b0), max(int(b0), int(b1))
    rec = np.zeros((), dtype=B.FILL_POLISH_GAPPED)
    rec["len"], rec["n_cols"] = len(contig), b1 - b0
    flag = FR.skip_flag(contig, B.PL_F_LONG, B.PL_F_NON_ACGT)
    if flag:
        rec["flags"] = flag
        return (contig, rec, [], {}) if detail else (contig, rec)
    cc = _LUT[np.frombuffer(contig.encode(), dtype=np.uint8)]
    n = len(cc)
    where = placements_gapped((codes, valid), contig, s, mm_max, mo, G) if len(codes) else []
    votes = np.zeros((n, 4), dtype=np.int64)
    ev_votes, rows, outside = {}, [], 0                # rows: (parts as column ranges, the event the row votes or None) of the placed rows
    for r, w in enumerate(where):
        if w is None or w == "ambiguous":
            continue
        q, v = _strand(codes, valid, r, w[0])
        parts = parts_of(w, q, n)
        for a, b, d in parts:
            for i in range(max(a, b0 - d), min(b, b1 - d)):
                if v[i]:
                    votes[d + i, q[i]] += 1
        e = None
        if len(w) == 6:
            e = event_of(w, q)
            if in_body(e, b0, b1):
                ev_votes[e] = ev_votes.get(e, 0) + 1
            else:
                outside, e = outside + 1, None
        rows.append(([(d + a, d + b) for a, b, d in parts], e))
    out = cc.copy()
    for j in range(b0, b1):
        best = int(np.argmax(votes[j]))
        if votes[j, best] >= mv and votes[j, best] > votes[j, cc[j]]:
            out[j] = best
    against = {}
    for e in ev_votes:
        lo, hi = max(0, e[1] - s), min(n, e[1] + (e[2] if e[0] == DEL else 0) + s)
        against[e] = sum(ev != e and any(a <= lo and hi <= b for a, b in cols) for cols, ev in rows)
    taken, capped = ([], False) if len(ev_votes) > MAX_EVENTS else decide_events(ev_votes, against, mv)
    ins = {e[1]: e for e in taken if e[0] == INS}
    gone = np.zeros(n + 1, dtype=bool)
    for e in taken:
        if e[0] == DEL:
            gone[e[1]:e[1] + e[2]] = True
    text = []
    for j in range(n + 1):
        if j in ins:
            text.append("".join("ACGT"[(ins[j][3] >> (2 * k)) & 3] for k in range(ins[j][2] - 1, -1, -1)))
        if j < n and not gone[j]:
            text.append("ACGT"[out[j]])
    text = "".join(text)
    rec["flags"] = (B.PL_F_EVENTS if len(ev_votes) > MAX_EVENTS else 0) | (B.PL_F_INS_CAP if capped else 0)
    rec["n_changed"] = int((out != cc).sum())
    rec["n_uncovered"] = int((votes[b0:b1].sum(axis=1) == 0).sum())
    rec["reads_placed"] = len(rows)
    rec["reads_ambiguous"] = sum(w == "ambiguous" for w in where)
    rec["n_events"] = len(taken)
    rec["n_inserted"] = sum(e[2] for e in taken if e[0] == INS)
    rec["n_deleted"] = sum(e[2] for e in taken if e[0] == DEL)
    rec["reads_split"] = sum(w is not None and w != "ambiguous" and len(w) == 6 for w in where)
    rec["events_seen"] = min(len(ev_votes), MAX_EVENTS + 1)
    rec["events_outside"] = outside
    rec["len"] = len(text)
    assert len(text) == n + int(rec["n_inserted"]) - int(rec["n_deleted"])
    return (text, rec, where, {e: (ev_votes[e], against[e]) for e in ev_votes}) if detail else (text, rec)


STAT_KEYS = POL.STAT_KEYS + ("events", "inserted", "deleted", "split", "flagged_events", "flagged_ins_cap")


def add_stats(stats, rec, n_out):
    """One gap's record into the twin's statistics."""
    f = int(rec["flags"])
    stats["skipped_long"] += bool(f & B.PL_F_LONG)
    stats["skipped_non_acgt"] += bool(f & B.PL_F_NON_ACGT)
    stats["gaps"] += not f & (B.PL_F_LONG | B.PL_F_NON_ACGT)
    stats["changed"] += int(rec["n_changed"])
    stats["placed"] += int(rec["reads_placed"])
    stats["ambiguous"] += int(rec["reads_ambiguous"])
    stats["bases"] += n_out
    stats["events"] += int(rec["n_events"])
    stats["inserted"] += int(rec["n_inserted"])
    stats["deleted"] += int(rec["n_deleted"])
    stats["split"] += int(rec["reads_split"])
    stats["flagged_events"] += bool(f & B.PL_F_EVENTS)
    stats["flagged_ins_cap"] += bool(f & B.PL_F_INS_CAP)


def polish_gapped_of_results(res, flanks, L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES,
                             max_indel=MAX_INDEL, nmask=None):
    """The twin over a whole step: (records with off = 0, {gap: polished contig}, stats) from fetch(pools=True)'s pools and the fetched
    contigs and picks."""
    check_params(L, seed, max_mismatch, min_overlap, min_votes, max_indel)
    out, texts = np.zeros(len(res.best), dtype=B.FILL_POLISH_GAPPED), {}
    stats = dict.fromkeys(STAT_KEYS, 0)
    for g, contig, body in FR.closed_fills(res, flanks):
        if body is None:
            stats["mismatches"] += 1
            continue
        reads = FR.fill_reads(res, g, L, nmask)
        texts[int(g)], out[g] = polish_gapped_host(reads, contig, body[0], body[1], seed, max_mismatch, min_overlap, min_votes, max_indel)
        add_stats(stats, out[g], len(texts[int(g)]))
    return out, texts, stats


def stats_of(words):
    """The statistics words of gf_fill_polish_gapped_dev (u32[PLG_WORDS]) as polish_gapped_of_results' dictionary."""
    st = np.asarray(words).view(np.uint32)
    return dict(POL.stats_of(st), events=P.counter_u64(st, B.PLG_EVENTS), inserted=P.counter_u64(st, B.PLG_INSERTED),
                deleted=P.counter_u64(st, B.PLG_DELETED), split=P.counter_u64(st, B.PLG_SPLIT), flagged_events=int(st[B.PLG_F_EVENTS]),
                flagged_ins_cap=int(st[B.PLG_F_INS_CAP]))


class FillPolishGapped(POL.FillPolish):
    """The round in the plain polish's place: the same Results fields, the 64-byte record, the wider statistics."""
    RECORD = B.FILL_POLISH_GAPPED

    def __init__(self, pipe, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES, max_indel=MAX_INDEL, read_len=None):
        FR.FillRound.__init__(self, pipe)
        self.params = check_params(read_len, seed, max_mismatch, min_overlap, min_votes, max_indel)

    def prepare(self):
        """The base buffer takes what the contig bases take and MAX_INSERTED bases per gap: exact, given the insertion cap."""
        p = self.p
        self.base_cap = p.seq_cap + MAX_INSERTED * p.n_gaps
        self.d_rec = p._u8(max(1, p.n_gaps) * self.RECORD.itemsize)
        self.d_bases = p._u8(max(1, self.base_cap))
        self.d_stats = torch.zeros(B.PLG_WORDS, dtype=torch.int32, device=p.dev)

    def _launch(self, d_nmask):
        p = self.p
        p._chk(p.lib.gf_fill_polish_gapped_dev(p.h, *self.pool_args(d_nmask), p.L, *self.shared_args(), *self.params,
                                               self.d_rec.data_ptr(), self.d_bases.data_ptr(), self.base_cap, self.d_stats.data_ptr()),
               "gf_fill_polish_gapped_dev")

    STATS_OF = staticmethod(stats_of)
