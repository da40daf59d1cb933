"""Pipeline(polish=True): a consensus polish of the fills the step closed — the reads of a gap's own pool are placed, without gaps in the
alignment, on the gap's winning contig, every column of the fill takes a vote, and the polished contig comes out with one record per gap
(gf_fill_polish, _lib.FILL_POLISH; gf_fill_polish_dev, csrc/fill_polish.hip) at the end of the step.  The reference has nothing like it.
Results.polish (the records), .polish_bases (the polished contigs, rec["off"] / rec["len"]) and .polish_stats; single rank; not with
second_round, whose pool is not the step's.  The step's contigs, bases and pick words do not change.

The definition is the host twin below (polish_host).  For a closed gap with winning contig c of n bases (stored orientation):
  body       [b0, b1) exactly as the read-support round locates it (read_support.locate); a contig that does not carry the word's pick is
             the same MISMATCH: zero record, counted, fetch() raises;
  strands    every pool row gives two sequences q of L bases: the row, and its reverse complement with the N mask reversed to match;
  diagonal   d places q[i] on c[d + i]; the overlap is i in [max(0, -d), min(L, n - d)), ov its size;
  accepted   ov >= min_overlap; mm <= max_mismatch, mm = overlap positions with an unmasked read base different from c[d + i]; and at
             least one seed window [j * s, j * s + s), j < L // s, lies wholly inside the overlap, holds no masked base and equals the
             contig there.  L // s > max_mismatch is required, so that every in-contig placement within the budget has a clean seed;
  placement  the accepted (strand, diagonal) pairs of a row, both strands together, by (mm ascending, ov descending): exactly one pair
             with the best key: the row is PLACED there; more than one: AMBIGUOUS, no vote (a read inside an exact repeat, a palindromic
             read); none: ignored.  Best-of, so that a read of one copy of a near-identical repeat votes only on its own copy;
  votes      a placed row votes q[i] at column d + i for every unmasked i whose column lies in the body;
  decision   for a body column j with cur = c[j] and best = the base with the most votes (the smaller code wins ties): the column becomes
             best when votes[best] >= min_votes and votes[best] > votes[cur].  A tie with cur changes nothing, no column outside the body
             ever changes, and all votes are taken against the unpolished contig: the round runs once;
  skipped    a contig longer than MAX_CONTIG bases (the kernel's limit) or with a byte other than A, C, G, T is copied out unpolished with
             a flag in its record (n_cols set, the other counts zero) and counted — never truncated, never a failure;
  record     off, len (the polished contig in the base buffer, stored orientation), flags, n_cols (body columns), n_changed, n_uncovered
             (body columns with no vote at all), reads_placed, reads_ambiguous (rows, wherever on the contig); all zero for an open gap."""
import numpy as np
import torch

from . import _lib as B
from . import fill_rounds as FR
from . import pipeline as P
from . import read_support as SUP
from .fill_rounds import MAX_CONTIG, _LUT

SEED, MAX_MISMATCH, MIN_OVERLAP, MIN_VOTES = 16, 4, 48, 2


def check_params(L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES):
    """The four parameters as integers; ValueError for a value out of range (module docstring; the ABI answers GF_E_UNSUPPORTED)."""
    mv = int(min_votes)
    return FR.check_placement("polish", L, seed, max_mismatch, min_overlap, [(mv < 1, "min_votes %r: at least 1" % (min_votes,))]) + (mv,)


def _reads(reads):
    return SUP.codes_of(reads) if isinstance(reads, (list, tuple)) and (not reads or isinstance(reads[0], str)) else reads


def placements(reads, contig, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP):
    """Per row None (no accepted pair), "ambiguous" or (strand, d, mm, ov): strand 1 is the reverse complement of the row.  The candidate
    diagonals come from the contig's s-mers — the definition accepts no diagonal without a seed that equals the contig —, everything else
    is the definition word for word.  contig: A, C, G, T only."""
    codes, valid = _reads(reads)
    s, mm_max, mo = int(seed), int(max_mismatch), int(min_overlap)
    cc = _LUT[np.frombuffer(contig.encode(), dtype=np.uint8)]
    assert (cc < 4).all()
    n, L = len(cc), codes.shape[1] if len(codes) else 0
    index = {}
    for p in range(n - s + 1):
        index.setdefault(cc[p:p + s].tobytes(), []).append(p)
    out = []
    for r in range(len(codes)):
        accepted = []
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
                if mm <= mm_max:
                    accepted.append((mm, -(i1 - i0), strand, d))
        if not accepted:
            out.append(None)
            continue
        key = min(a[:2] for a in accepted)
        best = [a for a in accepted if a[:2] == key]
        out.append((best[0][2], best[0][3], best[0][0], -best[0][1]) if len(best) == 1 else "ambiguous")
    return out


def polish_host(reads, contig, b0, b1, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES, detail=False):
    """(polished contig, gf_fill_polish with off = 0) of one closed gap: the pool's reads (texts of one length, a byte other than A, C, G, T
    a masked base; or (codes, valid) arrays), the winning contig as stored, its body [b0, b1).  detail: the rows' placements as well."""
    codes, valid = _reads(reads)
    L = codes.shape[1] if len(codes) else None
    s, mm_max, mo, mv = check_params(L if L is not None else 1 << 20, seed, max_mismatch, min_overlap, min_votes)   # (no read: no length to check against)
    b0, b1 = int(b0), max(int(b0), int(b1))
    rec = np.zeros((), dtype=B.FILL_POLISH)
    rec["len"], rec["n_cols"] = len(contig), b1 - b0
    flag = FR.skip_flag(contig, B.PL_F_LONG, B.PL_F_NON_ACGT)
    if flag:
        rec["flags"] = flag
        return (contig, rec, []) if detail else (contig, rec)
    cc = _LUT[np.frombuffer(contig.encode(), dtype=np.uint8)]
    where = placements((codes, valid), contig, s, mm_max, mo) if len(codes) else []
    votes = np.zeros((len(cc), 4), dtype=np.int64)
    for r, w in enumerate(where):
        if w is None or w == "ambiguous":
            continue
        strand, d = w[0], w[1]
        q, v = (codes[r], valid[r]) if strand == 0 else (3 - codes[r][::-1], valid[r][::-1])
        for i in range(max(0, -d, b0 - d), min(L, len(cc) - d, b1 - d)):
            if v[i]:
                votes[d + i, q[i]] += 1
    out = cc.copy()
    for j in range(b0, b1):
        best = int(np.argmax(votes[j]))          # (the first of equal counts: the smaller code)
        if votes[j, best] >= mv and votes[j, best] > votes[j, cc[j]]:
            out[j] = best
    rec["n_changed"] = int((out != cc).sum())
    rec["n_uncovered"] = int((votes[b0:b1].sum(axis=1) == 0).sum())
    rec["reads_placed"] = sum(w is not None and w != "ambiguous" for w in where)
    rec["reads_ambiguous"] = sum(w == "ambiguous" for w in where)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[out].tobytes().decode()
    return (text, rec, where) if detail else (text, rec)


STAT_KEYS = ("gaps", "mismatches", "skipped_long", "skipped_non_acgt", "changed", "placed", "ambiguous", "bases", "overflow")


def polish_of_results(res, flanks, L, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES, nmask=None):
    """The twin over a whole step: (records with off = 0, {gap: polished contig}, stats) from fetch(pools=True)'s pools and the fetched
    contigs and picks."""
    check_params(L, seed, max_mismatch, min_overlap, min_votes)
    out, texts = np.zeros(len(res.best), dtype=B.FILL_POLISH), {}
    stats = dict.fromkeys(STAT_KEYS, 0)
    for g, contig, body in FR.closed_fills(res, flanks):
        if body is None:
            stats["mismatches"] += 1
            continue
        reads = FR.fill_reads(res, g, L, nmask)
        texts[int(g)], out[g] = polish_host(reads, contig, body[0], body[1], seed, max_mismatch, min_overlap, min_votes)
        f = int(out[g]["flags"])
        stats["skipped_long"] += bool(f & B.PL_F_LONG)
        stats["skipped_non_acgt"] += bool(f & B.PL_F_NON_ACGT)
        stats["gaps"] += not f
        stats["changed"] += int(out[g]["n_changed"])
        stats["placed"] += int(out[g]["reads_placed"])
        stats["ambiguous"] += int(out[g]["reads_ambiguous"])
        stats["bases"] += len(contig)
    return out, texts, stats


def stats_of(words):
    """The statistics words of gf_fill_polish_dev (u32[PL_WORDS]) as polish_of_results' dictionary."""
    st = np.asarray(words).view(np.uint32)
    return {"gaps": int(st[B.PL_GAPS]), "mismatches": int(st[B.PL_MISMATCH]), "skipped_long": int(st[B.PL_SKIPPED_LONG]),
            "skipped_non_acgt": int(st[B.PL_SKIPPED_NON_ACGT]), "changed": P.counter_u64(st, B.PL_CHANGED),
            "placed": P.counter_u64(st, B.PL_PLACED), "ambiguous": P.counter_u64(st, B.PL_AMBIGUOUS), "bases": P.counter_u64(st, B.PL_BASES),
            "overflow": int(st[B.PL_OVERFLOW])}


class FillPolish(FR.FillRound):
    WHAT, RECORD = "polish", B.FILL_POLISH
    STATS_OF = staticmethod(stats_of)            # (polish_gapped.py's round has more words)

    def __init__(self, pipe, seed=SEED, max_mismatch=MAX_MISMATCH, min_overlap=MIN_OVERLAP, min_votes=MIN_VOTES, read_len=None):
        super().__init__(pipe)
        self.params = check_params(read_len, seed, max_mismatch, min_overlap, min_votes)

    def prepare(self):
        """The base buffer takes what the contig bases take: no set of winners is longer."""
        p = self.p
        self.base_cap = p.seq_cap
        self.d_rec = p._u8(max(1, p.n_gaps) * B.FILL_POLISH.itemsize)
        self.d_bases = p._u8(max(1, self.base_cap))
        self.d_stats = torch.zeros(B.PL_WORDS, dtype=torch.int32, device=p.dev)

    def _launch(self, d_nmask):
        """On the pool the step assembled (after the read-support round)."""
        p = self.p
        p._chk(p.lib.gf_fill_polish_dev(p.h, *self.pool_args(d_nmask), p.L, *self.shared_args(), *self.params,
                                        self.d_rec.data_ptr(), self.d_bases.data_ptr(), self.base_cap, self.d_stats.data_ptr()), "gf_fill_polish_dev")

    def fetch(self, r):
        r.polish_stats = self.STATS_OF(self.d_stats.cpu().numpy())
        self.check_mismatches(r.polish_stats["mismatches"])
        if r.polish_stats["overflow"] or r.polish_stats["bases"] > self.base_cap:
            raise RuntimeError("polish: %d polished bases (cap %d)" % (r.polish_stats["bases"], self.base_cap))
        r.polish = self.records()[0]
        r.polish_bases = self.d_bases[:r.polish_stats["bases"]].cpu().numpy().tobytes()


def polished_text(res, g):
    """The polished contig of gap g (stored orientation) of a Results, or None for an open gap."""
    rec = res.polish[g]
    return res.polish_bases[int(rec["off"]):int(rec["off"]) + int(rec["len"])].decode() if res.best[g] else None
