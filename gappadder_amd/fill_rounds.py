"""What the rounds that look at the closed fills after the last pick of the step share on the host (read_support.py, polish.py,
polish_gapped.py, pileup.py, pair_span.py, pair_anchors.py, fill_adjudication.py; the device side: csrc/fill_round.hpp, fill_body.hpp, fill_place.hpp, fill_place_split.hpp): the twins' walk over a step's
Results (closed_fills, pool_reads), the placing rounds' skip classification and parameter check (skip_flag, check_placement), and the
base of the round objects the Pipeline holds (FillRound).  A rule about closed fills exists once here and once on the device."""
import numpy as np

from . import _lib as B

MAX_CONTIG = B.PL_MAX_CONTIG
_LUT = np.full(256, 4, dtype=np.uint8)          # A, C, G, T -> 0..3; any other byte -> 4
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _i

# why a round that reads the step's pools does not run with second_round (Pipeline's refusals) unless the step rebuilds the closing pools
NOT_WITH_SECOND_ROUND = {"read_support": "the support is defined on the step's pool", "polish": "the polish is defined on the step's pool",
                         "pileup": "the pile-up is defined on the step's pool",
                         "pair_span": "the pairs are looked up in the step's pools",
                         "pair_anchors": "the anchored pairs are looked up in the step's pools",
                         "adjudicate": "the adjudication is defined on the step's pool"}


def refusals(name, on, single_rank, second_round):
    """Pipeline's two (refused?, message) pairs of the after-pick round `name`."""
    return ((on and not single_rank, "%s runs on a single rank" % name),
            (on and second_round, "%s with second_round: the second round assembles a pool of its own, not the step's, and %s"
             % (name, NOT_WITH_SECOND_ROUND[name])))


def closed_fills(res, flanks):
    """(g, contig, body) for every closed gap of a Results, in gap order: the winning contig as stored and the body (b0, b1) of the
    fill on it (read_support.locate) — or ("", None) / (contig, None): the word names no contig of the list, a contig of another gap,
    or a pick the contig does not carry.  An open gap is not yielded."""
    from . import pipeline as P                  # (here, not above: pipeline imports the rounds, which import this module)
    from .read_support import locate
    for g in np.nonzero(res.best)[0]:
        ci = P.decode_best(res.best[g])[2]
        ok = ci < len(res.contigs) and int(res.contigs[ci]["gap"]) == g
        contig = P.contig_text(res, ci) if ok else ""
        yield g, contig, locate(res.best[g], contig, flanks[g], res.ctg_pick[ci] if res.ctg_pick is not None else None) if ok else None


def pool_reads(off, rows, g, L, nmask=None):
    """(r0, r1, (codes, valid)) of gap g's rows of a pool (offsets, packed rows, N-mask rows or None)."""
    from .read_support import codes_of_rows
    r0, r1 = int(off[g]), int(off[g + 1])
    return r0, r1, codes_of_rows(rows[r0:r1], L, None if nmask is None else nmask[r0:r1])


def fill_pool(res, nmask=None):
    """(offsets, rows, N-mask rows or None) of the pool the after-pick rounds of a step read: the closing pool when the Results carry one
    (Pipeline(closing_pools=True), with its own masks), else the step's pool with the caller's masks."""
    if getattr(res, "closing_pool_off", None) is not None:
        return res.closing_pool_off, res.closing_pool_rows, res.closing_pool_nmask
    return res.pool_off, res.pool_rows, nmask


def fill_lib_pool(res, l, nmask=None):
    """fill_pool for library l's own pool: (offsets, rows, read ids, N-mask rows or None)."""
    if getattr(res, "closing_lib_pool_off", None) is not None:
        return res.closing_lib_pool_off[l], res.closing_lib_pool_rows[l], res.closing_lib_pool_ids[l], \
            None if res.closing_lib_pool_nmask is None else res.closing_lib_pool_nmask[l]
    return res.lib_pool_off[l], res.lib_pool_rows[l], res.lib_pool_ids[l], nmask


def fill_reads(res, g, L, nmask=None):
    """(codes, valid) of gap g's rows of fill_pool(res, nmask)."""
    off, rows, nm = fill_pool(res, nmask)
    return pool_reads(off, rows, g, L, nm)[2]


def skip_flag(contig, f_long, f_non_acgt):
    """0, or the flag a placing round gives a contig it does not place: longer than MAX_CONTIG bases, a byte other than A, C, G, T."""
    return f_long if len(contig) > MAX_CONTIG else f_non_acgt if (_LUT[np.frombuffer(contig.encode(), dtype=np.uint8)] > 3).any() else 0


def check_placement(what, L, seed, max_mismatch, min_overlap, own=()):
    """(seed, max_mismatch, min_overlap) as integers; ValueError "<what> ..." for a value out of range (the ABI answers
    GF_E_UNSUPPORTED).  own: the round's own (out of range?, message) pairs, checked before the seeds are counted."""
    L, s, mm, mo = int(L), int(seed), int(max_mismatch), int(min_overlap)
    if not 12 <= s <= 32:
        raise ValueError("%s seed %r: 12..32" % (what, seed))
    if not 0 <= mm <= 15:
        raise ValueError("%s max_mismatch %r: 0..15" % (what, max_mismatch))
    if not s <= mo <= L:
        raise ValueError("%s min_overlap %r: at least the seed (%d), at most the read length (%d)" % (what, min_overlap, s, L))
    for bad, why in own:
        if bad:
            raise ValueError("%s %s" % (what, why))
    if L // s <= mm:
        raise ValueError("%s seed %d with max_mismatch %d: a read of %d bases has %d seeds, and more seeds than mismatches are needed"
                         % (what, s, mm, L, L // s))
    return s, mm, mo


class FillRound:
    """A round after the last pick of the step.  A subclass names itself (WHAT, in messages), its record (RECORD), allocates d_rec and
    d_stats in prepare(), launches in _launch(d_nmask) and fills its Results fields in fetch(r)."""
    WHAT = RECORD = None

    def __init__(self, pipe):
        self.p = pipe
        self.d_rec = None

    def shared_args(self):
        """The ABI arguments every gf_fill_*_dev takes after read_len: the contig list, its counter and capacity, the bases, the pick
        words, the selection per contig (align / gapped) or None, the two exact anchor lengths (0, 0 with a selection)."""
        p = self.p
        return (p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), p.d_best.data_ptr(),
                p.d_ctg_pick.data_ptr() if p.per_contig else None) + (p.anchor_pair if not p.per_contig else (0, 0))

    def pool_args(self, d_nmask):
        """(pool, N masks or None, offsets, capacity in rows): the four ABI arguments of the pool a round reads — the closing pool where
        the step builds one (second_round.ClosingPools), else the pool the step assembled with the masks assemble() was given."""
        p = self.p
        return p.closing.pool_args() if p.closing is not None else (p.asm_ptr, d_nmask, p.asm_off, p.asm_rows)

    def pool_cap(self):
        """Rows of the array pool_args() names: what a round sizes its scratch per row by."""
        p = self.p
        return p.closing.cap if p.closing is not None else p.merged_cap if p.need_merge else p.lib_cap

    def enqueue(self, d_nmask=None):
        """After the last pick of the step, in the order support, polish, pile-up, pairs.  d_nmask: the N masks assemble() was given."""
        if self.d_rec is None:        # a sizing run of one of the rounds: nobody reads its records
            return
        self._launch(d_nmask)

    def check_mismatches(self, n, more=""):
        if n:
            raise RuntimeError("%s: %d closed gaps whose winning contig does not carry the pick the word states%s" % (self.WHAT, n, more))

    def records(self, planes=1):
        """The record buffer — `planes` planes of max(1, n_gaps) records — as [planes, n_gaps] of RECORD."""
        n = self.p.n_gaps * self.RECORD.itemsize
        raw = np.ascontiguousarray(self.d_rec.cpu().numpy().reshape(planes, -1)[:, :n])
        return np.frombuffer(raw.tobytes(), dtype=self.RECORD).reshape(planes, self.p.n_gaps)
