"""Pipeline(extended_fill=True): the reference's last stage (pick_extended_contigs, assemble_gaps.py:367-368) after the last pick of the
step.  Every gap still open is filled from each side as far as a contig reaches, the parts joined by "NN" (gf_pick_extended_dev; the
shorter anchor, anchors[-1], in anchor_mode; over the round-2 contigs with second_round, else over all of the step's contigs).
Results.ext (gf_ext_pick per gap), .ext_bases and .extended (counts); Pipeline.extended_sequences decodes them.  Single rank.
ext_base_cap: bytes of the fill buffer (default: the contig bases' capacity + 2 per gap, which no fill set can exceed); fetch() raises
when the fills do not fit."""
import numpy as np
import torch

from . import _lib as B
from . import pipeline as P


class ExtendedFill:
    def __init__(self, pipe, base_cap=None):
        self.p, self.base_cap = pipe, base_cap
        self.d_ext = None

    def prepare(self):
        """Called once, after the rounds have settled the capacities of the step's contig list."""
        p = self.p
        if self.base_cap is None:
            self.base_cap = p.seq_cap + 2 * p.n_gaps
        self.d_ext = p._u8(p.n_gaps * B.EXT_PICK.itemsize)
        self.d_bases = p._u8(self.base_cap)
        self.d_stats = torch.zeros(B.EXT_WORDS, dtype=torch.int32, device=p.dev)

    def enqueue(self):
        """After the last pick of the step: the partial fills of the gaps d_best leaves open."""
        p = self.p
        if self.d_ext is None:        # a sizing run of one of the rounds: nobody reads its fills
            return
        first = p.round2.first_ptr() if p.round2 is not None else None
        what = P.PICKS[p.anchor_mode][2]
        p._chk(getattr(p.lib, what)(p.h, p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), p.anchors[-1], p.k_arr, p.kv_arr, len(p.kk), first,
                  p.d_best.data_ptr(), self.d_ext.data_ptr(), self.d_bases.data_ptr(), self.base_cap, self.d_stats.data_ptr()), what)

    def fetch(self, r):
        p = self.p
        st = self.d_stats.cpu().numpy().view(np.uint32)
        total = P.counter_u64(st, B.EXT_BASES)
        if int(st[B.EXT_OVERFLOW]) or total > self.base_cap:
            raise RuntimeError("extended fill overflow: %d fill bases, buffer of %d (Pipeline(ext_base_cap=...))" % (total, self.base_cap))
        r.extended = {"gaps_extended": int(st[B.EXT_EXTENDED]), "left_only": int(st[B.EXT_LEFT_ONLY]), "right_only": int(st[B.EXT_RIGHT_ONLY]),
                      "both_sides": int(st[B.EXT_BOTH]), "bases": total}
        if p.per_contig:
            r.extended["align_dropped"], r.extended["align_seed_overflow"] = int(st[B.EXT_ALIGN_DROPPED]), int(st[B.EXT_ALIGN_SEED_OVERFLOW])
        r.ext = np.frombuffer(self.d_ext[:p.n_gaps * B.EXT_PICK.itemsize].cpu().numpy().tobytes(), dtype=B.EXT_PICK)
        r.ext_bases = self.d_bases[:total].cpu().numpy().tobytes()
