"""Pipeline(rescue_round=True): the reference's rescue round (assemble_gaps.py:357-366) after the merge round's pick.
Per gap still open, its high-quality reads (the tagger hits of MAPQ-60 records) that align clipped to two or more of its merged contigs
are bridges; they are appended as records with k = kv = RESCUE_MARK, the gap's own contigs and its bridges are merged again (merged
contigs appended with k = kv = 0), and the records the round appended are picked at anchors[-1] (Results.rescue / rescue_first).
Needs merge_in_step; single rank, without second_round.  Like the second round's candidates, the read ids assume that the libraries'
read names are distinct."""
import ctypes as C

import numpy as np
import torch

from . import _lib as B
from . import pipeline as P


class RescueRound:
    def __init__(self, pipe):
        self.p = pipe

    def _alloc(self):
        p = self.p
        sizes = (p.n_gaps, self.hq_cap, self.seed_cap, self.log2)
        work_bytes = int(p.lib.gf_rescue_work_bytes(*sizes))
        if not work_bytes:
            raise ValueError("rescue_round: unsupported sizes (%d gaps)" % p.n_gaps)
        self.d_work = p._u8(work_bytes)
        self.gap_bridges = p.lib.gf_rescue_gap_bridges(self.d_work.data_ptr(), *sizes)

    def _work(self):
        return self.d_work.data_ptr(), self.hq_cap, self.seed_cap, self.log2

    # ---- sizing (untimed) ------------------------------------------------------------------------------------------------------
    def prepare(self):
        """The step with the round run again and again, every buffer grown to the exact count the run before reported, until nothing
        is beyond a capacity (the HQ keys, the window table, the seeds, the step's contig list that the round appends to twice)."""
        p = self.p
        if len(p.libs) > B.R2_MAX_LIBS:
            raise ValueError("rescue_round: at most %d libraries" % B.R2_MAX_LIBS)
        if not p.kk or not p.assemble_in_step or p.n_gaps < 1:
            raise ValueError("rescue_round runs inside the step's assembly (k_pairs, assemble_in_step and gaps)")
        if not 30 <= p.L <= 1000:
            raise ValueError("rescue_round: read length %d outside 30..1000" % p.L)
        self.reads = (C.c_void_p * len(p.libs))(*[lb.d_reads.data_ptr() for lb in p.libs])
        self.nmask = (C.c_void_p * len(p.libs))(*[lb.d_nmask.data_ptr() if lb.d_nmask is not None else None for lb in p.libs])
        self.d_st = torch.zeros(B.RS_WORDS, dtype=torch.int32, device=p.dev)
        self.d_sets = torch.zeros(B.MG_WORDS, dtype=torch.int32, device=p.dev)      # the alignment sets' dedup
        self.d_mstats = torch.zeros(B.MG_WORDS, dtype=torch.int32, device=p.dev)    # the rescue's merge
        self.hq_cap, self.seed_cap, self.log2 = 4096, 4096, 12
        self._alloc()
        p._size_round("rescue round", self._grow)

    def _grow(self):
        p = self.p
        st = self.d_st.cpu().numpy().view(np.uint32)
        ms = self.d_mstats.cpu().numpy().view(np.uint32)
        a1 = p.d_acnt.cpu().numpy()
        n, q = int(a1[0]), P.counter_u64(a1)
        grown = False
        if int(st[B.RS_HQ_KEYS]) > self.hq_cap:
            self.hq_cap, grown = int(1.25 * int(st[B.RS_HQ_KEYS])) + 4096, True
        need_log2 = max(12, int(2 * int(st[B.RS_WINDOWS]) + 16).bit_length())
        if need_log2 > self.log2 or int(st[B.RS_TAB_FULL]):
            self.log2, grown = max(need_log2, self.log2 + 1), True
        if int(st[B.RS_SEEDS]) > self.seed_cap:
            self.seed_cap, grown = int(1.25 * int(st[B.RS_SEEDS])) + 4096, True
        if n > p.contig_cap or q > p.seq_cap or int(st[B.RS_APPEND_ERR]) or (int(ms[B.MG_ERR]) & 96):
            # (the merges' own outputs count beyond the list too: MG_E_CONTIGS / MG_E_OUTSEQ)
            p._alloc_contig_list(int(1.5 * max(n, p.contig_cap)) + 4096, int(1.5 * max(q, p.seq_cap)) + (1 << 20))
            grown = True
        if grown:
            self._alloc()
        return grown

    # ---- in the step -----------------------------------------------------------------------------------------------------------
    def enqueue_keys(self):
        """After the pools: every library's HQ keys from its tagger hits (the tried gaps are chosen later, on the device)."""
        p = self.p
        p._chk(p.lib.gf_rescue_reset_dev(p.h, self.d_work.data_ptr(), p.n_gaps, self.hq_cap, self.seed_cap, self.log2, self.d_st.data_ptr()),
               "gf_rescue_reset_dev")
        for l, lb in enumerate(p.libs):
            p._chk(p.lib.gf_rescue_hq_keys_dev(p.h, lb.d_thits.data_ptr(), lb.cp + 4 * P.CNT_TAG, lb.hit_cap, lb.d_recs.data_ptr(), lb.n_reads, l,
                                               p.n_gaps, *self._work(), self.d_st.data_ptr()), "gf_rescue_hq_keys_dev")

    def enqueue(self):
        """After the merge round's pick: bridges appended, the rescue sets merged, the appended records picked at anchors[-1]."""
        p = self.p
        lib, h = p.lib, p.h
        ctg, seq, best = p.d_ctg.data_ptr(), p.d_seq.data_ptr(), p.d_best.data_ptr()
        p._chk(lib.gf_rescue_bridges_dev(h, ctg, p.ap, p.contig_cap, seq, p.ap + 8, p.seq_cap, best, p.n_gaps, self.reads, self.nmask, len(p.libs),
                                         p.L, *self._work(), self.d_sets.data_ptr(), self.d_st.data_ptr()), "gf_rescue_bridges_dev")
        first = self.d_st.data_ptr() + 4 * B.RS_FIRST
        p._chk(lib.gf_merge_rescue_dev(h, ctg, p.ap, p.contig_cap, seq, p.ap + 8, p.seq_cap, best, p.n_gaps, B._p(p.merge_params), 10,
                                       p.merge_max_set, p.k_arr, p.kv_arr, min(16, len(p.kk)), p.d_mstats.data_ptr(), first, self.gap_bridges,
                                       self.d_mstats.data_ptr()), "gf_merge_rescue_dev")
        p._pick(p.anchors[-1], 0, first=first)

    # ---- results ---------------------------------------------------------------------------------------------------------------
    def fetch(self, r):
        p = self.p
        st = self.d_st.cpu().numpy().view(np.uint32)
        ms = self.d_mstats.cpu().numpy().view(np.uint32)
        ss = self.d_sets.cpu().numpy().view(np.uint32)
        if int(st[B.RS_APPEND_ERR]) or int(ms[B.MG_ERR]):
            raise RuntimeError("rescue round overflow: append flag %d, merge capacity flags %#x, %d contigs (cap %d), %d contig bases (cap %d)"
                               % (int(st[B.RS_APPEND_ERR]), int(ms[B.MG_ERR]), r.n_contigs, p.contig_cap, r.n_seq, p.seq_cap))
        first = int(st[B.RS_FIRST])
        # HQ reads the round could not take: keys beyond their buffer, windows without room, seeds beyond their buffer, reads with more
        # placements than the bridge kernel holds, contigs too long to seed, gaps with more records than the dedup takes
        dropped = (max(0, int(st[B.RS_HQ_KEYS]) - self.hq_cap) + int(st[B.RS_TAB_FULL]) + max(0, int(st[B.RS_SEEDS]) - self.seed_cap)
                   + int(st[B.RS_PLACE_OVF]) + int(st[B.RS_LONG]) + int(ss[B.MG_SKIPPED]))
        r.rescue_first = first
        r.rescue = {"gaps_tried": int(st[B.RS_TRIED]), "hq_reads": int(st[B.RS_HQ]), "gaps_with_bridges": int(st[B.RS_GAPS_BRIDGED]),
                    "bridges": int(st[B.RS_BRIDGES]), "merged_contigs": int(ms[B.MG_N_JOBS]),
                    "closed": int(((r.best != 0) & (P.pick_index(r.best) >= first)).sum()), "dropped": int(dropped)}
