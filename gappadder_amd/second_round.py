"""Pipeline(second_round=True): the reference's second assembly round (assemble_gaps.py:344-351) inside the step for the gaps the first
pick leaves open.  The pairs with both mates unmapped (FLAG & 12 == 12) that share a canonical k-mer (the smallest k of k_pairs in
16..64) with a gap's round-1 contigs are appended to its pool, the gap is assembled again at every (k, kv) and picked over the round-2
contigs only (appended after round 1's; Results.round2 / round2_first / round2_reads).  Single rank, without merge_in_step.
The candidate pairs are listed from the libraries' alignment records once, in prepare(): like the key column, they assume the records
do not change after prepare() (a caller that rewrites d_recs prepares a new Pipeline)."""
import ctypes as C

import numpy as np
import torch

from . import _lib as B
from . import pipeline as P


class SecondRound:
    def __init__(self, pipe, k):
        self.p, self.k = pipe, int(k)

    def _alloc(self):
        p = self.p
        self.d_tab = p._u8(24 << self.log2)
        self.d_keys = torch.empty(self.key_cap, dtype=torch.int64, device=p.dev)
        self.d_sorted = torch.empty(self.key_cap, dtype=torch.int64, device=p.dev)
        self.d_work = torch.empty(int(p.lib.gf_round2_work_words(self.key_cap, p.n_gaps)), dtype=torch.int32, device=p.dev)
        self.d_pool = p._u8(self.pool_cap * p.rb + 64)
        self.d_ctg = p._u8(self.ctg_cap * 32)
        self.d_seq = p._u8(self.seq_cap)

    # ---- sizing (untimed) ------------------------------------------------------------------------------------------------------
    def prepare(self):
        """Candidates of every library (they depend on the records alone: listed once), then the step with the round run again and
        again, every buffer grown to the exact count the run before reported, until nothing is beyond a capacity."""
        p = self.p
        dev, n_gaps = p.dev, p.n_gaps
        if len(p.libs) > B.R2_MAX_LIBS:
            raise ValueError("second_round: at most %d libraries" % B.R2_MAX_LIBS)
        if not p.kk or not p.assemble_in_step:
            raise ValueError("second_round runs inside the step's assembly (k_pairs and assemble_in_step)")
        self.cand = []          # per library: (candidate pair ids, their count on the device, capacity)
        for lb in p.libs:
            d_bits = p._u8(((lb.n_reads // 2 + 31) // 32) * 4)
            d_n = torch.zeros(4, dtype=torch.int32, device=dev)
            cap, d_pairs = 0, torch.empty(1, dtype=torch.int32, device=dev)
            for _ in range(2):
                torch.cuda.synchronize()
                p._chk(p.lib.gf_both_unmapped_reads_dev(p.h, lb.d_recs.data_ptr(), lb.n_recs, lb.n_reads, d_bits.data_ptr(), d_pairs.data_ptr(),
                                                        cap, d_n.data_ptr()), "gf_both_unmapped_reads_dev")
                p.gf.sync()
                n = int(d_n[0])
                if n <= cap:
                    break
                cap, d_pairs = n, torch.empty(n + 1, dtype=torch.int32, device=dev)
            self.cand.append((d_pairs, d_n, cap))
        self.lib_ptrs = (C.c_void_p * len(p.libs))(*[lb.d_reads.data_ptr() for lb in p.libs])
        self.d_st = torch.zeros(B.R2_WORDS, dtype=torch.int32, device=dev)
        self.d_acnt = torch.zeros(8, dtype=torch.int32, device=dev)
        self.d_gap_err = torch.zeros(max(1, n_gaps), dtype=torch.int32, device=dev)
        # round-2 rows per gap, then their offsets (the pool_off of the round-2 assembly)
        self.d_rows_all = torch.zeros(2 * (n_gaps + 1), dtype=torch.int64, device=dev)
        self.d_rows, self.d_off = self.d_rows_all[:n_gaps + 1], self.d_rows_all[n_gaps + 1:]
        self.log2, self.key_cap, self.pool_cap = 12, 4096, 4096
        self.ctg_cap, self.seq_cap = p.contig_caps(0)
        self._alloc()
        self.deepest = int(p.max_pool_rows)
        p._size_round("second round", self._grow)

    def _grow(self):
        p = self.p
        st = self.d_st.cpu().numpy().view(np.uint32)
        a1, a2 = p.d_acnt.cpu().numpy(), self.d_acnt.cpu().numpy()
        n2, s2 = int(a2[0]), P.counter_u64(a2)
        rows = P.counter_u64(st, B.R2_ROWS)
        grown = False
        need_log2 = max(12, int(2 * int(st[B.R2_KMERS]) + 16).bit_length())
        if need_log2 > self.log2 or int(st[B.R2_TAB_FULL]):
            self.log2, grown = max(need_log2, self.log2 + 1), True
        if int(st[B.R2_HITS]) > self.key_cap:
            self.key_cap, grown = int(1.25 * int(st[B.R2_HITS])) + 4096, True
        if rows > self.pool_cap:
            self.pool_cap, grown = int(1.25 * rows) + 4096, True
        if n2 > self.ctg_cap or s2 > self.seq_cap:
            c2, q2 = p.contig_caps(rows)
            self.ctg_cap, self.seq_cap, grown = max(c2, int(1.25 * n2)), max(q2, int(1.25 * s2)), True
        # the step's list holds both rounds' contigs
        n1, q1 = int(st[B.R2_FIRST]), P.counter_u64(a1) - (0 if int(st[B.R2_APPEND_ERR]) else s2)
        if n1 + n2 > p.contig_cap or q1 + s2 > p.seq_cap:
            p._alloc_contig_list(max(p.contig_cap, int(1.25 * (n1 + n2)) + 4096), max(p.seq_cap, int(1.25 * (q1 + s2)) + (1 << 20)))
            grown = True
        # the assembly's workspace bounds cover the round-2 pools too (a pool beyond asm_big_pool_reads would set its gap error)
        sizes = self.d_rows[:p.n_gaps].cpu().numpy()
        deep = int(sizes.max()) if len(sizes) else 0
        if deep > self.deepest:
            self.deepest = deep
            bound = deep if deep <= 4096 else max(4096, p.asm_bound, int(np.percentile(sizes[sizes > 0], 99)))
            p.gf.set_option("asm_max_pool_reads", max(1, bound))
            p.gf.set_option("asm_big_pool_reads", max(1, min(0x1FFFFF, deep)))
            grown = True
        if grown:
            self._alloc()
        return grown

    # ---- in the step -----------------------------------------------------------------------------------------------------------
    def first_ptr(self):
        """Device address of the index of the first round-2 contig in the step's list."""
        return self.d_st.data_ptr() + 4 * B.R2_FIRST

    def enqueue(self):
        """Right after the first pick: recruitment, round-2 pools, assembly, append, pick over the round-2 contigs."""
        p = self.p
        lib, h, n_gaps, k = p.lib, p.h, p.n_gaps, self.k
        st = self.d_st.data_ptr()
        p._chk(lib.gf_memset_dev(h, st, 0, 4 * B.R2_WORDS) or lib.gf_memset_dev(h, self.d_keys.data_ptr(), 0xFF, 8 * self.key_cap), "gf_memset_dev")
        p._chk(lib.gf_contig_kmer_table_dev(h, p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), p.d_best.data_ptr(), n_gaps, k,
                                            self.d_tab.data_ptr(), self.log2, st), "gf_contig_kmer_table_dev")
        for l, (lb, (d_pairs, d_n, cap)) in enumerate(zip(p.libs, self.cand)):
            p._chk(lib.gf_recruit_by_contigs_dev(h, lb.d_reads.data_ptr(), lb.d_nmask.data_ptr() if lb.d_nmask is not None else None, lb.n_reads, p.L,
                                                 d_pairs.data_ptr(), d_n.data_ptr(), cap, l, k, self.d_tab.data_ptr(), self.log2,
                                                 self.d_keys.data_ptr(), self.key_cap, st), "gf_recruit_by_contigs_dev")
        p._chk(lib.gf_round2_pools_dev(h, self.d_keys.data_ptr(), self.d_sorted.data_ptr(), self.key_cap, self.lib_ptrs, len(p.libs), p.L, p.asm_ptr,
                                       p.asm_off, p.d_best.data_ptr(), n_gaps, self.d_work.data_ptr(), self.d_rows_all.data_ptr(),
                                       self.d_pool.data_ptr(), self.pool_cap, st), "gf_round2_pools_dev")
        ap2 = self.d_acnt.data_ptr()
        p._chk(lib.gf_assemble_multi_dev(h, self.d_pool.data_ptr(), None, self.d_off.data_ptr(), n_gaps, self.pool_cap, p.L, p.k_arr, p.kv_arr,
                                         len(p.kk), p.min_count, p.min_contig, self.d_ctg.data_ptr(), self.ctg_cap, ap2, self.d_seq.data_ptr(),
                                         self.seq_cap, ap2 + 8, self.d_gap_err.data_ptr()), "gf_assemble_multi_dev (round 2)")
        p._chk(lib.gf_contigs_append_dev(h, p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), p.ap + 8, p.seq_cap, self.d_ctg.data_ptr(), ap2,
                                         self.ctg_cap, self.d_seq.data_ptr(), ap2 + 8, self.seq_cap, st), "gf_contigs_append_dev")
        p._pick(*p.anchor_pair, first=self.first_ptr())

    # ---- results ---------------------------------------------------------------------------------------------------------------
    def fetch(self, r):
        st = self.d_st.cpu().numpy().view(np.uint32)
        a2 = self.d_acnt.cpu().numpy()
        n2, s2 = int(a2[0]), P.counter_u64(a2)
        n_err = int(self.d_gap_err.sum())
        if n_err or int(st[B.R2_APPEND_ERR]) or n2 > self.ctg_cap or s2 > self.seq_cap:
            raise RuntimeError("second round overflow: %d gap errors, append flag %d, %d contigs (cap %d), %d contig bases (cap %d)"
                               % (n_err, int(st[B.R2_APPEND_ERR]), n2, self.ctg_cap, s2, self.seq_cap))
        first = int(st[B.R2_FIRST])
        n_keys = min(int(st[B.R2_HITS]), self.key_cap)
        cand = [int(d_n[0]) for _, d_n, _ in self.cand]
        # recruits the round could not take: table entries without room, keys beyond their buffer, candidates beyond theirs, pools beyond theirs
        dropped = (int(st[B.R2_TAB_FULL]) + max(0, int(st[B.R2_HITS]) - self.key_cap) + sum(max(0, c - cap) for c, (_, _, cap) in zip(cand, self.cand))
                   + (2 * int(st[B.R2_UNIQUE]) if int(st[B.R2_POOL_OVF]) else 0))
        r.round2_first = first
        r.round2 = {"gaps_tried": int(st[B.R2_TRIED]), "gaps_with_recruits": int(st[B.R2_WITH]), "reads_recruited": 2 * int(st[B.R2_UNIQUE]),
                    "contigs": int(st[B.R2_N2]), "gaps_closed": int(((r.best != 0) & (P.pick_index(r.best) >= first)).sum()), "dropped": int(dropped),
                    "candidates": 2 * sum(cand)}
        if self.p.keep_read_ids:      # per gap with recruits: [(library, read id)] in round-2 pool order
            keys = np.unique(self.d_sorted[:n_keys].cpu().numpy().view(np.uint64))
            keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
            gap, libi, pair = (keys >> np.uint64(40)).astype(np.int64), ((keys >> np.uint64(36)) & np.uint64(15)).astype(np.int64), \
                (keys & np.uint64((1 << 36) - 1)).astype(np.int64)
            out = {}
            for g, l, q in zip(gap.tolist(), libi.tolist(), pair.tolist()):
                out.setdefault(g, []).extend([(l, 2 * q), (l, 2 * q + 1)])
            r.round2_reads = out
