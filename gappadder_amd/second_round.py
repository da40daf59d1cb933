"""Pipeline(second_round=True): the reference's second assembly round (assemble_gaps.py:344-351) inside the step for the gaps the first
pick leaves open.  The pairs with both mates unmapped (FLAG & 12 == 12) that share a canonical k-mer (the smallest k of k_pairs in
16..64) with a gap's round-1 contigs are appended to its pool, the gap is assembled again at every (k, kv) and picked over the round-2
contigs only (appended after round 1's; Results.round2 / round2_first / round2_reads).  Single rank, without merge_in_step.
The candidate pairs are listed from the libraries' alignment records once, in prepare(): like the key column, they assume the records
do not change after prepare() (a caller that rewrites d_recs prepares a new Pipeline).
recruit_rounds=R (1..16) repeats the round: round r >= 2 builds its table from the contigs round r - 1 appended, carries the keys recruited
so far, recruits behind them, gives a pool (round-1 rows, then every pair recruited so far) to the open gaps whose recruits grew, assembles
them, appends and picks over its own contigs; a round after one that grew no gap is gated on the device and does nothing
(Results.recruit_rounds / recruit_rounds_run / recruit_reads).  rounds_host() is the same in plain Python."""
import ctypes as C

import numpy as np
import torch

from . import _lib as B
from . import pipeline as P


class SecondRound:
    def __init__(self, pipe, k, rounds=1):
        self.p, self.k, self.R = pipe, int(k), int(rounds)

    def _alloc(self):
        p = self.p
        self.d_tab = p._u8(24 << self.log2)
        self.d_keys = torch.empty(self.key_cap, dtype=torch.int64, device=p.dev)
        self.d_sorted = torch.empty(self.key_cap, dtype=torch.int64, device=p.dev)
        self.d_work = torch.empty(int(p.lib.gf_round2_work_words(self.key_cap, p.n_gaps)), dtype=torch.int32, device=p.dev)
        self.d_pool = p._u8(self.pool_cap * p.rb + 64)
        self.d_ctg = p._u8(self.ctg_cap * 32)
        self.d_seq = p._u8(self.seq_cap)
        if self.R > 1 and p.keep_read_ids:      # round j's distinct keys, j < R: written by round j + 1's carry
            self.d_snap = torch.empty((self.R - 1) * self.key_cap, dtype=torch.int64, device=p.dev)

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
        # one block per recruitment round of each of: statistics, assembly counters, gap errors, pool rows + offsets
        R = self.R
        self.d_st = torch.zeros(R * B.R2_WORDS, dtype=torch.int32, device=dev)
        self.d_acnt = torch.zeros(R * 8, dtype=torch.int32, device=dev)
        self.d_gap_err = torch.zeros(R * max(1, n_gaps), dtype=torch.int32, device=dev)
        # round-2 rows per gap, then their offsets (the pool_off of the round-2 assembly)
        self.d_rows_all = torch.zeros(R * 2 * (n_gaps + 1), dtype=torch.int64, device=dev)
        self.d_rows, self.d_off = self.d_rows_all[:n_gaps + 1], self.d_rows_all[n_gaps + 1:2 * (n_gaps + 1)]
        if R > 1:       # the carry's per-gap counts; the candidate counts in one array, and the copy a gated round zeroes
            self.d_prev = torch.zeros(max(1, n_gaps), dtype=torch.int32, device=dev)
            self.d_np = torch.cat([d_n[:1] for _, d_n, _ in self.cand]).contiguous()
            self.d_np_live = torch.zeros(len(p.libs), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
        self.log2, self.key_cap, self.pool_cap = 12, 4096, 4096
        self.ctg_cap, self.seq_cap = p.contig_caps(0)
        self._alloc()
        self.deepest = int(p.max_pool_rows)
        p._size_round("second round", self._grow, tries=8 + 4 * (self.R - 1))    # (a later round shows its counts once the earlier ones fit)

    def _grow(self):
        """Every capacity from the maximum over the rounds' blocks."""
        p, R = self.p, self.R
        st = self.d_st.cpu().numpy().view(np.uint32).reshape(R, B.R2_WORDS)
        a1, a2 = p.d_acnt.cpu().numpy(), self.d_acnt.cpu().numpy().reshape(R, 8)
        n2s, s2s = [int(a[0]) for a in a2], [P.counter_u64(a) for a in a2]
        n2, s2 = max(n2s), max(s2s)
        rows = max(P.counter_u64(b, B.R2_ROWS) for b in st)
        kmers, hits = int(st[:, B.R2_KMERS].max()), int(st[:, B.R2_HITS].max())
        grown = False
        need_log2 = max(12, int(2 * kmers + 16).bit_length())
        if need_log2 > self.log2 or int(st[:, B.R2_TAB_FULL].max()):
            self.log2, grown = max(need_log2, self.log2 + 1), True
        if hits > self.key_cap:
            self.key_cap, grown = int(1.25 * hits) + 4096, True
        if rows > self.pool_cap:
            self.pool_cap, grown = int(1.25 * rows) + 4096, True
        if n2 > self.ctg_cap or s2 > self.seq_cap:
            c2, q2 = p.contig_caps(rows)
            self.ctg_cap, self.seq_cap, grown = max(c2, int(1.25 * n2)), max(q2, int(1.25 * s2)), True
        # the step's list holds every round's contigs: what it holds now plus what the refused appends would have added
        failed = [r for r in range(R) if int(st[r, B.R2_APPEND_ERR])]
        n_all, q_all = int(a1[0]) + sum(n2s[r] for r in failed), P.counter_u64(a1) + sum(s2s[r] for r in failed)
        if n_all > p.contig_cap or q_all > p.seq_cap:
            p._alloc_contig_list(max(p.contig_cap, int(1.25 * n_all) + 4096), max(p.seq_cap, int(1.25 * q_all) + (1 << 20)))
            grown = True
        # the assembly's workspace bounds cover the rounds' pools too (a pool beyond asm_big_pool_reads would set its gap error)
        sizes = self.d_rows_all.cpu().numpy().reshape(R, 2, p.n_gaps + 1)[:, 0, :p.n_gaps]
        sizes = sizes[int(np.argmax(sizes.max(axis=1)))] if sizes.size else sizes.reshape(-1)      # the round with the deepest pool
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
        p._chk(lib.gf_memset_dev(h, st, 0, 4 * B.R2_WORDS * self.R) or lib.gf_memset_dev(h, self.d_keys.data_ptr(), 0xFF, 8 * self.key_cap), "gf_memset_dev")
        if self.R > 1:      # the later rounds' rows and offsets: a gated round leaves them alone, and its assembly must see empty pools
            p._chk(lib.gf_memset_dev(h, self.d_rows_all.data_ptr() + 16 * (n_gaps + 1), 0, 16 * (n_gaps + 1) * (self.R - 1)), "gf_memset_dev")
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
        for r in range(1, self.R):
            self._enqueue_later(r)

    def _enqueue_later(self, r):
        """Round r + 1 (r >= 1 counts from 0): carry, table of the contigs round r appended, recruitment behind the carried keys, pools of
        the gaps that grew, assembly, append, pick over the round's own contigs — every new launch gated by round r's GROWN word."""
        p = self.p
        lib, h, n_gaps, k = p.lib, p.h, p.n_gaps, self.k
        prev = self.d_st.data_ptr() + 4 * B.R2_WORDS * (r - 1)
        st = prev + 4 * B.R2_WORDS
        live = prev + 4 * (B.R2_GROWN if r > 1 else B.R2_WITH)
        snap = self.d_snap.data_ptr() + 8 * self.key_cap * (r - 1) if p.keep_read_ids else None
        p._chk(lib.gf_round_carry_dev(h, self.d_keys.data_ptr(), self.d_sorted.data_ptr(), self.key_cap, n_gaps, self.d_work.data_ptr(),
                                      self.d_prev.data_ptr(), prev, st, p.ap, self.d_np.data_ptr(), self.d_np_live.data_ptr(), len(p.libs), snap,
                                      live), "gf_round_carry_dev")
        p._chk(lib.gf_contig_kmer_table_from_dev(h, p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), p.d_best.data_ptr(), n_gaps, k,
                                                 prev + 4 * B.R2_FIRST, self.d_tab.data_ptr(), self.log2, st, live), "gf_contig_kmer_table_from_dev")
        for l, (lb, (d_pairs, _, cap)) in enumerate(zip(p.libs, self.cand)):     # (round 1's entry: a gated round has no candidates)
            p._chk(lib.gf_recruit_by_contigs_dev(h, lb.d_reads.data_ptr(), lb.d_nmask.data_ptr() if lb.d_nmask is not None else None, lb.n_reads, p.L,
                                                 d_pairs.data_ptr(), self.d_np_live.data_ptr() + 4 * l, cap, l, k, self.d_tab.data_ptr(), self.log2,
                                                 self.d_keys.data_ptr(), self.key_cap, st), "gf_recruit_by_contigs_dev")
        rows = self.d_rows_all.data_ptr() + 16 * (n_gaps + 1) * r
        p._chk(lib.gf_round_pools_dev(h, self.d_keys.data_ptr(), self.d_sorted.data_ptr(), self.key_cap, self.lib_ptrs, len(p.libs), p.L, p.asm_ptr,
                                      p.asm_off, p.d_best.data_ptr(), n_gaps, self.d_prev.data_ptr(), self.d_work.data_ptr(), rows,
                                      self.d_pool.data_ptr(), self.pool_cap, st, live), "gf_round_pools_dev")
        ap2 = self.d_acnt.data_ptr() + 32 * r
        p._chk(lib.gf_assemble_multi_dev(h, self.d_pool.data_ptr(), None, rows + 8 * (n_gaps + 1), n_gaps, self.pool_cap, p.L, p.k_arr, p.kv_arr,
                                         len(p.kk), p.min_count, p.min_contig, self.d_ctg.data_ptr(), self.ctg_cap, ap2, self.d_seq.data_ptr(),
                                         self.seq_cap, ap2 + 8, self.d_gap_err.data_ptr() + 4 * max(1, n_gaps) * r),
               "gf_assemble_multi_dev (round %d)" % (r + 1))
        p._chk(lib.gf_contigs_append_dev(h, p.d_ctg.data_ptr(), p.ap, p.contig_cap, p.d_seq.data_ptr(), p.ap + 8, p.seq_cap, self.d_ctg.data_ptr(), ap2,
                                         self.ctg_cap, self.d_seq.data_ptr(), ap2 + 8, self.seq_cap, st), "gf_contigs_append_dev")
        p._pick(*p.anchor_pair, first=st + 4 * B.R2_FIRST)

    # ---- results ---------------------------------------------------------------------------------------------------------------
    def fetch(self, r):
        R = self.R
        st_all = self.d_st.cpu().numpy().view(np.uint32).reshape(R, B.R2_WORDS)
        a2_all = self.d_acnt.cpu().numpy().reshape(R, 8)
        n_err = int(self.d_gap_err.sum())
        for st, a2 in zip(st_all, a2_all):
            n2, s2 = int(a2[0]), P.counter_u64(a2)
            if n_err or int(st[B.R2_APPEND_ERR]) or n2 > self.ctg_cap or s2 > self.seq_cap:
                raise RuntimeError("second round overflow: %d gap errors, append flag %d, %d contigs (cap %d), %d contig bases (cap %d)"
                                   % (n_err, int(st[B.R2_APPEND_ERR]), n2, self.ctg_cap, s2, self.seq_cap))
        cand = [int(d_n[0]) for _, d_n, _ in self.cand]
        firsts = [int(st[B.R2_FIRST]) for st in st_all]
        idx = P.pick_index(r.best)
        rounds = []
        for j, st in enumerate(st_all):
            # recruits the round could not take: table entries without room, keys beyond their buffer, candidates beyond theirs, pools beyond theirs
            dropped = (int(st[B.R2_TAB_FULL]) + max(0, int(st[B.R2_HITS]) - self.key_cap)
                       + (sum(max(0, c - cap) for c, (_, _, cap) in zip(cand, self.cand)) if j == 0 else 0)
                       + (2 * int(st[B.R2_UNIQUE]) if int(st[B.R2_POOL_OVF]) else 0))
            closed = (r.best != 0) & (idx >= firsts[j])
            if j + 1 < R:
                closed &= idx < firsts[j + 1]
            rounds.append({"gaps_tried": int(st[B.R2_TRIED]), "gaps_with_recruits": int(st[B.R2_WITH]), "reads_recruited": 2 * int(st[B.R2_UNIQUE]),
                           "contigs": int(st[B.R2_N2]), "gaps_closed": int(closed.sum()), "dropped": int(dropped), "candidates": 2 * sum(cand),
                           "new_pairs": int(st[B.R2_NEW] if j else st[B.R2_UNIQUE]), "gaps_grown": int(st[B.R2_GROWN] if j else st[B.R2_WITH]),
                           "first": firsts[j], "gated": bool(st[B.R2_GATED])})
        r.round2_first = firsts[0]
        r.round2 = {key: rounds[0][key] for key in ("gaps_tried", "gaps_with_recruits", "reads_recruited", "contigs", "gaps_closed", "dropped",
                                                    "candidates")}
        r.round2["dropped"] = sum(d["dropped"] for d in rounds)
        r.recruit_rounds = rounds
        # the rounds that ran: up to and with the first that grew no gap (the rounds behind it are gated)
        r.recruit_rounds_run = next((j + 1 for j, d in enumerate(rounds) if not d["gaps_grown"]), R)
        if self.p.keep_read_ids:      # per gap with recruits: [(library, read id)] in round-2 pool order, after the last round that ran
            live = [j for j, d in enumerate(rounds) if not d["gated"]]
            last = live[-1]
            n_keys = min(int(st_all[last][B.R2_HITS]), self.key_cap)
            keys = np.unique(self.d_sorted[:n_keys].cpu().numpy().view(np.uint64))
            keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
            r.round2_reads = _reads_of_keys(keys)
            # the pairs new in each round: its distinct keys (round j < last: the snapshot round j + 1's carry took) without the round before's
            per, before = [], np.zeros(0, dtype=np.uint64)
            for j in range(R):
                if j > last:
                    per.append({})
                    continue
                if j < last:
                    n = min(int(st_all[j][B.R2_UNIQUE]), self.key_cap)
                    now = self.d_snap[j * self.key_cap:j * self.key_cap + n].cpu().numpy().view(np.uint64)
                else:
                    now = keys[(keys >> np.uint64(40)) < np.uint64(self.p.n_gaps)]
                per.append(_reads_of_keys(np.setdiff1d(now, before)))
                before = now
            r.recruit_reads = per


class ClosingPools:
    """Pipeline(closing_pools=True): after the last recruitment round's pick, the closing pool of every closed gap (DESIGN.md §27;
    closing_pools_host is the definition) — the pool of the step's first assembly, then every pair recruited for the gap — built by
    gf_closing_pools_dev from the keys the last pools call left in the second round's buffers, and handed to the after-pick rounds in
    place of the step's pool (fill_rounds.FillRound.pool_args).  per_library: one more pool per library, from the library's own pool and
    keys, with read ids (pair_span.PairSpan.lib_pool_args)."""

    def __init__(self, pipe, per_library=False):
        self.p, self.per_library = pipe, bool(per_library)
        self.d_pool = None

    def _alloc(self):
        p = self.p
        i32 = lambda n: torch.zeros(max(1, n), dtype=torch.int32, device=p.dev)
        self.d_pool = p._u8(self.cap * p.rb + 64)
        self.d_nm = i32(self.cap * self.nmw) if self.masks else None
        self.d_ids = i32(self.cap) if p.keep_read_ids else None
        self.d_lib = p._u8(self.cap) if p.keep_read_ids else None
        if self.per_library:
            n = len(p.libs)
            self.d_lib_pool = [p._u8(self.lib_cap * p.rb + 64) for _ in range(n)]
            self.d_lib_ids = [i32(self.lib_cap) for _ in range(n)]
            self.d_lib_nm = [i32(self.lib_cap * self.nmw) if self.masks else None for _ in range(n)]

    def prepare(self):
        """Behind the second round's own sizing: the step runs until the merged pool and the largest library's fit their capacities."""
        p = self.p
        n_lib, n_gaps = len(p.libs), p.n_gaps
        self.nmw = (p.L + 31) // 32
        self.masks = any(lb.d_nmask is not None for lb in p.libs)
        self.lib_nm_ptrs = (C.c_void_p * n_lib)(*[lb.d_nmask.data_ptr() if lb.d_nmask is not None else None for lb in p.libs]) if self.masks else None
        self.d_work = torch.zeros(int(p.lib.gf_closing_pools_work_words(n_gaps)), dtype=torch.int32, device=p.dev)
        self.n_blocks = 1 + (n_lib if self.per_library else 0)         # statistics: the merged pool's block, then one per library
        self.d_stats = torch.zeros(self.n_blocks * B.CP_WORDS, dtype=torch.int32, device=p.dev)
        self.d_off = torch.zeros(self.n_blocks * (n_gaps + 1), dtype=torch.int64, device=p.dev)
        # a library's masks in the order of its own pool's rows (gathered by the pool's read ids before the library's call)
        self.d_src_nm = torch.zeros(p.lib_cap * self.nmw, dtype=torch.int32, device=p.dev) if self.masks and self.per_library else None
        self.cap = self.lib_cap = 4096
        self._alloc()
        p._size_round("closing pools", self._grow)

    def _rows(self):
        st = self.d_stats.cpu().numpy().view(np.uint32).reshape(self.n_blocks, B.CP_WORDS)
        return st, [P.counter_u64(b, B.CP_ROWS) for b in st]

    def _grow(self):
        _, rows = self._rows()
        grown = False
        if rows[0] > self.cap:
            self.cap, grown = int(1.25 * rows[0]) + 1024, True
        if max(rows[1:], default=0) > self.lib_cap:
            self.lib_cap, grown = int(1.25 * max(rows[1:])) + 1024, True
        if grown:
            self._alloc()
        return grown

    def off_ptr(self, block):
        return self.d_off.data_ptr() + 8 * block * (self.p.n_gaps + 1)

    def pool_args(self):
        """FillRound.pool_args' four arguments for the merged closing pool."""
        return (self.d_pool.data_ptr(), self.d_nm.data_ptr() if self.d_nm is not None else None, self.off_ptr(0), self.cap)

    def lib_pool_args(self, l):
        """PairSpan.lib_pool_args' six arguments for library l's closing pool (its head: the library's own pool of the step)."""
        nm = self.d_lib_nm[l]
        return (self.d_lib_pool[l].data_ptr(), nm.data_ptr() if nm is not None else None, self.off_ptr(1 + l), self.d_lib_ids[l].data_ptr(), self.lib_cap,
                self.p.libs[l].d_pool_off.data_ptr())

    def _call(self, block, filt, src, src_off, src_nm, src_ids, src_lib, pool, cap, nm, ids, libs):
        p, r2 = self.p, self.p.round2
        ptr = lambda t: t.data_ptr() if t is not None else None
        p._chk(p.lib.gf_closing_pools_dev(p.h, r2.d_sorted.data_ptr(), r2.d_work.data_ptr(), r2.key_cap, r2.lib_ptrs, self.lib_nm_ptrs, len(p.libs),
                                          filt, p.L, src, src_off, src_nm, ptr(src_ids), src_lib, p.d_best.data_ptr(), p.n_gaps,
                                          self.d_work.data_ptr(), self.off_ptr(block), pool.data_ptr(), cap, ptr(nm), ptr(ids), ptr(libs),
                                          self.d_stats.data_ptr() + 4 * B.CP_WORDS * block), "gf_closing_pools_dev")

    def enqueue(self, d_nmask=None):
        """Behind the last pick of the step, before the after-pick rounds.  d_nmask: the N masks assemble() was given."""
        p = self.p
        if self.d_pool is None:       # the second round's own sizing runs: nobody reads a closing pool yet
            return
        if d_nmask is not None and not self.masks:
            raise RuntimeError("closing_pools: masks of the step's pool without a library that has masks")
        one = not p.need_merge        # the step's pool is library 0's own: its rows have read ids
        self._call(0, -1, p.asm_ptr, p.asm_off, d_nmask, p.libs[0].d_ids if one else None, 0 if one else -1, self.d_pool, self.cap, self.d_nm,
                   self.d_ids, self.d_lib)
        for l, lb in enumerate(p.libs if self.per_library else ()):
            src_nm = None
            if lb.d_nmask is not None:
                p._chk(p.lib.gf_gather_rows_dev(p.h, lb.d_nmask.data_ptr(), lb.n_reads, 4 * self.nmw, lb.d_ids.data_ptr(),
                                                lb.d_pool_off.data_ptr() + 8 * p.n_gaps, p.lib_cap, self.d_src_nm.data_ptr()), "gf_gather_rows_dev")
                src_nm = self.d_src_nm.data_ptr()
            self._call(1 + l, l, p.pool_ptr[l], lb.d_pool_off.data_ptr(), src_nm, lb.d_ids, l, self.d_lib_pool[l], self.lib_cap, self.d_lib_nm[l],
                       self.d_lib_ids[l], None)

    def fetch(self, r, pools):
        p = self.p
        st, rows = self._rows()
        caps = [self.cap] + [self.lib_cap] * (self.n_blocks - 1)
        for b, (need, cap) in enumerate(zip(rows, caps)):
            if int(st[b][B.CP_OVF]) or need > cap:
                raise RuntimeError("closing pools: %d rows of %s exceed the capacity %d"
                                   % (need, "the merged pool" if b == 0 else "library %s" % p.libs[b - 1].name, cap))
        blocks = [{"rows": rows[b], "gaps": int(st[b][B.CP_GAPS]), "recruited_rows": int(st[b][B.CP_RECRUITED]), "capacity": caps[b]}
                  for b in range(self.n_blocks)]
        r.closing_pools = dict(blocks[0], per_library=blocks[1:])
        if not pools:
            return
        off = self.d_off.cpu().numpy().astype(np.int64).reshape(self.n_blocks, p.n_gaps + 1)
        rows_of = lambda t, n: t[:n * p.rb].cpu().numpy().reshape(-1, p.rb)
        nm_of = lambda t, n: None if t is None else t[:n * self.nmw].cpu().numpy().view(np.uint32).reshape(-1, self.nmw)
        n = rows[0]
        r.closing_pool_off, r.closing_pool_rows, r.closing_pool_nmask = off[0], rows_of(self.d_pool, n), nm_of(self.d_nm, n)
        if self.d_ids is not None:
            r.closing_pool_ids, r.closing_pool_lib = self.d_ids[:n].cpu().numpy().view(np.uint32), self.d_lib[:n].cpu().numpy()
        if self.per_library:
            r.closing_lib_pool_off = [off[1 + l] for l in range(len(p.libs))]
            r.closing_lib_pool_rows = [rows_of(self.d_lib_pool[l], rows[1 + l]) for l in range(len(p.libs))]
            r.closing_lib_pool_ids = [self.d_lib_ids[l][:rows[1 + l]].cpu().numpy().view(np.uint32) for l in range(len(p.libs))]
            r.closing_lib_pool_nmask = [nm_of(self.d_lib_nm[l], rows[1 + l]) for l in range(len(p.libs))] if self.masks else None


def closing_pools_host(n_src, best, keys, library=None):
    """The closing pools' definition in plain Python.  n_src[g]: rows of the source pool of gap g (the pool the step's first assembly saw;
    library l's own pool with library=l); best[g]: the pick word, 0 for an open gap; keys: (gap, library, pair) of the final recruit sets,
    in any order, repeats allowed.  -> per gap the rows in pool order: (-1, j) for row j of the gap's source rows, (library, read id) for a
    recruit — reads 2p, 2p + 1 of every pair in (library, pair) order, each pair once; [] for an open gap, whatever keys it holds."""
    S = {}
    for g, l, q in keys:
        if 0 <= g < len(best) and (library is None or l == library):
            S.setdefault(g, set()).add((l, q))
    return [([(-1, j) for j in range(n_src[g])] + [(l, 2 * q + m) for l, q in sorted(S.get(g, ())) for m in (0, 1)]) if best[g] else []
            for g in range(len(best))]


def _reads_of_keys(keys):
    """{gap: [(library, read id)]} of sorted keys gap << 40 | library << 36 | pair: both reads of every pair."""
    gap, libi, pair = (keys >> np.uint64(40)).astype(np.int64), ((keys >> np.uint64(36)) & np.uint64(15)).astype(np.int64), \
        (keys & np.uint64((1 << 36) - 1)).astype(np.int64)
    out = {}
    for g, l, q in zip(gap.tolist(), libi.tolist(), pair.tolist()):
        out.setdefault(g, []).extend([(l, 2 * q), (l, 2 * q + 1)])
    return out


_RC = str.maketrans("ACGT", "TGCA")


def _canonical_kmers(text, k):
    out = set()
    for i in range(len(text) - k + 1):
        w = text[i:i + k]
        if w.count("A") + w.count("C") + w.count("G") + w.count("T") == k:
            out.add(min(w, w[::-1].translate(_RC)))
    return out


def rounds_host(pools, candidates, contigs, open_gaps, k, assemble, pick, max_rounds):
    """The recruitment rounds in plain Python, from the state the first pick leaves.
    pools: {gap: [read text]} as the assembly saw them; candidates: {(library, pair): (text of read 2 * pair, of read 2 * pair + 1)}, an N
    where a base is masked; contigs: [(gap, text)], the step's list after the first pick (a tombstone: empty text); open_gaps: the gaps with
    pick word 0; assemble(gap, [read text]) -> [contig text] over every (k, kv); pick(gap, [contig text]) -> closed?.
    -> (rounds, rounds_run): per round {"hits": {gap: set of (library, pair)} (H), "new": {gap: set} (S_r - S_(r-1)), "grown": [gap],
    "reads": {gap: [(library, pair)]} (S_r of the grown gaps in pool order), "contigs": [(gap, text)] (appended), "closed": [gap],
    "gated": bool}; rounds_run counts the first round that grew no gap."""
    open_now = set(open_gaps)
    cand_kmers = {key: _canonical_kmers(a, k) | _canonical_kmers(b, k) for key, (a, b) in candidates.items()}
    seen = {}                               # S: per gap, every pair recruited so far
    last, rounds, rounds_run = list(contigs), [], None
    for r in range(1, max_rounds + 1):
        if rounds_run is not None:
            rounds.append({"hits": {}, "new": {}, "grown": [], "reads": {}, "contigs": [], "closed": [], "gated": True})
            continue
        table = {}
        for g, text in last:
            if g in open_now and len(text) >= k:
                for w in _canonical_kmers(text, k):
                    table.setdefault(w, set()).add(g)
        hits = {}
        for key, ws in cand_kmers.items():
            for w in ws & table.keys():
                for g in table[w]:
                    hits.setdefault(g, set()).add(key)
        new = {g: h - seen.get(g, set()) for g, h in hits.items()}
        new = {g: v for g, v in new.items() if v}
        for g, v in new.items():
            seen.setdefault(g, set()).update(v)
        grown = sorted(g for g in new if g in open_now)
        reads, last, closed = {}, [], []
        for g in grown:
            reads[g] = sorted(seen[g])
            rows = list(pools.get(g, ())) + [t for key in reads[g] for t in candidates[key]]
            mine = list(assemble(g, rows))
            last += [(g, t) for t in mine]
            if pick(g, mine):
                closed.append(g)
        open_now -= set(closed)
        rounds.append({"hits": hits, "new": new, "grown": grown, "reads": reads, "contigs": last, "closed": closed, "gated": False})
        if not grown:
            rounds_run = r
    return rounds, (max_rounds if rounds_run is None else rounds_run)
