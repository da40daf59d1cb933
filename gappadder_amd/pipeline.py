"""The device-resident hot path as ONE object: recruit -> per-gap pools -> per-gap assembly -> flank anchoring.

What the reference does with files between processes —
    run_multi_threads_collect_reads.py:16-38 + collect_reads_for_gaps.py:68-263        (alignment tagger, per scaffold)
    run_multi_threads_discordant.py:19-138 + collect_discordant_low_mapq_reads.py:4-84 (second hop)
    run_multi_threads_discordant.py:141-317                                            (FASTQ join -> gap_reads/{id}.fastq)
    merge_reads.py:12-56                                                               (`cat` over the libraries)
    assemble_gaps.py:82-136, 277-299                                                   (KMC + Velvet per gap and (k, kv))
    pick_contigs.py:64-358 at scores 30 then 15 (assemble_gaps.py:336, 365)            (which gaps are closed)
— runs here as a chain of launches on libraries that stay in HBM (packed reads + 32-byte alignment records, `DeviceLibrary`):

    gf_screen_reads_dev + gf_tag_alignments_low_dev            recruit (k-mer screen: north_star; tagger: a-2)
    gf_second_hop_table_dev + gf_tag_low_mapq_table_dev        second hop (a-3)            [N > 1: union of the ranks' rows]
    gf_pool_keys_all_dev + gf_build_pools_dev                  pools per library (a-4)
    gf_pools_merge_dev                                         libraries in order (a-5)    [N > 1: sharding.OwnerExchange]
    gf_assemble_multi_dev                                      every (k, kv) pair (a-6)
    gf_pick_anchored2_dev                                      closed gaps (f-1)
    gf_merge_open_gaps_dev + gf_pick_anchored2_from_dev        contig merger for the gaps still open, second pick (f-3; merge_in_step)
    gf_contig_kmer_table_dev + gf_recruit_by_contigs_dev       second assembly round for the gaps still open (second_round.py):
      + gf_round2_pools_dev + gf_assemble_multi_dev            both-unmapped pairs recruited by the round-1 contigs' k-mers, pools
      + gf_contigs_append_dev + gf_pick_*_from_dev             = round-1 rows + recruits, assembled and picked again
    gf_closing_pools_dev                                       behind the last of those rounds: the pool every closed gap was closed from, for the rounds that read the fills' pools (closing_pools)
    gf_rescue_hq_keys_dev + gf_rescue_bridges_dev              rescue round for the gaps still open after the merge pick (rescue_round.py):
      + gf_merge_rescue_dev + gf_pick_*_from_dev               high-quality reads clipped at two contigs join the own contigs, merge, pick at 15
    gf_pick_joins_dev                                          the open gaps whose flanks overlap on a contig that runs through the junction (flank_joins.py)
    gf_fill_alts_dev                                           the closed gaps' other contigs with both anchors: identical, near or far rivals (fill_alternatives.py)
    gf_pick_extended[_aligned|_gapped]_dev                             partial fills of the gaps every pick left open (extended_fill.py)
    gf_fill_support_dev                                        how the pool of every closed gap backs the k-mers of its fill (read_support.py)
    gf_fill_polish_dev                                         the pool of every closed gap piled up on its fill: a vote per column (polish.py)
    gf_fill_polish_gapped_dev                                  ... with rows placed with one indel and votes on indel events (polish_gapped.py)
    gf_fill_pileup_dev                                         the same pool piled up on the whole winning contig: eight counters per column, a record per gap (pileup.py)
    gf_fill_pairs_dev                                          per library: the read pairs of every closed gap placed on its fill (pair_span.py)
    gf_fill_adjudicate_dev                                     the pool of every contested gap placed on the winner's and the rival's fill: votes and a verdict (fill_adjudication.py)
    gf_gap_span_dev                                            per library, behind its tagger: the size of every gap from the pairs that span it (gap_span.py)

`Pipeline` owns the sizing pass (capacities follow what the libraries actually recruit), every buffer of the core step, the stream
wiring and — in a multi-rank run — the one exchange step; an optional round keeps its buffers, sizing, launches and
results in its own module, and the step calls the rounds that are switched on by name.  Two callers: bench.py (libraries synthesised on the
device; `step()` is what it times) and the CLI (`gappadder_amd/device_collect.py`: libraries ingested from BAM + FASTQ files,
per-gap FASTQ / FASTA files WRITTEN FROM the results).  torch is the device-memory and collective plumbing; every kernel is
behind the C ABI.  There is no CPU path: `_lib.lib()` raises when libgapfill_hip.so is missing."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as B
from . import extended_fill as EXT
from . import fill_adjudication as FADJ
from . import fill_alternatives as FA
from . import flank_joins as FJ
from . import fill_rounds as FR
from . import gap_span as GSP
from . import pair_anchors as PAN
from . import pair_span as PSP
from . import polish as POL
from . import read_support as SUP
from . import rescue_round as RS
from . import second_round as R2
from . import sharding as SH

# counters of a library (device u32 words of `d_cnt`): 0 screen hits, 4 tagger hits, 8 second-hop hits, 12 pool keys,
# 24 pool error, 28 MAPQ==0 records, 29 second-hop table rows
CNT_SCREEN, CNT_TAG, CNT_HOP, CNT_KEYS, CNT_POOLERR, CNT_LOW, CNT_ROWS = 0, 4, 8, 12, 24, 28, 29


class DeviceLibrary:
    """One read library (an `alignments[]` + `raw_reads[]` entry of the reference's JSON, main.py:63-95) resident on this rank:
    `n_reads` packed reads (read 2*pair + mate; gf_pack_reads layout) and `n_recs` alignment records whose `.read` is the index
    of the record's read in THIS array.  `pull_mates`: a k-mer-screen hit also recruits the read's mate (north_star: "candidate
    read pairs").  `d_nmask`: the reads' N masks (files only; the synthetic reads have no N).  `n_total` = the library's reads
    over all ranks, `first_pair` = this rank's first pair (contiguous shards)."""

    def __init__(self, name, is_mean, is_sd, n_reads, d_reads, d_recs, n_recs=None, pull_mates=1, d_nmask=None, n_total=None,
                 first_pair=0, tag_ctx=None, screen=True, d_rec_keys=None, d_probes=None, probe_geom=None, d_lin_keys=None, lin_layout=None,
                 d_parts=None, parts_geom=None):
        self.name, self.is_mean, self.is_sd, self.pull_mates = name, int(is_mean), int(is_sd), int(pull_mates)
        self.n_reads, self.d_reads, self.d_recs, self.d_nmask = int(n_reads), d_reads, d_recs, d_nmask
        self.n_recs = int(n_reads if n_recs is None else n_recs)
        self.n_total = int(self.n_reads if n_total is None else n_total)
        self.first_pair, self.n_pairs = int(first_pair), self.n_reads // 2
        self.tag_ctx = tag_ctx          # a second GapFill (second stream) for the tagger + second hop, or None: the pipeline's
        self.screen = bool(screen)      # False: alignment-based recruitment only (the reference's own mode)
        self.d_rec_keys = d_rec_keys    # the records' key column (gf_alnrec_keys_dev); None: Pipeline.add_library builds it
        # the records' 4-byte linear key column and the layout it was built for (gf_alnrec_linkeys_dev); None: Pipeline.add_library builds it
        # where the draft fits one 32-bit line
        self.d_lin_keys, self.lin_layout = d_lin_keys, lin_layout
        # the reads' probe column and the geometry it was built for (gf_read_probes_dev, or the file path's packing kernels); None:
        # Pipeline.add_library builds it where it pays
        self.d_probes, self.probe_geom = d_probes, probe_geom
        # the reads' resident parts — the output of the filter's first pass — and what they were built for (gf_screen_parts_build_dev);
        # None: Pipeline.add_library builds them where parts are kept
        self.d_parts, self.parts_geom = d_parts, parts_geom
        self.counts = {}


class Results:
    """What one step left on the device, fetched once (contigs, their bases, the pick words, the pools when asked for).  The fields of
    the merge round and of the optional rounds are None unless the round ran."""
    merge = rescue = rescue_first = round2 = round2_first = round2_reads = recruit_rounds = recruit_rounds_run = recruit_reads = extended = ext = ext_bases = support = support_stats = None
    polish = polish_bases = polish_stats = pairs = pair_stats = lib_pool_off = lib_pool_rows = lib_pool_ids = None
    closing_pools = closing_pool_off = closing_pool_rows = closing_pool_nmask = closing_pool_ids = closing_pool_lib = None
    closing_lib_pool_off = closing_lib_pool_rows = closing_lib_pool_ids = closing_lib_pool_nmask = None
    pair_anchors = pair_anchor_stats = lib_taghits = gap_span = gap_span_stats = pileup = pileup_track = pileup_stats = joins = join_stats = alts = alt_contigs = alt_stats = adjudication = adj_stats = None


# anchor mode -> its pick, its pick over the contigs from an index on, its extended fill; do its picks leave a selection per contig
# (gf_ctg_pick) and two statistics words?
PICKS = {"exact": ("gf_pick_anchored2_dev", "gf_pick_anchored2_from_dev", "gf_pick_extended_dev", False),
         "align": ("gf_pick_aligned_dev", "gf_pick_aligned_from_dev", "gf_pick_extended_aligned_dev", True),
         "gapped": ("gf_pick_gapped_dev", "gf_pick_gapped_from_dev", "gf_pick_extended_gapped_dev", True)}


class Pipeline:
    def __init__(self, gf, n_gaps, read_len, k_pairs, device=None, world=1, rank=0, backend="nccl", force_exchange=False,
                 min_count=2, min_contig=40, anchors=(30, 15), clip_dist=250, anchor_mapq=30, k_screen=None, keep_read_ids=False,
                 key_column=True, linear_keys=True, probe_column=True, screen_parts=True, merge_in_step=False, merge_max_set=128, anchor_mode="exact", second_round=False,
                 recruit_rounds=1, extended_fill=False, ext_base_cap=None, rescue_round=False, read_support=False, support_k=None, polish=False,
                 polish_seed=16, polish_max_mismatch=4, polish_min_overlap=48, polish_min_votes=2, polish_indels=False, polish_max_indel=8,
                 pair_span=False, pair_seed=16,
                 pair_max_mismatch=4, pair_min_overlap=48, pair_z=3, pair_anchors=False, pair_min_pairs=8, gap_span=False, span_z=3,
                 span_shift=1000, span_min_pairs=8, pileup=False, pileup_seed=16, pileup_max_mismatch=4, pileup_min_overlap=48, pileup_min_depth=3,
                 pileup_min_agree=80, pileup_track=True, flank_joins=False, join_max_overlap=256, join_min_context=30, join_max_mismatch=2,
                 alternatives=False, alt_max_dist=16, adjudicate=False, adj_seed=16, adj_max_mismatch=4, adj_min_overlap=48, adj_context=None,
                 adj_min_votes=3, adj_ratio=2, closing_pools=False):
        """gf: a GapFill whose gaps (and flanks, when a library is screened) are set.  k_pairs: [(k, k_velvet)] of
        assemble_gaps.py:87-122.  The screen runs at the SMALLEST k of the list: a read that shares a 51-mer with a flank shares
        its 31-mers too, so this is the superset every assembly k needs (the reference recruits once, then assembles at every k).
        anchors: flank-anchor lengths of the two pick rounds (the reference's bwa scores 30 then 15, assemble_gaps.py:336, 365);
        clip_dist / anchor_mapq: main.py:215-216.  key_column: the libraries keep an 8-byte key per alignment record beside the records
        ({pos, scaffold | MAPQ-0 bit}, built once when a library is added: 7.2 GB for C4's 900 M records) and the tagger streams THAT —
        a record far from every gap, 99 % of a BAM, is decided by (scaffold, position) alone (the reference's `focal_region.has_key(POS)`,
        collect_reads_for_gaps.py:104) — fetching the 32-byte record only of what passes its bin maps.
        linear_keys (with key_column): where the scaffolds of the draft, laid end to end on granule boundaries, fit one 32-bit line (a draft
        below 4 Gb: gf_tag_layout), the library keeps a 4-byte key per record instead — its position on that line — with the MAPQ-0 bit in a
        bit plane (3.7 GB for C4), and the tagger streams that; the 8-byte column is then built only for a consumer of its own (gap_span)
        or where the line does not fit.  Same hits either way.
        probe_column: the screened libraries keep, beside the packed reads, the 16-mers the filter's first pass probes — np 4-byte words per
        read, built once when a library is added (k = 51 on 150 bases: 12 of a read's 38 bytes, 10.8 GB for C4's 900 M reads) — and that
        pass streams THEM; only where 4 * np is at most half a packed read and the column fits (else nothing is built and the pass reads
        the rows).  A column built for another geometry (k, read length, read count) is rebuilt before it is used.
        screen_parts: the screened libraries keep, beside the column, what the filter's first pass makes of it — every probe as a 4-byte
        pair in its bucket's part, with the parts' fill history and counts (gf_screen_parts_geom; 12.2 GB for C4) — built once when a
        library is added, from the column where there is one; the screen of every step then starts at its second pass.  None of it
        depends on the gaps or the draft.  Only where a column would be kept too (gf_screen_parts_geom::use) and the parts fit; parts
        built for another geometry or another plan (k, read count, writers) are rebuilt before they are used, and the column stays: it is
        what the first pass streams whenever the parts are refused.
        anchor_mode: how every pick of the step anchors the flanks on the contigs — "exact" anchors (gf_pick_anchored2_dev) or "align",
        seed-and-extend of the whole flanks (gf_pick_aligned_dev; `anchors` are then the score thresholds), or "gapped", the same with a
        banded affine-gap extension that aligns through a draft indel next to the gap (gf_pick_gapped_dev); with "align" and "gapped" the
        Results carry `ctg_pick` (gf_ctg_pick per contig) and `align_dropped` / `align_seed_overflow` (the pick's d_stats).
        second_round (second_round.py), rescue_round (rescue_round.py), extended_fill with ext_base_cap (extended_fill.py): the
        reference's later stages inside the step, each described in its module; in the step they run in this order after the merge
        round's pick.  recruit_rounds (1..16, with second_round): the second round repeated with the contigs of the round before until a
        round grows no gap (Results.recruit_rounds, .recruit_rounds_run, .recruit_reads).  read_support with support_k (read_support.py; default: the smallest k of k_pairs in 16..64): after all of them,
        a record per closed gap of how its pool backs the k-mers of its fill (Results.support).  polish with polish_seed,
        polish_max_mismatch, polish_min_overlap, polish_min_votes (polish.py): last of all, the pool of every closed gap is piled up on
        its winning contig and every column of the fill takes a vote (Results.polish, .polish_bases, .polish_stats;
        polished_sequences); the step's contigs and picks stay as they are, and read_support keeps describing the UNPOLISHED fill.
        polish_indels with polish_max_indel (polish_gapped.py; only with polish): the polish places rows with one indel of up to
        polish_max_indel bases as well and votes on indel events, so the polished contig may change length; Results.polish then has
        the 64-byte record gf_fill_polish_gapped and .polish_stats the event counts.
        pileup with pileup_seed, pileup_max_mismatch, pileup_min_overlap, pileup_min_depth, pileup_min_agree, pileup_track (pileup.py):
        behind the polish, the same pool piled up on the (unpolished) winning contig once more, the eight counters (base x read strand)
        of EVERY contig column kept in a track and the fill's weak columns summed up per gap (Results.pileup, .pileup_track [entries, 8]
        u16, .pileup_stats; fill_confidence); pileup_track=False: the records alone, no track buffer.
        pair_span with pair_seed, pair_max_mismatch, pair_min_overlap, pair_z (pair_span.py): after them, per library, the read pairs of
        every closed gap placed on its (unpolished) winning contig: inserts against is_mean -/+ pair_z * is_sd and the physical coverage
        of the fill (Results.pairs [n_lib, n_gaps], .pair_stats); it keeps the pools' read ids (keep_read_ids).
        pair_anchors with pair_min_pairs (pair_anchors.py; only with pair_span, not with tag_ahead): behind each library's pair span, the
        mates the tagger found anchored in a flank paired, at their draft coordinates, with the other mate's placement on the fill: the
        insert-size deviation per column of the fill (Results.pair_anchors [n_lib, n_gaps], .pair_anchor_stats).
        gap_span with span_z, span_shift, span_min_pairs (gap_span.py): per library, behind its tagger pass and on the tagger's stream, the
        read pairs whose mates map cleanly on either side of a gap, for EVERY gap, open or closed: their number and the sums of their
        template lengths (Results.gap_span [n_lib, n_gaps], .gap_span_stats; gap_span.estimate turns a record into a gap size).  It reads the
        libraries' records and the gap table only, so it goes with every other option, tag_ahead included; single rank.
        flank_joins with join_max_overlap, join_min_context, join_max_mismatch (flank_joins.py): after the last pick (behind the rescue
        round, before the extended fill), every gap still open is looked at for a contig that carries both anchors OUT of order — the
        flanks overlap, nothing is missing (Results.joins, gf_flank_join per gap; .join_stats; joined_gaps).  Exact anchors only; it reads
        the step's contigs and the flanks and no pool, so it goes with second_round, merge_in_step, rescue_round and extended_fill;
        single rank.
        alternatives with alt_max_dist (fill_alternatives.py): after the last pick, beside the joins, every CLOSED gap's contigs are
        looked at again: those that carry both anchors as the winner does are classed by their fill — the winner's byte for byte,
        within alt_max_dist edits of it, or further away — and the best of the differing ones is the gap's rival (Results.alts,
        gf_fill_alt per gap; .alt_contigs, gf_fill_alt_contig per contig; .alt_stats; alternative_sequences).  Exact anchors only; it
        reads the step's contigs, the flanks and the pick words, so it goes with second_round, merge_in_step, rescue_round,
        extended_fill and flank_joins; single rank.
        adjudicate with adj_seed, adj_max_mismatch, adj_min_overlap, adj_context, adj_min_votes, adj_ratio (fill_adjudication.py; only
        with alternatives): last of the after-pick rounds, the pool of every CONTESTED gap is placed on the winner's and on the rival's
        fill, each between adj_context bases of the flanks (default: the read length), and every row votes for the one it fits strictly
        better: KEEP, SWITCH or UNDECIDED per gap (Results.adjudication, gf_fill_adj per gap; .adj_stats; adjudicated_sequences).
        Advice only: the picks, the contigs and picked_sequences stay as they are.
        closing_pools (second_round.ClosingPools; only with second_round): behind the last recruitment round's pick the closing pool of
        every closed gap is built — the rows the step's first assembly saw, then every pair recruited for the gap — and read_support,
        polish, pileup, pair_span (one pool per library, with read ids) and adjudicate, refused beside second_round without it, run on
        that pool (Results.closing_pools; with fetch(pools=True) .closing_pool_off, _rows, _nmask, _ids, _lib and .closing_lib_pool_*)."""
        # what the options exclude, before anything touches gf or the library
        single_rank = int(world) == 1 and not force_exchange
        k_round2 = min([int(a) for a, _ in k_pairs if 16 <= int(a) <= 64], default=None)
        own_pools = second_round and not closing_pools      # the second round's pools are not rebuilt for the rounds that read the fills' pools
        for bad, why in ((anchor_mode not in PICKS, "anchor_mode %r: 'exact', 'align' or 'gapped'" % (anchor_mode,)),
                         (rescue_round and not merge_in_step, "rescue_round needs merge_in_step: the reads are aligned to the merged contigs"),
                         (rescue_round and not single_rank, "rescue_round runs on a single rank"),
                         (rescue_round and second_round, "rescue_round with second_round: the order of the rounds is not settled"),
                         (second_round and not single_rank, "second_round runs on a single rank"),
                         (second_round and merge_in_step, "second_round with merge_in_step: the order of the merge and the second round is not settled"),
                         (second_round and k_round2 is None, "second_round needs a k in 16..64 among k_pairs"),
                         (isinstance(recruit_rounds, bool) or not isinstance(recruit_rounds, int) or not 1 <= recruit_rounds <= 16,
                          "recruit_rounds %r: an integer 1..16" % (recruit_rounds,)),
                         (not second_round and recruit_rounds != 1, "recruit_rounds repeats the second round: it needs second_round"),
                         (closing_pools and not second_round, "closing_pools needs second_round: it rebuilds the pools the recruitment rounds closed gaps from"),
                         *FR.refusals("read_support", read_support, single_rank, own_pools),
                         (read_support and support_k is None and k_round2 is None, "read_support needs support_k, or a k in 16..64 among k_pairs"),
                         *FR.refusals("polish", polish, single_rank, own_pools),
                         (polish_indels and not polish, "polish_indels needs polish: it is a mode of the polish round"),
                         *FR.refusals("pileup", pileup, single_rank, own_pools),
                         *FR.refusals("pair_span", pair_span, single_rank, own_pools),
                         (pair_anchors and not pair_span, "pair_anchors needs pair_span: it reads the pair span's placements"),
                         *FR.refusals("pair_anchors", pair_anchors, single_rank, second_round),
                         (gap_span and not single_rank, "gap_span runs on a single rank: the sums are additive over ranks, and that reduction is left out"),
                         (flank_joins and anchor_mode in PICKS and anchor_mode != "exact", "flank_joins works with the exact anchors: not with anchor_mode %r" % (anchor_mode,)),
                         (flank_joins and not single_rank, "flank_joins runs on a single rank"),
                         (alternatives and anchor_mode in PICKS and anchor_mode != "exact", "alternatives works with the exact anchors: not with anchor_mode %r" % (anchor_mode,)),
                         (alternatives and not single_rank, "alternatives runs on a single rank"),
                         (adjudicate and not alternatives, "adjudicate needs alternatives: it reads the alternatives round's records"),
                         *FR.refusals("adjudicate", adjudicate, single_rank, own_pools),
                         (extended_fill and not single_rank, "extended_fill runs on a single rank"),
                         (extended_fill and len(k_pairs) > B.EXT_MAX_PAIRS, "extended_fill: at most %d (k, kv) pairs" % B.EXT_MAX_PAIRS)):
            if bad:
                raise ValueError(why)
        self.anchor_mode = anchor_mode
        self.per_contig = PICKS[anchor_mode][3]      # the mode's picks leave a selection per contig and two statistics words
        # the optional rounds, in the order the step runs them; None: off
        self.round2 = R2.SecondRound(self, k_round2, recruit_rounds) if second_round else None
        self.closing = R2.ClosingPools(self, per_library=pair_span) if closing_pools else None
        self.rescue = RS.RescueRound(self) if rescue_round else None
        self.joins = FJ.FlankJoins(self, join_max_overlap, join_min_context, join_max_mismatch) if flank_joins else None
        self.alts = FA.FillAlternatives(self, alt_max_dist) if alternatives else None
        self.ext = EXT.ExtendedFill(self, int(ext_base_cap) if ext_base_cap is not None else None) if extended_fill else None
        self.support = SUP.ReadSupport(self, k_round2 if support_k is None else support_k) if read_support else None
        if polish and polish_indels:
            from . import polish_gapped as PLG   # (here, not above: it builds on polish.py, which imports this module)
        self.polish = (PLG.FillPolishGapped(self, polish_seed, polish_max_mismatch, polish_min_overlap, polish_min_votes, polish_max_indel, read_len)
                       if polish and polish_indels else
                       POL.FillPolish(self, polish_seed, polish_max_mismatch, polish_min_overlap, polish_min_votes, read_len) if polish else None)
        if pileup:
            from . import pileup as PU           # (here, not above: it builds on polish.py, which imports this module)
        self.pileup = (PU.FillPileup(self, pileup_seed, pileup_max_mismatch, pileup_min_overlap, pileup_min_depth, pileup_min_agree, pileup_track,
                                     read_len) if pileup else None)
        self.pairs = PSP.PairSpan(self, pair_seed, pair_max_mismatch, pair_min_overlap, pair_z, read_len) if pair_span else None
        self.anchored = PAN.PairAnchors(self, pair_min_pairs, read_len) if pair_anchors else None        # (launched by self.pairs, per library)
        self.adj = (FADJ.FillAdjudication(self, adj_seed, adj_max_mismatch, adj_min_overlap, adj_context, adj_min_votes, adj_ratio, read_len)
                    if adjudicate else None)          # (reads the records self.alts wrote before the after-pick rounds)
        self.after_pick = [r for r in (self.support, self.polish, self.pileup, self.pairs, self.anchored, self.adj) if r is not None]      # (the order they run in)
        self.gap_span = GSP.GapSpan(self, span_z, span_shift, span_min_pairs) if gap_span else None      # (launched behind every tagger pass, per library)
        self.gf, self.lib, self.h = gf, B.lib(), gf.handle
        self.n_gaps, self.L, self.kk = int(n_gaps), int(read_len), [(int(a), int(b)) for a, b in k_pairs]
        self.rb = self.lib.gf_packed_read_bytes(self.L)
        self.dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.world, self.rank, self.backend = int(world), int(rank), backend
        self.multi = self.world > 1 or bool(force_exchange)
        self.coll_dev = self.dev if backend == "nccl" else torch.device("cpu")
        self.min_count, self.min_contig, self.anchors = int(min_count), int(min_contig), tuple(int(a) for a in anchors)
        self.anchor_pair = (self.anchors[0], self.anchors[1] if len(self.anchors) > 1 else 0)       # a pick's two rounds; 0: no second one
        self.clip_dist, self.anchor_mapq = int(clip_dist), int(anchor_mapq)
        self.k_screen = int(k_screen) if k_screen else (min(a for a, _ in self.kk) if self.kk else 31)
        self.keep_read_ids = bool(keep_read_ids) or bool(pair_span)
        self.key_column = bool(key_column)
        self.linear_keys = self.key_column and bool(linear_keys)
        self.probe_column = bool(probe_column)
        self.screen_parts = bool(screen_parts)
        # merge_in_step: the contig-merge round (assemble_gaps.py:301-306 run_contigs_merge: dedup + ContigsMerger per gap) runs INSIDE the
        # step, on the device, for the gaps the first pick leaves open, followed by a second pick over the merged contigs — the reference
        # merges before it picks (:335-339); a gap the pick closes from its own contigs gains nothing from merging.  Merged contigs are
        # appended to the step's contig list with k = kv = 0.  Sets of more than merge_max_set contigs after the dedup are left alone.
        self.merge_in_step, self.merge_max_set = bool(merge_in_step), int(merge_max_set)
        self.libs = []
        self.batch = SH.owner_batch(self.n_gaps, self.world)
        self.stream = None
        if self.multi:
            # the collectives are ordered against the kernels by running everything on ONE torch side stream (not the legacy
            # default stream): the library adopts it
            self.stream = torch.cuda.Stream(device=self.dev)
            self._chk(self.lib.gf_set_stream(self.h, C.c_void_p(self.stream.cuda_stream)), "gf_set_stream")
        self.tag_after_filter = False
        # True: the alignment tagger of the NEXT step's records is launched on the libraries' second stream right after this step's pools
        # are built, i.e. beside the assembly (latency-bound, little HBM traffic) instead of in a row with the memory-bound filter: a
        # software pipeline over successive steps (every step still runs one tagger pass; prepare() launches the first)
        self.tag_ahead = False
        self.assemble_in_step = True      # False: step() stops at the pools; the caller runs assemble() itself (N masks of file-born pools)
        self.fixed_spans, self.fixed_on = [], False
        self.screen_dropped = 0
        self.prepared = False

    # ---- plumbing ---------------------------------------------------------------------------------------------------------
    def _chk(self, rc, what):
        if rc:
            raise B.GapFillError(rc, what, self.lib.gf_last_error(self.h).decode())

    def _u8(self, n):
        return torch.empty(max(1, int(n)), dtype=torch.uint8, device=self.dev)

    def contexts(self):
        """The distinct GapFill contexts (= streams) the step runs on."""
        return list({id(x): x for x in [self.gf] + [lb.tag_ctx for lb in self.libs if lb.tag_ctx is not None]}.values())

    def sync(self):
        for g in self.contexts():
            g.sync()

    def add_library(self, lb, hit_cap=None):
        """Registers a library and allocates its recruit buffers.  hit_cap (hits of one kind per step) defaults to an eighth of the
        reads — the screen finds 0.5 %, the tagger 1-2 % on the BASELINE workloads —; prepare() grows the buffers of a library that finds
        more (the device calls report their counts beyond the capacity) and sizes again; a STEP that outgrows them later fails loudly
        in fetch()."""
        assert not self.prepared
        if self.gap_span is not None:
            self.gap_span.check_library(lb)        # (ValueError before anything touches the library)
        dev = self.dev
        lb.h2 = lb.tag_ctx.handle if lb.tag_ctx is not None else self.h
        lb.second_stream = lb.h2.value != self.h.value
        self._alloc_hit_buffers(lb, int(hit_cap) if hit_cap else max(1 << 20, max(lb.n_reads, lb.n_recs) // 8))
        lb.d_pool_off = torch.zeros(self.n_gaps + 1, dtype=torch.int64, device=dev)
        lb.d_cnt = torch.zeros(32, dtype=torch.int32, device=dev)
        lb.cp = lb.d_cnt.data_ptr()
        lb.d_ids = None
        if self.linear_keys:
            self._linear_keys(lb)
        # the 8-byte column: where there is no linear one, and for a consumer of its own (gap_span reads lb.d_rec_keys)
        if self.key_column and lb.d_rec_keys is None and (lb.d_lin_keys is None or self.gap_span is not None):
            lb.d_rec_keys = torch.empty(lb.n_recs + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            self._chk(self.lib.gf_alnrec_keys_dev(self.h, lb.d_recs.data_ptr(), lb.n_recs, lb.d_rec_keys.data_ptr()), "gf_alnrec_keys_dev")
            self.gf.sync()
        if self.probe_column and lb.screen:
            self._probe_column(lb)
        if self.screen_parts and lb.screen:
            self._screen_parts(lb)
        self.libs.append(lb)
        return lb

    def _linear_keys(self, lb):
        """The library's linear key column for THIS context's scaffolds: kept when it was built for the library's record count and these
        scaffolds (the tagger checks base[] against the layout's checksum at every map it builds), built otherwise; None where the draft
        does not fit one 32-bit line or the column does not fit the device (the 8-byte column then serves)."""
        ns = self.gf.n_scaffolds
        if lb.d_lin_keys is not None and lb.lin_layout is not None and lb.lin_layout.use and \
                (lb.lin_layout.n_recs, lb.lin_layout.n_scaffolds) == (lb.n_recs, ns):
            return
        lb.d_lin_keys = lb.lin_layout = None
        if not lb.n_recs or not ns:
            return
        try:
            d_col = torch.empty(self.lib.gf_alnrec_linkeys_bytes(lb.n_recs, ns) // 4, dtype=torch.int32, device=self.dev)
        except torch.cuda.OutOfMemoryError:
            return
        torch.cuda.synchronize()
        lay = B.TagLayout()
        self._chk(self.lib.gf_alnrec_linkeys_dev(self.h, lb.d_recs.data_ptr(), lb.n_recs, d_col.data_ptr(), 4 * d_col.numel(), C.byref(lay)),
                  "gf_alnrec_linkeys_dev")
        self.gf.sync()
        if lay.use:
            lb.d_lin_keys, lb.lin_layout = d_col, lay

    def _probe_column(self, lb):
        """The library's probe column for THIS pipeline's screen (k_screen, read length, the library's reads): kept when it was built for
        exactly that, built (again) otherwise; None where a column does not pay or does not fit (the filter then reads the rows)."""
        if not 16 <= self.k_screen <= min(64, self.L):
            return
        want = B.ProbeColumnGeom()
        self._chk(self.lib.gf_probe_geometry(self.h, lb.n_reads, self.L, self.k_screen, C.byref(want)), "gf_probe_geometry")
        if lb.d_probes is not None and lb.probe_geom is not None and lb.probe_geom.key() == want.key():
            return
        lb.d_probes = lb.probe_geom = None
        nbytes = self.lib.gf_probe_column_bytes(C.byref(want))
        if not want.use or not lb.n_reads:
            return
        try:
            d_probes = torch.empty(nbytes // 4, dtype=torch.int32, device=self.dev)
        except torch.cuda.OutOfMemoryError:
            return
        torch.cuda.synchronize()
        geom = B.ProbeColumnGeom()
        self._chk(self.lib.gf_read_probes_dev(self.h, lb.d_reads.data_ptr(), lb.n_reads, self.L, self.k_screen, d_probes.data_ptr(), C.byref(geom)),
                  "gf_read_probes_dev")
        self.gf.sync()
        lb.d_probes, lb.probe_geom = d_probes, geom

    def _screen_parts(self, lb):
        """The library's resident parts for THIS pipeline's screen: kept when they were built for exactly what the screen would build now,
        built (again) otherwise — from the column where the library has one; None where parts are not kept, do not fit the device, or a
        part ran full (the filter then runs its first pass, from the column or the rows)."""
        if not 16 <= self.k_screen <= min(64, self.L):
            return
        want = B.ScreenPartsGeom()
        self._chk(self.lib.gf_screen_parts_geometry(self.h, lb.n_reads, self.L, self.k_screen, C.byref(want)), "gf_screen_parts_geometry")
        if lb.d_parts is not None and lb.parts_geom is not None and lb.parts_geom.use and lb.parts_geom.key() == want.key():
            return
        lb.d_parts = lb.parts_geom = None
        if not want.use or not lb.n_reads:
            return
        try:
            d_parts = torch.empty(self.lib.gf_screen_parts_bytes(C.byref(want)) // 4, dtype=torch.int32, device=self.dev)
        except torch.cuda.OutOfMemoryError:
            return
        torch.cuda.synchronize()
        col = self.probe_column and lb.d_probes is not None
        geom = B.ScreenPartsGeom()
        self._chk(self.lib.gf_screen_parts_build_dev(self.h, lb.d_reads.data_ptr(), lb.d_probes.data_ptr() if col else None,
                                                     C.byref(lb.probe_geom) if col else None, lb.n_reads, self.L, self.k_screen, d_parts.data_ptr(),
                                                     C.byref(geom)), "gf_screen_parts_build_dev")
        self.gf.sync()
        if geom.use:
            lb.d_parts, lb.parts_geom = d_parts, geom

    def _alloc_hit_buffers(self, lb, hit_cap):
        lb.hit_cap = int(hit_cap)
        lb.d_hits = self._u8(lb.hit_cap * 8)
        lb.d_thits = self._u8(lb.hit_cap * 12)
        lb.d_lhits = self._u8(lb.hit_cap * 12)
        lb.d_low = self._u8(lb.hit_cap * 12)           # MAPQ==0 records compacted by the tagger (2 % of a typical BAM)
        lb.key_cap = 4 * lb.hit_cap
        lb.d_keys = torch.empty(lb.key_cap, dtype=torch.int64, device=self.dev)

    # ---- the phases of a step ---------------------------------------------------------------------------------------------
    def recruit(self, lb, tagger=True):
        lib, h = self.lib, self.h
        if lb.second_stream and tagger:
            self._chk(lib.gf_stream_wait(lb.h2, h), "gf_stream_wait")          # the previous consumers of the tagger buffers are done
            if self.tag_after_filter:
                # the tagger (a pure 32-B-record stream) starts when the k-mer FILTER has finished and runs beside the latency-bound
                # verification pass: beside the filter the two only took turns on the memory system (C4: 36.5 ms together, 26.6 + 10.5 alone)
                self._chk(lib.gf_stream_wait_after_filter(lb.h2, h), "gf_stream_wait_after_filter")
        if lb.screen:
            col = self.probe_column and lb.d_probes is not None     # (the library checks the geometry again: a stale column is not used)
            parts = self.screen_parts and lb.d_parts is not None    # (likewise: parts of another plan are not used)
            self._chk(lib.gf_screen_reads_parts_dev(h, lb.d_reads.data_ptr(), lb.d_nmask.data_ptr() if lb.d_nmask is not None else None,
                                                    lb.d_probes.data_ptr() if col else None, C.byref(lb.probe_geom) if col else None,
                                                    lb.d_parts.data_ptr() if parts else None, C.byref(lb.parts_geom) if parts else None, lb.n_reads,
                                                    self.L, self.k_screen, 1, lb.d_hits.data_ptr(), lb.hit_cap, lb.cp), "gf_screen_reads_parts_dev")
        if tagger:
            self.tagger(lb)

    def tagger(self, lb):
        self._tag(lb)
        if self.gap_span is not None:      # the same records once more, on the same stream: the pairs that span a gap
            self.gap_span.enqueue(lb)

    def _tag(self, lb):
        if self.linear_keys and lb.d_lin_keys is not None:   # (the library checks the layout again: a stale column is not used)
            keys8 = lb.d_rec_keys.data_ptr() if lb.d_rec_keys is not None else None
            self._chk(self.lib.gf_tag_alignments_linkeys_dev(lb.h2, lb.d_recs.data_ptr(), lb.d_lin_keys.data_ptr(), C.byref(lb.lin_layout), keys8,
                                                             lb.n_recs, lb.is_mean, lb.is_sd, self.clip_dist, self.anchor_mapq, lb.d_thits.data_ptr(),
                                                             lb.hit_cap, lb.cp + 4 * CNT_TAG, lb.d_low.data_ptr(), lb.hit_cap, lb.cp + 4 * CNT_LOW),
                      "gf_tag_alignments_linkeys_dev")
            return
        if self.key_column and lb.d_rec_keys is not None:
            self._chk(self.lib.gf_tag_alignments_keys_dev(lb.h2, lb.d_recs.data_ptr(), lb.d_rec_keys.data_ptr(), lb.n_recs, lb.is_mean, lb.is_sd, self.clip_dist,
                                                          self.anchor_mapq, lb.d_thits.data_ptr(), lb.hit_cap, lb.cp + 4 * CNT_TAG, lb.d_low.data_ptr(),
                                                          lb.hit_cap, lb.cp + 4 * CNT_LOW), "gf_tag_alignments_keys_dev")
            return
        self._chk(self.lib.gf_tag_alignments_low_dev(lb.h2, lb.d_recs.data_ptr(), lb.n_recs, lb.is_mean, lb.is_sd, self.clip_dist, self.anchor_mapq,
                                                     lb.d_thits.data_ptr(), lb.hit_cap, lb.cp + 4 * CNT_TAG, lb.d_low.data_ptr(), lb.hit_cap,
                                                     lb.cp + 4 * CNT_LOW), "gf_tag_alignments_low_dev")

    def _fixed_mark(self):
        if not self.fixed_on:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _fixed_span(self, name, e0):
        if e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.fixed_spans.append((name, e0, e1))

    def hop_and_keys(self, lb):
        lib, h, world = self.lib, self.h, self.world
        self._chk(lib.gf_second_hop_table_dev(lb.h2, lb.d_recs.data_ptr(), lb.d_thits.data_ptr(), lb.cp + 4 * CNT_TAG, lb.hit_cap,
                                              lb.d_rows.data_ptr(), lb.d_row_gap.data_ptr(), lb.row_cap, lb.cp + 4 * CNT_ROWS),
                  "gf_second_hop_table_dev")
        if not self.multi:
            rows_p, rowgap_p, nrows_p, rcap, hh = lb.d_rows.data_ptr(), lb.d_row_gap.data_ptr(), lb.cp + 4 * CNT_ROWS, lb.row_cap, lb.h2
        else:
            # the reads are sharded, the second hop is not: a MAPQ-0 record is linked to discordant mates of ANY rank's reads
            # (collect_discordant_low_mapq_reads.py reads the whole discordant_reads_pos file), so the ranks all-gather their
            # rows (fixed-size slots) and every rank merges the union
            if lb.second_stream:
                self._chk(lib.gf_stream_wait(h, lb.h2), "gf_stream_wait")
            ev0 = self._fixed_mark()
            # ONE all-gather: rows (16 B each), their gaps (4 B each) and the row count travel as one packed slot per rank
            # (lb.d_hop_pack: the table kernel writes rows and gaps straight into it), unpacked by three strided device copies
            rc16, pb = lb.row_cap * 16, lb.hop_pack_bytes
            lb.d_hop_pack[pb - 16:pb - 12].copy_(lb.d_cnt[CNT_ROWS:CNT_ROWS + 1].view(torch.uint8))
            SH.all_gather_slots(lb.d_hop_all, lb.d_hop_pack, self.backend)
            pk = lb.d_hop_all.view(world, pb)
            lb.d_rows_all.view(world, rc16).copy_(pk[:, :rc16])
            lb.d_rowgap_all.view(torch.uint8).view(world, lb.row_cap * 4).copy_(pk[:, rc16:rc16 + lb.row_cap * 4])
            lb.d_nrows_all.view(torch.uint8).view(world, 4).copy_(pk[:, pb - 16:pb - 12])
            self._chk(lib.gf_second_hop_table_merge_dev(h, lb.d_rows_all.data_ptr(), lb.d_rowgap_all.data_ptr(), lb.d_nrows_all.data_ptr(), world,
                                                        lb.row_cap, lb.d_rows_u.data_ptr(), lb.d_rowgap_u.data_ptr(), world * lb.row_cap,
                                                        lb.d_nrows_u.data_ptr()), "gf_second_hop_table_merge_dev")
            self._fixed_span("second_hop_union", ev0)
            rows_p, rowgap_p, nrows_p, rcap, hh = lb.d_rows_u.data_ptr(), lb.d_rowgap_u.data_ptr(), lb.d_nrows_u.data_ptr(), world * lb.row_cap, h
        self._chk(lib.gf_tag_low_mapq_table_dev(hh, lb.d_low.data_ptr(), lb.cp + 4 * CNT_LOW, lb.hit_cap, rows_p, nrows_p, rcap,
                                                lb.d_lhits.data_ptr(), lb.hit_cap, lb.cp + 4 * CNT_HOP), "gf_tag_low_mapq_table_dev")
        lb.rowgap_p = rowgap_p
        if hh.value != h.value:
            self._chk(lib.gf_stream_wait(h, lb.h2), "gf_stream_wait")          # pools need the tagger's and the second hop's hits
        self._chk(lib.gf_pool_keys_all_dev(h, lb.d_hits.data_ptr(), lb.cp + 4 * CNT_SCREEN, lb.hit_cap, lb.pull_mates,
                                           lb.d_recs.data_ptr(), lb.d_thits.data_ptr(), lb.cp + 4 * CNT_TAG, lb.hit_cap, lb.d_lhits.data_ptr(),
                                           lb.cp + 4 * CNT_HOP, lb.hit_cap, rowgap_p, lb.d_keys.data_ptr(), lb.key_cap, lb.cp + 4 * CNT_KEYS),
                  "gf_pool_keys_all_dev")

    def build_pools(self, lb, pool_ptr, pool_cap):
        self._chk(self.lib.gf_build_pools_dev(self.h, lb.d_reads.data_ptr(), lb.n_reads, self.L, lb.d_keys.data_ptr(), lb.cp + 4 * CNT_KEYS,
                                              lb.key_cap, pool_ptr, pool_cap, lb.d_pool_off.data_ptr(),
                                              lb.d_ids.data_ptr() if (lb.d_ids is not None and pool_ptr) else None, lb.cp + 4 * CNT_POOLERR),
                  "gf_build_pools_dev")

    def _on_stream(self, fn):
        if self.stream is not None:
            with torch.cuda.stream(self.stream):
                return fn()
        return fn()

    # ---- sizing pass (untimed): second-hop table rows, pooled reads, exchange slots, assembly workspace --------------------
    def prepare(self, strict_screen=False, _depth=0):
        import torch.distributed as dist
        lib, h, dev, world, n_gaps, rb = self.lib, self.h, self.dev, self.world, self.n_gaps, self.rb
        n_lib = len(self.libs)
        assert n_lib >= 1
        if self.gap_span is not None:      # (before the first tagger pass: every pass, the sizing ones included, leaves the records)
            self.gap_span.prepare()
        torch.cuda.synchronize()
        for attempt in range(4):
            self.screen_dropped = 0
            for lb in self.libs:
                self._on_stream(lambda: self.recruit(lb))
                if lb.screen:
                    nd = C.c_size_t(0)
                    self._chk(lib.gf_screen_last_overflow(h, C.byref(nd)), "gf_screen_last_overflow")
                    # reads with more (position, gap) matches than the verification lists (low-complexity reads against hundreds of flanks)
                    self.screen_dropped += nd.value
            self.sync()
            # a library that recruits more than an eighth of its reads (dense gaps, short scaffolds): the device calls report how many hits
            # they found beyond the capacity — the hit buffers grow to that and the pass runs again (the reference has no such bound)
            grown = False
            for lb in self.libs:
                c = lb.d_cnt.cpu().numpy()
                need = max(int(c[CNT_SCREEN]) if lb.screen else 0, int(c[CNT_TAG]), int(c[CNT_LOW]))
                if need > lb.hit_cap:
                    self._alloc_hit_buffers(lb, int(1.25 * need) + 1024)
                    grown = True
            if self.multi:      # (every rank repeats the pass together: the sizes below are all-reduced)
                g_t = torch.tensor([int(grown)], dtype=torch.int64, device=self.coll_dev)
                dist.all_reduce(g_t, op=dist.ReduceOp.MAX)
                grown = bool(int(g_t))
            if not grown:
                break
            torch.cuda.synchronize()
        if strict_screen and self.screen_dropped:
            raise RuntimeError("%d reads were not verified in full by the k-mer screen" % self.screen_dropped)
        for lb in self.libs:
            n_th = int(lb.d_cnt[CNT_TAG])
            self._check_cap(n_th, lb.hit_cap, "tagger hits", lb)
            th = np.frombuffer(lb.d_thits[:n_th * 12].cpu().numpy().tobytes(), dtype=B.TAGHIT)
            lb.row_cap = 2 * int((th["kind"] == B.KIND_DISCORDANT).sum()) + 4096
            if self.multi:
                rc_t = torch.tensor([lb.row_cap], dtype=torch.int64, device=self.coll_dev)
                dist.all_reduce(rc_t, op=dist.ReduceOp.MAX)
                lb.row_cap = int(rc_t)
                lb.d_rows_all = self._u8(world * lb.row_cap * 16)
                lb.d_rowgap_all = torch.empty(world * lb.row_cap, dtype=torch.int32, device=dev)
                lb.d_nrows_all = torch.zeros(world, dtype=torch.int32, device=dev)
                lb.d_rows_u = self._u8(world * lb.row_cap * 16)
                lb.d_rowgap_u = torch.empty(world * lb.row_cap, dtype=torch.int32, device=dev)
                lb.d_nrows_u = torch.zeros(4, dtype=torch.int32, device=dev)
            # (rows, their gaps and — multi-rank runs — the row count in ONE buffer: the slot of the second hop's single all-gather)
            lb.hop_pack_bytes = lb.row_cap * 20 + 16
            lb.d_hop_pack = torch.zeros(lb.hop_pack_bytes, dtype=torch.uint8, device=dev)
            lb.d_rows = lb.d_hop_pack[:lb.row_cap * 16]
            lb.d_row_gap = lb.d_hop_pack[lb.row_cap * 16:lb.row_cap * 20].view(torch.int32)
            if self.multi:
                lb.d_hop_all = torch.zeros(world * lb.hop_pack_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def sizing_pools():
            for lb in self.libs:
                self.hop_and_keys(lb)
                self.build_pools(lb, None, 0)        # offsets only
        self._on_stream(sizing_pools)
        self.sync()
        torch.cuda.synchronize()
        again = False
        for lb in self.libs:      # second-hop hits and pool keys have their own counts: grow for them too, then size everything once more
            n_hop, n_keys = int(lb.d_cnt[CNT_HOP]), int(lb.d_cnt[CNT_KEYS])
            if n_hop > lb.hit_cap or n_keys > lb.key_cap:
                self._alloc_hit_buffers(lb, int(1.25 * max(n_hop, (n_keys + 3) // 4)) + 1024)
                again = True
        if self.multi:
            g_t = torch.tensor([int(again)], dtype=torch.int64, device=self.coll_dev)
            dist.all_reduce(g_t, op=dist.ReduceOp.MAX)
            again = bool(int(g_t))
        if again:
            if _depth >= 3:
                raise RuntimeError("the hit buffers keep overflowing (%s)" % ", ".join("%s: %d" % (lb.name, lb.hit_cap) for lb in self.libs))
            return self.prepare(strict_screen, _depth + 1)
        self.rows_lib = [int(lb.d_pool_off[-1]) for lb in self.libs]
        # largest merged pool (all libraries, all ranks): bounds the assembly's per-workgroup workspace slices
        per_gap = sum((lb.d_pool_off[1:] - lb.d_pool_off[:-1]) for lb in self.libs).to(self.coll_dev)
        if self.multi:
            dist.all_reduce(per_gap, op=dist.ReduceOp.SUM)
        self.per_gap = per_gap.cpu().numpy()
        self.max_pool_rows = int(self.per_gap.max()) if n_gaps else 0
        # bound on the rows of one pool = the workspace slice of the assembly's main launch.  Deeper pools are not an error (they take the
        # assembly's last launch, option asm_big_pool_reads), so the bound needs no safety margin, and where a few repeat gaps hold many
        # times the reads of the others it follows the bulk of the pools, not the deepest one
        self.asm_bound = self.max_pool_rows if self.max_pool_rows <= 4096 else max(4096, int(np.percentile(self.per_gap, 99)))
        self.gf.set_option("asm_max_pool_reads", max(1, self.asm_bound))
        # ... and the slices of that last launch hold the deepest pool actually present (the library's default, 131 072 rows x 8 slices, is
        # 7-9 GB of workspace per context whether or not a pool needs it: ADVICE r4)
        self.gf.set_option("asm_big_pool_reads", max(1, min(0x1FFFFF, self.max_pool_rows)))
        self.lib_cap = max(4096, int(1.25 * max(self.rows_lib)) + 1024)            # rows of one library's pool array
        # local pool arrays: [n_lib][lib_cap] rows (slot l = library l: the source layout of gf_pools_merge_dev)
        self.d_pools = self._u8(n_lib * self.lib_cap * rb + 64)
        self.pool_ptr = [self.d_pools.data_ptr() + l * self.lib_cap * rb for l in range(n_lib)]
        if self.keep_read_ids:
            for lb in self.libs:
                lb.d_ids = torch.empty(self.lib_cap, dtype=torch.int32, device=dev)
        self.d_xerr = torch.zeros(4, dtype=torch.int32, device=dev)
        self.d_libcnt = torch.zeros(n_lib * n_gaps, dtype=torch.int32, device=dev)         # [n_lib][n_gaps]
        if self.multi:
            owner = SH.gap_owner(n_gaps, world).to(dev)
            per_dst = torch.zeros(n_lib, world, dtype=torch.int64, device=dev)
            for l, lb in enumerate(self.libs):
                cnt = (lb.d_pool_off[1:] - lb.d_pool_off[:-1])
                per_dst[l].index_add_(0, owner, cnt)
            mx = per_dst.max().to(self.coll_dev)
            dist.all_reduce(mx, op=dist.ReduceOp.MAX)
            self.slot_cap = max(1024, int(1.25 * int(mx)) + 256)
            tot = torch.stack([per_dst[:, r].sum() for r in range(world)]).to(self.coll_dev)
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
            self.merged_cap = max(4096, int(1.25 * int(tot.max())) + 1024)
            # exact split sizes (default): rows per (source, owner, library) from this sizing pass, the same table on every rank — one
            # all-to-all per step, nothing padded, the counts inside it.  GF_XCHG=slots: equal-sized slots padded to 1.25 x the largest
            # block + an all-gather of the counts (the form of rounds 2-5)
            self.exact_exchange = os.environ.get("GF_XCHG", "exact") != "slots"
            if self.exact_exchange:
                rows = SH.exchange_rows_table(per_dst, self.coll_dev, self.backend)
                self.xchg = SH.ExactOwnerExchange(world, self.rank, n_lib, n_gaps, rows, rb, dev, self.backend)
            else:
                self.xchg = SH.OwnerExchange(world, n_lib, n_gaps, self.slot_cap, rb, dev, self.backend)
            self.xchg_kernels = self._exchange_kernels()
        else:
            self.slot_cap = self.lib_cap
            self.merged_cap = max(4096, int(1.25 * sum(self.rows_lib)) + 1024)
        self.need_merge = self.multi or n_lib > 1
        self.d_merged = self._u8(self.merged_cap * rb + 64) if self.need_merge else None
        self.d_moff = torch.zeros(n_gaps + 1, dtype=torch.int64, device=dev)
        # (contigs: a few dozen per gap and k on an i.i.d. draft; the deep pools of a repeat-bearing draft fragment into many more:
        # room grows with the pooled reads)
        nk = max(1, len(self.kk))
        self._alloc_contig_list(*self.contig_caps(sum(self.rows_lib)))
        self.d_gap_err = torch.zeros(max(1, n_gaps), dtype=torch.int32, device=dev)
        self.d_best = torch.zeros(max(1, n_gaps), dtype=torch.int64, device=dev)
        # assembly counters: 0 contigs (u32), 2-3 contig bases (u64), 4 gaps closed (u32)
        self.d_acnt = torch.zeros(8, dtype=torch.int32, device=dev)
        self.ap = self.d_acnt.data_ptr()
        self.d_mstats = torch.zeros(B.MG_WORDS, dtype=torch.int32, device=dev)      # statistics of the merge round (gf_merge_open_gaps_dev)
        if self.per_contig:        # the picks' two statistics words (their selection per contig: _alloc_contig_list)
            self.d_pstats = torch.zeros(2, dtype=torch.int32, device=dev)
        pr = np.zeros(1, dtype=B.OVL_PARAMS)
        pr[0] = tuple(self.gf.MERGER_PARAMS)[:7] + (0.0,)       # ContigsMerger's options as GAPPadder sets them (MergeContigs.py:75)
        self.merge_params = pr
        self.k_arr = (C.c_int * nk)(*[a for a, _ in self.kk])
        self.kv_arr = (C.c_int * nk)(*[b for _, b in self.kk])
        torch.cuda.synchronize()
        if self.round2 is not None:
            self.round2.prepare()
        if self.closing is not None:
            self.closing.prepare()
        if self.rescue is not None:
            self.rescue.prepare()
        if self.joins is not None:
            self.joins.prepare()
        if self.alts is not None:
            self.alts.prepare()
        if self.ext is not None:        # (after the rounds: either may have grown the contig list its buffer is sized by)
            self.ext.prepare()
        for rnd in self.after_pick:     # (after the rounds: the polish's base buffer takes what the contig bases take)
            rnd.prepare()
        if self.tag_ahead:          # the first step's tagger pass (untimed, like a warm-up step's)
            assert all(lb.second_stream for lb in self.libs), "tag_ahead needs DeviceLibrary(tag_ctx=...)"
            self._on_stream(lambda: [self.tagger(lb) for lb in self.libs])
            self.sync()
        self.prepared = True

    def contig_caps(self, rows):
        """Records and bases of the contig list of an assembly over `rows` pooled reads."""
        nk = max(1, len(self.kk))
        return (64 * self.n_gaps + 4096 + rows // 4) * nk, (24576 * self.n_gaps + (1 << 20) + 32 * rows) * nk

    def _alloc_contig_list(self, contig_cap, seq_cap):
        """The step's contig list: records, bases and (align and gapped mode) the picks' selection per contig."""
        self.contig_cap, self.seq_cap = int(contig_cap), int(seq_cap)
        self.d_ctg = self._u8(self.contig_cap * 32)
        self.d_seq = self._u8(self.seq_cap)
        if self.per_contig:
            self.d_ctg_pick = self._u8(self.contig_cap * B.CTG_PICK.itemsize)

    def _size_round(self, name, grow, tries=8):
        """Sizing of an optional round: the step with the round runs on the hits prepare() left until grow() — which reads the round's
        counters and enlarges what they outgrew — reports that everything fitted."""
        for _ in range(tries):
            torch.cuda.synchronize()
            self._on_stream(lambda: self._step(recruited=True))
            self.sync()
            torch.cuda.synchronize()
            if not grow():
                break
        else:
            raise RuntimeError("%s: the buffers keep growing" % name)
        torch.cuda.synchronize()

    def _exchange_kernels(self):
        """The (pack, merge) pair the chosen exchange form calls (sharding.ExactOwnerExchange.run / OwnerExchange.run)."""
        lib, h, n_gaps, n_lib, L, world = self.lib, self.h, self.n_gaps, len(self.libs), self.L, self.world

        def pack(l, send, cap, cnt):
            self._chk(lib.gf_pools_pack_for_owners_dev(h, self.pool_ptr[l], self.libs[l].d_pool_off.data_ptr(), n_gaps, L, world, self.batch,
                                                       l, n_lib, send.data_ptr(), cap, cnt.data_ptr(), self.d_xerr.data_ptr()),
                      "gf_pools_pack_for_owners_dev")

        def merge(recv, cap, all_cnt):
            self._chk(lib.gf_pools_merge_dev(h, recv.data_ptr(), cap, all_cnt.data_ptr(), n_lib, world, n_gaps, L, self.rank, world,
                                             self.batch, self.d_merged.data_ptr(), self.merged_cap, self.d_moff.data_ptr(), self.d_xerr.data_ptr()),
                      "gf_pools_merge_dev")

        def pack_v(l, send, slot_base, slot_cap, cnt_base, cnt):
            self._chk(lib.gf_pools_pack_for_owners_v_dev(h, self.pool_ptr[l], self.libs[l].d_pool_off.data_ptr(), n_gaps, L, world, self.batch,
                                                         l, n_lib, send.data_ptr(), slot_base.data_ptr(), slot_cap.data_ptr(), cnt_base.data_ptr(),
                                                         cnt.data_ptr(), self.d_xerr.data_ptr()), "gf_pools_pack_for_owners_v_dev")

        def merge_v(recv, slot_base, cnt_base):
            self._chk(lib.gf_pools_merge_v_dev(h, recv.data_ptr(), slot_base.data_ptr(), cnt_base.data_ptr(), n_lib, world, n_gaps, L, self.rank,
                                               world, self.batch, self.d_merged.data_ptr(), self.merged_cap, self.d_moff.data_ptr(),
                                               self.d_xerr.data_ptr()), "gf_pools_merge_v_dev")
        return (pack_v, merge_v) if self.exact_exchange else (pack, merge)

    def _check_cap(self, n, cap, what, lb):
        if n > cap:
            raise RuntimeError("library %s: %d %s exceed the capacity %d (add_library(hit_cap=...))" % (lb.name, n, what, cap))

    # ---- one pass of the hot path (enqueued; no host synchronisation) ------------------------------------------------------
    def _step(self, recruited=False):
        """recruited: the hit lists, second-hop rows and pool keys of the libraries are in place already (the sizing pass just left them:
        finish()) — only the pools are built."""
        lib, h, n_gaps, n_lib, L = self.lib, self.h, self.n_gaps, len(self.libs), self.L
        if not recruited:
            for lb in self.libs:
                self.recruit(lb, tagger=not self.tag_ahead)
        for l, lb in enumerate(self.libs):
            if not recruited:
                self.hop_and_keys(lb)
            self.build_pools(lb, self.pool_ptr[l], self.lib_cap)
        if self.rescue is not None:
            self.rescue.enqueue_keys()        # (they read this step's tagger hits: listed before the next step's tagger rewrites them)
        if self.tag_ahead:
            for lb in self.libs:        # the next step's tagger pass: behind every consumer of this step's hits, beside the assembly
                self._chk(lib.gf_stream_wait(lb.h2, h), "gf_stream_wait")
                self.tagger(lb)
        # (zeroed through the library = on its stream; a torch op here would run on torch's stream)
        self._chk(lib.gf_memset_dev(h, self.d_xerr.data_ptr(), 0, 16) or lib.gf_memset_dev(h, self.d_best.data_ptr(), 0, 8 * max(1, n_gaps))
                  or lib.gf_memset_dev(h, self.ap + 16, 0, 16), "gf_memset_dev")
        if self.per_contig:
            self._chk(lib.gf_memset_dev(h, self.d_ctg_pick.data_ptr(), 0, self.contig_cap * B.CTG_PICK.itemsize)
                      or lib.gf_memset_dev(h, self.d_pstats.data_ptr(), 0, 8), "gf_memset_dev")
        if not self.need_merge:
            self.asm_ptr, self.asm_off, self.asm_rows = self.pool_ptr[0], self.libs[0].d_pool_off.data_ptr(), self.lib_cap
        else:
            if not self.multi:
                for l, lb in enumerate(self.libs):
                    self._chk(lib.gf_pool_counts_dev(h, lb.d_pool_off.data_ptr(), n_gaps, self.d_libcnt.data_ptr() + 4 * l * n_gaps), "gf_pool_counts_dev")
                self._chk(lib.gf_pools_merge_dev(h, self.d_pools.data_ptr(), self.lib_cap, self.d_libcnt.data_ptr(), n_lib, 1, n_gaps, L, 0, 1, self.batch,
                                                 self.d_merged.data_ptr(), self.merged_cap, self.d_moff.data_ptr(), self.d_xerr.data_ptr()),
                          "gf_pools_merge_dev")
            else:
                # the one exchange step: rows regrouped by owner rank, counts all-gathered, slots all-to-all'ed
                # (equal-sized slots: no host sizes, no host sync), owners merge in (library, source rank) order
                ev0 = self._fixed_mark()
                self.xchg.run(*self.xchg_kernels)
                self._fixed_span("owner_exchange", ev0)
            self.asm_ptr, self.asm_off, self.asm_rows = self.d_merged.data_ptr(), self.d_moff.data_ptr(), self.merged_cap
        if self.kk and self.assemble_in_step:
            self.assemble()

    def assemble(self, d_nmask=None):
        """Assembly of the pools the step left (every (k, kv) pair) + flank anchoring; also callable on its own after the pools
        changed (a second recruitment round, assemble_gaps.py:349-351)."""
        lib, h = self.lib, self.h
        self._chk(lib.gf_assemble_multi_dev(h, self.asm_ptr, d_nmask, self.asm_off, self.n_gaps, self.asm_rows, self.L, self.k_arr, self.kv_arr,
                                            len(self.kk), self.min_count, self.min_contig, self.d_ctg.data_ptr(), self.contig_cap, self.ap,
                                            self.d_seq.data_ptr(), self.seq_cap, self.ap + 8, self.d_gap_err.data_ptr()), "gf_assemble_multi_dev")
        # which gaps are closed: both flanks anchored on one contig (pick_contigs.py:64-358; scores 30 then 15, assemble_gaps.py:336, 365)
        self._pick(*self.anchor_pair)
        if self.merge_in_step:
            # the open gaps' contigs through the contig merger, merged contigs appended (k = kv = 0), second pick over THEM only
            self._chk(lib.gf_merge_open_gaps_dev(h, self.d_ctg.data_ptr(), self.ap, self.contig_cap, self.d_seq.data_ptr(), self.ap + 8, self.seq_cap,
                                                 self.d_best.data_ptr(), self.n_gaps, B._p(self.merge_params), 10, self.merge_max_set,
                                                 self.k_arr, self.kv_arr, min(16, len(self.kk)), self.d_mstats.data_ptr()), "gf_merge_open_gaps_dev")
            self._pick(*self.anchor_pair, first=self.d_mstats.data_ptr() + 4 * B.MG_N0)
        if self.round2 is not None:
            self.round2.enqueue()
        if self.rescue is not None:
            self.rescue.enqueue()
        if self.joins is not None:
            self.joins.enqueue()
        if self.alts is not None:
            self.alts.enqueue()
        if self.ext is not None:
            self.ext.enqueue()
        # (neither the rescue's nor the extension's launches change d_best after the rescue's pick; every round here reads the step's
        # contigs and picks and writes buffers of its own; the pair span runs per library, on the libraries' own pools, ids and masks)
        if self.closing is not None:    # (the pool of every closed gap as its closing round assembled it: what the rounds below read)
            self.closing.enqueue(d_nmask)
        for rnd in self.after_pick:
            rnd.enqueue(d_nmask)

    def _pick(self, a_long, a_short, first=None, own=None):
        """One pick in the Pipeline's anchor mode over the contigs from index *first on (a device address; None: all of them) of the step's
        list — read when the call is enqueued: a caller may have changed the capacities — or of `own` = (contigs, their counter, capacity,
        bases, pick words, closed counter, selection per contig, statistics: the last two in align and gapped mode) device addresses."""
        if own is None:
            own = (self.d_ctg.data_ptr(), self.ap, self.contig_cap, self.d_seq.data_ptr(), self.d_best.data_ptr(), self.ap + 16) \
                + ((self.d_ctg_pick.data_ptr(), self.d_pstats.data_ptr()) if self.per_contig else ())
        what = PICKS[self.anchor_mode][0 if first is None else 1]
        self._chk(getattr(self.lib, what)(self.h, *own[:4], a_long, a_short, *(() if first is None else (first,)), *own[4:]), what)

    def step(self, n=1):
        assert self.prepared, "Pipeline.prepare() first"
        def run():
            for _ in range(n):
                self._step()
        self._on_stream(run)

    def finish(self):
        """A one-shot run (the CLI): prepare() has recruited every library once to size the buffers, and its hits and pool keys are still
        there — build the pools from them (and assemble, unless assemble_in_step is off) instead of recruiting a second time."""
        assert self.prepared, "Pipeline.prepare() first"
        self._on_stream(lambda: self._step(recruited=True))

    def barrier(self):
        self.sync()
        torch.cuda.synchronize()
        if self.multi:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    # ---- results of the last step -----------------------------------------------------------------------------------------
    def fetch(self, pools=False):
        """Synchronises and copies the last step's results to the host; raises on any overflow flag."""
        self.sync()
        torch.cuda.synchronize()
        r = Results()
        acnt = self.d_acnt.cpu().numpy()
        r.n_contigs, r.n_seq, r.n_closed = int(acnt[0]), counter_u64(acnt), int(acnt[4])
        xerr = int(self.d_xerr[0])
        for lb in self.libs:
            c = lb.d_cnt.cpu().numpy()
            lb.counts = {"screen_hits": int(c[CNT_SCREEN]) if lb.screen else 0, "tagger_hits": int(c[CNT_TAG]), "second_hop_hits": int(c[CNT_HOP]),
                         "pool_keys": int(c[CNT_KEYS]), "pooled_reads": int(lb.d_pool_off[-1])}
            for n_, cap, what in ((lb.counts["screen_hits"], lb.hit_cap, "screen hits"), (int(c[CNT_TAG]), lb.hit_cap, "tagger hits"),
                                  (int(c[CNT_HOP]), lb.hit_cap, "second-hop hits"), (int(c[CNT_KEYS]), lb.key_cap, "pool keys"),
                                  (int(c[CNT_LOW]), lb.hit_cap, "MAPQ-0 records"), (int(c[CNT_ROWS]), lb.row_cap, "second-hop rows")):
                self._check_cap(n_, cap, what, lb)
            if int(c[CNT_POOLERR]):
                raise RuntimeError("library %s: pool buffer too small (flag %#x)" % (lb.name, int(c[CNT_POOLERR]) & 0xFFFFFFFF))
        n_err = int(self.d_gap_err.sum())
        if xerr or n_err or r.n_contigs > self.contig_cap or r.n_seq > self.seq_cap:
            raise RuntimeError("step overflow: exchange/merge flag %#x, %d gap errors, %d contigs (cap %d), %d contig bases (cap %d)"
                               % (xerr & 0xFFFFFFFF, n_err, r.n_contigs, self.contig_cap, r.n_seq, self.seq_cap))
        if self.merge_in_step and self.kk:
            ms = self.d_mstats.cpu().numpy().view(np.uint32)
            if int(ms[B.MG_ERR]):
                raise RuntimeError("merge round: capacity flags %#x" % int(ms[B.MG_ERR]))
            r.merge = {"gaps_tried": int(ms[B.MG_N_SETS]), "gaps_skipped_large": int(ms[B.MG_SKIPPED]), "gaps_skipped_graph": int(ms[B.MG_SKIPPED_GRAPH]), "candidate_pairs": int(ms[B.MG_N_PAIRS]),
                       "edges": int(ms[B.MG_N_EDGES]), "new_contigs": int(ms[B.MG_N_JOBS]), "gaps_with_new_contigs": int(ms[B.MG_SETS_WITH_JOBS]),
                       "contigs_before": int(ms[B.MG_N0])}
        r.asm_off_t = self.d_moff if self.need_merge else self.libs[0].d_pool_off
        r.asm_pool_t = self.d_merged if self.need_merge else self.d_pools
        r.asm_rows_total = int(r.asm_off_t[-1])
        r.contigs = np.frombuffer(self.d_ctg[:r.n_contigs * 32].cpu().numpy().tobytes(), dtype=B.CONTIG)
        r.seq = self.d_seq[:r.n_seq].cpu().numpy().tobytes()
        r.best = self.d_best[:self.n_gaps].cpu().numpy().view(np.uint64)
        r.anchor_mode, r.ctg_pick, r.align_dropped, r.align_seed_overflow = self.anchor_mode, None, 0, 0
        if self.per_contig:
            r.ctg_pick = np.frombuffer(self.d_ctg_pick[:r.n_contigs * B.CTG_PICK.itemsize].cpu().numpy().tobytes(), dtype=B.CTG_PICK)
            r.align_dropped, r.align_seed_overflow = (int(x) for x in self.d_pstats.cpu().numpy())
        if self.rescue is not None:
            self.rescue.fetch(r)
        if r.merge is not None:      # gaps whose winning contig is a merged one (of the merge round: the rescue's records come after them)
            idx = pick_index(r.best)
            end = r.rescue_first if r.rescue_first is not None else np.iinfo(np.int64).max
            r.merge["gaps_closed_by_merging"] = int(((r.best != 0) & (idx >= r.merge["contigs_before"]) & (idx < end)).sum())
        if self.round2 is not None:
            self.round2.fetch(r)
        if self.closing is not None and self.kk:
            self.closing.fetch(r, pools)
        if self.joins is not None and self.kk:
            self.joins.fetch(r)
        if self.alts is not None and self.kk:
            self.alts.fetch(r)
        if self.ext is not None and self.kk:
            self.ext.fetch(r)
        for rnd in self.after_pick if self.kk else ():
            rnd.fetch(r)
        if self.gap_span is not None:
            self.gap_span.fetch(r)
        if pools:
            r.pool_off = r.asm_off_t.cpu().numpy().astype(np.int64)
            r.pool_rows = r.asm_pool_t[:r.asm_rows_total * self.rb].cpu().numpy().reshape(-1, self.rb)
            if self.pairs is not None:        # the libraries' own pools and read ids: what pair_span_of_results reads
                r.lib_pool_off = [lb.d_pool_off.cpu().numpy().astype(np.int64) for lb in self.libs]
                r.lib_pool_rows = [self.d_pools[l * self.lib_cap * self.rb:(l * self.lib_cap + int(o[-1])) * self.rb].cpu().numpy().reshape(-1, self.rb)
                                   for l, o in enumerate(r.lib_pool_off)]
                r.lib_pool_ids = [lb.d_ids[:int(o[-1])].cpu().numpy().view(np.uint32) for lb, o in zip(self.libs, r.lib_pool_off)]
            if self.anchored is not None:      # the libraries' tagger hits, clamped to the count: what anchors_of_results reads
                r.lib_taghits = [np.frombuffer(lb.d_thits[:min(lb.counts["tagger_hits"], lb.hit_cap) * 12].cpu().numpy().tobytes(), dtype=B.TAGHIT)
                                 for lb in self.libs]
        return r

    def extended_sequences(self, res):
        """The partial fills of the last step (extended_fill): {gap: (left contig index or -1, right contig index or -1, fill or None,
        picked_contigs text or None)} for every gap with a contig on either side — pick_extended_sequence's fields with contig indices for
        names (pick_contigs.decode_extended); the fill is the device's, checked against its record's slices."""
        from .pick_contigs import decode_extended
        if res.ext is None:
            raise ValueError("extended_sequences needs the Results of a Pipeline(extended_fill=True) step")
        out = {}
        for g in np.nonzero((res.ext["left"] != B.EXT_NONE) | (res.ext["right"] != B.EXT_NONE))[0]:
            rec = res.ext[g]
            d = decode_extended(rec, lambda i: contig_text(res, i))
            dev = res.ext_bases[int(rec["off"]):int(rec["off"]) + int(rec["len"])].decode() if int(rec["len"]) else None
            if dev != d[2]:
                raise RuntimeError("gap %d: the device's fill does not match its record" % g)
            out[int(g)] = d
        return out

    def joined_gaps(self, res):
        """{gap: overlap} of the usable flank-overlap joins of the last step (flank_joins.usable)."""
        if res.joins is None:
            raise ValueError("joined_gaps needs the Results of a Pipeline(flank_joins=True) step")
        return {int(g): int(res.joins[g]["overlap"]) for g in np.nonzero(res.joins["overlap"])[0] if FJ.usable(res.joins[g])}

    def alternative_sequences(self, res):
        """{gap: (rival contig index, the rival's gap sequence, reverse?)} of the contested gaps of the last step (fill_alternatives.contested):
        the rival's sequence cut as picked_sequences cuts the winner's (_contig_cut)."""
        from .pick_contigs import revcomp
        if res.alts is None:
            raise ValueError("alternative_sequences needs the Results of a Pipeline(alternatives=True) step")
        out = {}
        for g in np.nonzero(res.alts["flags"] & B.FA_F_HAS_RIVAL)[0]:
            rec = res.alts[g]
            ci, first, end, flip, rev = Pipeline._contig_cut(self, res, g, int(rec["rival"]), int(rec["level"]), bool(int(rec["flags"]) & B.FA_F_RIVAL_REVERSE))
            body = contig_text(res, ci)[first:end]
            out[int(g)] = (ci, revcomp(body) if flip else body, rev)
        return out

    def adjudicated_sequences(self, res):
        """{gap: (gap sequence, "picked" | "rival")} of every closed gap of the last step: picked_sequences' text, and
        alternative_sequences' text where the adjudication's verdict is SWITCH."""
        if res.adjudication is None:
            raise ValueError("adjudicated_sequences needs the Results of a Pipeline(alternatives=True, adjudicate=True) step")
        rivals = self.alternative_sequences(res)
        out = {g: (text, "picked") for g, (_, text, _) in self.picked_sequences(res).items()}
        for g in np.nonzero(res.adjudication["verdict"] == B.AJ_SWITCH)[0]:
            out[int(g)] = (rivals[int(g)][1], "rival")
        return out

    def merge_open_gaps(self, res, max_set=128):
        """The reference merges a gap's contigs BEFORE it picks (assemble_gaps.py:301-306, 335-339: run_contigs_merge, then
        pick_full_constructed_contigs); the step picks first, so only the gaps that pick left open can gain from merging: their
        contigs go through the contig merger (MergeContigs.merge_sets: exact-containment dedup, all-pairs prefilter + overlap
        evaluation on the GPU, path search on the host) and the NEW_CONTIG_MERGE sequences through a second pick on the device.
        res: fetch()'s Results.  Returns {"gaps_tried", "gaps_with_new_contigs", "new_contigs", "closed": {gap: (anchor, span + 1,
        index into "contigs", reverse)}, "contigs": [(gap, seq)]}.  Gaps with more than max_set contigs after the dedup are left alone
        ("gaps_skipped_large"): the contig graph of a repeat-bearing gap has thousands of paths (C2 with planted repeats and mate pairs:
        53 641 merged strings for 176 gaps, 158 s on the host, and 50 of the 174 gaps they close are closed with a wrong sequence)."""
        from .MergeContigs import MAX_SET, drop_contained, merge_sets
        ctg = res.contigs
        open_gaps = np.nonzero(res.best == 0)[0]
        order = np.argsort(ctg["gap"], kind="stable")
        gs = ctg["gap"][order]
        lo, hi = np.searchsorted(gs, open_gaps), np.searchsorted(gs, open_gaps, side="right")
        sets, gaps_of, skipped = [], [], 0
        for g, a, z in zip(open_gaps, lo, hi):
            if z - a >= 2:
                recs = [("c%d" % i, contig_text(res, i)) for i in order[a:z]]
                recs = drop_contained(recs) if len(recs) <= MAX_SET else recs
                if 2 <= len(recs) <= min(MAX_SET, max_set):
                    sets.append(recs)
                    gaps_of.append(int(g))
                elif len(recs) > max_set:
                    skipped += 1
        out = {"gaps_tried": len(sets), "gaps_skipped_large": skipped, "gaps_with_new_contigs": 0, "new_contigs": 0, "closed": {}, "contigs": []}
        if not sets:
            return out
        new = []
        for g, m in zip(gaps_of, merge_sets(self.gf, sets)):
            out["gaps_with_new_contigs"] += bool(m["new"])
            new += [(g, s) for _, s, _ in m["new"]]
        out["new_contigs"], out["contigs"] = len(new), new
        if not new:
            return out
        c2 = np.zeros(len(new), dtype=B.CONTIG)
        off = 0
        for i, (g, s) in enumerate(new):
            c2[i] = (g, 0, 0, 0, len(s), 0, 0, off)
            off += len(s)
        d_c2 = torch.from_numpy(c2.view(np.uint8).copy()).to(self.dev)
        d_s2 = torch.from_numpy(np.frombuffer("".join(s for _, s in new).encode(), dtype=np.uint8).copy()).to(self.dev)
        d_b2 = torch.zeros(max(1, self.n_gaps), dtype=torch.int64, device=self.dev)
        d_n2 = torch.tensor([len(new), 0, 0, 0], dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize()
        own = (d_c2.data_ptr(), d_n2.data_ptr(), len(new), d_s2.data_ptr(), d_b2.data_ptr(), d_n2.data_ptr() + 8)
        if self.per_contig:
            d_p2 = torch.zeros(len(new) * B.CTG_PICK.itemsize, dtype=torch.uint8, device=self.dev)
            d_st2 = torch.zeros(2, dtype=torch.int32, device=self.dev)
            torch.cuda.synchronize()
            own += (d_p2.data_ptr(), d_st2.data_ptr())
        self._pick(*self.anchor_pair, own=own)
        self.gf.sync()
        b2 = d_b2[:self.n_gaps].cpu().numpy().view(np.uint64)
        out["closed"] = {int(g): decode_best(b2[g]) for g in np.nonzero(b2)[0]}
        if self.per_contig:       # (the selections of the merged contigs, indexed like "contigs")
            out["ctg_pick"] = np.frombuffer(d_p2.cpu().numpy().tobytes(), dtype=B.CTG_PICK)
            out["align_dropped"], out["align_seed_overflow"] = (int(x) for x in d_st2.cpu().numpy())
        out["arrays"] = (c2, "".join(s for _, s in new).encode(), b2)       # the second pick's contig table, bases and pick words
        return out

    def _pick_cut(self, res, g):
        """(contig index, first, end, reverse-complement the cut?, the word's strand) of the gap sequence of closed gap g on its winning
        contig as stored: contig[first:end], reverse-complemented for a reverse selection, is what ContigsSelection writes (pick_contigs.py:341-349).  "align" and "gapped": from
        the contig's selection in res.ctg_pick; "exact": the host picker's selection (pick_contigs.select_full over the exact anchors' hits)
        on the winning contig alone, at the word's anchor length, with the flanks given to gf_set_gaps."""
        a_len, span1, ci, rev = decode_best(res.best[g])
        return Pipeline._contig_cut(self, res, g, ci, a_len, rev)      # (by the class: a stand-in for `self` needs its .gf alone)

    def _contig_cut(self, res, g, ci, a_len, rev):
        """_pick_cut's rule for any contig ci of gap g with a selection at anchor length a_len on strand rev (the winner; a rival)."""
        from .pick_contigs import select_full, stand_in_hits
        if res.ctg_pick is not None:
            p = res.ctg_pick[ci]
            lp, rp, lm, rm = int(p["lp"]), int(p["rp"]), int(p["lm"]), int(p["rm"])
            assert int(p["threshold"]) == a_len and int(p["reverse"]) == rev, (int(g), p, a_len, rev)
        else:
            if self.gf.flanks is None:
                raise ValueError("picked_sequences in exact mode needs the flanks given to gf_set_gaps")
            l, r = self.gf.flanks[g]
            sel = select_full(stand_in_hits("exact", [("c", contig_text(res, ci))], l, r, a_len))
            if sel is None:
                raise RuntimeError("gap %d: the host picker does not confirm the device's pick" % g)
            _, lp, rp, lm, rm, cut_rev = sel
            return (int(ci), rp + rm - 1, lp, True, bool(rev)) if cut_rev else (int(ci), lp + lm - 1, rp, False, bool(rev))
        return (int(ci), rp + rm - 1, lp, True, True) if rev else (int(ci), lp + lm - 1, rp, False, False)

    def picked_sequences(self, res):
        """The gap sequence of every gap the step closed, cut from its winning contig as ContigsSelection writes it to picked_seqs.fa
        (_pick_cut): {gap: (contig index, gap sequence, reverse?)}."""
        from .pick_contigs import revcomp
        out = {}
        for g in np.nonzero(res.best)[0]:
            ci, first, end, flip, rev = self._pick_cut(res, g)
            body = contig_text(res, ci)[first:end]
            out[int(g)] = (ci, revcomp(body) if flip else body, rev)
        return out

    def polished_sequences(self, res):
        """picked_sequences after the polish round: {gap: (contig index, polished gap sequence, reverse?)} — the same cut, taken at the
        coordinates the UNPOLISHED contig gives (_pick_cut) and applied to the polished contig, which has the same length; the cut is
        not searched again on the polished text.  With polish_indels the polished contig may differ in length: the cut is [b0, b1 + 1) of
        the body the round located, every edit lies in [b0, b1], so the cut's end moves by the difference and its start stays."""
        from .pick_contigs import revcomp
        if res.polish is None:
            raise ValueError("polished_sequences needs the Results of a Pipeline(polish=True) step")
        out = {}
        for g in np.nonzero(res.best)[0]:
            ci, first, end, flip, rev = self._pick_cut(res, g)
            text = POL.polished_text(res, g)
            if res.polish.dtype == B.FILL_POLISH_GAPPED:
                body = SUP.locate(res.best[g], contig_text(res, ci), self.gf.flanks[g] if self.gf.flanks is not None else None,
                                   res.ctg_pick[ci] if res.ctg_pick is not None else None)
                assert body is not None and first == body[0], (int(g), first, end, body)
                end += len(text) - int(res.contigs[ci]["length"])
            elif len(text) != int(res.contigs[ci]["length"]):
                raise RuntimeError("gap %d: the polished contig has %d bases, the contig %d" % (g, len(text), int(res.contigs[ci]["length"])))
            out[int(g)] = (ci, revcomp(text[first:end]) if flip else text[first:end], rev)
        return out

    def fill_confidence(self, res):
        """picked_sequences with the pile-up track of every base: {gap: (contig index, gap sequence, entries [len(sequence), 8] u16,
        reverse?)} — the cut of _pick_cut taken from the gap's track and turned the way the sequence is written (pileup.oriented), so
        that entry i belongs to base i.  A gap whose contig the round skipped (long, non-ACGT) has None for its entries."""
        from . import pileup as PU
        if res.pileup is None or res.pileup_track is None:
            raise ValueError("fill_confidence needs the Results of a Pipeline(pileup=True) step with its track")
        from .pick_contigs import revcomp
        out = {}
        for g in np.nonzero(res.best)[0]:            # (one _pick_cut per gap: text and track are cut from the same coordinates)
            ci, first, end, flip, rev = self._pick_cut(res, g)
            body, track = contig_text(res, ci)[first:end], PU.track_of(res, g)
            out[int(g)] = (ci, revcomp(body) if flip else body, PU.oriented(track[first:end], flip) if track is not None else None, rev)
        return out

    def fixed_ms(self, steps):
        out = {}
        for name, e0, e1 in self.fixed_spans:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1) / steps
        return out


def pick_index(best):
    """Index of the winning contig of a gap_best word (an int) or of an array of them (u64)."""
    return 0x7FFFFFFF - ((best >> 1) & 0x7FFFFFFF)


def decode_best(b):
    """gap_best word (gf_pick_anchored_dev) -> (anchor length, span + 1, contig index, reverse strand?)."""
    b = int(b)
    return b >> 56, (b >> 32) & 0xFFFFFF, pick_index(b), b & 1


def counter_u64(a, word=2):
    """The u64 in words `word`, `word + 1` of a fetched array of 32-bit counters (the assembly's counters keep the contig bases in 2-3)."""
    return int(a[word:word + 2].view(np.uint64)[0])


def contig_text(res, i):
    """Bases of contig i of a Results."""
    c = res.contigs[i]
    return res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])].decode()
