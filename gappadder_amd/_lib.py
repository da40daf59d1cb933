"""ctypes binding of libgapfill_hip.so (include/gapfill_hip.h).  There is NO fallback: if the HIP library is
missing or fails to load, importing any compute entry point raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgapfill_hip.so")

GAP = np.dtype([("scaffold", "<u4"), ("start", "<u4"), ("end", "<u4"), ("idx_in_scaffold", "<u4")])
ALNREC = np.dtype([("pos", "<u4"), ("mate_pos", "<u4"), ("tlen", "<i4"), ("ref", "<u4"), ("mate_ref", "<u4"),
                   ("flag", "<u2"), ("mapq", "u1"), ("clipflag", "u1"), ("read", "<u8")])
TAGHIT = np.dtype([("rec", "<u4"), ("gap", "<u4"), ("kind", "<u2"), ("to_mate", "<u2")])
DPOS = np.dtype([("mate_scaffold", "<u4"), ("mate_pos", "<u4"), ("src_scaffold", "<u4"), ("src_gap", "<u4")])
HIT = np.dtype([("gap", "<u4"), ("read", "<u4")])
CONTIG = np.dtype([("gap", "<u4"), ("k", "<u2"), ("kv", "<u2"), ("n_nodes", "<u4"), ("length", "<u4"), ("cov_sum", "<u4"),
                   ("reserved", "<u4"), ("seq_off", "<u8")])
SYNTH_CFG = np.dtype([("seed", "<u8"), ("scaffold_len", "<u8"), ("n_scaffolds", "<u4"), ("gaps_per_scaffold", "<u4"),
                      ("gap_len", "<u4"), ("read_len", "<u4"), ("insert_mean", "<u4"), ("insert_sd", "<u4"),
                      ("err_q16", "<u4"), ("mapq0_q16", "<u4"), ("chimeric_q16", "<u4"), ("flank_len", "<u4"),
                      ("library", "<u4"), ("repeats", "<u4")])
CTG_PICK = np.dtype([("lp", "<u4"), ("rp", "<u4"), ("lm", "<u2"), ("rm", "<u2"), ("reverse", "u1"), ("threshold", "u1"), ("reserved", "<u2")])
QCPAIR = np.dtype([("set", "<u4"), ("i", "<u4"), ("j", "<u4")])
# the extended fill's record per gap (gf_ext_pick): contig per side (EXT_NONE: none), the slices of the two parts, the fill's place
EXT_PICK = np.dtype([("left", "<u4"), ("right", "<u4"), ("l_beg", "<u4"), ("l_len", "<u4"), ("r_beg", "<u4"), ("r_len", "<u4"), ("off", "<u8"),
                     ("len", "<u4"), ("l_rev", "u1"), ("r_rev", "u1"), ("reserved", "<u2")])
EXT_NONE = 0xFFFFFFFF
OVL_PARAMS = np.dtype([("mismatch", "<f8"), ("indel", "<f8"), ("max_clip", "<f8"), ("frac_min_overlap", "<f8"), ("frac_loss", "<f8"),
                       ("min_overlap", "<f8"), ("min_overlap_scaffold", "<f8"), ("relax", "<f8")])
OVL_RESULT = np.dtype([(n, "<i4") for n in ("res", "row_end", "col_end", "nclip", "score", "contained", "merged_len", "overlap",
                                            "containment", "first_goes_first")])
assert CONTIG.itemsize == 32 and EXT_PICK.itemsize == 40 and GAP.itemsize == 16 and ALNREC.itemsize == 32 and TAGHIT.itemsize == 12 and DPOS.itemsize == 16 and HIT.itemsize == 8

GF_OK, GF_E_INVAL, GF_E_NODEV, GF_E_NOMEM, GF_E_NOSPACE, GF_E_STATE, GF_E_UNSUPPORTED, GF_E_FORMAT = 0, -1, -2, -3, -4, -5, -6, -7
KIND_CLIP, KIND_DISCORDANT, KIND_UNMAP, KIND_LOWMAPQ = 0, 1, 2, 3
KIND_NAMES = {KIND_CLIP: "clip", KIND_DISCORDANT: "discordant", KIND_UNMAP: "unmap"}
KERNEL_SCREEN, KERNEL_TAG, KERNEL_LOWMAPQ, KERNEL_ASSEMBLE, KERNEL_POOL, KERNEL_SYNTH, KERNEL_COUNT, KERNEL_VERIFY, KERNEL_INGEST, KERNEL_PICK, KERNEL_MERGE, KERNEL_SUPPORT, KERNEL_POLISH, KERNEL_PAIRS, KERNEL_ANCHORS, KERNEL_GAPSPAN, KERNEL_POLISH_GAPPED, KERNEL_PILEUP, KERNEL_JOIN, KERNEL_ALT, KERNEL_ADJ = range(21)

# words of the merge round's statistics (gf_merge_open_gaps_dev, u32[32])
MG_N_PRE, MG_N_SETS, MG_SKIPPED, MG_N_PAIRS, MG_QC_FLAGS, MG_N_JOBS, MG_ERR, MG_N0, MG_N_EDGES, MG_SETS_WITH_JOBS = range(10)
MG_SKIPPED_GRAPH = 16
MG_WORDS = 32

# the merge round with its graph exported (gf_merge_sets, merge_export.hip): records, set statuses, statistics words (u32[16]), capacity flags
MSET = np.dtype([(n, "<u4") for n in ("status", "n_kept", "n_edges", "edge_off", "n_new", "new_off", "final_off", "n_truncated")])
MEDGE = np.dtype([(n, "<u4") for n in ("i", "j", "mode", "overlap")])
MNEW = np.dtype([("set", "<u4"), ("n_nodes", "<u4"), ("path_off", "<u4"), ("length", "<u4"), ("seq_off", "<u8")])
assert MSET.itemsize == 32 and MEDGE.itemsize == 16 and MNEW.itemsize == 24
MSET_MERGED, MSET_NOTHING, MSET_SIZE, MSET_GRAPH = range(4)
MSET_NAMES = {MSET_MERGED: "merged", MSET_NOTHING: "nothing", MSET_SIZE: "size", MSET_GRAPH: "graph"}
(MX_TRIED, MX_NOTHING, MX_SKIPPED_SIZE, MX_SKIPPED_GRAPH, MX_PAIRS, MX_EDGES, MX_PATHS, MX_TRUNCATED, MX_FLAGS, MX_PATH_BYTES, MX_FINALS,
 MX_ROUND_ERR, MX_SEQ_BYTES) = range(13)
MX_NEW_RECORDS, MX_EDGE_RECORDS, MX_WORDS = 14, 15, 16

# words of the second round's statistics (round2.hip, u32[16])
R2_KMERS, R2_TAB_FULL, R2_HITS, R2_UNIQUE, R2_TRIED, R2_WITH, R2_ROWS, R2_FIRST, R2_APPEND_ERR, R2_N2, R2_POOL_OVF = 0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11
R2_NEW, R2_GROWN, R2_GATED = 12, 13, 14          # rounds 2 and later (round_n.hip): one block of R2_WORDS per round
R2_WORDS, R2_MAX_LIBS = 16, 16
# the closing pools (closing_pools.hip, u32[CP_WORDS] statistics): rows needed (u64), gaps with a pool, recruited rows copied, overflow
CP_ROWS, CP_GAPS, CP_RECRUITED, CP_OVF, CP_WORDS, CP_NO_ID = 0, 2, 3, 4, 8, 0xFFFFFFFF

# the rescue round (rescue.hip, u32[16] statistics): marker of the bridge records (k = kv = RESCUE_MARK), the words of the statistics
RESCUE_MARK = 0xFFFF
RS_TRIED, RS_HQ_KEYS, RS_HQ, RS_WINDOWS, RS_TAB_FULL, RS_SEEDS, RS_PLACE_OVF, RS_GAPS_BRIDGED, RS_BRIDGES, RS_FIRST, RS_APPEND_ERR, RS_LONG = range(12)
RS_WORDS = 16

# words of the extended fill's statistics (gf_pick_extended_dev, u32[12]): fills (left only, right only, both sides), u64 bases, overflow flag
EXT_EXTENDED, EXT_LEFT_ONLY, EXT_RIGHT_ONLY, EXT_BOTH, EXT_BASES, EXT_OVERFLOW, EXT_ALIGN_DROPPED, EXT_ALIGN_SEED_OVERFLOW = 0, 1, 2, 3, 4, 6, 8, 9
EXT_WORDS, EXT_MAX_PAIRS = 12, 32

# the read support of the closed gaps (gf_fill_support_dev): the record per gap and the words of its statistics (u32[4]): gaps evaluated,
# closed gaps whose contig does not carry the word's pick, u64 windows evaluated
FILL_SUPPORT = np.dtype([("n_windows", "<u4"), ("n_zero", "<u4"), ("n_below", "<u4"), ("min", "<u4"), ("max", "<u4"), ("zero_run", "<u4"),
                         ("sum", "<u8")])
assert FILL_SUPPORT.itemsize == 32
FS_GAPS, FS_MISMATCH, FS_WINDOWS, FS_WORDS = 0, 1, 2, 4

# the consensus polish of the closed gaps (gf_fill_polish_dev): the record per gap, its flags, the longest contig the kernel polishes and
# the words of its statistics (u32[16]): gaps polished, closed gaps whose contig does not carry the word's pick, gaps skipped for a
# contig too long / with a byte that is no base, then u64 each: changed columns, placed rows, ambiguous rows, output bases; overflow
FILL_POLISH = np.dtype([("off", "<u8"), ("len", "<u4"), ("flags", "<u4"), ("n_cols", "<u4"), ("n_changed", "<u4"), ("n_uncovered", "<u4"),
                        ("reads_placed", "<u4"), ("reads_ambiguous", "<u4"), ("reserved", "<u4")])
assert FILL_POLISH.itemsize == 40
PL_F_LONG, PL_F_NON_ACGT, PL_F_OVERFLOW = 1, 2, 4
PL_MAX_CONTIG = 8192
PL_GAPS, PL_MISMATCH, PL_SKIPPED_LONG, PL_SKIPPED_NON_ACGT, PL_CHANGED, PL_PLACED, PL_AMBIGUOUS, PL_BASES, PL_OVERFLOW, PL_WORDS = 0, 1, 2, 3, 4, 6, 8, 10, 12, 16

# the indel-aware polish (gf_fill_polish_gapped_dev): the record — FILL_POLISH's 40 bytes, then the event counts —, its two flags, the
# caps on distinct events and inserted bases per contig, and the statistics words beyond PL_*'s (u32[32]): u64 each accepted events,
# inserted bases, deleted columns, rows placed split; gaps flagged EVENTS / INS_CAP
FILL_POLISH_GAPPED = np.dtype(FILL_POLISH.descr + [(n, "<u4") for n in ("n_events", "n_inserted", "n_deleted", "reads_split", "events_seen",
                                                                        "events_outside")])
assert FILL_POLISH_GAPPED.itemsize == 64
PL_F_EVENTS, PL_F_INS_CAP = 8, 16
PLG_MAX_EVENTS, PLG_MAX_INSERTED, PLG_MAX_INDEL = 64, 64, 16
PLG_EVENTS, PLG_INSERTED, PLG_DELETED, PLG_SPLIT, PLG_F_EVENTS, PLG_F_INS_CAP, PLG_WORDS = 16, 18, 20, 22, 24, 25, 32

# the per-base pile-up of the closed gaps (gf_fill_pileup_dev): the record per gap (72 bytes), the track entry of a contig column (u16
# fwd[4], rev[4]: a row of a [entries, 8] u16 array), the flags and the words of its statistics (u32[16]): gaps piled up, closed gaps whose
# contig does not carry the word's pick, gaps skipped for a contig too long / with a byte that is no base, then u64 each: placed rows,
# ambiguous rows, track entries handed out, low body columns; overflow
FILL_PILEUP = np.dtype([("off", "<u8"), ("len", "<u4"), ("flags", "<u4"), ("n_cols", "<u4"), ("n_uncovered", "<u4"), ("n_thin", "<u4"),
                        ("n_contested", "<u4"), ("n_minority", "<u4"), ("n_one_strand", "<u4"), ("low_run", "<u4"), ("low_run_col", "<u4"),
                        ("min_depth_seen", "<u4"), ("min_depth_col", "<u4"), ("depth_sum", "<u8"), ("reads_placed", "<u4"),
                        ("reads_ambiguous", "<u4")])
assert FILL_PILEUP.itemsize == 72
PU_ENTRY_BYTES = 16
PU_F_LONG, PU_F_NON_ACGT, PU_F_OVERFLOW = 1, 2, 4
PU_GAPS, PU_MISMATCH, PU_SKIPPED_LONG, PU_SKIPPED_NON_ACGT, PU_PLACED, PU_AMBIGUOUS, PU_ENTRIES, PU_LOW, PU_OVERFLOW, PU_WORDS = 0, 1, 2, 3, 4, 6, 8, 10, 12, 16

# the pair-span check of the closed gaps (gf_fill_pairs_dev): the record per (library, gap), its flags and the words of its statistics
# (u32[16]): gaps examined, closed gaps whose contig does not carry the word's pick, gaps skipped for a contig too long / with a byte
# that is no base, examined gaps with a body column no in-range pair covers, then u64 each: complete, placed, proper, in-range, spanning pairs
FILL_PAIRS = np.dtype([("flags", "<u4"), ("rows", "<u4"), ("pairs_complete", "<u4"), ("pairs_placed", "<u4"), ("n_proper", "<u4"),
                       ("n_misoriented", "<u4"), ("n_in_range", "<u4"), ("n_short", "<u4"), ("n_long", "<u4"), ("n_span", "<u4"),
                       ("span_insert_sum", "<i8"), ("n_cols", "<u4"), ("min_cover", "<u4"), ("min_col", "<u4"), ("n_unspanned", "<u4")])
assert FILL_PAIRS.itemsize == 64
PS_F_LONG, PS_F_NON_ACGT = 1, 2
PS_GAPS, PS_MISMATCH, PS_SKIPPED_LONG, PS_SKIPPED_NON_ACGT, PS_UNSPANNED, PS_COMPLETE, PS_PLACED, PS_PROPER, PS_IN_RANGE, PS_SPAN, PS_WORDS = 0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16

# the anchored pair span (gf_fill_pairs_anchored_dev): the record per (library, gap) — its flags are PS_F_* — and the words of its
# statistics (u32[20]): gaps examined, mismatches, skipped long / non-ACGT, hits kept, dropped for a clipped anchor / an anchor inside the
# gap / a secondary or supplementary record, hits whose target has no row, every other dropped hit, then u64 each: anchored, placed,
# proper, in-range, spanning pairs
FILL_ANCHORS = np.dtype([("flags", "<u4"), ("rows", "<u4"), ("n_anchored", "<u4"), ("n_placed", "<u4"), ("n_proper", "<u4"),
                         ("n_misoriented", "<u4"), ("n_in_range", "<u4"), ("n_short", "<u4"), ("n_long", "<u4"), ("n_left", "<u4"),
                         ("n_span", "<u4"), ("n_cols", "<u4"), ("span_insert_sum", "<i8"), ("dev_sum", "<i8"), ("min_cover", "<u4"),
                         ("min_col", "<u4"), ("n_unspanned", "<u4"), ("n_eval", "<u4"), ("dev_min_col", "<u4"), ("dev_min_n", "<u4"),
                         ("dev_min_sum", "<i8"), ("dev_max_col", "<u4"), ("dev_max_n", "<u4"), ("dev_max_sum", "<i8")])
assert FILL_ANCHORS.itemsize == 112
(PA_GAPS, PA_MISMATCH, PA_SKIPPED_LONG, PA_SKIPPED_NON_ACGT, PA_KEPT, PA_DROP_CLIPPED, PA_DROP_IN_GAP, PA_DROP_SECONDARY, PA_ABSENT,
 PA_DROP_OTHER, PA_ANCHORED, PA_PLACED, PA_PROPER, PA_IN_RANGE, PA_SPAN, PA_WORDS) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20

# the flank-overlap joins of the open gaps (gf_pick_joins_dev): the record per gap (32 bytes, all zero: no join), its flags, the words of
# its statistics (u32[16]) and the limits of its parameters
FLANK_JOIN = np.dtype([("contig", "<u4"), ("left_pos", "<u4"), ("right_pos", "<u4"), ("overlap", "<u2"), ("m_left", "<u2"), ("m_right", "<u2"),
                       ("m_flanks", "<u2"), ("n_candidates", "<u2"), ("n_accepted", "<u2"), ("o_min", "<u2"), ("o_max", "<u2"), ("level", "u1"),
                       ("flags", "u1"), ("reserved", "<u2")])
assert FLANK_JOIN.itemsize == 32
FJ_F_REVERSE, FJ_F_AMBIGUOUS, FJ_F_MULTI = 1, 2, 4
FJ_OPEN, FJ_JOINED, FJ_USABLE, FJ_CANDIDATES, FJ_FAR, FJ_SHORT_FLANK, FJ_NO_CONTEXT, FJ_MISMATCH, FJ_NO_ANCHORS, FJ_WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16
FJ_MAX_OVERLAP, FJ_MAX_CONTEXT, FJ_MAX_MISMATCH, FJ_FLANK_LIMIT = 1024, 255, 15, 65536

# the fill alternatives of the closed gaps (gf_fill_alts_dev): the record per gap (48 bytes, all zero: the gap is open), the record per
# contig (8 bytes), the flags, the classes, the words of the statistics (u32[16]) and the limit of max_dist
FILL_ALT = np.dtype([("contig", "<u4"), ("rival", "<u4"), ("fill_len", "<u4"), ("rival_len", "<u4"), ("lcp", "<u4"), ("lcs", "<u4"), ("len_min", "<u4"),
                     ("len_max", "<u4"), ("n_candidates", "<u2"), ("n_lower", "<u2"), ("n_identical", "<u2"), ("n_near", "<u2"), ("n_far", "<u2"),
                     ("dist", "<u2"), ("level", "u1"), ("flags", "u1"), ("reserved", "<u2")])
FILL_ALT_CONTIG = np.dtype([("length", "<u4"), ("dist", "<u2"), ("cls", "u1"), ("strand", "u1")])
assert FILL_ALT.itemsize == 48 and FILL_ALT_CONTIG.itemsize == 8
FA_F_REVERSE, FA_F_RIVAL_REVERSE, FA_F_HAS_RIVAL, FA_F_LENGTH_VARIES, FA_F_OUTRANKED, FA_F_LOST = 1, 2, 4, 8, 16, 32
FA_C_NONE, FA_C_WINNER, FA_C_IDENTICAL, FA_C_NEAR, FA_C_FAR, FA_C_LOWER = range(6)
FA_CLOSED, FA_CONTESTED, FA_LENGTH_VARIES, FA_CANDIDATES, FA_LOWER, FA_IDENTICAL, FA_NEAR, FA_FAR, FA_OUTRANKED, FA_LOST, FA_WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16
FA_MAX_DIST, FA_DIST_FAR = 31, 0xFFFF

# the read adjudication of the contested fills (gf_fill_adjudicate_dev): the record per gap (48 bytes, all zero: not contested), the
# verdicts, the flags, the words of the statistics (u32[16]; VOTES_W, VOTES_R, TIES are u64) and the limits of context and ratio
FILL_ADJ = np.dtype([("contig", "<u4"), ("rival", "<u4"), ("locus_w", "<u4"), ("locus_r", "<u4"), ("votes_w", "<u4"), ("votes_r", "<u4"),
                     ("votes_w_s0", "<u4"), ("votes_r_s0", "<u4"), ("ties", "<u4"), ("unplaced", "<u4"), ("only", "<u4"), ("verdict", "u1"),
                     ("flags", "u1"), ("reserved", "<u2")])
assert FILL_ADJ.itemsize == 48
AJ_KEEP, AJ_SWITCH, AJ_UNDECIDED = 1, 2, 3
AJ_F_LONG, AJ_F_NON_ACGT, AJ_F_RIVAL_FAR, AJ_F_NO_ROWS = 1, 2, 4, 8
(AJ_SEEN, AJ_ADJUDICATED, AJ_N_KEEP, AJ_N_SWITCH, AJ_N_UNDECIDED, AJ_SKIPPED_LONG, AJ_SKIPPED_NON_ACGT, AJ_MISMATCH, AJ_VOTES_W, AJ_VOTES_R, AJ_TIES,
 AJ_WORDS) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16
AJ_MAX_CONTEXT, AJ_MAX_RATIO = 1000, 16

# the gap-size measurement (gf_gap_span_dev): the record per (library, gap), its flag (n >= 1) and the words of its statistics (u32[16]):
# u64 each: candidates, accepted, multi, clipped, lowq, low, high; then u32 gaps with n >= 1
GAP_SPAN = np.dtype([("flags", "<u4"), ("n_cand", "<u4"), ("n", "<u4"), ("n_multi", "<u4"), ("n_clipped", "<u4"), ("n_lowq", "<u4"),
                     ("n_low", "<u4"), ("n_high", "<u4"), ("tlen_min", "<u4"), ("tlen_max", "<u4"), ("sum", "<i8"), ("sum_sq", "<u8"),
                     ("reserved", "<u8")])
assert GAP_SPAN.itemsize == 64
GS_F_PAIRS = 1
GS_CANDIDATES, GS_ACCEPTED, GS_MULTI, GS_CLIPPED, GS_LOWQ, GS_LOW, GS_HIGH, GS_GAPS_WITH_PAIRS, GS_WORDS = 0, 2, 4, 6, 8, 10, 12, 14, 16

_lib = None


class ProbeColumnGeom(C.Structure):
    """gf_probe_geom: the probe geometry a library's probe column was built for (include/gapfill_hip.h)."""
    _fields_ = [("n_reads", C.c_uint64), ("read_len", C.c_uint32), ("k", C.c_uint32), ("first", C.c_uint32), ("stride", C.c_uint32),
                ("np", C.c_uint32), ("ext", C.c_uint32), ("use", C.c_uint32), ("reserved", C.c_uint32)]

    def key(self):
        """What a column depends on (not `use`, which is advice, nor the reserved word)."""
        return (self.n_reads, self.read_len, self.k, self.first, self.stride, self.np, self.ext)


class ScreenPartsGeom(C.Structure):
    """gf_screen_parts_geom: what a library's resident parts (pass A's output) were built for (include/gapfill_hip.h)."""
    _fields_ = [("probe", ProbeColumnGeom)] + [(n, C.c_uint32) for n in ("n_writers", "cap", "gs", "n_groups", "n_grp", "tiles_wg", "use", "reserved")]

    def key(self):
        """What the parts depend on (not `use`, which is advice, nor the reserved word)."""
        return self.probe.key() + (self.n_writers, self.cap, self.gs, self.n_groups, self.n_grp, self.tiles_wg)


class TagLayout(C.Structure):
    """gf_tag_layout: the linear layout a library's 4-byte key column was built for (include/gapfill_hip.h)."""
    _fields_ = [("n_recs", C.c_uint64), ("span", C.c_uint64), ("checksum", C.c_uint64), ("n_scaffolds", C.c_uint32),
                ("granule_log2", C.c_uint32), ("use", C.c_uint32), ("reserved", C.c_uint32)]

    def key(self):
        """What a column and its tag maps depend on (not `use`, which is advice, nor the reserved word)."""
        return (self.n_recs, self.n_scaffolds, self.granule_log2, self.checksum)


def linkeys_layout(n, n_scaffolds):
    """The parts of a linear key column of n records (gf_alnrec_linkeys_bytes), in 32-bit words: (key words, first plane word, plane words,
    first base word, words in all)."""
    key_words = ((n + 3) & ~3) + 4
    plane_at = (key_words * 4 + 31) // 32 * 8
    plane_words = (n + 255) // 256 * 8
    return key_words, plane_at, plane_words, plane_at + plane_words, plane_at + plane_words + n_scaffolds + 1


class MergeCaps(C.Structure):
    """gf_mcaps: capacities of gf_merge_sets' output lists."""
    _fields_ = [(n, C.c_size_t) for n in ("edges", "news", "path_bytes", "seq_bytes", "finals")]


class ScreenView(C.Structure):
    """gf_screen_view (test aid, gf_screen_debug_view)."""
    _fields_ = [(n, C.c_void_p) for n in ("count", "fills", "pairs", "n_cand", "cand")] + [(n, C.c_uint32) for n in ("n_writers", "cap", "gs", "n_groups")]


class GapFillError(RuntimeError):
    def __init__(self, code, what, detail=""):
        self.code = code
        RuntimeError.__init__(self, "%s failed: %s (%d)%s" % (what, lib().gf_strerror(code).decode(), code,
                                                            (" — " + detail) if detail else ""))


def lib():
    """The loaded library; raises (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libgapfill_hip.so not built (%s missing): run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C gappadder_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    try:
        import torch  # noqa: F401  -- load torch's HIP runtime first: one libamdhip64 per process
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u32, u64p = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)
    szp = C.POINTER(C.c_size_t)
    sig = {
        "gf_init": (i32, [i32, C.POINTER(vp)]),
        "gf_destroy": (None, [vp]),
        "gf_strerror": (C.c_char_p, [i32]),
        "gf_last_error": (C.c_char_p, [vp]),
        "gf_screen_kernels": (C.c_char_p, [vp]),
        "gf_screen_last_overflow": (i32, [vp, vp]),
        "gf_set_stream": (i32, [vp, vp]),
        "gf_sync": (i32, [vp]),
        "gf_stream_wait": (i32, [vp, vp]),
        "gf_stream_wait_after_filter": (i32, [vp, vp]),
        "gf_set_option": (i32, [vp, C.c_char_p, C.c_long]),
        "gf_set_gaps": (i32, [vp, vp, sz, u32, C.c_char_p, vp]),
        "gf_pack_reads": (i32, [C.c_char_p, sz, i32, vp, vp]),
        "gf_packed_read_bytes": (sz, [i32]),
        "gf_fastq_pack": (i32, [vp, C.c_char_p, sz, i32, vp, sz, vp, vp, szp, C.POINTER(C.c_uint32)]),
        "gf_sam_pack": (i32, [vp, C.c_char_p, sz, C.c_char_p, vp, sz, vp, sz, vp, szp]),
        "gf_bgzf_inflate": (i32, [vp, C.c_char_p, sz, C.c_char_p, sz, vp, sz, szp, szp]),
        "gf_tag_alignments_bam": (i32, [vp, i32, i32, i32, i32, vp, sz, szp]),
        "gf_tag_low_mapq_bam": (i32, [vp, vp, sz, vp, sz, szp]),
        "gf_bam_fetch": (i32, [vp, vp, vp, sz, vp, sz, szp]),
        "gf_bam_pack": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, vp, szp, szp]),
        "gf_fastq_pack_dev": (i32, [vp, vp, sz, i32, vp, sz, vp, vp, vp, vp]),
        "gf_fastq_index_dev": (i32, [vp, vp, sz, vp, sz, vp, vp]),
        "gf_bam_append_dev": (i32, [vp, sz, sz, vp, sz, vp, sz, sz, vp, vp, sz, sz, vp, vp, sz, vp, szp, szp, szp]),
        "gf_read_join_dev": (i32, [vp, vp, sz, vp, vp, sz, vp]),
        "gf_fetch_slices": (i32, [vp, vp, sz, vp, vp, sz, vp, sz, szp]),
        "gf_gather_rows_dev": (i32, [vp, vp, sz, sz, vp, vp, sz, vp]),
        "gf_bam_records_text": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, sz, szp, vp, sz, szp]),
        "gf_fastq_records_text": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, vp, vp, sz, vp, szp, szp]),
        "gf_screen_reads": (i32, [vp, vp, vp, sz, i32, i32, i32, vp, sz, szp]),
        "gf_screen_reads_dev": (i32, [vp, vp, vp, sz, i32, i32, i32, vp, sz, vp]),
        "gf_screen_debug_view": (i32, [vp, C.POINTER(ScreenView)]),
        "gf_probe_geometry": (i32, [vp, sz, i32, i32, C.POINTER(ProbeColumnGeom)]),
        "gf_probe_column_bytes": (sz, [C.POINTER(ProbeColumnGeom)]),
        "gf_read_probes_dev": (i32, [vp, vp, sz, i32, i32, vp, C.POINTER(ProbeColumnGeom)]),
        "gf_screen_reads_probes_dev": (i32, [vp, vp, vp, vp, C.POINTER(ProbeColumnGeom), sz, i32, i32, i32, vp, sz, vp]),
        "gf_screen_parts_geometry": (i32, [vp, sz, i32, i32, C.POINTER(ScreenPartsGeom)]),
        "gf_screen_parts_bytes": (sz, [C.POINTER(ScreenPartsGeom)]),
        "gf_screen_parts_build_dev": (i32, [vp, vp, vp, C.POINTER(ProbeColumnGeom), sz, i32, i32, vp, C.POINTER(ScreenPartsGeom)]),
        "gf_screen_reads_parts_dev": (i32, [vp, vp, vp, vp, C.POINTER(ProbeColumnGeom), vp, C.POINTER(ScreenPartsGeom), sz, i32, i32, i32, vp, sz, vp]),
        "gf_tag_alignments": (i32, [vp, vp, sz, i32, i32, i32, i32, vp, sz, szp]),
        "gf_tag_alignments_dev": (i32, [vp, vp, sz, i32, i32, i32, i32, vp, sz, vp]),
        "gf_tag_low_mapq": (i32, [vp, vp, sz, vp, sz, vp, sz, szp]),
        "gf_tag_low_mapq_dev": (i32, [vp, vp, sz, vp, sz, vp, sz, vp]),
        "gf_second_hop_table_dev": (i32, [vp, vp, vp, vp, sz, vp, vp, sz, vp]),
        "gf_second_hop_table_merge_dev": (i32, [vp, vp, vp, vp, i32, sz, vp, vp, sz, vp]),
        "gf_tag_low_mapq_table_dev": (i32, [vp, vp, vp, sz, vp, vp, sz, vp, sz, vp]),
        "gf_pool_keys_all_dev": (i32, [vp, vp, vp, sz, i32, vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp]),
        "gf_pool_keys_from_second_hop_dev": (i32, [vp, vp, vp, vp, sz, vp, vp, sz, vp]),
        "gf_tag_alignments_low_dev": (i32, [vp, vp, sz, i32, i32, i32, i32, vp, sz, vp, vp, sz, vp]),
        "gf_tag_low_mapq_compact_dev": (i32, [vp, vp, vp, sz, vp, sz, vp, sz, vp]),
        "gf_alnrec_keys_dev": (i32, [vp, vp, sz, vp]),
        "gf_tag_alignments_keys_dev": (i32, [vp, vp, vp, sz, i32, i32, i32, i32, vp, sz, vp, vp, sz, vp]),
        "gf_tag_layout_from_ends": (i32, [vp, u32, C.c_uint64, C.POINTER(TagLayout), vp]),
        "gf_alnrec_linkeys_bytes": (sz, [sz, u32]),
        "gf_alnrec_linkeys_dev": (i32, [vp, vp, sz, vp, sz, C.POINTER(TagLayout)]),
        "gf_tag_alignments_linkeys_dev": (i32, [vp, vp, vp, C.POINTER(TagLayout), vp, sz, i32, i32, i32, i32, vp, sz, vp, vp, sz, vp]),
        "gf_tag_last_launch": (i32, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "gf_tag_kernel": (C.c_char_p, [vp]),
        "gf_assemble": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, i32, i32, i32, vp, sz, szp, vp, sz, szp]),
        "gf_assemble_dev": (i32, [vp, vp, vp, vp, sz, sz, i32, i32, i32, i32, i32, vp, sz, vp, vp, sz, vp, vp]),
        "gf_assemble_multi_dev": (i32, [vp, vp, vp, vp, sz, sz, i32, vp, vp, i32, i32, i32, vp, sz, vp, vp, sz, vp, vp]),
        "gf_assemble_last_launch": (i32, [vp, vp, vp, vp]),
        "gf_pool_counts_dev": (i32, [vp, vp, sz, vp]),
        "gf_pools_pack_for_owners_dev": (i32, [vp, vp, vp, sz, i32, i32, i32, i32, i32, vp, sz, vp, vp]),
        "gf_pools_merge_dev": (i32, [vp, vp, sz, vp, i32, i32, sz, i32, i32, i32, i32, vp, sz, vp, vp]),
        "gf_pools_pack_for_owners_v_dev": (i32, [vp, vp, vp, sz, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
        "gf_pools_merge_v_dev": (i32, [vp, vp, vp, vp, i32, i32, sz, i32, i32, i32, i32, vp, sz, vp, vp]),
        "gf_quick_check": (i32, [vp, C.c_char_p, vp, vp, sz, i32, vp, sz, szp]),
        "gf_quick_check_dev": (i32, [vp, vp, vp, vp, sz, sz, i32, vp, sz, vp]),
        "gf_overlap_evaluate": (i32, [vp, C.c_char_p, vp, vp, sz, vp, sz, vp, vp]),
        "gf_overlap_evaluate_dev": (i32, [vp, vp, vp, vp, vp, sz, vp, vp]),
        "gf_pick_anchored_dev": (i32, [vp, vp, vp, sz, vp, i32, vp, vp]),
        "gf_pick_anchored2_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp]),
        "gf_pick_anchored2_from_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp, vp]),
        "gf_pick_aligned_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp, vp, vp]),
        "gf_pick_aligned_from_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp, vp, vp, vp]),
        "gf_pick_gapped_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp, vp, vp]),
        "gf_pick_gapped_from_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp, vp, vp, vp]),
        "gf_bridging_reads": (i32, [vp, C.c_char_p, vp, vp, C.c_char_p, vp, vp, sz, i32, i32, vp]),
        "gf_merge_open_gaps_dev": (i32, [vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, i32, i32, vp, vp, i32, vp]),
        "gf_merge_sets_dev": (i32, [vp, vp, sz, sz, vp, vp, sz, sz, vp, i32, i32, vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, vp]),
        "gf_merge_sets": (i32, [vp, C.c_char_p, vp, vp, sz, vp, i32, i32, C.POINTER(MergeCaps), vp, vp, vp, vp, vp, vp, vp, vp]),
        "gf_both_unmapped_reads_dev": (i32, [vp, vp, sz, sz, vp, vp, sz, vp]),
        "gf_contig_kmer_table_dev": (i32, [vp, vp, vp, sz, vp, vp, sz, i32, vp, i32, vp]),
        "gf_recruit_by_contigs_dev": (i32, [vp, vp, vp, sz, i32, vp, vp, sz, i32, i32, vp, i32, vp, sz, vp]),
        "gf_round2_work_words": (sz, [sz, sz]),
        "gf_round2_pools_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp, vp, sz, vp, vp, vp, sz, vp]),
        "gf_pick_extended_dev": (i32, [vp, vp, vp, sz, vp, i32, vp, vp, i32, vp, vp, vp, vp, sz, vp]),
        "gf_pick_extended_aligned_dev": (i32, [vp, vp, vp, sz, vp, i32, vp, vp, i32, vp, vp, vp, vp, sz, vp]),
        "gf_pick_joins_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
        "gf_fill_alts_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "gf_fill_adjudicate_dev": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, sz, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        "gf_pick_extended_gapped_dev": (i32, [vp, vp, vp, sz, vp, i32, vp, vp, i32, vp, vp, vp, vp, sz, vp]),
        "gf_fill_support_dev": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, sz, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
        "gf_fill_polish_dev": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, sz, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp]),
        "gf_fill_pileup_dev": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, sz, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp]),
        "gf_fill_polish_gapped_dev": (i32, [vp, vp, vp, vp, sz, i32, vp, vp, sz, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp]),
        "gf_fill_pairs_dev": (i32, [vp, vp, vp, vp, vp, sz, i32, vp, vp, sz, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
        "gf_fill_pairs_split_dev": (i32, [vp, vp, vp, vp, vp, sz, vp, i32, vp, vp, sz, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
        "gf_fill_pairs_anchored_dev": (i32, [vp, vp, vp, sz, i32, vp, vp, sz, vp, vp, vp, i32, i32, vp, vp, sz, vp, vp, sz, i32, i32, i32, i32, vp, vp, vp]),
        "gf_gap_span_dev": (i32, [vp, vp, vp, sz, i32, i32, i32, i32, i32, i32, vp, vp]),
        "gf_contigs_append_dev": (i32, [vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp]),
        "gf_contig_kmer_table_from_dev": (i32, [vp, vp, vp, sz, vp, vp, sz, i32, vp, vp, i32, vp, vp]),
        "gf_round_carry_dev": (i32, [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "gf_round_pools_dev": (i32, [vp, vp, vp, sz, vp, i32, i32, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, vp]),
        "gf_closing_pools_work_words": (sz, [sz]),
        "gf_closing_pools_dev": (i32, [vp, vp, vp, sz, vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp]),
        "gf_rescue_work_bytes": (sz, [sz, sz, sz, i32]),
        "gf_rescue_reset_dev": (i32, [vp, vp, sz, sz, sz, i32, vp]),
        "gf_rescue_hq_keys_dev": (i32, [vp, vp, vp, sz, vp, sz, i32, sz, vp, sz, sz, i32, vp]),
        "gf_rescue_bridges_dev": (i32, [vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, i32, i32, vp, sz, sz, i32, vp, vp]),
        "gf_rescue_gap_bridges": (vp, [vp, sz, sz, sz, i32]),
        "gf_merge_rescue_dev": (i32, [vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]),
        "gf_count_kmers": (i32, [vp, vp, vp, sz, i32, i32, i32, vp, vp, sz, szp]),
        "gf_pool_keys_reset": (i32, [vp, vp]),
        "gf_pool_keys_from_screen_dev": (i32, [vp, vp, vp, sz, i32, vp, sz, vp]),
        "gf_pool_keys_from_tags_dev": (i32, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp]),
        "gf_build_pools_dev": (i32, [vp, vp, sz, i32, vp, vp, sz, vp, sz, vp, vp, vp]),
        "gf_dev_alloc": (i32, [vp, sz, C.POINTER(vp)]),
        "gf_dev_free": (i32, [vp, vp]),
        "gf_memcpy_h2d": (i32, [vp, vp, vp, sz]),
        "gf_memcpy_d2h": (i32, [vp, vp, vp, sz]),
        "gf_memset_dev": (i32, [vp, vp, i32, sz]),
        "gf_timing_enable": (i32, [vp, i32]),
        "gf_timing_read": (i32, [vp, i32, C.POINTER(C.c_double), u64p]),
        "gf_timing_reset": (i32, [vp]),
        "gf_synth_pairs_dev": (i32, [vp, vp, C.c_uint64, sz, vp, vp]),
        "gf_synth_layout": (i32, [vp, vp, vp, vp]),
        "gf_synth_truth": (i32, [vp, C.c_uint32, C.c_uint64, sz, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)   # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
