/* gapfill_hip.h — C ABI of libgapfill_hip.so: the MI355X (gfx950) implementation of GAPPadder's
 * read-recruitment + per-gap local-assembly hot path.
 *
 * The reference (simoncchu/GAPPadder) has no FFI for this path; its seams are process + file contracts
 * (SURVEY.md §8b).  Each entry point below names the reference interface whose arithmetic it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions: return 0 (GF_OK) or a negative GF_E_* code; never throws, never exits.  The caller owns
 * every buffer.  Plain entry points take HOST pointers and stage through HBM; the *_dev entry points take
 * DEVICE pointers, enqueue on the context's stream and do not synchronise (they are what bench.py times
 * with inputs already resident in HBM).  Output goes into caller-provided capacity; on overflow the call
 * returns GF_E_NOSPACE and *n_out holds the required element count.  One gf_ctx per device; a ctx is not
 * thread-safe; different ctxs may be driven from different threads/processes.
 */
#ifndef GAPFILL_HIP_H
#define GAPFILL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_OK 0
#define GF_E_INVAL (-1)    /* bad argument */
#define GF_E_NODEV (-2)    /* no usable HIP device / HIP runtime error (see gf_last_error) */
#define GF_E_NOMEM (-3)    /* host or device allocation failed */
#define GF_E_NOSPACE (-4)  /* output capacity too small; *n_out = required count */
#define GF_E_STATE (-5)    /* call order violated (e.g. screen before gf_set_gaps) */
#define GF_E_UNSUPPORTED (-6)
#define GF_E_FORMAT (-7)   /* malformed input file bytes (BGZF / BAM); see gf_last_error */

typedef struct gf_ctx gf_ctx;

/* One gap of the draft (one line of gap_positions.txt: gnrt_pos_true_seqs.py:54).  Gaps are passed grouped
 * by scaffold in file order; idx_in_scaffold is the reference's 1-based per-scaffold counter
 * (collect_reads_for_gaps.py:34-63, merge_reads.py:27-41). */
typedef struct {
    uint32_t scaffold;        /* index of the scaffold in the .fai (0-based) */
    uint32_t start;           /* 0-based position of the first N */
    uint32_t end;             /* position of the first upper-case ACGT after the run */
    uint32_t idx_in_scaffold; /* 1-based */
} gf_gap;

/* One alignment record = the 9 SAM columns the reference reads (collect_reads_for_gaps.py:76-91),
 * decoded: 32 bytes. */
typedef struct {
    uint32_t pos;      /* SAM POS (1-based, un-shifted as the reference uses it) */
    uint32_t mate_pos; /* SAM PNEXT */
    int32_t tlen;      /* SAM TLEN */
    uint32_t ref;      /* RNAME as .fai index; 0xFFFFFFFF for '*' */
    uint32_t mate_ref; /* RNEXT as .fai index ('=' -> same value as ref); 0xFFFFFFFF for '*' */
    uint16_t flag;     /* SAM FLAG */
    uint8_t mapq;      /* SAM MAPQ */
    uint8_t clipflag;  /* GapReadsCollector.is_clipped(CIGAR): +2 right S/H, +1 left S/H (:13-26) */
    uint64_t read;     /* caller's read id: 2*pair + (mate number - 1) */
} gf_alnrec;

/* kinds of a tagger hit = the 4th column of the reference's list lines */
#define GF_KIND_CLIP 0       /* collect_reads_for_gaps.py:119-123  -> the read's OWN left/right list */
#define GF_KIND_DISCORDANT 1 /* :126-150                           -> the MATE's list */
#define GF_KIND_UNMAP 2      /* :153-159                           -> the MATE's list */
#define GF_KIND_LOWMAPQ 3    /* collect_discordant_low_mapq_reads.py:74-79 -> the read's OWN list */

typedef struct {
    uint32_t rec;  /* index of the record in the batch */
    uint32_t gap;  /* gf_tag_alignments: index into the gf_set_gaps array; gf_tag_low_mapq: row of the table */
    uint16_t kind; /* GF_KIND_* */
    uint16_t to_mate; /* 1: the line goes to the list of the read's mate, 0: to its own list */
} gf_taghit;

/* One row of discordant_reads_pos.txt.sorted.txt (run_multi_threads_discordant.py:87-103). */
typedef struct {
    uint32_t mate_scaffold; /* scaffold index the discordant mate maps to */
    uint32_t mate_pos;
    uint32_t src_scaffold;
    uint32_t src_gap;       /* 1-based gap index inside src_scaffold */
} gf_dpos;

typedef struct {
    uint32_t gap;  /* index into the gf_set_gaps array */
    uint32_t read; /* index of the read in the batch */
} gf_hit;

/* ---- context ------------------------------------------------------------------------------------- */
int gf_init(int device_ordinal, gf_ctx** out);
void gf_destroy(gf_ctx* ctx);
const char* gf_strerror(int code);
const char* gf_last_error(gf_ctx* ctx);       /* text of the last HIP error seen by this ctx */
/* the filter kernels the last gf_screen_reads[_dev] call launched, comma separated, as a profiler names them without namespace and
 * argument list (e.g. "pf4_scatter_lines_kernel<3u, false>,pf4_probe_kernel,pf4_resolve_kernel,pf4_list_kernel"): lets a caller
 * tie a committed rocprofv3 summary to the build that is running.  A screen from a library's resident parts names no first-pass kernel
 * ("pf4_probe_kernel,pf4_resolve_kernel,pf4_list_kernel"); after gf_screen_parts_build_dev: the first-pass kernel the build launched */
const char* gf_screen_kernels(gf_ctx* ctx);
int gf_set_stream(gf_ctx* ctx, void* hip_stream); /* adopt a caller's hipStream_t (NULL: back to the ctx's own) */
int gf_sync(gf_ctx* ctx);
/* Two contexts on one device run their work on two streams (e.g. the k-mer screen on one, the alignment tagger on the
 * other: they are independent until the pools are built).  gf_stream_wait makes everything enqueued on `waiter` after
 * this call wait for everything enqueued on `producer` before it — no host synchronisation. */
int gf_stream_wait(gf_ctx* waiter, gf_ctx* producer);
/* One-shot: everything enqueued on `waiter` after the NEXT gf_screen_reads_dev call on `producer` waits until that call's FILTER pass
 * has finished — not for its verification pass.  The filter owns every CU's LDS and most of the memory system, the verification pass
 * is a latency-bound look-up kernel: a bandwidth-bound stream (the alignment tagger) overlaps the second, not the first. */
int gf_stream_wait_after_filter(gf_ctx* waiter, gf_ctx* producer);
/* options: "max_gaps_per_kmer" (0 = unlimited; flank k-mers shared by more gaps are dropped from the index),
 * "bitmap_log2" (size of the screen's level-1 16-mer bitmap, 0 = automatic), "index_host" (1: build the flank k-mer index with
 * the host comparator instead of the device kernels — same index up to slot order; a test aid, refused unless the environment
 * has GF_DIAGNOSTICS set).
 * Ablation / diagnostic switches (results never change): "screen_variant" (0 automatic, 9 plain, 13 pipelined,
 * 16 partitioned with 256 buckets and 4-byte pairs, 17 the same with unaligned pair runs in its first pass, 18 = 16 with the first pass
 * on the packed rows even where a probe column is given), "screen_ext" (1: the
 * partitioned filter drops seeds whose neighbouring bases are none of the flanks'; 0: 16-base seeds as they are),
 * "screen_verify_ext" (1: seed-and-extend verification when min_hits == 1), "screen_verify_gate",
 * "screen_verify_batch", "screen_stream_policy", "screen_lds_log2_max", "screen_pf4_cap8",
 * "screen_pf4_writers" (a test aid, refused unless GF_DIAGNOSTICS is set: at most this many writers in the partitioned filter's first pass,
 * 0 = automatic),
 * "asm_keyslot", "asm_precount", "asm_ranked", "asm_lds_pool_kb", "asm_threads" (threads per gap: 1024 / 512 / 256; 0 = automatic:
 * 512 — two gaps per CU — when there are >= 8 gaps per CU and asm_max_pool_reads says that most pools fit half a CU's LDS, the gaps
 * that do not are handed to a second launch with 1024), "asm_stats_ptr" (device u64[4] the assembly adds its window / k-mer / survivor / node counts to), "asm_dbg_ptr".
 * Tagger: "tag_light" (1: one-wave workgroups that read the coarse bin map through L1/L2 instead of staging it in LDS — same hits;
 * for a pipeline that runs the tagger on a second context beside the k-mer filter, whose workgroups own most of every CU's LDS).
 * Assembly: "asm_tiebreak" (error removal between branches of EQUAL coverage: 1 (default) = the branch with fewer weak nodes — k-mers seen
 * at most min_count + 1 times — wins, then sequence order; 0 = sequence order alone: the reference-shaped mode, nothing that Velvet
 * could not have known, since cvtFaToFq drops the counts before Velvet reads a k-mer, assemble_gaps.py:56-79),
 * "asm_simplify" (rounds of tip clipping + bubble popping — Velvet's defaults, which the reference runs with
 * (assemble_gaps.py:117); default 8 (where the rounds have converged), 0 = raw unitigs), "asm_max_pool_reads" (device variants: upper bound on the rows of one
 * pool; the assembly workspace is then one slice of that size per workgroup instead of one per pool row — a pool beyond the bound
 * sets its gap_error; 0 = no bound), "asm_sweep" (1: gf_assemble_multi_dev runs the k list 31/29, 41/39, 51/49 as ONE launch in which a
 * workgroup assembles a gap three times — same contigs, a gap's contigs in (k, kv) order; default 0 = one launch per pair, which measured
 * 1 % faster at C5). */
int gf_set_option(gf_ctx* ctx, const char* name, long value);

/* ---- gaps + flanks (gnrt_pos_true_seqs.py:12-100 defines them; host-side there and here) ----------- */
/* flank_ascii: concatenated flank sequences, left then right per gap; flank_off[2*g], [2*g+1], ... are the
 * start offsets, flank_off[2*n_gaps] the total length.  Bases other than upper-case ACGT break k-mers. */
int gf_set_gaps(gf_ctx* ctx, const gf_gap* gaps, size_t n_gaps, uint32_t n_scaffolds,
                const char* flank_ascii, const uint64_t* flank_off);

/* ---- a-7: 2-bit packing (KmerUtils.cpp:22-58 layout: A=00 C=01 G=10 T=11, base i MSB-first) --------- */
/* Packs n_reads fixed-length reads (ASCII, read_len bases each, contiguous) into ceil(read_len/4) bytes per
 * read, base i in byte i/4 at bits 7-2(i%4)..6-2(i%4); non-ACGT -> A (KmerUtils.cpp:25) and, when n_mask is
 * non-NULL, bit (i%32) of word n_mask[r*ceil(read_len/32) + i/32] is set. */
int gf_pack_reads(const char* ascii, size_t n_reads, int read_len, uint8_t* packed, uint32_t* n_mask);
size_t gf_packed_read_bytes(int read_len);

/* ---- ingest: FASTQ TEXT -> the packed layout above, on the device.  `text` is the content of a FASTQ file
 * (or a chunk that starts at a record boundary): strict 4-line records as the reference's line machine assumes
 * (run_multi_threads_discordant.py:205-232); the last line may lack its newline; CRLF tolerated.  Read r = sequence line of
 * record r, padded with masked A (N) up to read_len.  hdr_begin[r] = byte offset of record r's '@' line (ids are cut from the
 * host's copy of the text: first whitespace token, up to '/', :212-214); needs cap_reads + 1 entries.
 * *n_reads = records found (may exceed cap_reads: GF_E_NOSPACE from the host variant, status bit 4 from the device variant).
 * status bits: 1 = a sequence line longer than read_len was truncated, 2 = trailing partial record ignored, 4 = capacity,
 * 8 = the quality line of the last record ends without a newline (a whole file: fine; a piece of one: that record may be cut). */
int gf_fastq_pack(gf_ctx* ctx, const char* text, size_t n_bytes, int read_len, uint8_t* packed, size_t cap_reads,
                  uint32_t* n_mask_or_null, uint64_t* hdr_begin_or_null, size_t* n_reads, uint32_t* status);
/* device variant: d_n_reads = u64, d_status = u32 (both written by the call; it synchronises the stream once to size the
 * second pass). */
int gf_fastq_pack_dev(gf_ctx* ctx, const void* d_text, size_t n_bytes, int read_len, void* d_packed, size_t cap_reads,
                      void* d_n_mask_or_null, void* d_hdr_begin_or_null, void* d_n_reads, void* d_status);

/* SAM TEXT (alignment lines as `samtools view` prints them) -> gf_alnrec, parsed on the device exactly as the reference reads
 * a line (collect_reads_for_gaps.py:76-91: whitespace-split, columns 0-8; clipflag per is_clipped :13-26): '@' lines and
 * lines with fewer than nine fields yield no record; the others are numbered in line order (rec.read = record index).
 * names_blob/name_off: the scaffold names of the .fai in order (n_names + 1 offsets); RNAME/RNEXT decode to the name's index,
 * '=' to RNAME's index, an unknown name to 0xFFFFFFFF.  line_begin[r] = byte offset of record r's line (QNAME and the other
 * text columns are cut from the host's copy for the few records that produce a hit).  GF_E_NOSPACE: *n_recs = needed. */
int gf_sam_pack(gf_ctx* ctx, const char* text, size_t n_bytes, const char* names_blob, const uint32_t* name_off, size_t n_names,
                gf_alnrec* recs, size_t cap_recs, uint64_t* line_begin_or_null, size_t* n_recs);

/* BGZF (the blocked gzip container of BAM, SAMv1 §4.1) inflated on the device, one wavefront per block, every block's CRC-32
 * and ISIZE checked (GF_E_FORMAT + gf_last_error on a mismatch).  `bgzf` = file bytes starting at a block boundary; only whole
 * blocks are taken: *n_consumed = bytes used (bring the rest back in front of the next chunk).  The inflated stream is
 * `carry` (bytes the previous gf_bam_pack call left unconsumed: a partial record) followed by the blocks' contents; it STAYS ON
 * THE DEVICE for gf_bam_pack / gf_bam_fetch; out_or_null (capacity `cap`; GF_E_NOSPACE with *n_out = needed) additionally
 * receives a host copy of all of it (NULL: none — the usual case, see gf_bam_fetch).
 * Replaces the `samtools view` pipe of run_multi_threads_collect_reads.py:30-32 / run_multi_threads_discordant.py:131-133. */
int gf_bgzf_inflate(gf_ctx* ctx, const uint8_t* bgzf, size_t n_bytes, const uint8_t* carry, size_t n_carry, uint8_t* out_or_null,
                    size_t cap, size_t* n_out, size_t* n_consumed);
/* BAM alignment records (SAMv1 §4.2) -> gf_alnrec, the same values gf_sam_pack gives for the `samtools view` line of the
 * record (POS/PNEXT 1-based, clipflag from the first/last CIGAR operation, rec.read = record index in stream order).
 * stream_or_null: the inflated bytes (NULL: the n_bytes left on the device by the last gf_bgzf_inflate); `first` = offset of
 * the first alignment record (after the header in the first chunk, 0 afterwards); ref_map[refID] = .fai index of that BAM
 * reference or 0xFFFFFFFF.  Only complete records are taken: *n_consumed = offset of the first incomplete one (== n_bytes when
 * none).  rec_begin[r] = offset of record r's block_size field.  GF_E_NOSPACE: *n_recs = needed. */
int gf_bam_pack(gf_ctx* ctx, const uint8_t* stream_or_null, size_t n_bytes, size_t first, const uint32_t* ref_map, size_t n_ref,
                gf_alnrec* recs, size_t cap_recs, uint64_t* rec_begin_or_null, size_t* n_recs, size_t* n_consumed);

/* gf_tag_alignments / gf_tag_low_mapq on the records the last gf_bam_pack left on the device (no second trip of the 32-byte
 * records over PCIe); GF_E_STATE when there are none. */
int gf_tag_alignments_bam(gf_ctx* ctx, int insert_size, int sd, int clip_dist, int anchor_mapq, gf_taghit* out, size_t cap,
                          size_t* n_out);
int gf_tag_low_mapq_bam(gf_ctx* ctx, const gf_dpos* table, size_t n_rows, gf_taghit* out, size_t cap, size_t* n_out);
/* Slices [begin[i], end[i]) of the inflated stream that gf_bgzf_inflate / gf_bam_pack left on the device, packed back to back
 * into dst (one small gather + one copy): the host asks for the header and for the few records that produced a hit instead of
 * copying every inflated byte back.  *n_bytes = total size; GF_E_NOSPACE when cap is smaller. */
int gf_bam_fetch(gf_ctx* ctx, const uint64_t* begin, const uint64_t* end, size_t n, uint8_t* dst, size_t cap, size_t* n_bytes);

/* ---- files -> a library RESIDENT in HBM (the device pipeline of the CLI, gappadder_amd/device_collect.py; csrc/resident.hip).
 * The reference joins alignments and reads by NAME (list lines carry QNAME, collect_reads_for_gaps.py:119-159; the FASTQ line machine
 * looks the id of every record up in {readId -> set(gapKey)}, run_multi_threads_discordant.py:153-185, 209-241); the device pipeline
 * addresses reads by index (gf_alnrec.read = 2 * FASTQ record number + mate), which these calls establish once per library. */
/* 64-bit hash of the id of every record of a FASTQ chunk on the device — the id as the reference cuts it: first whitespace token of the
 * header line, up to the first '/', first character ('@') dropped (run_multi_threads_discordant.py:212-214) — and the length of the
 * longest sequence line (atomicMax into *d_max_len, u32: the caller zeroes it).  d_hdr_begin as written by gf_fastq_pack_dev. */
int gf_fastq_index_dev(gf_ctx* ctx, const void* d_text, size_t n_bytes, const void* d_hdr_begin, size_t n_reads, void* d_id_hash /* u64[n_reads] */,
                       void* d_max_len);
/* gf_bam_pack for a resident library: the records of the inflated stream gf_bgzf_inflate left on the device are APPENDED to the caller's
 * device array d_recs at index rec_base (capacity rec_cap records), with
 *   d_qhash[rec]     the same 64-bit hash of the record's QNAME (raw, as the reference compares it), or NULL;
 *   d_names / d_name_off[rec]  the QNAME bytes back to back in a caller's arena (appended at name_base, capacity name_cap bytes) and the
 *                    offset of each (d_name_off[rec_base + n] = end of the last), or NULL: the host later fetches the names of the few
 *                    records that produce a hit (gf_fetch_slices) for the list files of the reference's file contract;
 *   d_ref_seen[scaffold] |= 1 for a record on that scaffold, |= 2 for a MAPQ-0 record (u32 per .fai scaffold, caller zeroes), or NULL:
 *                    which per-scaffold list files the reference would have opened (collect_reads_for_gaps.py:93-102);
 *   d_rec_begin[n]   for the n-th record of THIS chunk (not offset by rec_base; room for n_bytes / 36 + 1 entries) the offset of its
 *                    block_size field in the inflated stream, or NULL: with the FLAGs in d_recs the caller selects records (e.g. both
 *                    mates unmapped) and fetches their bytes while the stream is still there (gf_bam_fetch).
 * gf_alnrec.read is left 0xFFFFFFFF ("no read") until gf_read_join_dev.  *n_recs / *n_name_bytes = what the chunk holds; GF_E_NOSPACE
 * (nothing written) when a capacity is too small: grow and call again, the stream is still there. */
int gf_bam_append_dev(gf_ctx* ctx, size_t n_bytes, size_t first, const uint32_t* ref_map, size_t n_ref, void* d_recs, size_t rec_base, size_t rec_cap,
                      void* d_qhash_or_null, void* d_names_or_null, size_t name_base, size_t name_cap, void* d_name_off_or_null,
                      void* d_ref_seen_or_null, size_t n_scaffolds, void* d_rec_begin_or_null, size_t* n_recs, size_t* n_name_bytes,
                      size_t* n_consumed);
/* the join: gf_alnrec.read = 2 * (number of the FASTQ record whose id hash equals the record's QNAME hash) + (FLAG & 0x40 ? 0 : 1), or
 * 0xFFFFFFFF when there is none (such a record recruits nothing).  d_id_hash = the ids of ONE mate file (both files of a pair carry the
 * same ids in the same order: the caller checks that).  d_stats (u32[4], written): [0] ids that occur more than once, [1] records
 * without a read.  By hash: the caller verifies the names of the records that matter (the hits) and fails loudly on a mismatch. */
int gf_read_join_dev(gf_ctx* ctx, const void* d_id_hash, size_t n_ids, void* d_recs, const void* d_qhash, size_t n_recs, void* d_stats);
/* gf_bam_fetch on any device buffer: slices [begin[i], end[i]) of d_src back to back into the host buffer dst */
int gf_fetch_slices(gf_ctx* ctx, const void* d_src, size_t src_len, const uint64_t* begin, const uint64_t* end, size_t n, uint8_t* dst, size_t cap,
                    size_t* n_bytes);
/* d_dst[i] = row d_ids[i] of d_src for i < min(*d_n, cap) (rows of row_bytes, a multiple of 4; *d_n a device u64 — e.g. d_pool_off[n_gaps];
 * an id beyond n_src_rows yields all-ones): the N masks of pooled reads from the read ids gf_build_pools_dev reports */
int gf_gather_rows_dev(gf_ctx* ctx, const void* d_src, size_t n_src_rows, size_t row_bytes, const void* d_ids, const void* d_n, size_t cap,
                       void* d_dst);

/* ---- host-side text of the reference's file contract, for the records that leave the device pipeline.  No GPU work: plain C loops
 * over bytes the caller already holds (a run formats one record per recruited read; the reference does it in its FASTQ line machine,
 * run_multi_threads_discordant.py:209-241, and through `samtools view`).  ctx may be NULL (it only carries the error text). */
/* BAM alignment records, raw as in the inflated stream (record i starts at blob[rec_begin[i]] with its block_size field) ->
 *   sam: the eleven mandatory SAM columns as `samtools view` prints them, one line per record: the builtin stand-in of
 *        `samtools view -f 12` (collect_both_unmapped_reads.py:14-22)
 *   fq:  the same records in that module's FASTQ form: `@{QNAME}_2` when FLAG > 128 (a comparison, :26) else `@{QNAME}_1`, SEQ, `+`, QUAL
 *        (:24-33); NULL: sized only.
 * ref_names = the header's n_ref reference names, NUL-terminated, back to back.  *sam_len / *fq_len = bytes needed; GF_E_NOSPACE when a
 * given buffer is smaller (what was written is then incomplete), GF_E_FORMAT for bytes that are no BAM record. */
int gf_bam_records_text(gf_ctx* ctx_or_null, const uint8_t* blob, size_t blob_len, const uint64_t* rec_begin, size_t n_recs, const char* ref_names,
                        size_t n_ref, char* sam, size_t sam_cap, size_t* sam_len, char* fq_or_null, size_t fq_cap, size_t* fq_len);
/* FASTQ records [begin[i], end[i]) of file which[i] — given as images in memory (files) or, when files is NULL, as open descriptors read
 * with one pread per record (fds) — as the reference re-writes them into the per-gap files (run_multi_threads_discordant.py:212-221):
 * `@{id}{suffix[which[i]]}` — id = the header's first word up to its first '/', without the '@' —, the sequence line, a bare `+`, the
 * quality line, trailing white space dropped.  out_end[i] = where record i ends in `out`; ids_or_null / ids_end_or_null: the bare ids
 * back to back.  *out_len / *ids_len = bytes needed, GF_E_NOSPACE when a buffer is smaller. */
int gf_fastq_records_text(gf_ctx* ctx_or_null, const uint8_t* const* files_or_null, const int* fds_or_null, const uint64_t* file_len, size_t n_files,
                          const uint64_t* begin, const uint64_t* end, const uint8_t* which, const char* const* suffix, size_t n, char* out, size_t cap,
                          uint64_t* out_end,
                          char* ids_or_null, size_t ids_cap, uint64_t* ids_end_or_null, size_t* out_len, size_t* ids_len);

/* ---- north-star flank-k-mer screen ("flank-k-mer lookup to tag reads") ------------------------------
 * Emits (gap, read) for every read that has >= min_hits k-mer positions whose canonical k-mer occurs in the
 * gap's flank k-mer set (predicate shape of IsReadContainingFreqKmers, KmerUtils.cpp:215-241, on canonical
 * k-mers, per gap).  16 <= k <= 64.  Host variant returns hits sorted by (gap, read). */
int gf_screen_reads(gf_ctx* ctx, const uint8_t* packed_reads, const uint32_t* n_mask_or_null, size_t n_reads,
                    int read_len, int k, int min_hits, gf_hit* out, size_t cap, size_t* n_out);
/* device variant: d_out order is unspecified; *d_n_out (device u32, zeroed by the call) = hits produced. */
int gf_screen_reads_dev(gf_ctx* ctx, const void* d_packed_reads, const void* d_n_mask_or_null, size_t n_reads,
                        int read_len, int k, int min_hits, void* d_out, size_t cap, void* d_n_out);
/* The same screen over a library that keeps a PROBE COLUMN beside its packed reads.  The partitioned filter's first pass needs np
 * 16-mers of a read (k = 51 on 150-base reads: 3 x 4 of its 38 bytes); the column holds exactly those, as the scrambled canonical words
 * that pass ranks (definition and layout: kmer_dev.hpp, probe_word), one plane per probe, a plane = n_reads rounded up to 64 words.
 *   gf_probe_geometry     what the partitioned filter probes for (n_reads, read_len, k) — one source with the screen itself — and `use`:
 *                         whether a column is worth keeping.  It is not where it would not pay or not be taken: more than 4 probes per
 *                         read, 4 * np above half the packed read bytes (k = 31 on 150 bases: 32 of 38), reads the whole-line filter does
 *                         not take, and — when the context has its gaps — a key set or read count for which the screen picks another
 *                         filter (small key sets: the pipelined kernel).  ctx may be NULL: the geometry under the default options.
 *   gf_probe_column_bytes bytes of the column: np planes of n_reads rounded up to 64 words
 *   gf_read_probes_dev    builds the column from the packed reads (one pass over them) and reports the geometry it built for
 *   gf_screen_reads_probes_dev  gf_screen_reads_dev; the first pass streams the column when `built_for` equals the geometry of THIS call
 *                         and the filter chosen is the whole-line partitioned one — otherwise the packed rows, as without a column
 *                         (gf_screen_kernels tells which: pf4_scatter_col_kernel / pf4_scatter_lines_kernel).  Same hits either way. */
typedef struct {
    uint64_t n_reads;
    uint32_t read_len, k;
    uint32_t first, stride, np;   /* probe j of a read: the 16 bases at offset first + j * stride */
    uint32_t ext;                 /* bases the filter checks behind a seed (they set the stride) */
    uint32_t use;                 /* 1: the first pass would stream a column of this geometry; 0: it reads the rows, keep none */
    uint32_t reserved;
} gf_probe_geom;
int gf_probe_geometry(gf_ctx* ctx, size_t n_reads, int read_len, int k, gf_probe_geom* out);
size_t gf_probe_column_bytes(const gf_probe_geom* geom);
int gf_read_probes_dev(gf_ctx* ctx, const void* d_packed_reads, size_t n_reads, int read_len, int k, void* d_probes /* gf_probe_column_bytes */,
                       gf_probe_geom* built_for);
int gf_screen_reads_probes_dev(gf_ctx* ctx, const void* d_packed_reads, const void* d_n_mask_or_null, const void* d_probes_or_null,
                               const gf_probe_geom* built_for, size_t n_reads, int read_len, int k, int min_hits, void* d_out, size_t cap,
                               void* d_n_out);
/* The same screen over a library that keeps its RESIDENT PARTS: what the partitioned filter's first pass leaves — every probe of every
 * read as a 4-byte pair in its bucket's part, the parts' fill history and their counts — depends on the reads, the probe geometry and
 * the shape of the parts alone, never on the gaps, the draft or the index built from them.  A library that is screened step after step
 * keeps it, and the screen starts at its second pass.
 *   gf_screen_parts_geometry   the probe geometry (as gf_probe_geometry) and, from the same plan the screen makes, the numbers that shape
 *                              the first pass's output; `use`: whether parts are kept — exactly where a probe column is (probe.use) and
 *                              the screen takes the whole-line partitioned filter.  ctx may be NULL: the default options, 256 CUs.
 *   gf_screen_parts_bytes      bytes of the one buffer [count | fills | pairs + the 64 words idle lanes of the first pass store to]
 *   gf_screen_parts_build_dev  runs the first pass alone into d_parts — from the column when d_probes / probe_geom fit this geometry, else
 *                              from the packed rows; no gaps are needed — and reports what it built for.  A set-up call: it waits for the
 *                              stream.  `use` comes back 0 where no parts are kept (nothing was launched) or where a part ran full
 *                              (degenerate reads: a screen tests such pairs on the spot, which needs the index): keep none then.
 *   gf_screen_reads_parts_dev  gf_screen_reads_probes_dev; where `parts_for` equals what THIS call would build (read count, read length, k,
 *                              probe geometry, writers, capacity, groups) the first pass is not launched and the later passes read d_parts
 *                              (they write none of it: one buffer serves any number of screens, under any gaps) — otherwise today's path,
 *                              column or rows.  gf_screen_kernels tells which.  Same hits either way. */
typedef struct {
    gf_probe_geom probe;
    uint32_t n_writers, cap;          /* parts: [256 buckets][n_writers][cap] entries */
    uint32_t gs, n_groups, n_grp;     /* fill history: [bucket][writer][gs] words, n_groups + 1 used; groups per tile iteration */
    uint32_t tiles_wg;                /* 64-read tiles per writer and tile iteration */
    uint32_t use;                     /* 1: keep the parts, a screen of this geometry starts at its second pass; 0: keep none */
    uint32_t reserved;
} gf_screen_parts_geom;
int gf_screen_parts_geometry(gf_ctx* ctx, size_t n_reads, int read_len, int k, gf_screen_parts_geom* out);
size_t gf_screen_parts_bytes(const gf_screen_parts_geom* geom);
int gf_screen_parts_build_dev(gf_ctx* ctx, const void* d_packed_reads, const void* d_probes_or_null, const gf_probe_geom* probe_geom_or_null,
                              size_t n_reads, int read_len, int k, void* d_parts /* gf_screen_parts_bytes */, gf_screen_parts_geom* built_for);
int gf_screen_reads_parts_dev(gf_ctx* ctx, const void* d_packed_reads, const void* d_n_mask_or_null, const void* d_probes_or_null,
                              const gf_probe_geom* probe_geom_or_null, const void* d_parts_or_null, const gf_screen_parts_geom* parts_for,
                              size_t n_reads, int read_len, int k, int min_hits, void* d_out, size_t cap, void* d_n_out);
/* Test aid (GF_E_UNSUPPORTED unless GF_DIAGNOSTICS is set in the environment): what the last screen on this context that took the
 * partitioned filter left in its workspace, as device pointers that stay valid until the next screen — the pairs of its first pass
 * ([256 buckets][n_writers][cap] entries, `count` of them written per part, in generation order), the fill history ([bucket][writer][gs]
 * words, n_groups + 1 of them used) and, with the option "screen_keep_cand" set, a copy of the candidate list the filter handed to the
 * verification (order unspecified).  The row form and the column form of the first pass must leave all of it identical. */
typedef struct {
    const uint32_t *count, *fills, *pairs, *n_cand, *cand;
    uint32_t n_writers, cap, gs, n_groups;
} gf_screen_view;
int gf_screen_debug_view(gf_ctx* ctx, gf_screen_view* out);
/* The device variant cannot return GF_E_UNSUPPORTED for the one thing the verification may not be able to finish — a read with more
 * than 15 000 (k-mer position, gap) matches, i.e. a low-complexity read against hundreds of flanks that share its k-mers: such a read
 * is counted and its hits are incomplete.  This reads the counter of the LAST gf_screen_reads_dev call on this context (it waits for
 * the context's stream); 0 = every read was verified in full.  The remedy on such drafts is the repeat mask, option
 * "max_gaps_per_kmer". */
int gf_screen_last_overflow(gf_ctx* ctx, size_t* n_reads_dropped);

/* ---- a-2: alignment-record tagger (GapReadsCollector.parse_reads_fall_in_gaps_one_scaffold[_short_is],
 * collect_reads_for_gaps.py:68-263; mode switch at IS >= 750, :275).  Host variant: sorted by
 * (rec, gap, kind). */
int gf_tag_alignments(gf_ctx* ctx, const gf_alnrec* recs, size_t n, int insert_size, int sd, int clip_dist,
                      int anchor_mapq, gf_taghit* out, size_t cap, size_t* n_out);
int gf_tag_alignments_dev(gf_ctx* ctx, const void* d_recs, size_t n, int insert_size, int sd, int clip_dist,
                          int anchor_mapq, void* d_out, size_t cap, void* d_n_out);

/* ---- a-3: second hop (collect_discordant_low_mapq_reads.py:4-84).  table = rows sorted by
 * (mate_scaffold, mate_pos, src_scaffold, src_gap), duplicates kept; a MAPQ==0 record at POS p on scaffold s
 * is linked to the LAST position q of s with q-199 <= p <= q+299 and emits one hit per row of q
 * (hit.gap = row index).  Host variant: sorted by (rec, row). */
int gf_tag_low_mapq(gf_ctx* ctx, const gf_alnrec* recs, size_t n, const gf_dpos* table, size_t n_rows,
                    gf_taghit* out, size_t cap, size_t* n_out);
int gf_tag_low_mapq_dev(gf_ctx* ctx, const void* d_recs, size_t n, const gf_dpos* table, size_t n_rows,
                        void* d_out, size_t cap, void* d_n_out);

/* ---- a-6: per-gap local assembly (run_assembly, assemble_gaps.py:82-136: `kmc -k{k}` | `kmc_dump` | `velveth {kv}` |
 * `velvetg -min_contig_lgth 40`).  Pools are packed reads (gf_pack_reads layout) concatenated per gap: pool g owns
 * reads pool_off[g] .. pool_off[g+1]-1.  The k-mer counting and graph arithmetic of the reference live in un-vendored
 * KMC and Velvet, so the semantics are DEFINED by this build (DESIGN.md "Assembly semantics", oracle/gp_oracle.c):
 * canonical k-mers with count >= min_count; nodes = their canonical kv-mers (kv odd, 15 <= kv < k <= 64); contigs =
 * unitigs of >= min_contig bases, each reported once in the orientation min(seq, revcomp(seq)). */
typedef struct {
    uint32_t gap;      /* index of the pool */
    uint16_t k, kv;
    uint32_t n_nodes;  /* kv-mers in the contig (Velvet's NODE_n_length_{n_nodes}) */
    uint32_t length;   /* bases = n_nodes + kv - 1 */
    uint32_t cov_sum;  /* sum over the contig's nodes of their multiplicity among the surviving k-mers (cov = cov_sum / n_nodes) */
    uint32_t reserved;
    uint64_t seq_off;  /* offset of the contig's ASCII bases in the sequence buffer */
} gf_contig;

/* host variant: every (k_list[i], kv_list[i]) pair in turn (assemble_gaps.py:87-122); contigs sorted by
 * (gap, pair index, length descending, sequence ascending).  Returns GF_E_NOSPACE with the needed counts in
 * *n_contigs / *seq_len when a capacity is too small. */
int gf_assemble(gf_ctx* ctx, const uint8_t* pool_packed, const uint32_t* pool_n_mask_or_null, const uint64_t* pool_off,
                size_t n_pools, int read_len, const int* k_list, const int* kv_list, int n_k, int min_count, int min_contig,
                gf_contig* contigs, size_t contig_cap, size_t* n_contigs, char* seq, size_t seq_cap, size_t* seq_len);
/* device variant, one (k, kv) pair: total_reads = pool_off[n_pools] (upper bound used to size the workspace);
 * d_n_contigs: u32, d_seq_len: u64, d_gap_error: n_pools x u32 (1 = that pool overflowed an internal table).
 * Contig order is unspecified. */
int gf_assemble_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_pool_n_mask_or_null, const void* d_pool_off,
                    size_t n_pools, size_t total_reads, int read_len, int k, int kv, int min_count, int min_contig,
                    void* d_contigs, size_t contig_cap, void* d_n_contigs, void* d_seq, size_t seq_cap, void* d_seq_len,
                    void* d_gap_error);
/* every (k_list[i], kv_list[i]) pair of run_assembly's loop (assemble_gaps.py:87-122) in one call: one launch per pair, all
 * appending to the same contig list (gf_contig.k / .kv tell the pairs apart); counters and error flags as gf_assemble_dev.
 * Capacities (this call and gf_assemble_dev): the counters count every contig and base, also those beyond contig_cap / seq_cap; every
 * record below min(*d_n_contigs, contig_cap) is written, and one whose bases do not fit seq_cap is a TOMBSTONE {length = 0, seq_off = 0}
 * (the contig list's consumers skip it); nothing is written beyond either capacity. */
int gf_assemble_multi_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_pool_n_mask_or_null, const void* d_pool_off,
                          size_t n_pools, size_t total_reads, int read_len, const int* k_list, const int* kv_list, int n_k,
                          int min_count, int min_contig, void* d_contigs, size_t contig_cap, void* d_n_contigs, void* d_seq,
                          size_t seq_cap, void* d_seq_len, void* d_gap_error);
/* What the LAST assembly launch group of this context did (the last (k, kv) pair of a multi-k call): threads per gap of its main launch
 * (1024: one gap per CU; 512: two, each with half of the CU's LDS), the gaps that left it for the middle launch (1 024 threads: pools
 * too deep for, or graphs too large for, half a CU's LDS) and the pools beyond asm_max_pool_reads that the last launch took.
 * Synchronises the stream.  Diagnostic: results never depend on it. */
int gf_assemble_last_launch(gf_ctx* ctx, int* threads_per_gap, uint32_t* to_middle, uint32_t* to_last);

/* counted canonical k-mers of ONE pool, ascending (what `kmc_dump -ci0` lists after `kmc -k{k}`, assemble_gaps.py:96-102).
 * kmers: 2 x uint64 per k-mer (hi, lo), left-aligned KmerUtils layout; counts capped at 10^7 (-cs10000000). */
int gf_count_kmers(gf_ctx* ctx, const uint8_t* pool_packed, const uint32_t* pool_n_mask_or_null, size_t n_reads,
                   int read_len, int k, int min_count, uint64_t* kmers, uint32_t* counts, size_t cap, size_t* n_out);

/* One-pass form of the two hops for device-resident pipelines: the tagger also compacts every MAPQ==0 record (2 % of a
 * typical BAM) into {pos, ref, record index}, and the second hop scans that list instead of re-reading every record
 * (the reference makes a second full `samtools view` pass, run_multi_threads_discordant.py:125-138).  Same hits. */
typedef struct {
    uint32_t pos;
    uint32_t ref;
    uint32_t rec;
} gf_lowrec;
int gf_tag_alignments_low_dev(gf_ctx* ctx, const void* d_recs, size_t n, int insert_size, int sd, int clip_dist,
                              int anchor_mapq, void* d_out, size_t cap, void* d_n_out, void* d_low /* gf_lowrec */,
                              size_t low_cap, void* d_n_low /* u32 */);
/* The same pass over a library that keeps a KEY COLUMN beside its records: 8 bytes per record, {pos, ref | (mapq == 0) << 31}, n + 1 entries
 * (gf_alnrec_keys_dev builds it from the records, once, at ingest).  99 % of the records of a BAM lie far from every gap and are decided by
 * (scaffold, position) alone — the reference's `focal_region.has_key(POS)` (collect_reads_for_gaps.py:104) —, the MAPQ-0 by-product needs one
 * more bit: the tagger streams the key column (a quarter of the bytes) and fetches the 32-byte record only of what passes its bin maps.
 * Same hits, same MAPQ-0 list as gf_tag_alignments_low_dev (order unspecified in both). */
int gf_alnrec_keys_dev(gf_ctx* ctx, const void* d_recs, size_t n, void* d_keys /* 8 * (n + 1) bytes */);
int gf_tag_alignments_keys_dev(gf_ctx* ctx, const void* d_recs, const void* d_keys, size_t n, int insert_size, int sd, int clip_dist,
                               int anchor_mapq, void* d_out, size_t cap, void* d_n_out, void* d_low /* gf_lowrec or NULL */, size_t low_cap,
                               void* d_n_low /* u32 or NULL */);
/* The same pass over a LINEAR KEY COLUMN: 4 bytes per record.  The scaffolds of the draft are laid end to end — scaffold s starts at base[s], the
 * prefix sum of the scaffolds' ends (max(pos) + 1 over the library's placed records), each rounded up to a granule of 2^granule_log2 — and a
 * record's key is base[ref] + pos, 0xFFFFFFFF for an unplaced record, a scaffold the context does not know and the pad.  Every tag map bins with
 * a shift of at most granule_log2, so no bin covers two scaffolds and "which bin of which scaffold" is one shift of the key.  The MAPQ-0 bit
 * of the 8-byte key moves to a bit plane, one bit per record.
 *   gf_tag_layout_from_ends  the layout of given scaffold ends (host only, no context): base[] (n_scaffolds + 1 words, optional), the largest
 *                          granule for which the whole line stays below 2^32 - 2^granule_log2 and the default LDS map's bins are no wider than
 *                          a granule; `use` = 0 when there is none (a draft beyond 4 Gb): the 8-byte column then serves
 *   gf_alnrec_linkeys_bytes  bytes of the column: [keys: n rounded up to 4, + 4 | plane: 32 bytes per 256 records, from a 32-byte boundary |
 *                          base: n_scaffolds + 1 words]
 *   gf_alnrec_linkeys_dev  measures the ends (one pass over the records), lays the scaffolds out and, where built_for->use comes back 1, writes
 *                          the column (a second pass)
 *   gf_tag_alignments_linkeys_dev  gf_tag_alignments_keys_dev on the linear column when it was built for THIS call — record count, scaffold
 *                          count, a checksum of base[] — and the maps' bins fit its granule; otherwise the call answers from d_keys_or_null
 *                          (the 8-byte column) or, without one, from the records.  Same hits and MAPQ-0 list either way. */
typedef struct {
    uint64_t n_recs;
    uint64_t span;            /* base[n_scaffolds]: the length of the line */
    uint64_t checksum;        /* FNV-1a (64 bit) over the n_scaffolds + 1 words of base[], low byte first */
    uint32_t n_scaffolds;
    uint32_t granule_log2;
    uint32_t use;             /* 1: a column of this layout can be built and streamed; 0: keep none */
    uint32_t reserved;
} gf_tag_layout;
int gf_tag_layout_from_ends(const uint32_t* ends, uint32_t n_scaffolds, uint64_t n_recs, gf_tag_layout* out, uint32_t* base_or_null);
size_t gf_alnrec_linkeys_bytes(size_t n, uint32_t n_scaffolds);
int gf_alnrec_linkeys_dev(gf_ctx* ctx, const void* d_recs, size_t n, void* d_col, size_t col_bytes /* >= gf_alnrec_linkeys_bytes: GF_E_NOSPACE */,
                          gf_tag_layout* built_for);
int gf_tag_alignments_linkeys_dev(gf_ctx* ctx, const void* d_recs, const void* d_col, const gf_tag_layout* built_for, const void* d_keys_or_null,
                                  size_t n, int insert_size, int sd, int clip_dist, int anchor_mapq, void* d_out, size_t cap, void* d_n_out,
                                  void* d_low /* gf_lowrec or NULL */, size_t low_cap, void* d_n_low /* u32 or NULL */);
/* What the last tagger pass on this context launched: waves per workgroup (1, 4 or 16) and what it streamed — 0 the records, 1 the 8-byte key
 * column, 2 the linear key column. */
int gf_tag_last_launch(gf_ctx* ctx, int* waves_per_workgroup, int* stream_form);
/* The kernel that pass launched, as a profiler names it without namespace and argument list — tag_kernel<waves, map staged in LDS, records
 * queued in front of a fine map, stream form>, e.g. "tag_kernel<16, true, false, 2>" —, with "+fine" behind it where the bin map of that
 * launch had a fine map behind it ("" before the first launch). */
const char* gf_tag_kernel(gf_ctx* ctx);
int gf_tag_low_mapq_compact_dev(gf_ctx* ctx, const void* d_low, const void* d_n_low, size_t low_cap, const gf_dpos* table,
                                size_t n_rows, void* d_out, size_t cap, void* d_n_out);
/* The second-hop table itself on the device (replaces collect_discordant_regions_v2 + sort(1) + the per-scaffold split,
 * run_multi_threads_discordant.py:19-122): one row per DISCORDANT tagger hit whose mate lies on a known scaffold,
 * {mate_ref, mate_pos of the hit's record; scaffold, idx_in_scaffold of the hit's gap}, sorted by (mate scaffold, mate
 * position): a counting sort into at most 2^14 buckets of (scaffold, top bits of the position), then one wave's bitonic
 * network per bucket — no library sort.  d_rows (gf_dpos[row_cap]) and d_row_gap (u32[row_cap]: index of each row's gap, for
 * gf_pool_keys_from_second_hop_dev) are the caller's device buffers; *d_n_rows (device u32) = rows found — more than row_cap
 * means the table is truncated (size row_cap from the number of tagger hits; which rows it then holds is unspecified).
 * Rows with equal (scaffold, position) are ordered by gap index: the reference's -k3n -k4n for gaps listed in scaffold
 * order, so the table is the reference's file row for row. */
int gf_second_hop_table_dev(gf_ctx* ctx, const void* d_recs, const void* d_taghits, const void* d_n_taghits, size_t hit_cap,
                            void* d_rows, void* d_row_gap, size_t row_cap, void* d_n_rows);
/* Multi-GPU runs shard the reads, but the second hop links a MAPQ-0 record to discordant mates of ANY read: every rank builds the
 * rows of its records (gf_second_hop_table_dev), the ranks all-gather rows / row gaps / counts (fixed part_cap slots), and this
 * call merges the n_parts sorted slots by rank (a row's place = its index in its own slot + the rows <= its key in earlier slots
 * + the rows < its key in later slots; nothing is sorted again) — the table of a single-process run up to the order of equal
 * keys: among them an earlier slot comes first and the rows of one slot keep their order.  A count above part_cap is read as
 * part_cap; *d_n_rows = the clamped total, of which the first row_cap rows are written.
 * d_rows_all: gf_dpos [n_parts][part_cap]; d_row_gap_all: u32 [n_parts][part_cap]; d_n_rows_all: u32 [n_parts]. */
int gf_second_hop_table_merge_dev(gf_ctx* ctx, const void* d_rows_all, const void* d_row_gap_all, const void* d_n_rows_all, int n_parts,
                                  size_t part_cap, void* d_rows, void* d_row_gap, size_t row_cap, void* d_n_rows);
/* second hop over the compacted MAPQ-0 list against a DEVICE table (d_rows / d_n_rows as written by gf_second_hop_table_dev,
 * or any sorted gf_dpos array in HBM); hit.gap = row index, as with gf_tag_low_mapq */
int gf_tag_low_mapq_table_dev(gf_ctx* ctx, const void* d_low, const void* d_n_low, size_t low_cap, const void* d_rows,
                              const void* d_n_rows, size_t row_cap, void* d_out, size_t cap, void* d_n_out);

/* ---- a-4 / a-5 on the device: per-gap read pools.  The reference joins read IDs against whole FASTQ files
 * ({readId -> set(gapKey)}, run_multi_threads_discordant.py:153-185; stream + append, :209-241, 283-316; `cat` across
 * libraries, merge_reads.py:43-51).  With reads addressed by index (read = 2*pair + mate) that is the SET of (gap, read)
 * keys, per gap ordered by (mate, pair) = left-file stream order then right-file stream order, and a gather.
 * Keys are uint64 (gap << 32 | read); *d_n_keys is a device u32 that the key producers advance. */
int gf_pool_keys_reset(gf_ctx* ctx, void* d_n_keys);
/* screen hits -> keys; pairs != 0 also adds each hit's mate ("pulls candidate read pairs", north_star) */
int gf_pool_keys_from_screen_dev(gf_ctx* ctx, const void* d_hits, const void* d_n_hits, size_t hit_cap, int pairs,
                                 void* d_keys, size_t key_cap, void* d_n_keys);
/* tagger hits -> keys (target read = the record's read, or its mate when to_mate is set: the reference writes
 * discordant/unmap lines to the MATE's list, collect_reads_for_gaps.py:126-159).  For second-hop hits pass the row
 * table so that hit.gap (a row) resolves to its (src_scaffold, src_gap). */
int gf_pool_keys_from_tags_dev(gf_ctx* ctx, const void* d_recs, const void* d_taghits, const void* d_n_taghits,
                               size_t hit_cap, const gf_dpos* lowmapq_table_or_null, size_t n_rows, void* d_keys,
                               size_t key_cap, void* d_n_keys);
/* the three producers above in ONE launch without atomics (the counts are device words, so every key has a fixed place: screen
 * hits and their mates, then tagger hits, then second-hop hits); writes *d_n_keys = number of keys (no reset needed).
 * d_taghits / d_hophits may be NULL. */
int gf_pool_keys_all_dev(gf_ctx* ctx, const void* d_hits, const void* d_n_hits, size_t hit_cap, int pairs, const void* d_recs,
                         const void* d_taghits, const void* d_n_taghits, size_t taghit_cap, const void* d_hophits,
                         const void* d_n_hophits, size_t hophit_cap, const void* d_row_gap, void* d_keys, size_t key_cap,
                         void* d_n_keys);
/* second-hop hits against a device table: hit.gap (a row) resolves through d_row_gap (gf_second_hop_table_dev) */
int gf_pool_keys_from_second_hop_dev(gf_ctx* ctx, const void* d_recs, const void* d_taghits, const void* d_n_taghits,
                                     size_t hit_cap, const void* d_row_gap, void* d_keys, size_t key_cap, void* d_n_keys);
/* keys -> d_pool_off (n_gaps+1 x u64), d_pool_packed (pool_cap_reads reads), d_pool_read_ids (u32 per pooled read, or
 * null).  A gap may have any number of keys (up to 4 096 are sorted in LDS, longer lists in place in global memory: slower, never
 * dropped — the reference has no bound either, run_multi_threads_discordant.py:209-241).  *d_error (u32): bit 31 set =
 * d_pool_off[n_gaps] > pool_cap_reads, the pool buffer was too small (reads beyond it are not written; d_pool_off stays exact).
 * A key whose read is >= n_reads is counted and listed in d_pool_read_ids like any other, and its row of d_pool_packed is left
 * as it was.  pool_cap_reads == 0 (d_pool_packed may be null) asks for d_pool_off alone: nothing is gathered, *d_error stays 0. */
int gf_build_pools_dev(gf_ctx* ctx, const void* d_packed_reads, size_t n_reads, int read_len, const void* d_keys,
                       const void* d_n_keys, size_t key_cap, void* d_pool_packed, size_t pool_cap_reads, void* d_pool_off,
                       void* d_pool_read_ids, void* d_error);

/* ---- pools of several sources -> one pool per gap.  Two uses, one primitive:
 *  (a-5) library merge, merge_reads.py:43-51 (`cat` of the per-library gap_reads/{id}.fastq in library order): build one pool
 *        array per library (gf_build_pools_dev into slot l of a [n_lib][cap_rows] buffer), gf_pool_counts_dev per library, then
 *        gf_pools_merge_dev(n_lib, n_src_ranks = 1, rank 0 of world 1);
 *  (§8e) the one exchange step of a multi-GPU run: every rank regroups its pools by OWNER rank (gf_pools_pack_for_owners_dev:
 *        owner(g) = (g / batch) % world; slot (owner * n_lib + lib) of the send buffer holds that owner's gaps' rows in gap
 *        order), the ranks all-gather the per-gap counts and all-to-all the slots (RCCL: equal-sized slots, no host sizes), and
 *        every owner merges its gaps' rows (gf_pools_merge_dev: libraries in order, inside a library the source ranks in order
 *        — with contiguous read shards that is the order of a single-process run over all reads; the reference assembles each gap
 *        exactly once from all of its reads, assemble_gaps.py:296-299).
 * Row = one packed read (gf_packed_read_bytes(read_len) bytes).  d_cnt = u32 per gap.  *d_error (u32, not reset by these calls)
 * gets bit 30 when a send slot, bit 31 when the merged buffer is too small (rows beyond the capacity are dropped). */
int gf_pool_counts_dev(gf_ctx* ctx, const void* d_pool_off /* u64[n_gaps+1] */, size_t n_gaps, void* d_cnt);
int gf_pools_pack_for_owners_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_pool_off, size_t n_gaps, int read_len,
                                 int world, int batch, int lib, int n_lib, void* d_send /* [world][n_lib][cap_rows] rows */,
                                 size_t cap_rows, void* d_cnt /* u32[n_gaps]: this library's rows per gap */, void* d_error);
/* d_src: [n_src_ranks][n_lib][cap_rows] rows (slot (r, l) = rows of MY gaps from source rank r, library l, in gap order);
 * d_cnt: u32 [n_src_ranks][n_lib][n_gaps] (the all-gathered pack counts; for a local library merge the per-library counts).
 * Writes d_merged_off (u64[n_gaps+1]; gaps this rank does not own are empty) and the rows. */
int gf_pools_merge_dev(gf_ctx* ctx, const void* d_src, size_t cap_rows, const void* d_cnt, int n_lib, int n_src_ranks,
                       size_t n_gaps, int read_len, int rank, int world, int batch, void* d_merged, size_t merged_cap_rows,
                       void* d_merged_off, void* d_error);

/* The same two steps for an EXACT-SIZE exchange (all-to-all-v of the recruited rows): the send / receive buffer is one
 * byte array of per-peer chunks of different sizes, described by device tables with one entry per slot s = peer * n_lib + lib:
 * d_slot_base[s] (u64) = byte offset of the slot's first row (even when the row size is even), d_slot_cap[s] (u32) = its rows,
 * d_cnt_base[s] (u64, multiple of 4) = byte offset of the slot's per-gap counts u32[n_gaps] INSIDE the same buffer — pack writes them
 * there (zero for gaps the peer does not own), merge reads them from there: the counts ride in the all-to-all, no all-gather of
 * counts.  Error bits as above (bit 30: a step produced more rows for a slot than the table gives it). */
int gf_pools_pack_for_owners_v_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_pool_off, size_t n_gaps, int read_len,
                                   int world, int batch, int lib, int n_lib, void* d_send, const void* d_slot_base,
                                   const void* d_slot_cap, const void* d_cnt_base_or_null, void* d_cnt, void* d_error);
int gf_pools_merge_v_dev(gf_ctx* ctx, const void* d_src, const void* d_slot_base, const void* d_cnt_base, int n_lib,
                         int n_src_ranks, size_t n_gaps, int read_len, int rank, int world, int batch, void* d_merged,
                         size_t merged_cap_rows, void* d_merged_off, void* d_error);

/* ---- §8f-1 on the device: flank anchoring (ContigsSelection, pick_contigs.py:64-358, with exact anchors instead of
 * `bwa mem -T {score}`: the last / first anchor_len bases of the left / right flank given to gf_set_gaps; 8 <= anchor_len <= 32;
 * the reference's scores are 30, then 15: assemble_gaps.py:336, 365).  Per contig the reference's pair choice (:149-297) on the
 * exact-anchor hits: the forward pair (leftmost left anchor, rightmost right anchor) when both forward hits exist, else the
 * reverse-strand pair; a pair counts when the right anchor starts at or behind the left anchor's end (:313-321).
 * d_gap_best[gap] (u64, caller zeroes; atomicMax, so several calls — other anchor lengths, other contig lists — accumulate) =
 * anchor_len << 56 | (span + 1) << 32 | (0x7FFFFFFF - contig index) << 1 | reverse strand: the longest span wins, the earlier
 * contig on ties (:313-321), and a pick at a longer anchor outranks every pick at a shorter one (the pipeline tries 15 only on
 * what 30 left open); 0 = no contig of the gap is anchored = gap not closed; *d_n_closed (u32, caller zeroes) counts the gaps
 * that became non-zero.  The span field holds 24 bits: a span + 1 of 2^24 bases or more saturates at 0xFFFFFF (it still wins over
 * every shorter span and the gap counts as closed; contigs of the per-gap assembly are three orders of magnitude shorter). */
int gf_pick_anchored_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                         int anchor_len, void* d_gap_best, void* d_n_closed);
/* both scores of the pipeline in ONE pass over the contigs (anchor_len_short < anchor_len; 0: anchor_len only): the same words as
 * gf_pick_anchored_dev(anchor_len) followed by gf_pick_anchored_dev(anchor_len_short) leave in d_gap_best */
int gf_pick_anchored2_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                          int anchor_len, int anchor_len_short, void* d_gap_best, void* d_n_closed);

/* ---- flank anchoring in "align" mode: ungapped seed-and-extend of the WHOLE flanks instead of exact anchors (the stand-in for
 * `bwa mem -T {T} -a` that aligns through a draft base differing from the reads near a flank's gap-side end).  The definition, with
 * bwa mem's default parameters as constants, for every contig, side and strand: query Q = the flank, or revcomp(flank) on the
 * reverse strand, aligned to the forward contig (SAM's frame); seeds = maximal runs of >= 19 identical ACGT bases on one diagonal,
 * diagonals ascending, seeds left to right, a seed inside an alignment already produced on its diagonal skipped; extension left,
 * then right, ungapped, from the seed length as score: match +1, mismatch -4, non-ACGT on either side -1, the first maximum kept,
 * stop when the running score falls more than 100 below it; at a query end the contig reaches, the score g of extending to the end
 * wins when g > 0 and g > best - 5 (else the end is clipped); reported when score >= T: pos = contig index of the first aligned
 * query base + 1, M = aligned length, clip type from (query start > 0, query end < |Q|); at most 64 alignments per (contig, side,
 * strand) in production order (the rest are dropped and counted in d_stats[0]); a contig with more than 1 024 seeds over both
 * flanks and strands gives no hits (counted in d_stats[1]).  Per (side, clip type) the hit with the longest M, ties to the higher
 * score, the forward strand, the lower pos; then the reference's seven pairs (pick_contigs.py:149-297, the reverse flag never
 * cleared, :176-177) and the span as for gf_pick_anchored_dev.  Host twin: gappadder_amd/pick_contigs.py::align_hits.
 * t_long (1..255) and t_short (< t_long; 0 = one round) are the two score thresholds of the pipeline (30 and 15).
 * d_gap_best (u64 per gap, caller zeroes, atomicMax) = T << 56 | (span + 1) << 32 | (0x7FFFFFFF - contig index) << 1 | reverse,
 * T = the threshold the contig selects at (the higher one when both): decode exactly as gf_pick_anchored_dev's words, a pick at
 * t_long outranks any at t_short; *d_n_closed (u32, caller zeroes) counts gaps that became non-zero.
 * d_ctg_pick: gf_ctg_pick per contig index (contig_cap entries, caller zeroes): the contig's selection at the highest threshold it
 * selects at, over this and earlier calls (an entry is replaced only by one of a higher threshold); threshold 0 = none.
 * d_stats: 2 x u32 (caller zeroes; calls accumulate).  Flanks of more than 1 024 bases: GF_E_UNSUPPORTED (nothing is truncated). */
typedef struct {
    uint32_t lp, rp;      /* 1-based contig positions of the left and right flank alignments */
    uint16_t lm, rm;      /* their aligned lengths */
    uint8_t reverse;      /* the pair is on the reverse strand (the contig is written reverse-complemented) */
    uint8_t threshold;    /* the score threshold it was selected at; 0 = no selection */
    uint16_t reserved;
} gf_ctg_pick;
int gf_pick_aligned_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                        int t_short, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats);
/* gf_pick_aligned_dev over the contigs from *d_first (u32, device) on: the second pick after gf_merge_open_gaps_dev */
int gf_pick_aligned_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                             int t_short, const void* d_first, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats);
/* ---- flank anchoring in "gapped" mode: gf_pick_aligned[_from]_dev with a banded affine-gap extension, so that a flank aligns THROUGH
 * a draft indel next to the gap.  Queries, seeds, production order, thresholds, the hit order, the selection, every argument, the
 * d_gap_best words, gf_ctg_pick and the two d_stats words are those of gf_pick_aligned_dev.  What differs (the definition in full:
 * gappadder_amd/pick_contigs.py's docstring, host twin gapped_hits): from each end of the seed run, left first, a DP over (contig
 * bases, query bases) beyond the seed with match +1, mismatch -4, non-ACGT -1, a gap of g bases 6 + g, 31 diagonals either side of the
 * seed's, values <= 0 dead, no z-drop; per side the first maximum in (contig, query) order, and the end rule of the align mode on the
 * maximum of the query's last column; pos = the first aligned CONTIG base + 1 and M (gf_ctg_pick's lm / rm) = the CONTIG bases covered;
 * a seed is skipped when an alignment kept for its query contains it (query interval and first contig base); the first 64 alignments
 * per (contig, side, strand) are extended and kept, later ones counted in d_stats[0] and not extended. */
int gf_pick_gapped_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                       int t_short, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats);
int gf_pick_gapped_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t_long,
                            int t_short, const void* d_first, void* d_gap_best, void* d_n_closed, void* d_ctg_pick, void* d_stats);

/* ---- §8f-3, first piece: the all-pairs k-mer prefilter of the reference's ContigsMerger (QuickCheckerContigsMatch,
 * ContigsCompactor.cpp:1982-2095, applied by CompactVer3 :836-853 / threadQuickCheck :1073-1098).  A contig SET (one per gap: its
 * contigs.fa) becomes the node list [c0, revcomp(c0), c1, revcomp(c1), ...]; pair (i, j), i <= j, is feasible iff some k-mer of
 * the first or last 30 bases of node j occurs anywhere in node i (KmerUtils' 2-bit k-mers: any symbol but C/G/T counts as A).
 * Only feasible pairs go on to the overlap alignment (gf_overlap_evaluate below).  Contigs need >= 30 bases
 * (GF_E_INVAL; the reference reads out of bounds).  4 <= k <= 16 (the reference's default is 10).
 * seq: the contigs' ASCII bases back to back; contig_off[n_contigs+1]; set_off[n_sets+1] = contig index ranges of the sets.
 * Host variant: triples sorted by (set, i, j). */
typedef struct {
    uint32_t set; /* index of the contig set */
    uint32_t i, j; /* nodes: 2 * contig-in-set + strand (1 = reverse complement), i <= j */
} gf_qcpair;
int gf_quick_check(gf_ctx* ctx, const char* seq, const uint64_t* contig_off, const uint64_t* set_off, size_t n_sets, int k,
                   gf_qcpair* out, size_t cap, size_t* n_out);
/* device variant: max_set_contigs = contigs of the largest set (sizes the pair matrices); d_n_out = u32[2]: [0] triples found (more
 * than cap: truncated), [1] flags of SKIPPED sets (bit 0: a contig shorter than 30 bases, bit 1: more contigs than
 * max_set_contigs) — the host variant turns a non-zero flag into GF_E_INVAL; order unspecified */
int gf_quick_check_dev(gf_ctx* ctx, const void* d_seq, const void* d_contig_off, const void* d_set_off, size_t n_sets,
                       size_t max_set_contigs, int k, void* d_out, size_t cap, void* d_n_out);

/* ---- §8f-3, second stage: the contig merger's pairwise overlap evaluation (ContigsCompactor::Evaluate + IsScoreSignificant +
 * ContigsCompactorAction, ContigsCompactor-v0.2.0/ContigsMerger/ContigsCompactor.cpp:1572-1976, :108-159): an overlap alignment of
 * node i against node j (match +1, `mismatch` truncated to an int as the reference does, `indel`; ends may be clipped by up to
 * `max_clip` bases) classified like IsScoreSignificant.  Parameters = ContigsMerger's options (main.cpp:60-200): -i1 mismatch,
 * -i2 indel, -y max_clip, -c frac_min_overlap, -s frac_loss, -x min_overlap, -z min_overlap_scaffold; GAPPadder runs it with
 * -s 0.4 -i1 -2.0 -i2 -2.0 -x 12 -y 50 (MergeContigs.py:75).  The indel score must be integral (GF_E_UNSUPPORTED otherwise); contigs
 * up to 8190 bases.  Pairs are gf_qcpair {set, i, j} (ANY ordered node pair: i is the reference's pSeq1, j its pSeq2). */
typedef struct {
    double mismatch, indel, max_clip, frac_min_overlap, frac_loss, min_overlap, min_overlap_scaffold;
    double relax;             /* != 0: Evaluate's fRelax mode (FormMergedSeqFromPath, ContigsCompactor.cpp:1489): no significance test, res = 2 */
} gf_ovl_params;
typedef struct {
    int32_t res;              /* 0 no usable overlap, 1 overlap in [min_overlap_scaffold, min_overlap), 2 overlap >= min_overlap; -1: contig too long */
    int32_t row_end, col_end; /* end cell of the alignment (posRowEnd, posColEnd) */
    int32_t nclip;            /* bases clipped at one end */
    int32_t score;
    int32_t contained;        /* res != 0 only from here on: the action's contained flag */
    int32_t merged_len;       /* length of SetMergedStringConcat's string */
    int32_t overlap;          /* GetOverlapSize */
    int32_t containment;      /* IsContainment: such pairs form no edge (ContigsCompactor.cpp:672-674) */
    int32_t first_goes_first; /* 1: MODE_1_2 (node i then node j), 0: MODE_2_1 (:656-670) */
} gf_ovl_result;
int gf_overlap_evaluate(gf_ctx* ctx, const char* seq, const uint64_t* contig_off, const uint64_t* set_off, size_t n_sets, const gf_qcpair* pairs,
                        size_t n_pairs, const gf_ovl_params* params, gf_ovl_result* out);
int gf_overlap_evaluate_dev(gf_ctx* ctx, const void* d_seq, const void* d_contig_off, const void* d_set_off, const void* d_pairs, size_t n_pairs,
                            const gf_ovl_params* params, void* d_out);

/* ---- §8f-3 inside the step: the contig-merge ROUND for the gaps the pick left open (assemble_gaps.py:301-306 run_contigs_merge, which the
 * reference runs before it picks, :335-339; a gap its own contigs close gains nothing from merging).  For every gap g with
 * d_gap_best[g] == 0 and 2 .. 1 024 contigs in the list: exact-containment dedup (MergeContigs.drop_contained: a contig that occurs, on
 * either strand, inside another one goes; of identical ones the first stays), then — 2 .. max_set (<= 128) contigs left, those of
 * 30 .. 8 190 bases taking part — ContigsMerger itself: gf_quick_check's prefilter, gf_overlap_evaluate's edges (class 2, no containment),
 * strongly connected components in topological order, candidate roots and ends, a shortest-path DP per root with -overlap as edge length
 * (the 21 longest paths per root), removal of reverse-complement twin paths, and FormMergedSeqFromPath per path with Evaluate in its
 * relaxed mode (GraphUtils.cpp:625-859, 1028-1178, 1258-1344, 1422-1454; ContigsCompactor.cpp:773-983, 1456-1520).  The merged strings are
 * APPENDED to the contig list as records {gap, k = 0, kv = 0, n_nodes = nodes of the path, length, seq_off} in (gap, sorted path) order
 * (NEW_CONTIG_MERGE_1, _2, ... of each gap); *d_n_contigs and *d_seq_len grow.  Tombstones (length 0) take no part.  A list handed over
 * beyond its capacities (*d_n_contigs > contig_cap or *d_seq_len > seq_cap) is left as it is, counters included, and flags 32 / 64 are
 * set: the round is a no-op that keeps the overflow visible.  Everything is enqueued on the context's stream, no host
 * synchronisation.  A gap's contigs are taken in the order of its contigs.fa: the (k_list[i], kv_list[i]) pairs in list order, inside a pair
 * by (length descending, sequence) — n_k <= 16; n_k == 0: record order.
 * d_stats: u32[32] — [0] open gaps with 2 .. 1 024 contigs, [1] gaps that went through the merger, [2] gaps left alone for their size
 * (more than 1 024 contigs, or more than max_set after the dedup), [3] candidate pairs, [4] prefilter flags, [5] merged contigs, [6] capacity
 * flags of THIS call (1 node buffer, 2 pair list, 32 contig list, 64 sequence buffer: the caller raises), [7] contigs before the round,
 * [8] edges, [9] gaps that got merged contigs, [16] gaps left alone because their graph outgrew the round's limits (4 096 edges, 2 048
 * paths, the job list).  Follow with gf_pick_anchored2_from_dev(d_first = d_stats + 7) to pick among the merged contigs only. */
int gf_merge_open_gaps_dev(gf_ctx* ctx, void* d_contigs, void* d_n_contigs, size_t contig_cap, void* d_seq, void* d_seq_len,
                           size_t seq_cap, const void* d_gap_best, size_t n_gaps, const gf_ovl_params* params, int kmer_len_quick,
                           int max_set, const int* k_list, const int* kv_list, int n_k, void* d_stats);
/* gf_pick_anchored2_dev over the contigs from *d_first (u32, device) on: the pick words of earlier calls stay and compete (atomicMax) */
int gf_pick_anchored2_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                               int anchor_len, int anchor_len_short, const void* d_first, void* d_gap_best, void* d_n_closed);

/* ---- §8f-3 behind the CLI's merge_contigs: the merge round over contig SETS given as text, with its graph EXPORTED — per set what
 * MergeContigs.merge_contigs writes into the reference's files (MergeContigs.py:66-99): the de-duplicated set (contigs.fa_no_dup.fa), the
 * graph's edges (merge_edges.txt), the paths (…merge.info) with their merged strings, and the second dedup over [merged strings in order] +
 * [survivors in order] (contigs.fa).  Input as gf_quick_check: seq = the contigs' ASCII bases back to back (either case; upper-cased IN
 * PLACE on the device), contig_off[n_contigs + 1], set_off[n_sets + 1]; no contig may be empty.  The round is gf_merge_open_gaps_dev's
 * (every set counts as an open gap, its contigs in the order given), the limits are the same: 2 .. 1 024 contigs per set, 2 .. max_set
 * (<= 128) after the dedup, contigs of 30 .. 8 190 bases are the NODES and the others pass through.
 * Per set one gf_mset: status (GF_MSET_*), contigs the first dedup kept, its edges [edge_off, + n_edges), its paths [new_off, + n_new),
 * its final flags [final_off, + n_new + n_kept) and the paths among them that ended early.  A status of GF_MSET_SIZE / GF_MSET_GRAPH means
 * the set was LEFT ALONE (no edges, paths or final flags; kept flags only where the dedup ran, i.e. up to 1 024 contigs): the caller
 * handles such a set by other means.
 *   kept[n_contigs]   bit 0: the first dedup kept the contig (= MergeContigs.drop_contained: exact containment on either strand, longest
 *                     first, the first of identical copies stays); bit 1: it is a node.  Node n of a set = its n-th kept contig with bit 1.
 *   edges             {i, j, mode, overlap}: i, j = 2 * node + strand, mode 12 (i then j) or 21; class-2 pairs that are no containment, in
 *                     the prefilter's (i, j) order = the order of merge_edges.txt
 *   new               the paths after the reverse-complement twin removal with more than one node, in sorted order (NEW_CONTIG_MERGE_1, _2,
 *                     ...): n_nodes node bytes at paths[path_off], `length` bases at seq_off.  A path ends early when the running string
 *                     outgrows 8 190 bases (FormMergedSeqFromPath as restated in MergeContigs.merged_strings): n_nodes is then the number
 *                     of nodes actually merged, and the path counts in gf_mset.n_truncated / stats[GF_MX_TRUNCATED]
 *   finals            one flag per record of [the set's paths in order] + [its kept contigs in order]: the second dedup kept it
 * d_stats: u32[GF_MX_WORDS], see GF_MX_*.  Capacities: a total beyond its capacity sets a bit of stats[GF_MX_FLAGS]; then NOTHING but the
 * gf_mset records' counts, the kept flags and the statistics is written — no list is ever truncated — and the statistics hold the sizes
 * needed (GF_MX_EDGE_RECORDS, GF_MX_NEW_RECORDS, GF_MX_PATH_BYTES, GF_MX_SEQ_BYTES, GF_MX_FINALS).
 * Device variant: d_seq has room for seq_cap bytes, the first n_bytes hold the input; the merged strings are appended behind them
 * (gf_mnew.seq_off is an offset into d_seq; stats[GF_MX_SEQ_BYTES] = bytes of d_seq in use, as u64).  new_cap is the capacity of d_new AND
 * the room of the round's own contig list.  Everything is enqueued on the context's stream without a host synchronisation (workspaces
 * that have to grow synchronise when they are reallocated).
 * Host variant: one upload, the device call, ONE synchronisation to read the statistics that size the download, one download.
 * GF_E_NOSPACE when a flag is set (gf_last_error lists the sizes; nothing is returned truncated).  new_seq receives the merged strings,
 * gf_mnew.seq_off are offsets into it and stats[GF_MX_SEQ_BYTES] its bytes. */
enum { GF_MSET_MERGED = 0,   /* went through the merger (n_new may be 0) */
       GF_MSET_NOTHING = 1,  /* nothing to merge: fewer than 2 nodes (all kept contigs are final) */
       GF_MSET_SIZE = 2,     /* left alone for size: more than 1 024 contigs, or more than max_set after the dedup */
       GF_MSET_GRAPH = 3 };  /* left alone for the graph's limits: 4 096 edges, 2 048 paths, the job list, 1 024 records in the second dedup */
enum { GF_MX_TRIED = 0,          /* sets with status MERGED */
       GF_MX_NOTHING = 1, GF_MX_SKIPPED_SIZE = 2, GF_MX_SKIPPED_GRAPH = 3,   /* ... and with the other three */
       GF_MX_PAIRS = 4,          /* candidate pairs of the prefilter */
       GF_MX_EDGES = 5,          /* edges of the MERGED sets */
       GF_MX_PATHS = 6,          /* new contigs of the MERGED sets = the gf_mnew records their gf_mset point to */
       GF_MX_TRUNCATED = 7,      /* ... that ended early */
       GF_MX_FLAGS = 8,          /* capacity flags GF_MX_F_* */
       GF_MX_PATH_BYTES = 9, GF_MX_FINALS = 10,   /* bytes of d_paths / d_final in use */
       GF_MX_ROUND_ERR = 11,     /* the round's own flags (gf_merge_open_gaps_dev's word 6, its word 4 << 8) */
       GF_MX_SEQ_BYTES = 12,     /* u64 in words 12, 13 */
       GF_MX_NEW_RECORDS = 14, GF_MX_EDGE_RECORDS = 15,   /* records of d_new / d_edges in use */
       GF_MX_WORDS = 16 };
enum { GF_MX_F_EDGES = 1, GF_MX_F_NEW = 2, GF_MX_F_PATHS = 4, GF_MX_F_SEQ = 8, GF_MX_F_FINAL = 16,
       GF_MX_F_ROUND = 32 };     /* the round's pair list or node buffer (sized from the input: not the caller's to raise) */
typedef struct {
    uint32_t status, n_kept, n_edges, edge_off, n_new, new_off, final_off, n_truncated;
} gf_mset;
typedef struct {
    uint32_t i, j, mode, overlap;
} gf_medge;
typedef struct {
    uint32_t set, n_nodes, path_off, length;
    uint64_t seq_off;
} gf_mnew;
typedef struct {
    size_t edges, news, path_bytes, seq_bytes, finals; /* capacities of the host variant's edges / news / paths / new_seq / finals */
} gf_mcaps;
int gf_merge_sets_dev(gf_ctx* ctx, void* d_seq, size_t n_bytes, size_t seq_cap, const void* d_contig_off, const void* d_set_off, size_t n_sets,
                      size_t n_contigs, const gf_ovl_params* params, int kmer_len_quick, int max_set, void* d_sets, void* d_kept, void* d_edges,
                      size_t edge_cap, void* d_new, size_t new_cap, void* d_paths, size_t path_cap, void* d_final, size_t final_cap, void* d_stats);
int gf_merge_sets(gf_ctx* ctx, const char* seq, const uint64_t* contig_off, const uint64_t* set_off, size_t n_sets, const gf_ovl_params* params,
                  int kmer_len_quick, int max_set, const gf_mcaps* caps, gf_mset* sets, uint8_t* kept, gf_medge* edges, gf_mnew* news, uint8_t* paths,
                  char* new_seq, uint8_t* finals, uint32_t* stats);

/* ---- partial fills of the gaps no pick closed (run_pick_extended_contig, pick_contigs.py:361-539, called at assemble_gaps.py:367-368
 * with score 15; DESIGN.md "Extended fill").  Host twin: gappadder_amd/pick_contigs.py::pick_extended_sequence applied to a gap's
 * contigs in the order of pick_contigs.extension_order.  For every gap with d_gap_best == 0, over its contigs from *d_first on
 * (d_first NULL: from 0): per side the FIRST contig with a wanted (clipped) hit in the order (rank of the contig's (k, kv) among
 * k_list / kv_list, a pair not in the list — the merged contigs' k = kv = 0 — after every pair; length descending; bases ascending;
 * contig index), the same contig on both sides used on the right only, the parts sliced and oriented as the twin does and joined
 * by "NN".  Exact mode: the hits of anchor_hits (the anchor_len-base anchors of gf_pick_anchored_dev, any contig of >= anchor_len
 * bases); align mode: the first hit of align_hits' order with the wanted clip type (the hits of gf_pick_aligned_dev at threshold t).
 * d_ext: n_gaps gf_ext_pick (written for every gap); d_bases: the fills back to back in gap order (capacity base_cap); d_stats:
 * GF_EXT_WORDS u32, zeroed by the call.  Fills beyond base_cap are not written and set GF_EXT_OVERFLOW: the caller raises.  n_k <= 32.
 * Align mode: flanks of more than 1 024 bases give GF_E_UNSUPPORTED (as gf_pick_aligned_dev). */
#define GF_EXT_NONE 0xFFFFFFFFu
#define GF_EXT_MAX_PAIRS 32
typedef struct {
    uint32_t left, right;    /* contig of each side (before the same-contig rule), GF_EXT_NONE: none */
    uint32_t l_beg, l_len;   /* the left part: contig bases [l_beg, l_beg + l_len), reverse-complemented when l_rev */
    uint32_t r_beg, r_len;   /* the right part, likewise */
    uint64_t off;            /* the fill (left part + "NN" + right part) at d_bases + off ... */
    uint32_t len;            /* ... of len bases; 0 = no fill (no hit, or nothing but "NN") */
    uint8_t l_rev, r_rev;
    uint16_t reserved;
} gf_ext_pick;
/* words of d_stats: gaps with a fill; of them: left side only, right side only, both sides; u64 fill bases (words 4-5); overflow flag;
 * align mode: alignments beyond the cap and contigs beyond the seed limit (as gf_pick_aligned_dev's d_stats) */
#define GF_EXT_EXTENDED 0
#define GF_EXT_LEFT_ONLY 1
#define GF_EXT_RIGHT_ONLY 2
#define GF_EXT_BOTH 3
#define GF_EXT_BASES 4
#define GF_EXT_OVERFLOW 6
#define GF_EXT_ALIGN_DROPPED 8
#define GF_EXT_ALIGN_SEED_OVERFLOW 9
#define GF_EXT_WORDS 12
int gf_pick_extended_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int anchor_len,
                         const int* k_list, const int* kv_list, int n_k, const void* d_first, const void* d_gap_best, void* d_ext,
                         void* d_bases, size_t base_cap, void* d_stats);
int gf_pick_extended_aligned_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t,
                                 const int* k_list, const int* kv_list, int n_k, const void* d_first, const void* d_gap_best, void* d_ext,
                                 void* d_bases, size_t base_cap, void* d_stats);
/* the same with the gapped mode's hits (gf_pick_gapped_dev at threshold t; host twin pick_extended_sequence(mode="gapped")) */
int gf_pick_extended_gapped_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int t,
                                const int* k_list, const int* kv_list, int n_k, const void* d_first, const void* d_gap_best, void* d_ext,
                                void* d_bases, size_t base_cap, void* d_stats);

/* ---- flank-overlap joins of the gaps no pick closed (csrc/pick_join.hip; definition and host twin: gappadder_amd/flank_joins.py,
 * DESIGN.md §24).  A gap whose flanks overlap by o bases has no missing sequence: a contig that runs through the junction carries the
 * right anchor BEFORE the end of the left one, which the pick (span >= 0) drops.  For every gap with d_gap_best == 0, every contig of it
 * in [*d_first, min(*d_n_contigs, contig_cap)) (d_first NULL: from 0) and both strands (S = the contig, then its reverse complement):
 * at anchor_len, and where S does not carry both anchors of that length (or the gap has none), at anchor_len_short (0: none),
 * i = leftmost left anchor, j = rightmost right anchor; j >= i + a is the pick's case and skipped, else o = i + a - j is a candidate,
 * rejected in this order as far (o > max_overlap), short flank (o + min_context beyond a flank), no context (j < min_context or
 * i + a + min_context > |S|) or mismatch (more than max_mismatch differences between S and the left flank's last, or the right
 * flank's first, o + min_context bytes); the accepted candidates of a gap compete by (longer anchor, fewer mismatches, smaller o,
 * earlier contig, forward strand).  d_join: n_gaps gf_flank_join, written for every gap (all zero: closed, or no accepted candidate);
 * d_stats: GF_FJ_WORDS u32, zeroed by the call.  8 <= anchor_len_short < anchor_len <= 32, 1 <= max_overlap <= 1024,
 * 0 <= min_context <= 255, 0 <= max_mismatch <= 15: GF_E_INVAL otherwise; a flank of 65 536 bases or more: GF_E_UNSUPPORTED.  The
 * contig list is read as every consumer reads it (contig_cap <= 2^31 - 1).  Writes nothing but d_join, d_stats and scratch of the
 * context (24 bytes per gap; the flanks' last / first max_overlap + min_context bytes, built once per gf_set_gaps). */
typedef struct {
    uint32_t contig;                 /* the winner's index in the list */
    uint32_t left_pos, right_pos;    /* i and j on the oriented strand */
    uint16_t overlap;                /* o >= 1; 0: no join */
    uint16_t m_left, m_right;        /* differences of S against the left / right flank over the o + min_context compared bytes */
    uint16_t m_flanks;               /* differences between the flanks' own o overlapping bytes */
    uint16_t n_candidates, n_accepted;   /* of the gap, over contigs and strands (saturating) */
    uint16_t o_min, o_max;           /* over the accepted candidates */
    uint8_t level;                   /* the winner's anchor length */
    uint8_t flags;                   /* GF_FJ_F_* */
    uint16_t reserved;
} gf_flank_join;
#define GF_FJ_F_REVERSE 1     /* the winner is the reverse strand */
#define GF_FJ_F_AMBIGUOUS 2   /* the accepted candidates do not all have the same o */
#define GF_FJ_F_MULTI 4       /* on the winner an anchor of its level occurs at more than one position */
/* words of d_stats: open gaps seen, gaps joined, gaps with a usable join (joined, neither AMBIGUOUS nor MULTI), candidates, and of them
 * far, short flank, no context, mismatch; open gaps without anchors of either length */
#define GF_FJ_OPEN 0
#define GF_FJ_JOINED 1
#define GF_FJ_USABLE 2
#define GF_FJ_CANDIDATES 3
#define GF_FJ_FAR 4
#define GF_FJ_SHORT_FLANK 5
#define GF_FJ_NO_CONTEXT 6
#define GF_FJ_MISMATCH 7
#define GF_FJ_NO_ANCHORS 8
#define GF_FJ_WORDS 16
#define GF_FJ_MAX_OVERLAP 1024
#define GF_FJ_MAX_CONTEXT 255
#define GF_FJ_MAX_MISMATCH 15
int gf_pick_joins_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int anchor_len,
                      int anchor_len_short, int max_overlap, int min_context, int max_mismatch, const void* d_first, const void* d_gap_best,
                      void* d_join, void* d_stats);

/* ---- fill alternatives of the closed gaps (csrc/fill_alt.hip; definition and host twin: gappadder_amd/fill_alternatives.py).
 * The pick keeps one contig per gap (level, then span, then the earlier contig) and drops every other contig that carries both anchors.
 * For every gap with d_gap_best != 0 this round looks at them again.  A CANDIDATE is a contig of the gap in
 * [*d_first, min(*d_n_contigs, contig_cap)) (d_first NULL: from 0) to which gf_pick_anchored2_dev's own rule gives a non-zero word: its
 * level, span and strand.  The WINNER is the contig the gap's word names, re-located by its index (whatever *d_first is); when that
 * contig is no contig of the gap, or no candidate of the word's level, strand and span, the gap is LOST: its record holds the level and
 * GF_FA_F_LOST, its contigs are not looked at.  The oriented fill of a candidate is the span bytes between its anchors on the strand of
 * its hits (the reverse strand: the reverse complement, A<->T, C<->G, every other byte as it is).  A candidate below the winner's level is
 * LOWER (counted); one above it sets GF_FA_F_OUTRANKED and is counted as a candidate only; one of the winner's level is a PEER (and sets
 * GF_FA_F_OUTRANKED when its word is greater than the gap's): IDENTICAL (the winner's fill byte for byte), NEAR (Levenshtein distance
 * to the winner's fill <= max_dist, unit costs) or FAR.  The RIVAL is the NEAR or FAR peer with the largest word.  d_alt: n_gaps
 * gf_fill_alt, written for every gap (all zero: the gap is open); d_alt_contig: NULL, or contig_cap gf_fill_alt_contig, written for
 * every index in [0, min(*d_n_contigs, contig_cap)) (all zero: no candidate, or above the winner's level); d_stats: GF_FA_WORDS u32,
 * zeroed by the call.  8 <= anchor_len_short < anchor_len <= 32 (or anchor_len_short 0), 1 <= max_dist <= GF_FA_MAX_DIST: GF_E_INVAL
 * otherwise.  The contig list is read as every consumer reads it (contig_cap <= 2^31 - 1).  Writes nothing but d_alt, d_alt_contig,
 * d_stats and scratch of the context (48 bytes per gap). */
typedef struct {
    uint32_t contig;                 /* the winner's index in the list */
    uint32_t rival;                  /* the rival's index; 0 without GF_FA_F_HAS_RIVAL */
    uint32_t fill_len, rival_len;    /* bytes of the winner's and the rival's oriented fill */
    uint32_t lcp;                    /* longest common prefix of the two fills */
    uint32_t lcs;                    /* longest common suffix of what follows the prefix: the fills differ in [lcp, len - lcs) */
    uint32_t len_min, len_max;       /* fill lengths over the winner and its peers */
    uint16_t n_candidates;           /* all candidates, the winner included (this and the next four saturate at 65 535) */
    uint16_t n_lower, n_identical, n_near, n_far;
    uint16_t dist;                   /* the rival's distance; GF_FA_DIST_FAR for a FAR rival */
    uint8_t level;                   /* the winner's anchor length */
    uint8_t flags;                   /* GF_FA_F_* */
    uint16_t reserved;
} gf_fill_alt;
typedef struct {
    uint32_t length;                 /* bytes of the candidate's fill */
    uint16_t dist;                   /* the distance of a NEAR peer, else GF_FA_DIST_FAR */
    uint8_t cls;                     /* GF_FA_C_* */
    uint8_t strand;                  /* the strand of the candidate's hits */
} gf_fill_alt_contig;
#define GF_FA_F_REVERSE 1         /* the winner's hits are on the reverse strand */
#define GF_FA_F_RIVAL_REVERSE 2
#define GF_FA_F_HAS_RIVAL 4       /* the gap is contested */
#define GF_FA_F_LENGTH_VARIES 8   /* len_min != len_max */
#define GF_FA_F_OUTRANKED 16      /* a candidate's word is greater than the gap's */
#define GF_FA_F_LOST 32           /* the gap's word does not lead back to a candidate */
#define GF_FA_C_NONE 0
#define GF_FA_C_WINNER 1
#define GF_FA_C_IDENTICAL 2
#define GF_FA_C_NEAR 3
#define GF_FA_C_FAR 4
#define GF_FA_C_LOWER 5
/* words of d_stats: closed gaps seen, contested gaps, gaps with LENGTH_VARIES, candidates, and of them lower, identical, near, far;
 * outranked gaps, lost gaps */
#define GF_FA_CLOSED 0
#define GF_FA_CONTESTED 1
#define GF_FA_LENGTH_VARIES 2
#define GF_FA_CANDIDATES 3
#define GF_FA_LOWER 4
#define GF_FA_IDENTICAL 5
#define GF_FA_NEAR 6
#define GF_FA_FAR 7
#define GF_FA_OUTRANKED 8
#define GF_FA_LOST 9
#define GF_FA_WORDS 16
#define GF_FA_MAX_DIST 31
#define GF_FA_DIST_FAR 0xFFFF
int gf_fill_alts_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, int anchor_len,
                     int anchor_len_short, int max_dist, const void* d_first, const void* d_gap_best, void* d_alt, void* d_alt_contig,
                     void* d_stats);

/* ---- read support of the closed gaps (csrc/fill_support.hip; definition and host twin: gappadder_amd/read_support.py).
 * For every gap with d_gap_best != 0 one record that says how the k-mers of the gap's fill are backed by the gap's own pool: the
 * evaluated windows are the k-windows of the winning contig (as stored) that hold at least one base strictly between the two flank hits
 * of the pick — the windows over the junction when nothing lies between them —, starts max(0, b0 - k + 1) .. min(length - k,
 * max(b1, b0) - 1) for the body [b0, b1); a window's support = the read windows of the pool (rows d_pool_off[g] .. d_pool_off[g + 1],
 * offsets 0 .. read_len - k, both strands, windows over a base of d_nmask_or_null skipped as the assembly's count phase skips them) whose
 * canonical k-mer is the window's; a window with a byte other than A, C, G, T has support 0.  The hits: with d_ctg_pick_or_null the
 * winning contig's gf_ctg_pick (the align and gapped modes); without it the exact anchors re-located by gf_pick_anchored_dev's rule at
 * the anchor length the word carries (anchor_long or anchor_short, the lengths the pick ran at; anchor_short 0: one length) — and a
 * closed gap whose contig does not carry that pick with the word's (unsaturated) span is counted in d_stats[GF_FS_MISMATCH] and gets
 * the zero record, as does an open gap.  16 <= k <= 64 (GF_E_UNSUPPORTED otherwise); the contig list is read as every consumer reads
 * it ([0, min(*d_n_contigs, contig_cap)), winners only).  A fill of any length is evaluated, in chunks that stream the pool again.
 * d_support: gf_fill_support per gap (every record is written); d_stats: u32[GF_FS_WORDS] (set by the call).  pool_rows: rows of the
 * pool array.  GF_E_STATE without flanks. */
typedef struct {
    uint32_t n_windows;   /* evaluated windows */
    uint32_t n_zero;      /* ... with support 0 */
    uint32_t n_below;     /* ... with support < min_count (the zero ones included) */
    uint32_t min, max;    /* smallest and largest support */
    uint32_t zero_run;    /* longest run of consecutive windows with support 0 */
    uint64_t sum;         /* of the supports: mean = sum / n_windows */
} gf_fill_support;
#define GF_FS_GAPS 0      /* gaps evaluated */
#define GF_FS_MISMATCH 1  /* closed gaps whose winning contig does not carry the word's pick */
#define GF_FS_WINDOWS 2   /* u64: windows evaluated */
#define GF_FS_WORDS 4
int gf_fill_support_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                        int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                        const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int k, int min_count,
                        void* d_support, void* d_stats);

/* ---- consensus polish of the closed gaps (csrc/fill_polish.hip; definition and host twin: gappadder_amd/polish.py).
 * For every gap with d_gap_best != 0: the rows of the gap's pool (d_pool_off[g] .. d_pool_off[g + 1], bases of d_nmask_or_null masked), each
 * as stored and reverse-complemented, are placed without gaps on the winning contig c (as stored, n bases) — a diagonal d puts read
 * base i on c[d + i]; it is accepted with an overlap of at least min_overlap bases, at most max_mismatch unmasked read bases that differ
 * from the contig, and one of the read's seed windows [j * seed, (j + 1) * seed), j < read_len / seed, wholly inside the overlap, free
 * of masked bases and equal to the contig.  A row whose accepted (strand, diagonal) pairs have ONE best (fewest mismatches, then longest
 * overlap) is placed there and votes its unmasked bases on the columns of the body [b0, b1) — located exactly as gf_fill_support_dev
 * locates it, with the same arguments and the same GF_PL_MISMATCH rule —; a row with several best pairs is ambiguous and does not vote.
 * A body column becomes the base with the most votes (the smaller code on a tie) when that base has at least min_votes votes and
 * strictly more than the column's own base; nothing outside the body changes.  The polished contig (stored orientation) goes to
 * d_bases at an offset taken from the u64 counter d_stats[GF_PL_BASES] (any order), and the gap's record says where.  A contig of more
 * than GF_PL_MAX_CONTIG bases, or with a byte other than A, C, G, T, is copied unchanged and flagged (n_cols set, the other counts 0).  An
 * open gap and a mismatch get the zero record.  A contig that does not fit below base_cap sets GF_PL_F_OVERFLOW (off = len = 0) and
 * counts in d_stats[GF_PL_OVERFLOW].  seed 12..32, max_mismatch 0..15, seed <= min_overlap <= read_len, min_votes >= 1 and
 * read_len / seed > max_mismatch (then every placement inside the contig within the budget has a clean seed): GF_E_UNSUPPORTED otherwise.
 * d_polish: gf_fill_polish per gap (every record is written); d_stats: u32[GF_PL_WORDS] (set by the call).  GF_E_STATE without flanks. */
typedef struct {
    uint64_t off;              /* of the polished contig in d_bases */
    uint32_t len;              /* its bases = the contig's */
    uint32_t flags;            /* GF_PL_F_* */
    uint32_t n_cols;           /* body columns */
    uint32_t n_changed;        /* ... that the vote changed */
    uint32_t n_uncovered;      /* ... without any vote */
    uint32_t reads_placed;     /* rows placed (anywhere on the contig) */
    uint32_t reads_ambiguous;  /* rows with more than one best placement */
    uint32_t reserved;
} gf_fill_polish;
#define GF_PL_F_LONG 1         /* skipped: more than GF_PL_MAX_CONTIG bases */
#define GF_PL_F_NON_ACGT 2     /* skipped: a byte other than A, C, G, T */
#define GF_PL_F_OVERFLOW 4     /* d_bases is full: nothing was written */
#define GF_PL_MAX_CONTIG 8192
#define GF_PL_GAPS 0           /* gaps polished (not skipped) */
#define GF_PL_MISMATCH 1       /* closed gaps whose winning contig does not carry the word's pick */
#define GF_PL_SKIPPED_LONG 2
#define GF_PL_SKIPPED_NON_ACGT 3
#define GF_PL_CHANGED 4        /* u64: columns changed */
#define GF_PL_PLACED 6         /* u64: rows placed */
#define GF_PL_AMBIGUOUS 8      /* u64: rows ambiguous */
#define GF_PL_BASES 10         /* u64: bases handed out in d_bases (beyond base_cap: overflow) */
#define GF_PL_OVERFLOW 12      /* contigs that did not fit */
#define GF_PL_WORDS 16
int gf_fill_polish_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                       int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                       const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                       int min_overlap, int min_votes, void* d_polish, void* d_bases, size_t base_cap, void* d_stats);

/* ---- indel-aware consensus polish of the closed gaps (csrc/fill_polish_gapped.hip, fill_place_split.hpp; definition and host twin:
 * gappadder_amd/polish_gapped.py).  gf_fill_polish_dev's arguments and rules, plus max_indel (1..16, else
 * GF_E_UNSUPPORTED): beside the gapless candidates a row has split candidates — two of its seeded diagonals at most max_indel apart, the
 * breakpoint between a clean seed of the first and a clean seed of the second where the two parts differ from the contig least (leftmost
 * column of the stored contig on a tie), at the cost of its mismatches plus two.  The one best candidate of a row (cost, then overlap)
 * places it; a row placed split votes its columns and, once, its event: a deletion of contig columns [p, p + g) or an insertion of up
 * to 16 read bases before column p, when it lies in the body.  An event with at least min_votes votes and more votes than placed rows
 * that cross its site (p -/+ seed) in one piece without voting it passes; passing events are accepted by (votes descending, p, deletion
 * first, length, bases) unless they touch an accepted one, insertions up to GF_PLG_MAX_INSERTED bases per contig (else
 * GF_PL_F_INS_CAP); more than GF_PLG_MAX_EVENTS distinct events in one body: GF_PL_F_EVENTS, none applied.  The polished contig may
 * be up to GF_PLG_MAX_INSERTED bases longer than the contig; its place in d_bases is taken from d_stats[GF_PL_BASES] once its length
 * is known.  d_polish: gf_fill_polish_gapped per gap; d_stats: u32[GF_PLG_WORDS], gf_fill_polish_dev's words at their indices. */
typedef struct {
    uint64_t off;              /* the first 40 bytes: gf_fill_polish's fields with their meaning; len is the OUTPUT length */
    uint32_t len;
    uint32_t flags;            /* GF_PL_F_* */
    uint32_t n_cols;
    uint32_t n_changed;        /* substituted columns (whether or not an accepted deletion removes them) */
    uint32_t n_uncovered;
    uint32_t reads_placed;     /* rows placed, split ones included */
    uint32_t reads_ambiguous;
    uint32_t reserved;
    uint32_t n_events;         /* events accepted */
    uint32_t n_inserted;       /* bases they insert */
    uint32_t n_deleted;        /* columns they delete */
    uint32_t reads_split;      /* rows placed split */
    uint32_t events_seen;      /* distinct in-body events (GF_PLG_MAX_EVENTS + 1 with GF_PL_F_EVENTS) */
    uint32_t events_outside;   /* split rows whose event lies outside the body */
} gf_fill_polish_gapped;
#define GF_PL_F_EVENTS 8       /* more than GF_PLG_MAX_EVENTS distinct events in the body: none applied */
#define GF_PL_F_INS_CAP 16     /* a passing insertion was dropped: more than GF_PLG_MAX_INSERTED inserted bases */
#define GF_PLG_MAX_EVENTS 64
#define GF_PLG_MAX_INSERTED 64
#define GF_PLG_MAX_INDEL 16
#define GF_PLG_EVENTS 16       /* u64: events accepted */
#define GF_PLG_INSERTED 18     /* u64: bases inserted */
#define GF_PLG_DELETED 20      /* u64: columns deleted */
#define GF_PLG_SPLIT 22        /* u64: rows placed split */
#define GF_PLG_F_EVENTS 24     /* gaps flagged GF_PL_F_EVENTS */
#define GF_PLG_F_INS_CAP 25    /* gaps flagged GF_PL_F_INS_CAP */
#define GF_PLG_WORDS 32
int gf_fill_polish_gapped_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                              int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                              const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed,
                              int max_mismatch, int min_overlap, int min_votes, int max_indel, void* d_polish, void* d_bases, size_t base_cap,
                              void* d_stats);

/* ---- per-base pile-up of the closed gaps (csrc/fill_pileup.hip, fill_vote.hpp; definition and host twin: gappadder_amd/pileup.py,
 * DESIGN.md §23).  gf_fill_polish_dev's pool, shared arguments, placement rule (seed, max_mismatch, min_overlap) and GF_PL_MISMATCH
 * rule.  A placed row votes its unmasked bases on EVERY column of the winning contig c (as stored, n bases) it overlaps: counter
 * fwd[b] when the row lies on c as stored, rev[b] when its reverse complement does, b the base as it reads on c.  The track entry of a
 * column is u16 fwd[4], rev[4], each min(count, 65535); the n entries of a contig go to d_track at an offset taken from the u64
 * counter d_stats[GF_PU_ENTRIES] (any order).  Over the body [b0, b1), with the unsaturated counts, depth = their sum, agree = fwd[cur]
 * + rev[cur], alt = the largest fwd[b] + rev[b] over b != cur: a column is uncovered (depth 0), thin (0 < depth < min_depth), contested
 * (depth >= min_depth and 100 * agree < min_agree * depth), minority (alt > agree), one_strand (depth >= min_depth and one strand's four
 * counters all 0); low = uncovered, thin or contested.  low_run / low_run_col: the longest run of consecutive low body columns and its
 * first column (body-relative, the smallest on a tie, 0 without one); min_depth_seen / min_depth_col likewise.  A contig of more than
 * GF_PL_MAX_CONTIG bases, or with a byte other than A, C, G, T, is flagged and counted (n_cols set, everything else 0, no track).  A
 * track that does not fit below track_cap_entries sets GF_PU_F_OVERFLOW (off = len = 0, nothing written, the summary still computed)
 * and counts in d_stats[GF_PU_OVERFLOW].  d_track_or_null null with track_cap_entries 0: records only (off = len = 0, nothing handed
 * out, no overflow).  min_depth >= 1, 1 <= min_agree <= 100, the placement rule as for gf_fill_polish_dev: GF_E_UNSUPPORTED otherwise.
 * d_records: gf_fill_pileup per gap (every record is written; all zero for an open gap and a mismatch); d_stats: u32[GF_PU_WORDS]
 * (set by the call).  The rows' placements are kept in a scratch array of the context (4 bytes per pool row).  GF_E_STATE without flanks. */
typedef struct {
    uint64_t off;              /* the first track entry of the contig in d_track */
    uint32_t len;              /* its entries = the contig's bases; 0 when no track was written */
    uint32_t flags;            /* GF_PU_F_* */
    uint32_t n_cols;           /* body columns */
    uint32_t n_uncovered;
    uint32_t n_thin;
    uint32_t n_contested;
    uint32_t n_minority;
    uint32_t n_one_strand;
    uint32_t low_run;          /* the longest run of low body columns ... */
    uint32_t low_run_col;      /* ... and its first column, body-relative */
    uint32_t min_depth_seen;   /* the smallest depth of a body column ... */
    uint32_t min_depth_col;    /* ... and the first column with it, body-relative */
    uint64_t depth_sum;        /* the sum of the body columns' depths (unsaturated) */
    uint32_t reads_placed;     /* rows placed (anywhere on the contig) */
    uint32_t reads_ambiguous;  /* rows with more than one best placement */
} gf_fill_pileup;              /* 72 bytes */
#define GF_PU_F_LONG 1         /* skipped: more than GF_PL_MAX_CONTIG bases */
#define GF_PU_F_NON_ACGT 2     /* skipped: a byte other than A, C, G, T */
#define GF_PU_F_OVERFLOW 4     /* d_track is full: nothing was written */
#define GF_PU_GAPS 0           /* gaps piled up (not skipped) */
#define GF_PU_MISMATCH 1       /* closed gaps whose winning contig does not carry the word's pick */
#define GF_PU_SKIPPED_LONG 2
#define GF_PU_SKIPPED_NON_ACGT 3
#define GF_PU_PLACED 4         /* u64: rows placed */
#define GF_PU_AMBIGUOUS 6      /* u64: rows ambiguous */
#define GF_PU_ENTRIES 8        /* u64: track entries handed out (beyond track_cap_entries: overflow) */
#define GF_PU_LOW 10           /* u64: low body columns */
#define GF_PU_OVERFLOW 12      /* contigs whose track did not fit */
#define GF_PU_WORDS 16
int gf_fill_pileup_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                       int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                       const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                       int min_overlap, int min_depth, int min_agree, void* d_records, void* d_track_or_null, size_t track_cap_entries,
                       void* d_stats);

/* ---- pair-span check of the closed gaps (csrc/fill_pairs.hip; definition and host twin: gappadder_amd/pair_span.py).
 * One call per library, on THAT library's pool (gf_build_pools_dev: d_pool_packed, d_pool_off, d_pool_read_ids — read = 2 * pair + mate,
 * per gap ordered by (mate, pair), every read at most once per gap).  For every gap with d_gap_best != 0 the rows of the gap's slice are
 * placed on the winning contig c (as stored, n bases) by gf_fill_polish_dev's rule with the same seed / max_mismatch / min_overlap: a
 * row is PLACED (one best (strand, diagonal d)), ambiguous or unplaced.  Rows with the ids r and r ^ 1 both in the slice are a complete
 * pair; it is placed when both rows are; a placed pair is proper when its mates lie on opposite strands and the strand-0 mate's
 * diagonal d_f <= the strand-1 mate's d_r, and misoriented otherwise.  insert = d_r + read_len - d_f (signed).  With lo = is_mean -
 * z * is_sd and hi = is_mean + z * is_sd a proper pair is in range when lo < insert < hi, short when insert <= lo, long when insert >= hi.
 * A proper pair of any class spans the body [b0, b1) — located as gf_fill_support_dev locates it, same arguments, same mismatch rule —
 * when d_f <= b0 and b1 <= d_r + read_len.  Every in-range pair covers the columns [max(0, d_f), min(n, d_r + read_len)): min_cover,
 * min_col (the smallest column with that cover) and n_unspanned (columns with cover 0) are taken over the body; all 0 for an empty body.
 * A contig of more than GF_PL_MAX_CONTIG bases, or with a byte other than A, C, G, T, is flagged and counted (rows set, everything else 0).
 * An open gap and a mismatch get the zero record.  seed, max_mismatch, min_overlap as for gf_fill_polish_dev, z >= 1, is_sd >= 0:
 * GF_E_UNSUPPORTED otherwise.  d_nmask_or_null: mask rows aligned with the pool's rows.  d_place_scratch: u32 per pool row
 * (pool_cap_rows of them; the rows' placements, overwritten).  d_rec: gf_fill_pairs per gap (every record is written: the plane of this
 * library in a [n_lib][n_gaps] array); d_stats: u32[GF_PS_WORDS] (set by the call).  GF_E_STATE without flanks. */
typedef struct {
    uint32_t flags;            /* GF_PS_F_* */
    uint32_t rows;             /* rows of the library's pool for the gap */
    uint32_t pairs_complete;   /* both mates in the pool */
    uint32_t pairs_placed;     /* ... and both placed */
    uint32_t n_proper;         /* placed pairs facing each other (FR) */
    uint32_t n_misoriented;    /* placed pairs that do not */
    uint32_t n_in_range;       /* proper pairs by insert size */
    uint32_t n_short;
    uint32_t n_long;
    uint32_t n_span;           /* proper pairs that span the body */
    int64_t span_insert_sum;   /* the sum of their inserts */
    uint32_t n_cols;           /* body columns */
    uint32_t min_cover;        /* the fewest in-range pairs over a body column */
    uint32_t min_col;          /* the first column with that few */
    uint32_t n_unspanned;      /* body columns no in-range pair covers */
} gf_fill_pairs;
#define GF_PS_F_LONG 1         /* skipped: more than GF_PL_MAX_CONTIG bases */
#define GF_PS_F_NON_ACGT 2     /* skipped: a byte other than A, C, G, T */
#define GF_PS_GAPS 0           /* gaps examined (not skipped) */
#define GF_PS_MISMATCH 1       /* closed gaps whose winning contig does not carry the word's pick */
#define GF_PS_SKIPPED_LONG 2
#define GF_PS_SKIPPED_NON_ACGT 3
#define GF_PS_UNSPANNED 4      /* examined gaps with n_unspanned > 0 */
#define GF_PS_COMPLETE 6       /* u64 each: complete, placed, proper, in-range, spanning pairs */
#define GF_PS_PLACED 8
#define GF_PS_PROPER 10
#define GF_PS_IN_RANGE 12
#define GF_PS_SPAN 14
#define GF_PS_WORDS 16
int gf_fill_pairs_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, const void* d_pool_read_ids,
                      size_t pool_cap_rows, int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                      const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, int seed, int max_mismatch,
                      int min_overlap, int is_mean, int is_sd, int z, void* d_place_scratch, void* d_rec, void* d_stats);
/* gf_fill_pairs_dev on slices only whose head is ordered by (mate side, pair): d_head_off (u64[n_gaps + 1]) gives the head's rows of gap g as
 * d_head_off[g + 1] - d_head_off[g]; the rows behind it are whole pairs ordered by read id (a library's closing pool: gf_closing_pools_dev).
 * A read with a row in both parts counts at its first row, and so does its mate.  d_head_off_or_null == NULL: gf_fill_pairs_dev. */
int gf_fill_pairs_split_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, const void* d_pool_read_ids,
                            size_t pool_cap_rows, const void* d_head_off_or_null, int read_len, const void* d_contigs, const void* d_n_contigs,
                            size_t contig_cap, const void* d_seq, const void* d_gap_best, const void* d_ctg_pick_or_null, int anchor_long,
                            int anchor_short, int seed, int max_mismatch, int min_overlap, int is_mean, int is_sd, int z, void* d_place_scratch,
                            void* d_rec, void* d_stats);

/* ---- anchored pair span (csrc/fill_anchor.hip; definition and host twin: gappadder_amd/pair_anchors.py).  Called behind
 * gf_fill_pairs_dev of the SAME library in the same step, with that call's pool offsets, read ids, shared arguments and d_place_scratch
 * (an INPUT here: the rows' placement words as that call left them).  A tagger hit h of [0, min(*d_n_taghits, hit_cap)) with to_mate == 1
 * and kind GF_KIND_DISCORDANT or GF_KIND_UNMAP says: record A = d_recs[h.rec] is anchored in a flank of gap h.gap and A's mate B = A.read ^ 1
 * was recruited for it.  The hit is kept when A has clipflag == 0, flag & (0x100 | 0x800 | 4) == 0, a read (the low 32 bits of A.read are
 * not 0xFFFFFFFF), A0 = A.pos - 1 < gap.start (a left anchor) or >= gap.end (a right one), and B has a row in the gap's id slice; of
 * several kept hits of one (gap, B) the one with the smallest (A0 << 1 | sA), sA = (flag >> 4) & 1, counts.  For a closed gap with the
 * winning contig c (n bases, strand bit rev, body [b0, b1): all as gf_fill_pairs_dev) A lies, virtually and unbounded, on
 *   rev = 0: strand sA,     column b0 - (start - A0) (left) or b1 + (A0 - end) (right)
 *   rev = 1: strand 1 - sA, column b1 + (start - A0) - read_len (left) or b0 - (A0 - end) - read_len (right)
 * and together with a PLACED row B it is one placed pair, classified word for word as gf_fill_pairs_dev classifies its pairs (proper /
 * misoriented, insert, in range / short / long against is_mean -/+ z * is_sd, spanning).  Every in-range pair covers the columns
 * [max(0, d_f), min(n, d_r + read_len)) with dev = insert - is_mean: min_cover, min_col, n_unspanned over the body as there, and among the
 * body columns covered by at least min_pairs pairs (n_eval of them) the one with the smallest and the one with the largest mean dev, as
 * (column, pairs, sum of dev); means are compared exactly, the smaller column wins a tie.  A contig gf_fill_pairs_dev skips is skipped
 * (flags and rows); an open gap and a mismatch get the zero record.  min_pairs >= 1, z >= 1, is_sd >= 0, z * is_sd < 2^20:
 * GF_E_UNSUPPORTED otherwise.  d_anchor: u64 per pool row (pool_cap_rows of them; overwritten).  d_rec: gf_fill_anchors per gap;
 * d_stats: u32[GF_PA_WORDS] (set by the call).  Two kernels on the context's stream, no host synchronisation. */
typedef struct {
    uint32_t flags;            /* GF_PS_F_* */
    uint32_t rows;             /* rows of the library's pool for the gap */
    uint32_t n_anchored;       /* rows whose mate is anchored in a flank */
    uint32_t n_placed;         /* ... and that are PLACED: the placed pairs */
    uint32_t n_proper;
    uint32_t n_misoriented;
    uint32_t n_in_range;
    uint32_t n_short;
    uint32_t n_long;
    uint32_t n_left;           /* in-range pairs with a left anchor */
    uint32_t n_span;           /* proper pairs that span the body */
    uint32_t n_cols;           /* body columns */
    int64_t span_insert_sum;   /* the sum of the spanning pairs' inserts */
    int64_t dev_sum;           /* the sum of insert - is_mean over the in-range pairs */
    uint32_t min_cover;        /* the fewest in-range pairs over a body column */
    uint32_t min_col;          /* the first column with that few */
    uint32_t n_unspanned;      /* body columns no in-range pair covers */
    uint32_t n_eval;           /* body columns with at least min_pairs in-range pairs */
    uint32_t dev_min_col;      /* of those, the column with the smallest mean dev: its pairs and their sum of dev */
    uint32_t dev_min_n;
    int64_t dev_min_sum;
    uint32_t dev_max_col;      /* ... and the one with the largest */
    uint32_t dev_max_n;
    int64_t dev_max_sum;
} gf_fill_anchors;
#define GF_PA_GAPS 0           /* gaps examined (not skipped) */
#define GF_PA_MISMATCH 1
#define GF_PA_SKIPPED_LONG 2
#define GF_PA_SKIPPED_NON_ACGT 3
#define GF_PA_KEPT 4           /* hits kept (before the smallest of a (gap, read) is chosen) */
#define GF_PA_DROP_CLIPPED 5   /* hits dropped: a clipped anchor */
#define GF_PA_DROP_IN_GAP 6    /* ... an anchor that starts inside the gap */
#define GF_PA_DROP_SECONDARY 7 /* ... a secondary or supplementary record */
#define GF_PA_ABSENT 8         /* ... the mate has no row in the gap's slice */
#define GF_PA_DROP_OTHER 9     /* ... to_mate == 0, another kind, an unmapped record, no read, a record or gap out of range */
#define GF_PA_ANCHORED 10      /* u64 each: anchored, placed, proper, in-range, spanning pairs */
#define GF_PA_PLACED 12
#define GF_PA_PROPER 14
#define GF_PA_IN_RANGE 16
#define GF_PA_SPAN 18
#define GF_PA_WORDS 20
int gf_fill_pairs_anchored_dev(gf_ctx* ctx, const void* d_pool_off, const void* d_pool_read_ids, size_t pool_cap_rows, int read_len,
                               const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, const void* d_gap_best,
                               const void* d_ctg_pick_or_null, int anchor_long, int anchor_short, const void* d_place_scratch,
                               const void* d_recs, size_t n_recs, const void* d_taghits, const void* d_n_taghits, size_t hit_cap, int is_mean,
                               int is_sd, int z, int min_pairs, void* d_anchor, void* d_rec, void* d_stats);

/* ---- gap size from the gap-spanning read pairs (csrc/gap_span.hip; definition and host twin: gappadder_amd/gap_span.py).
 * One library's records against the gap table of gf_set_gaps, for EVERY gap, open or closed; it needs neither the recruitment nor a contig.
 * With dist2 = is_mean + 3 * is_sd (the tagger's own window: the call shares the tagger's bin map for that dist2), lo = is_mean - z * is_sd -
 * shift, hi = is_mean + z * is_sd + shift: record A is a CANDIDATE of gap g = [start, end) on scaffold s iff flag & 1, flag & (4 | 8 | 0x100 |
 * 0x800) == 0, flag & 0x10 == 0 and flag & 0x20 != 0 (A forward, its mate reverse), ref == mate_ref == s < n_scaffolds, pos >= 1,
 * mate_pos >= 1, tlen > 0, and with A0 = pos - 1, M0 = mate_pos - 1, M1 = A0 + tlen: A0 + read_len <= start, start - A0 <= dist2,
 * end <= M0 < M1.  The mate's own MAPQ and clip flag are not in A's record and are not consulted.  A candidate lands in exactly one
 * counter, tested in this order: n_multi (end[g - 1] > A0 or start[g + 1] < M1, each for a neighbour on the same scaffold), n_clipped
 * (clipflag != 0), n_lowq (mapq < min_mapq), n_low (tlen < lo), n_high (tlen > hi), else accepted: n, sum, sum_sq, tlen_min, tlen_max.
 * d_keys_or_null: the library's key column (gf_alnrec_keys_dev; n + 1 entries) — streamed instead of the records, which are then fetched
 * only for what passes the bin maps; a key that disagrees with its record drops the record.  A record with ref >= n_scaffolds or '*', on
 * a scaffold without gaps or beyond the bin map's span is ignored and indexes nothing.  z >= 1, shift >= 0, is_mean >= 0, is_sd >= 0,
 * 1 <= read_len, 0 <= min_mapq <= 255, hi < 2^20 (sum_sq then fits 64 bits for every n < 2^32): GF_E_UNSUPPORTED otherwise; GF_E_STATE
 * without gaps.  d_rec: gf_gap_span per gap; d_stats: u32[GF_GS_WORDS]; both are cleared and set by the call, on the context's stream,
 * without a host synchronisation (but for the first use of a dist2 on the context, which builds its bin map as the tagger would). */
typedef struct {
    uint32_t flags;      /* GF_GS_F_PAIRS iff n >= 1 */
    uint32_t n_cand;     /* candidates: the seven counters below together */
    uint32_t n;          /* accepted pairs */
    uint32_t n_multi;
    uint32_t n_clipped;
    uint32_t n_lowq;
    uint32_t n_low;
    uint32_t n_high;
    uint32_t tlen_min;   /* of the accepted pairs; 0 when n == 0 */
    uint32_t tlen_max;
    int64_t sum;         /* of the accepted pairs' tlen */
    uint64_t sum_sq;     /* ... of tlen^2 */
    uint64_t reserved;
} gf_gap_span;
#define GF_GS_F_PAIRS 1
#define GF_GS_CANDIDATES 0     /* u64 each, over the gaps: candidates, accepted, multi, clipped, lowq, low, high */
#define GF_GS_ACCEPTED 2
#define GF_GS_MULTI 4
#define GF_GS_CLIPPED 6
#define GF_GS_LOWQ 8
#define GF_GS_LOW 10
#define GF_GS_HIGH 12
#define GF_GS_GAPS_WITH_PAIRS 14   /* u32: gaps with n >= 1 */
#define GF_GS_WORDS 16
int gf_gap_span_dev(gf_ctx* ctx, const void* d_recs, const void* d_keys_or_null, size_t n, int read_len, int is_mean, int is_sd, int z,
                    int shift, int min_mapq, void* d_rec, void* d_stats);

/* ---- the second assembly round inside the step (assemble_gaps.py:328-368 with collect_both_unmapped_reads.py's recruitment; DESIGN.md
 * "Second round").  Predicate (the CLI's kmer_recruit_unmapped): a both-unmapped pair is recruited for an open gap when one of its reads shares
 * a canonical k-mer with one of the gap's round-1 contigs; k-mers touching a non-ACGT contig base or an N-masked read base do not count.
 * Every count below is exact whatever the capacities: a caller sizes from them and runs again (Pipeline.prepare). */
#define GF_R2_MAX_LIBS 16
/* candidate pairs of one library: every pair one of whose records has FLAG & 12 == 12 (`samtools view -f 12`), listed once (u32 pair ids,
 * unordered); d_pair_bits: (n_reads / 2 + 31) / 32 u32 words of scratch; *d_n_pairs (u32) = candidates found (beyond cap: not stored). */
int gf_both_unmapped_reads_dev(gf_ctx* ctx, const void* d_recs, size_t n_recs, size_t n_reads, void* d_pair_bits, void* d_pairs, size_t cap,
                               void* d_n_pairs);
/* the (canonical k-mer, gap) table of the contigs [0, *d_n_contigs) whose gap has d_gap_best == 0: 24-byte slots, 2^log2_slots of them
 * (cleared by the call).  d_stats: u32[16] (zeroed by the caller before the round): [0] k-mer positions (size the table at least twice
 * that), [1] entries without room. */
int gf_contig_kmer_table_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq, const void* d_gap_best,
                             size_t n_gaps, int k, void* d_table, int log2_slots, void* d_stats);
/* both reads of every candidate pair against the table: keys gap << 40 | lib << 36 | pair appended to d_keys (fill it with 0xFF before the
 * round; the same (gap, pair) may appear more than once); d_stats[2] = keys emitted. */
int gf_recruit_by_contigs_dev(gf_ctx* ctx, const void* d_reads, const void* d_nmask_or_null, size_t n_reads, int read_len, const void* d_pairs,
                              const void* d_n_pairs, size_t pair_cap, int lib, int k, const void* d_table, int log2_slots, void* d_keys,
                              size_t key_cap, void* d_stats);
/* u32 words of gf_round2_pools_dev's d_work */
size_t gf_round2_work_words(size_t key_cap, size_t n_gaps);
/* the round-2 pools: per gap with recruits its round-1 rows (d_asm_pool / d_asm_off, as they went to the assembly) followed by the recruited
 * pairs' reads in (library, read id) order, each pair once; other gaps get empty pools.  d_lib_reads: n_lib device pointers (host array).
 * d_rows: u64[2 * (n_gaps + 1)], the pool offsets in its second half (the d_pool_off of gf_assemble_multi_dev).  d_stats: [3] distinct
 * recruited pairs, [4] gaps with d_gap_best == 0, [5] gaps with recruits, [6-7] u64 rows, [11] 1 when the rows exceed pool_cap (every pool
 * is then left empty). */
int gf_round2_pools_dev(gf_ctx* ctx, void* d_keys, void* d_keys_sorted, size_t key_cap, const void* const* d_lib_reads, int n_lib, int read_len,
                        const void* d_asm_pool, const void* d_asm_off, const void* d_gap_best, size_t n_gaps, void* d_work, void* d_rows,
                        void* d_pool, size_t pool_cap, void* d_stats);
/* the contigs of a second list appended to the first (seq_off moved); d_stats[8] = the first appended index, [10] contigs appended, [9] = 1
 * when they do not fit (nothing appended).  Follow with gf_pick_*_from_dev(d_first = d_stats + 8). */
int gf_contigs_append_dev(gf_ctx* ctx, void* d_contigs, void* d_n_contigs, size_t contig_cap, void* d_seq, void* d_seq_len, size_t seq_cap,
                          const void* d_src_contigs, const void* d_src_n, size_t src_cap, const void* d_src_seq, const void* d_src_seq_len,
                          size_t src_seq_cap, void* d_stats);

/* ---- recruitment rounds 2 and later (csrc/round_n.hip; DESIGN.md §10 "Repeated rounds"): the round above run again with the contigs the round
 * before appended, until a round grows no gap.  Every round has a statistics block u32[16] of its own (zeroed by the caller before the step):
 * words 0-11 as above, [12] pairs new in this round (summed over the gaps open at its start), [13] gaps open at its start whose recruits grew,
 * [14] 1 when the round was gated.  THE GATE: every call here takes d_live, a device u32 — the round before's word [13], for round 2 round 1's
 * word [5].  Where *d_live == 0 every kernel of the call returns at once and no caller's buffer is written (gf_round_carry_dev alone then sets
 * [8] = *d_n_contigs and [14] = 1 and zeroes d_n_pairs_live).  d_live_or_null == NULL: not gated. */
/* gf_contig_kmer_table_dev over the contigs [*d_first, min(*d_n_contigs, contig_cap)) (d_first: device u32; at or beyond the end: an empty
 * table).  Same slots, same d_stats words [0] and [1]; the table is cleared by the call (unless gated). */
int gf_contig_kmer_table_from_dev(gf_ctx* ctx, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                                  const void* d_gap_best, size_t n_gaps, int k, const void* d_first, void* d_table, int log2_slots, void* d_stats,
                                  const void* d_live_or_null);
/* before a round recruits: the distinct valid keys of the round before (d_keys_sorted and d_work as its pools call left them; d_prev_stats:
 * its block) go to the front of d_keys in sorted order, the rest of d_keys is filled with 0xFF, their per-gap counts go to d_prev_cnt
 * (u32[n_gaps]) and their number becomes d_stats[2], so that gf_recruit_by_contigs_dev appends behind them.  d_n_pairs -> d_n_pairs_live:
 * u32[n_lib] candidate counts, copied (gated: zeroed) — the recruitment of the round reads d_n_pairs_live + l as its d_n_pairs.
 * d_snapshot_or_null: u64[key_cap], receives the same keys (the round before's recruits, for a caller that keeps read ids). */
int gf_round_carry_dev(gf_ctx* ctx, void* d_keys, const void* d_keys_sorted, size_t key_cap, size_t n_gaps, const void* d_work, void* d_prev_cnt,
                       const void* d_prev_stats, void* d_stats, const void* d_n_contigs, const void* d_n_pairs, void* d_n_pairs_live, int n_lib,
                       void* d_snapshot_or_null, const void* d_live);
/* gf_round2_pools_dev with d_prev_cnt (d_work: gf_round2_work_words): a gap gets a pool — its round-1 rows, then ALL its recruited pairs so
 * far in (library, pair) order — only when d_gap_best == 0 and its count exceeds d_prev_cnt; every other gap gets an empty pool, whatever
 * keys it has.  d_stats [3] [4] [5] [6-7] [11] as above (counts over all gaps, closed ones included), [12], [13]. */
int gf_round_pools_dev(gf_ctx* ctx, void* d_keys, void* d_keys_sorted, size_t key_cap, const void* const* d_lib_reads, int n_lib, int read_len,
                       const void* d_asm_pool, const void* d_asm_off, const void* d_gap_best, size_t n_gaps, const void* d_prev_cnt, void* d_work,
                       void* d_rows, void* d_pool, size_t pool_cap, void* d_stats, const void* d_live_or_null);

/* ---- the closing pools (closing_pools.hip): after the last recruitment round, per gap with d_gap_best != 0 the rows of a
 * source pool (d_src_pool / d_src_off, u64[n_gaps + 1]: the pool the step's first assembly saw, or one library's own pool) followed by reads
 * 2p, 2p + 1 of every distinct key (gap, library, p) of the gap in (library, pair) order; a gap with d_gap_best == 0 gets an empty pool,
 * whatever keys it has.  d_keys_sorted, d_round_work, key_cap: what the last gf_round2_pools_dev / gf_round_pools_dev call left (a gated call
 * leaves them as the call before did).  lib_filter: -1, or the one library whose keys count.  d_lib_reads / d_lib_nmask_or_null: n_lib device
 * pointers each (host arrays; a mask entry may be NULL).  d_work: gf_closing_pools_work_words(n_gaps) u32 words.
 * Out: d_off u64[n_gaps + 1]; d_pool, rows of gf_packed_read_bytes(read_len) bytes; optional d_nmask (ceil(read_len / 32) u32 words per row:
 * the source's, the library's, zero where there is none), d_ids (u32 per row: d_src_ids', 0xFFFFFFFF without them; 2p, 2p + 1) and d_lib
 * (u8 per row: src_lib; the key's library).  d_stats: u32[GF_CP_WORDS], set by the call: [0-1] u64 rows needed, [2] gaps with a non-empty
 * pool, [3] recruited rows copied, [4] 1 when the rows exceed pool_cap — every pool is then left empty ([2] = [3] = 0) and no row is written.
 * Enqueued on the context's stream; no host synchronisation. */
#define GF_CP_WORDS 8
size_t gf_closing_pools_work_words(size_t n_gaps);
int gf_closing_pools_dev(gf_ctx* ctx, const void* d_keys_sorted, const void* d_round_work, size_t key_cap, const void* const* d_lib_reads,
                         const void* const* d_lib_nmask_or_null, int n_lib, int lib_filter, int read_len, const void* d_src_pool,
                         const void* d_src_off, const void* d_src_nmask_or_null, const void* d_src_ids_or_null, int src_lib, const void* d_gap_best,
                         size_t n_gaps, void* d_work, void* d_off, void* d_pool, size_t pool_cap, void* d_nmask_or_null, void* d_ids_or_null,
                         void* d_lib_or_null, void* d_stats);

/* ---- the reference's rescue round (assemble_gaps.py:166-217 run_collect_high_quality_unmap_to_contig_reads: `bwa mem` of a gap's high-quality
 * reads against its merged contigs, reads that align CLIPPED to at least two contigs are bridges), for ALL gaps of a round in one host call (no GPU
 * work; ctx may be NULL).  Contigs of gap g = texts [ctg_set_off[g], ctg_set_off[g+1]) of ctg_text (text c at ctg_off[c] .. ctg_off[c+1]), reads
 * likewise.  bwa is replaced by seed and extend as gappadder_amd/assemble_gaps.py::bridging_reads defines it: exact seed of seed_len characters on
 * either strand (at most 8 occurrences of a window per contig strand), first seed per (read, contig, strand, diagonal), clipped = a read end beyond
 * the contig or more than `budget` mismatches on either side of the seed, clipped AT a contig = every placement there clipped.
 * out_bridge[r] = 1 for the reads that are clipped at two contigs at least. */
int gf_bridging_reads(gf_ctx* ctx_or_null, const char* ctg_text, const uint64_t* ctg_off, const uint64_t* ctg_set_off, const char* read_text,
                      const uint64_t* read_off, const uint64_t* read_set_off, size_t n_gaps, int seed_len, int budget, uint8_t* out_bridge);

/* ---- the rescue round inside the device step (assemble_gaps.py:357-366, body :166-217; csrc/rescue.hip), after the merge
 * round's pick.  Definition (the CLI's, GapAssembler.collect_high_quality_unmap_to_contigs_reads + gf_bridging_reads, seed 30, budget 2):
 *   tried gaps   d_gap_best == 0 when gf_rescue_bridges_dev runs;
 *   HQ reads     per tried gap the reads of the libraries' alignment-tagger hits whose record has MAPQ == 60 and a read (not 0xFFFFFFFF),
 *                read = record's read ^ to_mate; each (gap, library, mate, read) once, ordered by (library, mate side, pair) — the CLI's
 *                gap_reads_high_quality file; reads are identified by (library, read), which is the CLI's first-record-of-a-name rule when
 *                the libraries' read names are distinct;
 *   alignment set  the exact-containment dedup of the gap's records on the list (own contigs and the merge round's, k = kv = 0) = the CLI's
 *                contigs.fa after the merge (drop_contained(new + nodup)); gaps with more than 1 024 such records are not tried (stats[11]);
 *   bridge       gf_bridging_reads' predicate against the set: exact 30-base seed on either strand, at most 8 occurrences of a window per
 *                contig strand in offset order, first seed per (contig, strand, diagonal), clipped = a read end beyond the contig or more
 *                than 2 mismatches on either side of the seed, clipped AT a contig = every placement there clipped, a bridge is clipped at
 *                two contigs at least; N-masked read bases never seed and always mismatch;
 *   records      the bridges, in HQ order, appended to the list as records with k = kv = GF_RESCUE_MARK (tombstones, counters
 *                that count every bridge, no record at or beyond contig_cap, nothing appended to a list that arrives overflowed).
 * d_work: gf_rescue_work_bytes(n_gaps, hq_cap, seed_cap, log2_slots) bytes.  d_stats: u32[GF_RS_WORDS], every count exact whatever the
 * capacities (a caller sizes from them and runs again: Pipeline.prepare). */
#define GF_RESCUE_MARK 0xFFFF
#define GF_RS_TRIED 0          /* gaps with d_gap_best == 0 */
#define GF_RS_HQ_KEYS 1        /* keys listed by gf_rescue_hq_keys_dev (every gap; beyond hq_cap: not stored) */
#define GF_RS_HQ 2             /* HQ reads of the tried gaps */
#define GF_RS_WINDOWS 3        /* their 30-base windows (size the window table at least twice that) */
#define GF_RS_TAB_FULL 4       /* windows the table had no room for */
#define GF_RS_SEEDS 5          /* contig windows that an HQ read of the gap shares (beyond seed_cap: not stored) */
#define GF_RS_PLACE_OVF 6      /* reads with more than 512 (contig, strand, diagonal) placements (no bridge) */
#define GF_RS_GAPS_BRIDGED 7   /* tried gaps with a bridge */
#define GF_RS_BRIDGES 8        /* bridges */
#define GF_RS_FIRST 9          /* index of the first bridge record (d_first of the rescue's pick) */
#define GF_RS_APPEND_ERR 10    /* 1: the list arrived overflowed (nothing appended); 2: the bridges went beyond a capacity */
#define GF_RS_LONG 11          /* contigs of 2^24 bases or more (no seeds); gaps not tried, see above */
#define GF_RS_WORDS 16
size_t gf_rescue_work_bytes(size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2_slots);
/* zeroes d_stats and the key list: once per step, before the first gf_rescue_hq_keys_dev */
int gf_rescue_reset_dev(gf_ctx* ctx, void* d_work, size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2_slots, void* d_stats);
/* one library's HQ keys (gap << 40 | lib << 36 | mate side << 35 | pair) from its tagger hits, for every gap (the tried gaps are chosen by
 * gf_rescue_bridges_dev): may run before the pick, so that a tagger that rewrites d_thits next (Pipeline tag_ahead) can follow it */
int gf_rescue_hq_keys_dev(gf_ctx* ctx, const void* d_thits, const void* d_n_thits, size_t thit_cap, const void* d_recs, size_t n_reads, int lib,
                          size_t n_gaps, void* d_work, size_t hq_cap, size_t seed_cap, int log2_slots, void* d_stats);
/* HQ reads of the tried gaps, alignment sets, seeds, bridges, append.  d_lib_reads / d_lib_nmask: n_lib device pointers (host arrays; the nmask
 * array or its entries may be NULL); d_sets_stats: u32[32] of the alignment sets' dedup (gf_merge_open_gaps_dev's words). */
int gf_rescue_bridges_dev(gf_ctx* ctx, void* d_contigs, void* d_n_contigs, size_t contig_cap, void* d_seq, void* d_seq_len, size_t seq_cap,
                          const void* d_gap_best, size_t n_gaps, const void* const* d_lib_reads, const void* const* d_lib_nmask, int n_lib, int read_len,
                          void* d_work, size_t hq_cap, size_t seed_cap, int log2_slots, void* d_sets_stats, void* d_stats);
/* u32[n_gaps] bridges per gap inside d_work (the d_gap_bridges of gf_merge_rescue_dev) */
const void* gf_rescue_gap_bridges(void* d_work, size_t n_gaps, size_t hq_cap, size_t seed_cap, int log2_slots);
/* the rescue's merge: gf_merge_open_gaps_dev over the rescue SETS — per tried gap with a bridge its own contigs (the records before the merge
 * round's, *(d_merge_stats + 7)) followed by its bridges (records from *d_rescue_first on) in record order — merged contigs appended with
 * k = kv = 0.  Follow with gf_pick_*_from_dev(d_first = d_rescue_first). */
int gf_merge_rescue_dev(gf_ctx* ctx, void* d_contigs, void* d_n_contigs, size_t contig_cap, void* d_seq, void* d_seq_len, size_t seq_cap,
                        const void* d_gap_best, size_t n_gaps, const gf_ovl_params* params, int kmer_len_quick, int max_set, const int* k_list,
                        const int* kv_list, int n_k, const void* d_merge_stats, const void* d_rescue_first, const void* d_gap_bridges, void* d_stats);

/* ---- read adjudication of the contested fills (csrc/fill_adj.hip; definition and host twin: gappadder_amd/fill_adjudication.py,
 * DESIGN.md §26).  A gap is CONTESTED when its gf_fill_alt (d_alt, read only: what gf_fill_alts_dev wrote over the same list and pick
 * words) has GF_FA_F_HAS_RIVAL and not GF_FA_F_LOST.  For such a gap the oriented fills F_w of `contig` and F_r of `rival` are located
 * again by gf_fill_alts_dev's candidate rule; a contig that is no contig of the gap, that the gap's pick word does not name (the winner),
 * that is no candidate, or whose fill has another strand or length than the record states is a MISMATCH: zero record, counted.  The
 * LOCUS of a fill F is LC + F + RC, LC the last min(context, |LF|) bytes of the gap's left flank, RC the first min(context, |RF|) of
 * its right flank: d_flank_text holds n_gaps * 2 * context bytes (LC then RC, each from the start of its `context` bytes),
 * d_flank_len n_gaps * 2 u16 (their lengths).  Every row of the gap's pool (the pool arguments of gf_fill_polish_dev) is placed on
 * both loci by gf_fill_polish_dev's placement rule (seed, max_mismatch, min_overlap); its key on a locus is the smallest mismatches << 12
 * | (4095 - overlap) over its accepted (strand, diagonal) pairs whatever their number, its strand there 0 when a pair with that key
 * lies on strand 0.  The row votes for the locus with the smaller key (no pair: larger than every key), ties when both keys are equal,
 * is unplaced without a pair on either.  verdict: KEEP when votes_w >= min_votes and votes_w >= ratio * votes_r, SWITCH the same way
 * round, else UNDECIDED.  A locus of more than GF_PL_MAX_CONTIG bases (either one), or with a byte other than A, C, G, T, is flagged
 * and counted: the lengths set, votes and verdict zero.  d_place_scratch: u32 per pool row, overwritten.  d_adj: n_gaps gf_fill_adj,
 * written for every gap (all zero: not contested, or a mismatch); d_stats: GF_AJ_WORDS u32, zeroed by the call.  The placement rule
 * out of gf_fill_polish_dev's range: GF_E_UNSUPPORTED; context outside min_overlap..1000, min_votes < 1, ratio outside 2..GF_AJ_MAX_RATIO,
 * a missing argument or anchor lengths outside 8 <= short < long <= 32 (or short 0): GF_E_INVAL.  No host synchronisation. */
typedef struct {
    uint32_t contig, rival;          /* the winner's and the rival's index in the list */
    uint32_t locus_w, locus_r;       /* bases of the two loci */
    uint32_t votes_w, votes_r;       /* rows that fit the winner's / the rival's locus strictly better */
    uint32_t votes_w_s0, votes_r_s0; /* of them: rows placed as stored (strand 0) on the locus they vote for */
    uint32_t ties, unplaced;         /* rows with equal keys on both loci; rows with no accepted pair on either */
    uint32_t only;                   /* votes of rows with no accepted pair on the other locus */
    uint8_t verdict;                 /* GF_AJ_KEEP, GF_AJ_SWITCH, GF_AJ_UNDECIDED; 0: not adjudicated */
    uint8_t flags;                   /* GF_AJ_F_* */
    uint16_t reserved;
} gf_fill_adj;
#define GF_AJ_KEEP 1
#define GF_AJ_SWITCH 2
#define GF_AJ_UNDECIDED 3
#define GF_AJ_F_LONG 1            /* skipped: a locus of more than GF_PL_MAX_CONTIG bases */
#define GF_AJ_F_NON_ACGT 2        /* skipped: a locus byte other than A, C, G, T */
#define GF_AJ_F_RIVAL_FAR 4       /* the rival's dist is GF_FA_DIST_FAR */
#define GF_AJ_F_NO_ROWS 8         /* the gap's pool is empty */
/* words of d_stats: contested gaps seen, adjudicated, and of them keep, switch, undecided; skipped long, skipped non-ACGT, mismatches;
 * u64 each (two words, low first): votes_w, votes_r, ties over the adjudicated gaps */
#define GF_AJ_SEEN 0
#define GF_AJ_ADJUDICATED 1
#define GF_AJ_N_KEEP 2
#define GF_AJ_N_SWITCH 3
#define GF_AJ_N_UNDECIDED 4
#define GF_AJ_SKIPPED_LONG 5
#define GF_AJ_SKIPPED_NON_ACGT 6
#define GF_AJ_MISMATCH 7
#define GF_AJ_VOTES_W 8
#define GF_AJ_VOTES_R 10
#define GF_AJ_TIES 12
#define GF_AJ_WORDS 16
#define GF_AJ_MAX_CONTEXT 1000
#define GF_AJ_MAX_RATIO 16
int gf_fill_adjudicate_dev(gf_ctx* ctx, const void* d_pool_packed, const void* d_nmask_or_null, const void* d_pool_off, size_t pool_rows,
                           int read_len, const void* d_contigs, const void* d_n_contigs, size_t contig_cap, const void* d_seq,
                           const void* d_gap_best, int anchor_long, int anchor_short, const void* d_alt, const void* d_flank_text,
                           const void* d_flank_len, void* d_place_scratch, int seed, int max_mismatch, int min_overlap, int context,
                           int min_votes, int ratio, void* d_adj, void* d_stats);

/* ---- device memory + timing helpers (so a ctypes host needs no other HIP binding) ---------------------- */
int gf_dev_alloc(gf_ctx* ctx, size_t bytes, void** d_ptr);
int gf_dev_free(gf_ctx* ctx, void* d_ptr);
int gf_memcpy_h2d(gf_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int gf_memcpy_d2h(gf_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int gf_memset_dev(gf_ctx* ctx, void* d_ptr, int value, size_t bytes);
/* per-kernel HIP-event timing on the ctx's stream: enable, run, gf_sync, then read totals. */
#define GF_KERNEL_SCREEN 0
#define GF_KERNEL_TAG 1
#define GF_KERNEL_LOWMAPQ 2
#define GF_KERNEL_ASSEMBLE 3
#define GF_KERNEL_POOL 4
#define GF_KERNEL_SYNTH 5
#define GF_KERNEL_COUNT 6
#define GF_KERNEL_VERIFY 7  /* second kernel of the screen: exact per-candidate verification */
#define GF_KERNEL_INGEST 8  /* FASTQ text -> packed reads */
#define GF_KERNEL_PICK 9    /* flank anchoring */
#define GF_KERNEL_MERGE 10  /* contig-merge prefilter */
#define GF_KERNEL_SUPPORT 11  /* read support of the closed gaps */
#define GF_KERNEL_POLISH 12  /* consensus polish of the closed gaps */
#define GF_KERNEL_PAIRS 13  /* pair-span check of the closed gaps */
#define GF_KERNEL_ANCHORS 14  /* anchored pair span of the closed gaps */
#define GF_KERNEL_GAPSPAN 15  /* gap-size measurement from the gap-spanning pairs */
#define GF_KERNEL_POLISH_GAPPED 16  /* indel-aware consensus polish of the closed gaps */
#define GF_KERNEL_PILEUP 17  /* per-base pile-up of the closed gaps */
#define GF_KERNEL_JOIN 18  /* flank-overlap joins of the open gaps */
#define GF_KERNEL_ALT 19  /* fill alternatives of the closed gaps */
#define GF_KERNEL_ADJ 20  /* read adjudication of the contested fills */
int gf_timing_enable(gf_ctx* ctx, int on);
int gf_timing_read(gf_ctx* ctx, int which, double* total_ms, uint64_t* launches);
int gf_timing_reset(gf_ctx* ctx);

/* ---- synthetic workload (bench/test utility, not part of the reference's path; definition: include/gf_synth.h,
 * shared bit-for-bit with oracle/gp_oracle.c).  gf_synth_pairs_dev fills 2*n_pairs packed reads (read 2p+m =
 * mate m+1 of pair first_pair+p) and, optionally, 2*n_pairs gf_alnrec (record 2p+e = forward/reverse end; record.read = 2p+m,
 * the read's index in THIS batch).
 * gf_synth_layout writes the n_scaffolds*gaps_per_scaffold gaps and their flanks (2*(flank_len-5) bases per gap). */
int gf_synth_pairs_dev(gf_ctx* ctx, const void* cfg /* gf_synth_cfg */, uint64_t first_pair, size_t n_pairs,
                       void* d_packed_reads, void* d_alnrecs_or_null);
int gf_synth_layout(const void* cfg /* gf_synth_cfg */, gf_gap* gaps, char* flank_ascii, uint64_t* flank_off);
/* the true bases of [start, start + n) of a scaffold, the planted gaps' interiors included: ground truth for checking filled gaps
 * (the reference's own evaluation compares picked sequences with the true ones: validate_gap_seqs.py:5-75) */
int gf_synth_truth(const void* cfg /* gf_synth_cfg */, uint32_t scaffold, uint64_t start, size_t n, char* out_ascii);

#ifdef __cplusplus
}
#endif
#endif /* GAPFILL_HIP_H */
