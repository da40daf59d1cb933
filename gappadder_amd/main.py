"""CLI with the reference's interface (main.py:26-275): python -m gappadder_amd.main -c {Clean,All,Preprocess,Collect,Assembly}
-g config.json, same JSON keys, same working-folder layout.  Collect and the first assembly round run on the GPU."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

from . import assemble_gaps
from . import bam_io
from .gnrt_pos_true_seqs import DGProcessor
from .hip_api import GapFill
from .merge_reads import ReadsMerger
from .run_multi_threads_collect_reads import MultiThrdReadsCollector
from .run_multi_threads_discordant import DiscordantReadsCollector

MERGE_FOLDER = "merged/"
SUB = ("scaffold_reads_list_all", "gap_reads", "gap_reads_for_alignment", "gap_reads_high_quality", "discordant_reads_list",
       "discordant_temp")
SUB_MERGED = ("gap_reads", "gap_reads_for_alignment", "gap_reads_high_quality", "kmc_temp", "temp", "kmers", "velvet_temp",
              "both_unmapped", "unmapped_reads")


def parse_configuration(path):
    with open(path) as f:
        data = json.load(f)
    for key in ("draft_genome", "alignments", "raw_reads"):
        if key not in data:
            raise SystemExit("configuration lacks '%s'" % key)
    cfg = {"draft": data["draft_genome"]["fa"],
           "alignments": [(r["bam"], int(r["is"]), int(r["std"])) for r in data["alignments"]],
           "raw_reads": [(r["left"], r["right"]) for r in data["raw_reads"]],
           "kmers": [(int(r["k"]), int(s["k"])) for r in data.get("kmer_length", []) for s in r["k_velvet"]]}
    p = data.get("parameters", {})
    cfg["min_gap"] = int(p.get("min_gap_size", 100))
    cfg["flank"] = int(p.get("flank_length", 300))
    cfg["nthreads"] = int(p.get("nthreads", 15))
    cfg["wf"] = p.get("working_folder", "./GAPPadder_Output/")
    cfg["samtools"] = data.get("software_path", {}).get("samtools", "samtools")
    cfg["kmer_screen"] = int(p.get("kmer_screen", 0))   # extension: flank-k-mer recruitment from the FASTQ files (0 = off)
    # extension: how the picker anchors the flanks on the contigs — "exact" anchors (default), "align" (seed-and-extend of the whole
    # flanks, closer to the reference's bwa mem) or "gapped" (the same through a draft indel next to the gap); pick_contigs.py
    cfg["flank_anchor"] = str(p.get("flank_anchor", "exact"))
    if cfg["flank_anchor"] not in ("exact", "align", "gapped"):
        raise SystemExit("parameters.flank_anchor must be 'exact', 'align' or 'gapped', not %r" % (cfg["flank_anchor"],))
    # extension: the engine of the contig-merge rounds — "host" (default) or "device" (one device call per round with the merger's graph
    # exported, MergeContigs.merge_contigs); same files either way
    cfg["contig_merger"] = str(p.get("contig_merger", "host"))
    if cfg["contig_merger"] not in ("host", "device"):
        raise SystemExit("parameters.contig_merger must be 'host' or 'device', not %r" % (cfg["contig_merger"],))
    # extension: read support of the fills the device step closes (read_support.py): {wf}fill_support.tsv, one row per closed gap —
    # how the gap's own reads back the k-mers of the sequence about to be inserted; fill_support_k: its k (default: the smallest usable k)
    cfg["fill_support"] = bool(p.get("fill_support", False))
    cfg["fill_support_k"] = int(p["fill_support_k"]) if p.get("fill_support_k") is not None else None
    if cfg["fill_support_k"] is not None and not 16 <= cfg["fill_support_k"] <= 64:
        raise SystemExit("parameters.fill_support_k must be in 16..64, not %r" % (cfg["fill_support_k"],))
    # extension: consensus polish of the fills the device step closes (polish.py): {wf}polished_seqs.fa — picked_seqs.fa's cut of the
    # winning contig after the gap's own reads have voted on every column of the fill — and {wf}fill_polish.tsv, one row per closed gap
    cfg["fill_polish"] = bool(p.get("fill_polish", False))
    # extension: with fill_polish, the indel-aware polish (polish_gapped.py): rows are placed with one indel of up to fill_polish_max_indel
    # bases as well, polished_seqs.fa carries the result — which may differ in length — and fill_polish.tsv gains the six event columns
    cfg["fill_polish_indels"] = bool(p.get("fill_polish_indels", False))
    if cfg["fill_polish_indels"] and not cfg["fill_polish"]:
        raise SystemExit("parameters.fill_polish_indels needs fill_polish: it is a mode of the polish round")
    # extension: per-base confidence of the fills the device step closes (pileup.py): {wf}fill_pileup.tsv, one row per closed gap;
    # {wf}picked_seqs.fq, picked_seqs.fa's sequences with a score per base from the pile-up of the gap's own reads (pileup.phred: monotone,
    # not a calibrated probability); {wf}picked_seqs.masked.fa, the same sequences with the low columns (uncovered, thinner than
    # fill_pileup_min_depth, or with less than fill_pileup_min_agree per cent of the votes for the base) in lower case; and, with the plain
    # fill_polish, {wf}polished_seqs.fq, the polished base's score from the same counters.  With fill_polish_indels the polished text has
    # other columns than the contig the reads were piled on: no polished FASTQ is written
    cfg["fill_pileup"] = bool(p.get("fill_pileup", False))
    # extension: pair-span check of the fills the device step closes (pair_span.py): {wf}fill_pairs.tsv, one row per closed gap and library
    cfg["fill_pairs"] = bool(p.get("fill_pairs", False))
    # extension: with fill_pairs, the anchored pair span (pair_anchors.py): {wf}fill_pairs_anchored.tsv, one row per closed gap and library —
    # the mates anchored in the flanks against the fill; fill_pairs_min_pairs: the pairs a column needs for its mean insert deviation to count
    cfg["fill_pairs_anchored"] = bool(p.get("fill_pairs_anchored", False))
    if cfg["fill_pairs_anchored"] and not cfg["fill_pairs"]:
        raise SystemExit("parameters.fill_pairs_anchored needs fill_pairs: it reads the pair span's placements")
    # (name, default, lo, hi) of fill_<round>_<name>
    for rnd, own in (("polish", (("min_votes", 2, 1, None), ("max_indel", 8, 1, 16))), ("pairs", (("z", 3, 1, None), ("min_pairs", 8, 1, None))),
                     ("pileup", (("min_depth", 3, 1, None), ("min_agree", 80, 1, 100))),
                     ("adjudication", (("min_votes", 3, 1, None), ("ratio", 2, 2, 16), ("context", None, 12, 1000)))):
        for name, default, lo, hi in (("seed", 16, 12, 32), ("max_mismatch", 4, 0, 15), ("min_overlap", 48, 12, None)) + own:
            key = "fill_%s_%s" % (rnd, name)
            try:
                v = int(p[key]) if p.get(key) is not None else default
            except (TypeError, ValueError):
                raise SystemExit("parameters.%s must be an integer, not %r" % (key, p[key]))
            if v is None:                        # (fill_adjudication_context: the read length unless given)
                continue
            if v < lo or (hi is not None and v > hi):
                raise SystemExit("parameters.%s must be %s, not %r" % (key, "in %d..%d" % (lo, hi) if hi is not None else "at least %d" % lo, v))
            cfg[key] = v
        if cfg["fill_%s_min_overlap" % rnd] < cfg["fill_%s_seed" % rnd]:
            raise SystemExit("parameters.fill_%s_min_overlap must be at least fill_%s_seed (%d), not %d"
                             % (rnd, rnd, cfg["fill_%s_seed" % rnd], cfg["fill_%s_min_overlap" % rnd]))
    # extension: the size of every gap, open or closed, from the read pairs that span it (gap_span.py): {wf}gap_span.tsv, one row per gap
    # and library; gap_span_shift: how far off the draft's N-run may be; gap_span_min_pairs: the pairs an estimate needs
    cfg["gap_span"] = bool(p.get("gap_span", False))
    for key, default, lo in (("gap_span_shift", 1000, 0), ("gap_span_min_pairs", 8, 1)):
        v = p.get(key)
        if v is None:
            v = default
        if isinstance(v, bool) or not isinstance(v, int) or v < lo:
            raise SystemExit("parameters.%s must be an integer, at least %d, not %r" % (key, lo, p[key]))
        cfg[key] = v
    # extension: flank-overlap joins (flank_joins.py): the gaps the device step leaves open whose flanks OVERLAP on a contig that runs through
    # the junction — nothing is missing there: {wf}flank_joins.tsv, one row per joined gap, which put_gap_seq_back_to_scaffold takes as its
    # fifth argument; flank_joins_max_overlap: the longest overlap looked for; flank_joins_min_context: the bases beyond the overlap the
    # contig and each flank must share; flank_joins_max_mismatch: the differences allowed on either side
    cfg["flank_joins"] = bool(p.get("flank_joins", False))
    for key, default, lo, hi in (("flank_joins_max_overlap", 256, 1, 1024), ("flank_joins_min_context", 30, 0, 255), ("flank_joins_max_mismatch", 2, 0, 15)):
        v = p.get(key)
        if v is None:
            v = default
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise SystemExit("parameters.%s must be an integer in %d..%d, not %r" % (key, lo, hi, p[key]))
        cfg[key] = v
    # extension: fill alternatives (fill_alternatives.py): per gap the device step closes, the other contigs that carry both anchors as the
    # winner does — identical fills, fills within fill_alternatives_max_dist edits, fills further away — and the best of the differing
    # ones, the rival: {wf}fill_alternatives.tsv, one row per closed gap with more than one candidate, and {wf}alt_seqs.fa, the rival's
    # gap sequence of every contested gap
    cfg["fill_alternatives"] = bool(p.get("fill_alternatives", False))
    v = p.get("fill_alternatives_max_dist")
    if v is None:
        v = 16
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 31:
        raise SystemExit("parameters.fill_alternatives_max_dist must be an integer in 1..31, not %r" % (p["fill_alternatives_max_dist"],))
    cfg["fill_alternatives_max_dist"] = v
    # extension: with fill_alternatives, the read adjudication of the contested gaps (fill_adjudication.py): the gap's own reads placed on
    # the winner's and on the rival's fill, a vote per read: {wf}fill_adjudication.tsv, one row per contested gap with the votes and the
    # verdict keep / switch / undecided, and {wf}adjudicated_seqs.fa, picked_seqs.fa's records with the rival's sequence where the verdict
    # is switch.  Advice: picked_seqs.fa and the scaffold write-back do not change
    cfg["fill_adjudication"] = bool(p.get("fill_adjudication", False))
    if cfg["fill_adjudication"] and not cfg["fill_alternatives"]:
        raise SystemExit("parameters.fill_adjudication needs fill_alternatives: it reads the alternatives round's records")
    # extension: recruitment rounds (assemble_gaps.assemble_pipeline): how often the second round — both-unmapped pairs recruited by the
    # open gaps' contigs, assembly, pick — is repeated with the contigs the round before built; 1: the reference's single round
    v = p.get("recruit_rounds")
    if v is None:
        v = 1
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 16:
        raise SystemExit("parameters.recruit_rounds must be an integer in 1..16, not %r" % (p["recruit_rounds"],))
    cfg["recruit_rounds"] = v
    for path_, what in [(cfg["draft"], "draft genome")] + [(a[0], "bam") for a in cfg["alignments"]] + \
                       [(x, "raw reads") for pair in cfg["raw_reads"] for x in pair] + [(cfg["wf"], "working folder")]:
        if not os.path.exists(path_):
            raise SystemExit("The provided %s %s does not exist, please check!!!" % (what, path_))
    if not cfg["wf"].endswith("/"):
        cfg["wf"] += "/"
    return cfg


def prepare_folders(alignments, wf):
    folders = []
    for n, (_, is_, _) in enumerate(alignments, 1):
        p = "%s%d_is%d/" % (wf, n, is_)
        folders.append(p)
        for s in SUB:
            os.makedirs(p + s, exist_ok=True)
    for s in SUB_MERGED:
        os.makedirs(wf + MERGE_FOLDER + s, exist_ok=True)
    return folders


def collect_per_scaffold(cfg, gf, sf_fai, sf_gap_pos, folders, anchor_mapq, clip_dist, wf):
    """The reference's Collect stage call for call (main.py:226-270): a `samtools view` pipe per scaffold (or one decode pass over the
    BAM in builtin mode), list files, then the FASTQ join on the host."""
    for (bam, is_, sd), folder, (left, right) in zip(cfg["alignments"], folders, cfg["raw_reads"]):
        MultiThrdReadsCollector(sf_fai, bam, sf_gap_pos, anchor_mapq, gf).dispath_collect_jobs(
            cfg["nthreads"], cfg["samtools"], is_, sd, clip_dist, folder)
        drc = DiscordantReadsCollector(sf_fai, bam, folder, cfg["nthreads"], gf, cfg["samtools"])
        drc.collect_discordant_regions_v2(folder + "discordant_reads_pos.txt")
        drc.dispath_collect_jobs()
        extra = None
        if cfg["kmer_screen"]:
            from .kmer_recruit import screen_fastq_pair
            extra = screen_fastq_pair(gf, sf_fai, sf_gap_pos, wf, left, right, cfg["kmer_screen"])
        drc.merge_dispatch_reads_for_gaps_v2(left, right, extra)
        drc.dispatch_high_quality_reads_for_gaps(left, right)
    rm = ReadsMerger()
    for name in ("gap_reads", "gap_reads_alignment", "gap_reads_high_quality"):
        rm.merge_reads_v2(sf_fai, sf_gap_pos, folders, name, wf + MERGE_FOLDER, cfg["nthreads"])


def main_func(command, sf_config):
    cfg = parse_configuration(sf_config)
    wf = cfg["wf"]
    sf_fai = cfg["draft"] + ".fai"
    if not os.path.exists(sf_fai):
        if bam_io.is_builtin(cfg["samtools"]):
            bam_io.write_fai(cfg["draft"])
        else:
            subprocess.call([cfg["samtools"], "faidx", cfg["draft"]])
    sf_gap_pos = wf + "gap_positions.txt"
    anchor_mapq, clip_dist = 30, 250      # main.py:215-216
    if command in ("Clean", "All"):
        for fn in os.listdir(wf):
            p = os.path.join(wf, fn)
            shutil.rmtree(p) if os.path.isdir(p) else os.remove(p)
    timings = {"stages_s": {}}      # GF_TIMINGS=<file>: wall time per stage (+ the device Collect's own split) as JSON
    if command in ("Preprocess", "All"):
        t0 = time.perf_counter()
        dgp = DGProcessor(cfg["draft"], sf_gap_pos)
        dgp.gnrt_gap_positions(cfg["min_gap"])
        dgp.get_gap_flank_seqs(cfg["draft"], sf_gap_pos, cfg["flank"], sf_fai, wf)
        timings["stages_s"]["preprocess"] = time.perf_counter() - t0
    gf = GapFill(int(os.environ.get("GF_DEVICE", "0"))) if command in ("Collect", "Assembly", "All") else None
    first_round = None
    if command in ("Collect", "All"):
        t0 = time.perf_counter()
        folders = prepare_folders(cfg["alignments"], wf)
        if len(cfg["alignments"]) != len(cfg["raw_reads"]):
            raise SystemExit("# of alignment files and # of raw reads do not match!!!!!")
        # FASTQ(.gz): gzip / BGZF read files are inflated once into {wf}tmp_fastq/; every path below reads plain text
        from .fastq_io import plain_fastq
        cfg["raw_reads"] = [(plain_fastq(l, wf + "tmp_fastq"), plain_fastq(r, wf + "tmp_fastq")) for l, r in cfg["raw_reads"]]
        done = False
        if bam_io.is_builtin(cfg["samtools"]) and os.environ.get("GF_DEVICE_COLLECT", "1") != "0":
            # libraries resident in HBM, one pass over every file, the pipeline bench.py times (device_collect.py); with `-c All` the
            # first assembly round runs on the pools where they are
            from .device_collect import DeviceCollector, DeviceCollectUnsupported
            try:
                dc = DeviceCollector(gf, cfg, sf_fai, sf_gap_pos, anchor_mapq, clip_dist, kmers=cfg["kmers"] if command == "All" else None)
                res = dc.run(folders, wf + MERGE_FOLDER)
                done = True
                if command == "All" and res.k_pairs:
                    first_round = res
                timings["seconds"] = dc.t
                timings["libraries"] = [dict(lb.counts, reads=lb.n_reads, records=lb.n_recs, records_without_a_read=lb.records_without_a_read) for lb in dc.libs]
                timings["gaps"] = len(res.keys)
                timings["read_len"] = res.read_len        # the packed row length: the longest read of all libraries
                timings["gaps_closed_on_device"] = int(res.n_closed)
            except DeviceCollectUnsupported as e:
                sys.stderr.write("device-resident Collect not used (%s): per-scaffold path\n" % e)
            except (RuntimeError, MemoryError) as e:
                # out of device memory (torch's allocator or the library's GF_E_NOMEM) or a capacity of the one-shot step outgrown
                # (Pipeline.fetch's "step overflow"): inputs the streaming per-scaffold path handles chunk by chunk must not crash the
                # CLI — free the libraries, put the context back to its defaults, take that path.  Anything else is a real error.
                import torch
                from ._lib import GF_E_NOMEM, GF_E_NOSPACE, GapFillError
                oom = isinstance(e, (torch.cuda.OutOfMemoryError, MemoryError)) or "out of memory" in str(e).lower() or "step overflow" in str(e) \
                    or "keep overflowing" in str(e) or (isinstance(e, GapFillError) and e.code in (GF_E_NOMEM, GF_E_NOSPACE))
                if not oom:
                    raise
                sys.stderr.write("device-resident Collect gave up (%s): per-scaffold path\n" % (str(e).splitlines()[0][:200],))
                dc = res = first_round = None
                import gc
                gc.collect()
                torch.cuda.empty_cache()
                gf.set_option("asm_max_pool_reads", 0)
                gf.set_option("asm_big_pool_reads", 131072)
                for key in ("seconds", "libraries", "gaps", "read_len", "gaps_closed_on_device"):
                    timings.pop(key, None)
        if not done:
            collect_per_scaffold(cfg, gf, sf_fai, sf_gap_pos, folders, anchor_mapq, clip_dist, wf)
        for rnd, files in (("support", "no fill_support.tsv"), ("polish", "no polished_seqs.fa, no fill_polish.tsv"), ("pairs", "no fill_pairs.tsv"),
                           ("pileup", "no fill_pileup.tsv, no picked_seqs.fq, no picked_seqs.masked.fa" +      # (the polished FASTQ: only with the plain polish)
                            (", no polished_seqs.fq" if cfg["fill_polish"] and not cfg["fill_polish_indels"] else ""))):
            if cfg["fill_" + rnd] and (first_round is None or getattr(first_round, rnd) is None):
                sys.stderr.write("fill_%s: only the first assembly round of the device-resident Collect (-c All) computes it: %s\n" % (rnd, files))
        if cfg["fill_pairs_anchored"] and (first_round is None or first_round.pair_anchors is None):
            sys.stderr.write("fill_pairs_anchored: only the first assembly round of the device-resident Collect (-c All) computes it: "
                             "no fill_pairs_anchored.tsv\n")
        if cfg["flank_joins"] and (first_round is None or first_round.joins is None):
            sys.stderr.write("flank_joins: only the first assembly round of the device-resident Collect (-c All) computes it: no flank_joins.tsv\n")
        if cfg["fill_alternatives"] and (first_round is None or first_round.alts is None):
            sys.stderr.write("fill_alternatives: only the first assembly round of the device-resident Collect (-c All) computes it: "
                             "no fill_alternatives.tsv, no alt_seqs.fa\n")
        if cfg["fill_adjudication"] and (first_round is None or first_round.adjudication is None):
            sys.stderr.write("fill_adjudication: only the first assembly round of the device-resident Collect (-c All) computes it: "
                             "no fill_adjudication.tsv, no adjudicated_seqs.fa\n")
        if cfg["gap_span"] and not done:
            sys.stderr.write("gap_span: only the device-resident Collect computes it: no gap_span.tsv\n")
        timings["stages_s"]["collect" + ("_and_first_assembly_round" if first_round is not None else "")] = time.perf_counter() - t0
    if command in ("Assembly", "All"):
        t0 = time.perf_counter()
        for s in SUB_MERGED:
            os.makedirs(wf + MERGE_FOLDER + s, exist_ok=True)
        ga = assemble_gaps.GapAssembler(sf_fai, sf_gap_pos, cfg["nthreads"], wf + MERGE_FOLDER, cfg["kmers"], gf,
                                        bam_list=[bam for bam, _, _ in cfg["alignments"]], samtools_path=cfg["samtools"],
                                        flank_anchor=cfg["flank_anchor"], contig_merger=cfg["contig_merger"], recruit_rounds=cfg["recruit_rounds"])
        if first_round is not None:
            assemble_gaps.set_first_round(first_round)
        res = ga.assemble_pipeline()
        print("assembled %d gaps, %d closed (picked_seqs.fa), %d with an extended (partial) fill, %d gaps got both-unmapped pairs in the "
              "second round (%d recruitment rounds run), contigs merged in %d gap rounds (%d bridging high-quality reads); contigs in %svelvet_temp/*/contigs.fa"
              % (res["gaps"], res["closed"], res.get("extended", 0), res["second_round_gaps"], res["recruit_rounds_run"], res["gaps_with_merged_contigs"],
                 res["bridging_reads"], wf + MERGE_FOLDER))
        timings["stages_s"]["assembly_rounds"] = time.perf_counter() - t0
        timings["assembly"] = res
        from . import MergeContigs
        timings["contig_merger"] = dict(MergeContigs.DEVICE_COUNTS, engine=cfg["contig_merger"])
    if os.environ.get("GF_TIMINGS"):
        sys.stderr.write("stages: " + ", ".join("%s %.3f s" % kv for kv in timings["stages_s"].items()) +
                         ("; device collect: " + ", ".join("%s %.3f s" % kv for kv in timings["seconds"].items()) if "seconds" in timings else "") + "\n")
        if os.environ["GF_TIMINGS"] not in ("1", ""):
            with open(os.environ["GF_TIMINGS"], "w") as f:
                json.dump(timings, f)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Run the GAPPadder recruit + local-assembly hot path on MI355X")
    ap.add_argument("-g", "--config", type=str, required=True, help="Configuration file name")
    ap.add_argument("-c", "--command", type=str, required=True, help="Clean | All | Preprocess | Collect | Assembly")
    a = ap.parse_args(argv)
    main_func(a.command, a.config)


if __name__ == "__main__":
    main()
