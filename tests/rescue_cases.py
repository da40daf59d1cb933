"""Inputs of the rescue-round tests (tests/test_gpu_rescue_round.py): a one-gap layout whose coverage drops to one pair over a 40-base
stretch near the left flank, built in numpy with the record conventions of tests/synth_small.py, and helpers that restate the round's
definition on the host from what a step fetched."""
import numpy as np

from oracle.c_oracle import ALNREC, GAP

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
L, INSERT, SD, FLANK = 150, 300, 30, 300


def revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def _align(gaps, s, pos):
    """(mapped, 1-based position, clip flag, CIGAR) of the read at pos: a read that overlaps a gap by 20 bases or more on one side is
    clipped, one that lies inside a gap (fewer than 20 bases outside) is unmapped."""
    lo, hi = pos, pos + L
    for (gs, gst, gen, _) in gaps:
        if gs != s or gen <= lo or gst >= hi:
            continue
        left, right = max(0, gst - lo), max(0, hi - gen)
        if left >= right:
            return (True, lo + 1, 2 if left < L else 0, "%dM%dS" % (left, L - left) if left < L else "%dM" % L) if left >= 20 else (False, 0, 0, "*")
        return (True, gen + 1, 1, "%dS%dM" % (gen - lo, right)) if right >= 20 else (False, 0, 0, "*")
    return True, lo + 1, 0, "%dM" % L


def _pairs_to_arrays(truth, gaps, pairs, mapq=60):
    """pairs: [(scaffold, a, b)] FR pairs — first read forward at a, second reverse at b (b >= a) — without errors.  Returns (reads,
    records) in tests/synth_small.py's conventions (_align); record.read = the read's index."""
    def align(s, pos):
        return _align(gaps, s, pos)[:3]

    reads, recs = [], np.zeros(2 * len(pairs), dtype=ALNREC)
    for p, (s, a, b) in enumerate(pairs):
        t = truth[s]
        seqs = [t[a:a + L], t[b:b + L].translate(_COMP)[::-1]]
        al = [align(s, a), align(s, b)]
        for i in (0, 1):
            j = 1 - i
            m, pos, clip = al[i]
            mm, mpos, _ = al[j]
            flag = 1 | (0x40 if i == 0 else 0x80) | (0x10 if i == 1 else 0x20)
            if not m:
                flag |= 4
            if not mm:
                flag |= 8
            ref = s if (m or mm) else 0xFFFFFFFF
            rpos = pos if m else (mpos if mm else 0)
            mp = mpos if mm else rpos
            tlen = 0
            if m and mm:
                span = b + L - a
                tlen = span if i == 0 else -span
            recs[2 * p + i] = (rpos, mp, tlen, ref, ref, flag, mapq if m else 0, clip if m else 0, 2 * p + i)
        reads += seqs
    order = np.lexsort((recs["pos"], recs["ref"]))
    return b"".join(reads), recs[order].copy()


def one_hole_case(seed=7, scaffold_len=4000, gap=(1800, 2300), hole=(1870, 1910), n_pairs=2400):
    """One scaffold, one gap; every pair that would overlap the hole is left out but one, whose reverse read (the gap read, unmapped)
    spans the hole with 60 bases on either side and whose forward read lies in the left flank, mapped with MAPQ 60: the assembly's
    contigs break at the hole (min-count 2 drops the single read's k-mers) and only that read bridges them.  No pair has both mates
    unmapped (the CLI's second round then recruits nothing: one_hole_files runs the whole CLI on the same reads)."""
    rng = np.random.RandomState(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = lut[rng.randint(0, 4, scaffold_len)].tobytes()
    st, en = gap
    gaps = [(0, st, en, 1)]
    h0, h1 = hole
    pairs = []
    while len(pairs) < n_pairs:
        ins = int(np.clip(round(rng.normal(INSERT, SD)), L + 20, INSERT + 2 * SD))
        a = int(rng.randint(0, scaffold_len - ins))
        b = a + ins - L
        if any(x < h1 and x + L > h0 for x in (a, b)):
            continue
        if not _align(gaps, 0, a)[0] and not _align(gaps, 0, b)[0]:
            continue
        pairs.append((0, a, b))
    bridge_b = h0 - 60
    bridge_a = bridge_b + L - 340
    assert bridge_a + L <= st <= bridge_b and bridge_b + L <= en
    pairs.append((0, bridge_a, bridge_b))
    blob, recs = _pairs_to_arrays([t], gaps, pairs)
    flanks = [(t[st - FLANK:st - 5].decode(), t[en + 5:en + FLANK].decode())]
    return {"gaps": np.array(gaps, dtype=GAP), "flanks": flanks, "reads_blob": blob, "recs": recs, "n_reads": 2 * len(pairs), "truth": t.decode(),
            "bridge": t[bridge_b:bridge_b + L].translate(_COMP)[::-1].decode(), "gap": gap, "pairs": pairs, "raw_gaps": gaps}


def one_hole_files(c):
    """one_hole_case as the CLI's inputs, shaped like golden_util.Case for pipeline_util.materialise: the draft (the gap as an N-run),
    its .fai, and one library — SAM text with the records' fields (CIGAR from the clips), FASTQ pairs of the same reads."""
    class Files:
        pass
    t, gaps = c["truth"], c["raw_gaps"]
    st, en = c["gap"]
    draft = t[:st] + "N" * (en - st) + t[en:]
    hdr = ">scf0 synthetic\n"
    body = "\n".join(draft[i:i + 60] for i in range(0, len(draft), 60)) + "\n"
    sam, fq1, fq2 = [], [], []
    reads = [c["reads_blob"][i * L:(i + 1) * L].decode() for i in range(c["n_reads"])]
    for p, (s, a, b) in enumerate(c["pairs"]):
        qn = "r%d" % p
        al = [_align(gaps, s, a), _align(gaps, s, b)]
        for i in (0, 1):
            m, pos, _, cig = al[i]
            mm, mpos, _, _ = al[1 - i]
            flag = 1 | (0x40 if i == 0 else 0x80) | (0x10 if i == 1 else 0x20) | (0 if m else 4) | (0 if mm else 8)
            rpos = pos if m else mpos
            tlen = 0
            if m and mm:
                tlen = (b + L - a) if i == 0 else -(b + L - a)
            sam.append((rpos, len(sam), "\t".join([qn, str(flag), "scf0", str(rpos), "60" if m else "0", cig, "=", str(mpos if mm else rpos), str(tlen),
                                                   "*", "*"]) + "\n"))
        fq1.append("@%s/1\n%s\n+\n%s\n" % (qn, reads[2 * p], "I" * L))
        fq2.append("@%s/2\n%s\n+\n%s\n" % (qn, reads[2 * p + 1], "I" * L))
    sam.sort()
    f = Files()
    f.draft_fa, f.fai = hdr + body, "scf0\t%d\t%d\t60\t61\n" % (len(draft), len(hdr))
    f.libs = [{"sam": "".join(x[2] for x in sam), "fq1": "".join(fq1), "fq2": "".join(fq2), "is": 300, "sd": 30}]
    f.meta = {"min_gap": 100, "flank": 300}
    return f


def contig_text(res, i):
    c = res.contigs[i]
    return res.seq[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])].decode()


def hq_reads(recs, thits, n_gaps, reads_of, lib=0):
    """Definition 2 for one library: {gap: [(lib, read id, bases)]} in (mate side, pair) order — MAPQ-60 records with a read, read ^ to_mate."""
    out = {}
    keys = set()
    for h in thits:
        r = recs[int(h["rec"])]
        rd = int(r["read"]) & 0xFFFFFFFF
        if int(h["gap"]) >= n_gaps or int(r["mapq"]) != 60 or rd == 0xFFFFFFFF:
            continue
        t = rd ^ (int(h["to_mate"]) & 1)
        keys.add((int(h["gap"]), t & 1, t >> 1))
    for g, m, p in sorted(keys):
        out.setdefault(g, []).append((lib, 2 * p + m, reads_of(2 * p + m)))
    return out


def alignment_set(res, g, merge_first, end):
    """Definition 3: exact-containment dedup of gap g's records before `end` (own contigs and the merge round's)."""
    from gappadder_amd.MergeContigs import drop_contained
    recs = [("c%d" % i, contig_text(res, i)) for i in range(end) if int(res.contigs[i]["gap"]) == g and int(res.contigs[i]["length"])]
    return drop_contained(recs) if 2 <= len(recs) <= 1024 else recs
