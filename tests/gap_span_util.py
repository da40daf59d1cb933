"""Hand-built alignment records for the gap-span tests (test_gap_span_host.py, test_gpu_gap_span.py): one small gap table and, per
inequality of the definition (gappadder_amd/gap_span.py), records at the boundary and one base on either side of it, each with the
counter it must land in — written down by hand from the definition, not computed by the twin."""
import numpy as np

from gappadder_amd import _lib as B

L, MU, SD, Z, Q = 100, 1500, 100, 3, 30
DIST2 = MU + 3 * SD                 # 1800
N_SCAFFOLDS = 4
# scaffold 0: three gaps, the last two closer together than L; scaffold 1: two; scaffold 2: none; scaffold 3: one (the table's last)
GAPS = np.array([(0, 10000, 10500, 1), (0, 12000, 12300, 2), (0, 12350, 12400, 3), (1, 500, 800, 1), (1, 5000, 5200, 2), (3, 3000, 3100, 1)],
                dtype=B.GAP)
FLAG = 0x1 | 0x20 | 0x40            # paired, mate reverse, first in pair
CLASSES = ("n_multi", "n_clipped", "n_lowq", "n_low", "n_high", "n")


def rec(a0, m0, tlen=None, ref=0, mate_ref=None, flag=FLAG, mapq=60, clip=0, read=0):
    """A record whose read starts at 0-based a0 and whose mate starts at 0-based m0; tlen defaults to m0 + L - a0."""
    return (a0 + 1, m0 + 1, m0 + L - a0 if tlen is None else tlen, ref, ref if mate_ref is None else mate_ref, flag, mapq, clip, read)


def hand_cases():
    """[(name, shift D, record, {gap: counter})]: the record alone must give exactly these counters (an empty dictionary: no candidate).
    lo = 1200 - D, hi = 1800 + D."""
    c = []
    # A0 + L against start (gap 0: [10000, 10500)), the mate at the gap's end
    for a0, hit in ((9899, True), (9900, True), (9901, False)):
        c.append(("read end vs start %d" % a0, 1000, rec(a0, 10500), {0: "n"} if hit else {}))
    # start - A0 against dist2
    for a0, hit in ((8201, True), (8200, True), (8199, False)):
        c.append(("window %d" % a0, 1000, rec(a0, 10500), {0: "n"} if hit else {}))
    # M0 against end
    for m0, hit in ((10499, False), (10500, True), (10501, True)):
        c.append(("mate vs end %d" % m0, 1000, rec(9500, m0), {0: "n"} if hit else {}))
    # M0 against M1 = A0 + tlen (A0 = 9500, M0 = 10600)
    for tlen, hit in ((1099, False), (1100, False), (1101, True)):
        c.append(("mate vs template end %d" % tlen, 1000, rec(9500, 10600, tlen), {0: "n"} if hit else {}))
    # tlen against lo = 1200 and hi = 1800 (D = 0); A0 = 9600, M0 = 10600
    for tlen, cls in ((1199, "n_low"), (1200, "n"), (1201, "n"), (1799, "n"), (1800, "n"), (1801, "n_high")):
        c.append(("tlen %d" % tlen, 0, rec(9600, 10600, tlen), {0: cls}))
    # ... and against lo = 1000, hi = 2000 (D = 200)
    for tlen, cls in ((1101, "n"), (1999, "n"), (2000, "n"), (2001, "n_high")):
        c.append(("tlen %d with D = 200" % tlen, 200, rec(9600, 10600, tlen), {0: cls}))
    # mapq against q - 1 and q
    for mapq, cls in ((Q - 1, "n_lowq"), (Q, "n"), (0, "n_lowq"), (255, "n")):
        c.append(("mapq %d" % mapq, 0, rec(9500, 10900, mapq=mapq), {0: cls}))
    # flag bits, each alone
    for what, flag in (("unpaired", FLAG & ~0x1), ("unmapped", FLAG | 0x4), ("mate unmapped", FLAG | 0x8), ("secondary", FLAG | 0x100),
                       ("supplementary", FLAG | 0x800), ("reverse", FLAG | 0x10), ("mate forward", FLAG & ~0x20)):
        c.append((what, 0, rec(9500, 10900, flag=flag), {}))
    c.append(("second in pair", 0, rec(9500, 10900, flag=0x1 | 0x20 | 0x80), {0: "n"}))
    # other drops
    c.append(("tlen 0", 0, rec(9500, 10900, 0), {}))
    c.append(("tlen negative", 0, rec(9500, 10900, -1500), {}))
    c.append(("mate on another scaffold", 0, rec(9500, 10900, mate_ref=1), {}))
    c.append(("pos 0", 0, (0, 10901, 1500, 0, 0, FLAG, 60, 0, 0), {}))
    c.append(("mate_pos 0", 0, (9501, 0, 1500, 0, 0, FLAG, 60, 0, 0), {}))
    # order of the classification: the first test that holds counts
    c.append(("clipped", 0, rec(9500, 10900, clip=1), {0: "n_clipped"}))
    c.append(("clipped right", 0, rec(9500, 10900, clip=2), {0: "n_clipped"}))
    c.append(("clipped and lowq", 0, rec(9500, 10900, clip=3, mapq=0), {0: "n_clipped"}))
    c.append(("lowq and low", 0, rec(9600, 10600, 1100, mapq=3), {0: "n_lowq"}))
    c.append(("lowq and high", 0, rec(9600, 10600, 1900, mapq=3), {0: "n_lowq"}))
    c.append(("multi and clipped", 0, rec(10499, 12400, clip=1), {1: "n_multi"}))              # (gap 2 starts 1851 > dist2 bases behind A0)
    c.append(("multi, clipped, lowq and high", 0, rec(9000, 12400, clip=2, mapq=0), {0: "n_multi"}))
    # neighbours.  Gap 0 is the table's first (no gap before it); the next gap starts at 12000: M1 against it
    for m1, cls in ((11999, "n"), (12000, "n"), (12001, "n_multi")):
        c.append(("next gap vs template end %d" % m1, 1000, rec(9500, 10600, m1 - 9500), {0: cls}))
    # gap 1 = [12000, 12300): the gap before it ends at 10500: A0 against it (the mate inside [12300, 12350), short of gap 2)
    for a0, cls in ((10499, "n_multi"), (10500, "n"), (10501, "n")):
        c.append(("previous gap vs read start %d" % a0, 1000, rec(a0, 12300, 12340 - a0), {1: cls}))
    # gaps 1 and 2 lie 50 bases apart: a pair over both is a candidate of both, and multi in both
    c.append(("over two gaps", 1000, rec(11000, 12400), {1: "n_multi", 2: "n_multi"}))
    # gap 2 is the last of scaffold 0, gap 3 the first of scaffold 1: neither is the other's neighbour
    c.append(("last gap of a scaffold", 1000, rec(12200, 12400, 1500), {2: "n_multi"}))       # (the read lies in gap 1: end[1] > A0)
    c.append(("between gaps 1 and 2", 0, rec(12300, 13000, 1500), {}))                        # (50 bases: A0 + L > start of gap 2, no candidate)
    c.append(("first gap of the next scaffold", 0, rec(300, 1500, ref=1), {3: "n"}))         # (end[2] = 12400 > A0, but on scaffold 0)
    c.append(("second gap of scaffold 1", 0, rec(4500, 5700, ref=1), {4: "n"}))
    c.append(("the table's last gap", 0, rec(2500, 3700, ref=3), {5: "n"}))
    # fetch-side bounds: nothing is indexed
    c.append(("scaffold out of range", 0, rec(9500, 10900, ref=7), {}))
    c.append(("scaffold = n_scaffolds", 0, rec(9500, 10900, ref=N_SCAFFOLDS), {}))
    c.append(("unplaced", 0, rec(9500, 10900, ref=0xFFFFFFFF), {}))
    c.append(("scaffold without gaps", 0, rec(9500, 10900, ref=2), {}))
    c.append(("beyond the last window", 0, rec(50_000_000, 50_001_400), {}))
    c.append(("at the largest position", 0, (0xFFFFFFFF, 0xFFFFFFFF, 1500, 0, 0, FLAG, 60, 0, 0), {}))
    return c


def records(rows):
    return np.array(rows, dtype=B.ALNREC)


def expected(cases, shift):
    """The records every case of that shift gives TOGETHER: gf_gap_span per gap, from the hand-written counters alone (sum, sum_sq, min
    and max from the records' tlen)."""
    out = np.zeros(len(GAPS), dtype=B.GAP_SPAN)
    tl = {g: [] for g in range(len(GAPS))}
    for _, d, r, want in cases:
        if d != shift:
            continue
        for g, cls in want.items():
            out[g]["n_cand"] += 1
            out[g][cls] += 1
            if cls == "n":
                tl[g].append(int(r[2]))
    for g, t in tl.items():
        if t:
            out[g]["flags"], out[g]["sum"], out[g]["sum_sq"] = B.GS_F_PAIRS, sum(t), sum(x * x for x in t)
            out[g]["tlen_min"], out[g]["tlen_max"] = min(t), max(t)
    return out
