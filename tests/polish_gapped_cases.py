"""Hand-built inputs of the indel-aware polish (gappadder_amd/polish_gapped.py), shared by its host tests and its device tests: contigs with
a planted indel and the reads that settle it.  Every builder returns a dict with the TRUE sequence, the contig as stored, the stored body
(b0, b1), the reads and — where the answer is derived by hand — the one event the reads vote for, as polish_gapped.event_of gives it."""
import numpy as np

from gappadder_amd.pick_contigs import revcomp

DEL, INS = 0, 1


def seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def other(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def sub(text, at, step=1):
    return text[:at] + other(text[at], step) + text[at + 1:]


def num_of(bases):
    n = 0
    for b in bases:
        n = n * 4 + "ACGT".index(b)
    return n


def sample(rng, truth, n_reads, L, err=0.005, masked=False):
    """Rows of `truth`, either strand, sampled anywhere with substitutions at rate err and, when masked, a quarter with one N."""
    out = []
    for _ in range(n_reads):
        o = int(rng.integers(0, len(truth) - L + 1))
        r = list(truth[o:o + L])
        for i in np.nonzero(rng.random(L) < err)[0]:
            r[i] = other(r[i], int(rng.integers(1, 4)))
        if masked and rng.integers(0, 4) == 0:
            r[int(rng.integers(0, L))] = "N"
        r = "".join(r)
        out.append(revcomp(r) if rng.integers(0, 2) else r)
    return out


def exact_rows(truth, offsets, L):
    """Exact copies of truth at the offsets, alternating strands."""
    return [revcomp(truth[o:o + L]) if i % 2 else truth[o:o + L] for i, o in enumerate(offsets)]


def unique_pair(rng, n_left, n_right, inner=""):
    """(left, right) random texts such that an indel of `inner` planted between them cannot slide: the left one ends with a base that is
    neither inner's last nor the right one's first, the right one starts with a base that is not inner's first."""
    left, right = seq(rng, n_left), seq(rng, n_right)
    avoid = {right[0]} | ({inner[-1], inner[0]} if inner else set())
    left = left[:-1] + next(c for c in "ACGT" if c not in avoid)
    if inner and right[0] == inner[0]:
        right = other(right[0]) + right[1:]
        if left[-1] == right[0]:
            left = left[:-1] + next(c for c in "ACGT" if c not in {right[0], inner[-1], inner[0]})
    return left, right


def stored(case, reverse):
    """The case with its contig stored reverse-complemented: body and event mapped to the stored columns."""
    if not reverse:
        return dict(case, reverse=False)
    n = len(case["contig"])
    b0, b1 = case["body"]
    out = dict(case, contig=revcomp(case["contig"]), truth=revcomp(case["truth"]), body=(n - b1, n - b0), reverse=True)
    e = case.get("event")
    if "event_rev" in case:                       # an event that can slide: the leftmost column of the reversed contig is its other end
        out["event"] = case["event_rev"]
    elif e is not None:
        kind, p, g, num = e
        if kind == DEL:
            out["event"] = (DEL, n - p - g, g, 0)
        else:
            bases = "".join("ACGT"[(num >> (2 * k)) & 3] for k in range(g - 1, -1, -1))
            out["event"] = (INS, n - p, g, num_of(revcomp(bases)))
    return out


def missing_bases(rng, n=600, at=300, gone="GTC", L=150, n_reads=120, err=0.005, body=(100, 500)):
    """The contig lacks `gone` at column `at`: the reads insert it."""
    left, right = unique_pair(rng, at, n - at, gone)
    truth = left + gone + right
    return {"truth": truth, "contig": left + right, "body": body, "reads": sample(rng, truth, n_reads, L, err), "event": (INS, at, len(gone), num_of(gone))}


def extra_bases(rng, n=600, at=300, extra="CA", L=150, n_reads=120, err=0.005, body=(100, 500)):
    """The contig has `extra` at column `at` that the truth has not: the reads delete it."""
    left, right = unique_pair(rng, at, n - at, extra)
    truth = left + right
    return {"truth": truth, "contig": left + extra + right, "body": body, "reads": sample(rng, truth, n_reads, L, err), "event": (DEL, at, len(extra), 0)}


def homopolymer(rng, L=150, run=8, extra=2, offsets=None):
    """A run of `run` A's in the truth, run + extra in the contig; exact rows of both strands with the run well inside them: every one
    of them has to name the deletion at the run's first column."""
    left, right = seq(rng, 300)[:-1] + "C", "G" + seq(rng, 300)
    truth = left + "A" * run + right
    offsets = offsets if offsets is not None else [300 - L // 2 + d for d in range(-24, 25, 4)]
    return {"truth": truth, "contig": left + "A" * (run + extra) + right, "body": (100, 500 + extra), "reads": exact_rows(truth, offsets, L),
            "event": (DEL, 300, extra, 0), "event_rev": (DEL, len(right), extra, 0)}


def tandem(rng, L=150, unit="ACG", copies=5, offsets=None):
    """`copies` units in the truth, one fewer in the contig: the insertion of one unit, in the rotation that stands at the repeat's
    first column."""
    left, right = seq(rng, 300)[:-1] + "T", "T" + seq(rng, 300)
    truth = left + unit * copies + right
    offsets = offsets if offsets is not None else [300 - L // 2 + d for d in range(-24, 25, 4)]
    return {"truth": truth, "contig": left + unit * (copies - 1) + right, "body": (100, 500), "reads": exact_rows(truth, offsets, L),
            "event": (INS, 300, len(unit), num_of(unit)), "event_rev": (INS, len(right), len(unit), num_of(revcomp(unit)))}


def minority(rng, L=150, n_reads=300, share=0.3):
    """Reads of the contig itself, and a share of reads — sampled the same way — that lack three bases of it: nothing may change."""
    left, right = unique_pair(rng, 300, 300, "GTC")
    truth = left + "GTC" + right
    variant = left + right
    n_var = int(n_reads * share)
    return {"truth": truth, "contig": truth, "body": (100, 503),
            "reads": sample(rng, truth, n_reads - n_var, L, 0.0) + sample(rng, variant, n_var, L, 0.0),
            "event": (DEL, 300, 3, 0)}
