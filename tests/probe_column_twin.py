"""numpy twin of the reads' probe column (gappadder_amd/csrc/kmer_dev.hpp `probe_word`, screen.hip `probe_geometry`): the geometry of the
probed 16-mers and the column words, written from the definition, independent of the library."""
import numpy as np

S16_MUL = 0x9E3779B1


def geometry(L, k, ext_allowed=True):
    """(first, stride, np, ext): probe j of a read = the 16 bases at offset first + j * stride."""
    stride, ext = k - 15, 0
    if ext_allowed:
        for e in (2, 1):
            if stride - e >= 1 and (L - k) // (stride - e) == (L - k) // stride:
                ext = e
                break
    stride -= ext
    n_probes = (L - k) // stride + 1
    first = k - 16 - ext
    lo = (L - k) - (n_probes - 1) * stride
    if (first & ~3) >= lo:
        first &= ~3
    # every k-mer position [0, L - k] holds a whole probe and its ext bases
    for p in range(L - k + 1):
        assert any(p <= first + j * stride and first + j * stride + 16 + ext <= p + k for j in range(n_probes)), (L, k, p)
    return first, stride, n_probes, ext


def plane_words(n_reads):
    return (int(n_reads) + 63) // 64 * 64


def word_index(n_reads, r, j):
    """Word of (read r, probe j) in the column: plane j, read r (Python integers: no wrap)."""
    return j * plane_words(n_reads) + r


def canon16(w):
    """min(w, reverse complement of w) of 16 bases packed 2 bits each, first base in the top bits."""
    w = w.astype(np.uint64)
    c = (~w) & np.uint64(0xFFFFFFFF)
    rc = np.zeros_like(w)
    for i in range(16):
        rc |= ((c >> np.uint64(2 * i)) & np.uint64(3)) << np.uint64(30 - 2 * i)
    return np.minimum(w, rc)


def column(packed, L, k, ext_allowed=True):
    """packed: (n, ceil(L / 4)) uint8 rows (4 bases per byte, first base in the top bits) -> the column, np * plane uint32 words."""
    first, stride, n_probes, _ = geometry(L, k, ext_allowed)
    n = packed.shape[0]
    bases = np.zeros((n, 4 * packed.shape[1]), dtype=np.uint64)
    for q in range(4):
        bases[:, q::4] = (packed >> (6 - 2 * q)) & 3
    out = np.zeros((n_probes, plane_words(n)), dtype=np.uint32)
    for j in range(n_probes):
        w = np.zeros(n, dtype=np.uint64)
        for i in range(16):
            w = (w << np.uint64(2)) | bases[:, first + j * stride + i]
        out[j, :n] = ((canon16(w) * np.uint64(S16_MUL)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out.reshape(-1)
