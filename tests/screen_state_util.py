"""What a device screen left behind, for the GPU tests of the partitioned filter: the hits, the kernels launched and (gf_screen_debug_view, with
GF_DIAGNOSTICS and the option screen_keep_cand set) pass A's parts, their fill history and the candidate list handed to the verification."""
import ctypes as C

import numpy as np


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to("cuda")


def fetch(gf, ptr, n_words):
    from gappadder_amd import _lib as B
    out = np.empty(n_words, dtype=np.uint32)
    assert B.lib().gf_memcpy_d2h(gf.handle, out.ctypes.data, ptr, 4 * n_words) == 0
    return out


def filter_state(gf):
    """What the partitioned filter left behind: per part the number of pairs and the pairs themselves in generation order — (batch, octet,
    position) of every pair —, the fill history of every part, and the candidate list handed to the verification (sorted: its order is
    the order of the appends)."""
    from gappadder_amd import _lib as B
    v = B.ScreenView()
    assert B.lib().gf_screen_debug_view(gf.handle, C.byref(v)) == 0
    parts = 256 * v.n_writers
    count = fetch(gf, v.count, parts)
    assert (count <= v.cap).all()
    fills = fetch(gf, v.fills, parts * v.gs).reshape(parts, v.gs)[:, :v.n_groups + 1].copy()
    pairs = fetch(gf, v.pairs, parts * v.cap).reshape(parts, v.cap)
    # A pair's place inside its group's run is its rank from an LDS atomic — the order in which the waves arrive, different from launch to
    # launch of the SAME kernel — so the pairs are compared as the sorted content of every (part, group) run: which batch, which octet,
    # which key bits, and where the run lies in the part.
    part, pos = np.nonzero(np.arange(v.cap)[None, :] < count[:, None])
    big = np.int64(2 * v.cap + 2)
    bounds = (np.arange(parts, dtype=np.int64)[:, None] * big + fills[:, 1:]).ravel()
    run = np.searchsorted(bounds, part.astype(np.int64) * big + pos, side="right")
    assert (np.diff(run) >= 0).all()
    pairs = pairs[part, pos]
    pairs = pairs[np.lexsort((pairs, run))]
    n_cand = int(fetch(gf, v.n_cand, 1)[0])
    cand = np.sort(fetch(gf, v.cand, n_cand))
    return {"shape": np.array([v.n_writers, v.cap, v.gs, v.n_groups]), "count": count, "fills": fills, "pairs": pairs, "runs": run, "cand": cand}


def screen(gf, d_reads, n, L, k, d_col, geom, cap=1 << 21):
    """(sorted hits, hit count, reads dropped, kernels, filter state or None) of one device screen."""
    import torch
    from gappadder_amd import _lib as B
    d_out = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert B.lib().gf_screen_reads_probes_dev(gf.handle, d_reads.data_ptr(), None, d_col.data_ptr() if d_col is not None else None,
                                              C.byref(geom) if d_col is not None else None, n, L, k, 1, d_out.data_ptr(), cap, d_n.data_ptr()) == 0
    gf.sync()
    dropped = C.c_size_t(0)
    assert B.lib().gf_screen_last_overflow(gf.handle, C.byref(dropped)) == 0
    n_hits = int(d_n[0].item())
    assert n_hits <= cap
    hits = d_out[:n_hits * 8].cpu().numpy().view(B.HIT)
    kernels = B.lib().gf_screen_kernels(gf.handle).decode()
    return np.sort(hits, order=("gap", "read")), n_hits, dropped.value, kernels, filter_state(gf) if "pf4_" in kernels else None


def build_column(gf, d_reads, n, L, k):
    """The probe column of the reads (gf_read_probes_dev) and the geometry it was built for."""
    import torch
    from gappadder_amd import _lib as B
    want = B.ProbeColumnGeom()
    assert B.lib().gf_probe_geometry(gf.handle, n, L, k, C.byref(want)) == 0
    d_col = torch.full((max(1, B.lib().gf_probe_column_bytes(C.byref(want)) // 4),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    geom = B.ProbeColumnGeom()
    assert B.lib().gf_read_probes_dev(gf.handle, d_reads.data_ptr(), n, L, k, d_col.data_ptr(), C.byref(geom)) == 0
    gf.sync()
    assert geom.key() == want.key()
    return d_col, geom
