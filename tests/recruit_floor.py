"""Repeated recruitment rounds (the device step's second round, second_round.py, run again and again with the contigs of the round
before) restated on the host for the synthetic step of step_util.py (24 gaps, 80 000 pairs), from the
oracle's pieces: round-1 pools = the oracle's flank screen at the smallest k plus mates (close to the step's tagger pools, not identical
to them), recruitment by shared canonical k-mer with the contigs of the round before, recruits kept, assembly by
oracle.c_oracle.assemble_pool at every (k, kv), pick by the exact host picker at 30 then 15 over the round's own contigs."""
import numpy as np

from step_util import GPS, L, N_PAIRS, NSCF, SEED, SLEN

_RC = str.maketrans("ACGT", "TGCA")


def _kmers(text, k):
    for i in range(len(text) - k + 1):
        w = text[i:i + k]
        if w.count("A") + w.count("C") + w.count("G") + w.count("T") == k:
            r = w[::-1].translate(_RC)
            yield w if w < r else r


def _pick(contigs, flank):
    from oracle import gp_oracle as PO
    want = [("c%d" % i, t) for i, t in enumerate(contigs)]
    return any(PO.pick_gap("0_1", want, flank[0], flank[1], a)[0] for a in (30, 15)) if want else False


def rounds(gap_len, kk, max_rounds):
    """-> (closed after the first pick and after every recruitment round, pairs newly recruited per round); stops behind the first
    round that recruits nothing."""
    from oracle import c_oracle as CO
    cfg = CO.synth_cfg(seed=SEED, scaffold_len=SLEN, n_scaffolds=NSCF, gaps_per_scaffold=GPS, gap_len=gap_len, read_len=L)
    gaps, flanks = CO.synth_layout(cfg)
    packed, recs = CO.synth_pairs(cfg, 0, N_PAIRS)
    codes = np.stack([(packed >> s) & 3 for s in (6, 4, 2, 0)], axis=-1).reshape(len(packed), -1)[:, :L]
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    read = lambda r: text[r].tobytes().decode()
    k0 = min(k for k, _ in kk)
    hits = CO.screen_reads(text.tobytes(), L, flanks, k0)
    n = len(flanks)
    pool = [set() for _ in range(n)]
    for g, r in zip(hits["gap"].tolist(), hits["read"].tolist()):
        pool[g].update((r, r ^ 1))
    cand = sorted(set(int(r) >> 1 for r in recs["read"][(recs["flag"] & 12) == 12]))
    cand_kmers = {p: set(_kmers(read(2 * p), k0)) | set(_kmers(read(2 * p + 1), k0)) for p in cand}

    def assemble(g, extra):
        blob = "".join(read(r) for r in sorted(pool[g]) + [x for p in sorted(extra) for x in (2 * p, 2 * p + 1)]).encode()
        return [s for k, kv in kk for s, _, _ in CO.assemble_pool(blob, L, k, kv)]
    last = {g: assemble(g, ()) for g in range(n)}            # the contigs of the round before, per open gap that got some
    open_ = set(g for g in range(n) if not _pick(last[g], flanks[g]))
    closed, fresh = [n - len(open_)], []
    rec = [set() for _ in range(n)]
    for _ in range(max_rounds):
        table = {}
        for g in open_:
            for t in last.get(g, ()):
                for w in _kmers(t, k0):
                    table.setdefault(w, set()).add(g)
        new = {}
        for p, ws in cand_kmers.items():
            for w in ws & table.keys():
                for g in table[w]:
                    if p not in rec[g]:
                        new.setdefault(g, set()).add(p)
        fresh.append(sum(len(v) for v in new.values()))
        last = {}
        for g, ps in new.items():
            rec[g] |= ps
            last[g] = assemble(g, rec[g])
            if _pick(last[g], flanks[g]):
                open_.discard(g)
        closed.append(n - len(open_))
        if not fresh[-1]:
            break
    return closed, fresh
