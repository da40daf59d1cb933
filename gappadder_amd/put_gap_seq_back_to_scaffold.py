"""Write the closed gap sequences back into the draft scaffolds (mirrors put_gap_seq_back_to_scaffold.py:8-95).

Host-only text work.  Reproduced as the reference does it, quirks included, and pinned by a reference-generated fixture
(tests/golden/twolib/writeback.json.gz):
  * a picked record `>{scaffoldIdx}_{gapIdx}_...` fills gap gapIdx (1-based, gap_positions.txt order) of scaffold scaffoldIdx
    (.fai order); a later record for the same gap replaces an earlier one (:11-20);
  * a filled gap [start, end) is replaced by the sequence and copying resumes at end + 1 — the base at `end` (the first non-N
    base after the run) is DROPPED (:88), mirroring the one right-flank base the picker keeps (pick_contigs.py slice);
  * an unfilled gap of a scaffold that has other filled gaps keeps its N run (:80-82); a scaffold with no filled gap, or no gap at
    all, is written unchanged, header description included (:63-75); rebuilt scaffolds get the bare id as header (:93);
  * FASTA out in Biopython's writer convention: 60 columns.
An extension, only with the optional fifth argument (without it every byte is as above): flank_joins.tsv of the device-resident Collect
(device_collect.flank_joins_tsv).  A gap with a usable row there has NO missing sequence — its flanks overlap — and is joined when it has
no picked record, or only an `_extended` one (a partial fill around sequence that is already there): the scaffold is copied up to
`cut_from` and resumes at `resume_at`; a join that would reach back before what the previous gap consumed is skipped with a message; a
scaffold whose only changes are joins is rebuilt like one with fills.
usage: python -m gappadder_amd.put_gap_seq_back_to_scaffold scaffolds.fa gap_positions.txt picked_seqs.fa new_scaffolds.fa [flank_joins.tsv]"""
import sys


def _records(path):
    """(id, full header line without '>', sequence) per FASTA record."""
    out, name, desc, chunks = [], None, None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if name is not None:
                    out.append((name, desc, "".join(chunks)))
                name, desc, chunks = line[1:].split()[0], line[1:], []
            else:
                chunks.append(line)
    if name is not None:
        out.append((name, desc, "".join(chunks)))
    return out


def _wrap(title, seq):
    return ">" + title + "\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60))


def read_joins(path):
    """{scaffold index: {gap number: (cut_from, resume_at)}} of the usable rows of a flank_joins.tsv (columns by their header names)."""
    out = {}
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        col = {name: head.index(name) for name in ("gap", "usable", "cut_from", "resume_at")}
        for line in f:
            c = line.rstrip("\n").split("\t")
            if len(c) < len(head) or int(c[col["usable"]]) != 1:
                continue
            sid, gid = c[col["gap"]].split("_")[:2]
            out.setdefault(int(sid), {})[int(gid)] = (int(c[col["cut_from"]]), int(c[col["resume_at"]]))
    return out


def put_gap_seq_back_to_scaffold(sf_scf, sf_gap_pos, sf_gap_seq, sf_new_scf, sf_joins=None):
    gap_seq, partial = {}, set()
    for name, _, seq in _records(sf_gap_seq):
        f = name.split("_")
        gap_seq.setdefault(int(f[0]), {})[int(f[1])] = seq
        (partial.add if name.endswith("_extended") else partial.discard)((int(f[0]), int(f[1])))
    joins = read_joins(sf_joins) if sf_joins else {}
    scaffold_id = {}
    with open(sf_scf + ".fai") as fin:
        for cnt, line in enumerate(fin):
            scaffold_id[line.split()[0]] = cnt
    gap_pos, cnt, pre_id = {}, 1, 0
    with open(sf_gap_pos) as fin:
        for line in fin:
            f = line.split()
            sid = scaffold_id[f[3]]
            if pre_id != sid:
                cnt = 1
            gap_pos.setdefault(sid, {})[cnt] = (int(f[0]), int(f[1]))
            cnt += 1
            pre_id = sid
    with open(sf_new_scf, "w") as out:
        for name, desc, seq in _records(sf_scf):
            sid = scaffold_id[name]
            filled = gap_seq.get(sid, {})
            # the joins that apply: a gap of this scaffold without a picked record, or with a partial fill only
            joined = {gid: j for gid, j in joins.get(sid, {}).items()
                      if gid in gap_pos.get(sid, {}) and (gid not in filled or (sid, gid) in partial)}
            if sid not in gap_pos or not gap_pos[sid] or (sid not in gap_seq and not joined):
                out.write(_wrap(desc, seq))
                continue
            pre_pos, parts = 0, []
            for gid in range(1, len(gap_pos[sid]) + 1):
                if gid in joined:
                    cut_from, resume_at = joined[gid]
                    if cut_from >= pre_pos:
                        parts.append(seq[pre_pos:cut_from])
                        pre_pos = resume_at
                        continue
                    print("Join of Gap ", gid, "of Scaffold ", sid, "reaches before the previous gap!!!")
                if gid not in filled:
                    print("Gap ", gid, "of Scaffold ", sid, "does not exist!!!")
                    continue
                start, end = gap_pos[sid][gid]
                parts.append(seq[pre_pos:start])
                parts.append(filled[gid])
                pre_pos = end + 1
            parts.append(seq[pre_pos:])
            out.write(_wrap(name, "".join(parts)))


if __name__ == "__main__":
    put_gap_seq_back_to_scaffold(*sys.argv[1:6])
