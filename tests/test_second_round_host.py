"""The second assembly round's entry points (csrc/round2.hip): exported by the built library, declared in the header and typed in
gappadder_amd/_lib.py (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND2 = ["gf_both_unmapped_reads_dev", "gf_contig_kmer_table_dev", "gf_recruit_by_contigs_dev", "gf_round2_work_words",
          "gf_round2_pools_dev", "gf_contigs_append_dev"]


def test_round2_entry_points_are_declared_exported_and_typed():
    import __graft_entry__ as G
    G.build()
    from gappadder_amd import _lib as B
    txt = open(os.path.join(ROOT, "include", "gapfill_hip.h")).read()
    L = ctypes.CDLL(B.LIB_PATH)
    lib = B.lib()
    for name in ROUND2:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert getattr(lib, name).argtypes, name
    # work words: two per key (unique flag + its scan), two per gap (count + first index), two spare
    assert lib.gf_round2_work_words(1000, 24) == 2 * 1000 + 2 * 24 + 2
