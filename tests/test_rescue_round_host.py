"""The rescue round's entry points (csrc/rescue.hip, merge.hip): exported by the built library, declared in the header and typed in
gappadder_amd/_lib.py; the bridges' place in the extended fill's order and the Pipeline's refused combinations (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESCUE = ["gf_rescue_work_bytes", "gf_rescue_reset_dev", "gf_rescue_hq_keys_dev", "gf_rescue_bridges_dev", "gf_rescue_gap_bridges",
          "gf_merge_rescue_dev"]


def test_rescue_entry_points_are_declared_exported_and_typed():
    import __graft_entry__ as G
    G.build()
    from gappadder_amd import _lib as B
    txt = open(os.path.join(ROOT, "include", "gapfill_hip.h")).read()
    L = ctypes.CDLL(B.LIB_PATH)
    lib = B.lib()
    for name in RESCUE:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert getattr(lib, name).argtypes, name
    for name in ("GF_RESCUE_MARK", "GF_RS_FIRST", "GF_RS_WORDS"):
        assert re.search(r"#define %s\b" % name, txt), name
    assert int(re.search(r"#define GF_RESCUE_MARK (\w+)", txt).group(1), 0) == B.RESCUE_MARK
    assert int(re.search(r"#define GF_RS_FIRST (\d+)", txt).group(1)) == B.RS_FIRST
    # the work buffer grows with every capacity; unsupported sizes give 0
    w = lib.gf_rescue_work_bytes(100, 4096, 4096, 12)
    assert w > 16 << 12 and lib.gf_rescue_work_bytes(100, 8192, 4096, 12) > w and lib.gf_rescue_work_bytes(100, 4096, 4096, 13) > w
    assert lib.gf_rescue_work_bytes(0, 4096, 4096, 12) == 0 and lib.gf_rescue_work_bytes(100, 4096, 4096, 3) == 0


def test_bridges_rank_after_the_merged_contigs_in_the_extension_order():
    from gappadder_amd._lib import RESCUE_MARK
    from gappadder_amd.pick_contigs import extension_order
    cs = [(RESCUE_MARK, RESCUE_MARK, "ACGTACGTAC"), (0, 0, "A" * 5), (31, 29, "C" * 4), (99, 97, "G" * 3), (RESCUE_MARK, RESCUE_MARK, "AAAA")]
    assert extension_order(cs, [(31, 29)]) == [2, 1, 3, 0, 4]


@pytest.mark.parametrize("kw, why", [(dict(), "needs merge_in_step"), (dict(merge_in_step=True, world=2), "single rank"),
                                     (dict(merge_in_step=True, force_exchange=True), "single rank"),
                                     (dict(merge_in_step=True, second_round=True), "rescue_round with second_round")])
def test_refused_combinations(kw, why):
    """Checked before the Pipeline touches a device, by the rescue round's own checks (the message says which)."""
    from gappadder_amd.pipeline import Pipeline
    with pytest.raises(ValueError, match="rescue_round.*" + why if not why.startswith("rescue_round") else why):
        Pipeline(None, 4, 150, [(31, 29)], rescue_round=True, **kw)
