"""Static check on the compiled join of the vocabulary-parallel scoring head (csrc/tp_heads.hip; tools/isa_check.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_check  # noqa: E402


def test_score_join_kernel_is_compiled_and_pulls_whole_records():
    """Present in the compiled object; a peer's record is ONE 16-byte system-scope load per rank pass through a descriptor in
    SGPRs; no spill; the LDS of the shared fold (row_heads.h).  The one-rank join of row_heads.hip uses the same fold: same LDS."""
    report, errors = isa_check.check_tp_score_join(isa_check.device_asm("tp_heads.hip"))
    assert not errors, "\n".join(errors)
    assert len(report) == 1 and report[0][1] == 8            # one load form per possible owner (TP_MAX = 8)
    assert not isa_check.check_tp_pull(isa_check.device_asm("tp_comm.hip"))[1]   # the exchange's own kernels are what they were
    body, meta = isa_check.kernels(isa_check.device_asm("row_heads.hip"))
    one_rank = [n for n in body if "rowstat_combine_kernel" in n]
    assert len(one_rank) == 1 and int(meta[one_rank[0]]["group_segment_fixed_size"]) == report[0][2]
