"""Static check on the compiled joins of the vocabulary-parallel top-k head and draw (csrc/tp_heads.hip; tools/isa_check.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_check  # noqa: E402


def test_key_joins_pull_records_as_single_16_byte_system_scope_loads():
    asm = isa_check.device_asm("tp_heads.hip")
    report, errors = isa_check.check_tp_key_joins(asm)
    for name, x4, lds in report:
        print(f"{name}: {x4} buffer_load_dwordx4 sc0 sc1, {lds} B of LDS")
    assert not errors, "\n".join(errors)
    assert sorted("topk" if "tp_topk_join_kernel" in name else "sample" for name, _, _ in report) == ["sample", "topk"]
    # the score join is still the one kernel of its name, with the properties it had
    score, errors = isa_check.check_tp_score_join(asm)
    assert not errors and len(score) == 1
