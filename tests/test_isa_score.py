"""Static checks on the compiled row-statistics epilogue of the 8-phase GEMM (the scoring head; tools/isa_check.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_check  # noqa: E402


def test_rowstat_instantiations_get_the_checks_of_the_other_epilogues():
    """Counted waits behind LDS-DMA only, M0 contract, no static LDS, no spill, no scalar memory write; three 256-column tile
    configurations; one v_exp_f32 per logit and code path; per kernel one 16-byte record store, no logit store."""
    asm = isa_check.device_asm("gemm8.hip")
    report, errors = isa_check.check_gemm8_rowstat(asm)
    assert not errors, "\n".join(errors)
    assert len(report) == 3
    for name, n_dma, n_wait, n_exp, x4, x1 in report:
        assert n_dma >= 20 and n_wait >= 12 and n_exp >= 80 and x4 == 1, (name, n_dma, n_wait, n_exp, x4, x1)
    # the other epilogues' report is what it was: 4 epilogues x 4 tile configurations
    assert len(isa_check.check_gemm8(asm)[0]) == 16
