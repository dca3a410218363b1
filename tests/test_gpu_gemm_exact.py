"""Exact tests of the GEMM epilogues STORE, RESID and SWIGLU (csrc/gemm_epilogue.h) through the launcher probe mmada_probe_gemm.

Every launch must return the expected BITS — integer arithmetic and single IEEE operations on the CPU (tests/helpers.py, checked by
tests/test_gemm_exact_host.py) — under every tile configuration of both kernels; the probe must report the configuration that
was pinned wherever the shape contract admits it, and the automatic pick where it does not; and C is a window inside a larger
allocation filled with a canary NaN, of which every element outside [0, M) x [0, N) must survive (guard rows before and after,
ldc > N by 8 or 24 elements).  tests/test_gpu_kernels.py::test_gemm_bt stays as the random-data sanity check.

What each defect of tests/test_gemm_exact_host.py::test_every_listed_mutation_is_rejected would hit here, and the code it guards:
  * a transposed 16 x 16 fragment — the two accumulator layouts: m = mrow0 + mi * 16 + r, n = wcol0 + ni * 16 + frow in gemm_epilogue
    against one row and four consecutive columns per lane in gemm_epilogue_t (gemm8.hip issues its MFMAs with swapped operands);
    every store and one-hot case under configurations 0..3 and 1000 + BM.
  * an 8-column run shifted by 8 — run8_col(lq) and swap_halves16 in gemm_epilogue_t: which half-row a lane holds after the
    v_permlane16_swap; the 8-phase configurations of every case.
  * a K-tile dropped or counted twice — the stage / wait ring of gemm.hip's mainloop (kt + STAGES - 1 < k1, two and three stages)
    and the two-tile tail of gemm8.hip's run(): the store cases at K = 64, 128, 192, 256 (tail only), 384, 640 and 16512.
  * the residual on the wrong owner's fragment rows — ((m >> 4) % g.resid_mod) == g.resid_rank, in all three epilogue forms
    (16-wave; batched, FM = 5: the 160 x 256 and 320 x 128 tiles; row by row, FM = 8 and 10): test_resid_ownership_and_rounding_order.
  * the residual added by every rank — the `if (radd[mj])` in front of the batched 16-byte loads and the `if (add)` of the other
    forms: the NaN on every row the rank does not own would come out.
  * single instead of double rounding — v = bfround(v) before the add in gemm_epilogue, pack_bf2 of the accumulators before the
    add in gemm_epilogue_t: every residual case (5 % of the outputs or more tell the two apart).
  * rbeg off by one row, or the window ignored — rrow = bb * g.rlp + g.rbeg + (m - bb * g.rwin), including its clamped form
    min(m, m_lim - 1) in the batched path: test_resid_row_window.
  * gate and up halves swapped — acc[mi][2 * q2] is the gate, acc[mi][2 * q2 + 1] the up fragment, SiLU on the gate only, table and
    evaluating path: test_swiglu_is_exact.
  * and the canaries guard `m >= m_lim`, `n >= g.N` and `wcol0 + q2 * 32 >= g.N` in front of the 16-byte stores.
62 cases x 12 configurations = 744 launches; the file takes 3 s on an MI355X, no case more than 0.3 s."""
import ctypes as C

import pytest
import torch

from helpers import (GEMM_BM16, GEMM_CANARY, GEMM_CONFIGS, gemm8_admits, gemm_exact_verdict, gemm_expected_resid, gemm_expected_store,
                     gemm_int_operands, gemm_onehot, gemm_owner, gemm_poison_resid, gemm_pre, gemm_random_w, gemm_resid, gemm_resid_rows,
                     silu_margin_ok, swiglu_expected, swiglu_pack, swiglu_weights)
from mmada_parallel_amd import abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 32                                                   # canary rows in front of row 0 and behind row M - 1
RUNS = [(c, 1) for c in GEMM_CONFIGS] + [(0, 0)]             # ("gemm_config", "gemm_short_tiles")


def _run_case(epi, A, W, exp, *, resid=None, ldr=0, mod=1, rank=0, rwin=0, rlp=0, rbeg=0, publish=0, c_offset=0, silu_lut=1, pads=(8, 24), what=""):
    """One case (operands and expected output on the CPU) under every configuration.  Collects every violation, then asserts."""
    lib = abi.lib()
    M, K = A.shape
    N = W.shape[0]
    ncol = exp.shape[1]
    assert exp.shape[0] == M and ncol == (N // 2 if epi == 2 else N)
    Ad, Wd = A.to(DEV), W.to(DEV)
    Rd = resid.to(DEV) if resid is not None else None
    exp_bits = exp.view(torch.int16).to(DEV)
    errors, auto = [], None
    try:
        for i, (cfg, short) in enumerate(RUNS):
            ldc = ncol + pads[i % len(pads)]
            abi.check(lib.mmada_set_option(b"gemm_config", cfg), "set_option")
            abi.check(lib.mmada_set_option(b"gemm_short_tiles", short), "set_option")
            abi.check(lib.mmada_set_option(b"gemm_silu_lut", silu_lut), "set_option")
            rows = M + 2 * GUARD
            flat = torch.full((rows * ldc + 16,), GEMM_CANARY, dtype=torch.int16, device=DEV)
            area = flat[c_offset:c_offset + rows * ldc].view(rows, ldc)
            window = area[GUARD:GUARD + M, :ncol]
            p = abi.MmadaGemmProbe(A=Ad.data_ptr(), W=Wd.data_ptr(), C=window.data_ptr(), resid=abi.ptr(Rd), epi=epi, M=M, N=N, K=K, ldc=ldc,
                                   ldr=ldr, resid_mod=mod, resid_rank=rank, rwin=rwin, rlp=rlp, rbeg=rbeg, publish=publish)
            abi.check(lib.mmada_probe_gemm(C.byref(p), abi.stream_ptr()), "probe_gemm")
            torch.cuda.synchronize()
            tag = f"{what} config {cfg}{'' if short else ', full-height row tiles'} (ran {p.ran}, ldc {ldc})"
            # ---- which kernel ran ----
            can8 = gemm8_admits(M, N, K, ldc, ldr if epi == 1 else None, 2 * c_offset)
            if cfg == -1:
                auto = p.ran
                if not (p.ran - 1000 in GEMM_BM16 or (can8 and 0 <= p.ran <= 3)):
                    errors.append(f"{tag}: the automatic pick is no configuration this shape admits")
            elif cfg >= 1000 or can8:
                if p.ran != cfg:
                    errors.append(f"{tag}: the pinned configuration did not run")
            elif p.ran != auto or p.ran < 1000:   # a pinned 8-phase tile the shape contract rejects: the automatic pick, a 16-wave kernel
                errors.append(f"{tag}: expected the fallback {auto}")
            # ---- the bits ----
            if not torch.equal(window, exp_bits):
                v = gemm_exact_verdict(window.cpu().view(torch.bfloat16), exp)
                errors.append(f"{tag}: {v['count']} of {M * ncol} outputs wrong, first at (m, n) = {v['first']}: got {v['got']:#06x}, "
                              f"expected {v['expected']:#06x}")
            # ---- the canaries: everything outside the window ----
            window.fill_(GEMM_CANARY)
            dead = flat != GEMM_CANARY
            if bool(dead.any()):
                at = int(dead.nonzero()[0]) - c_offset
                errors.append(f"{tag}: {int(dead.sum())} elements outside C overwritten, first at row {at // ldc - GUARD}, column {at % ldc}")
            flat.zero_()      # no NaN goes back to the caching allocator: a later test's uninitialised buffer may be this memory
    finally:
        if Rd is not None:
            Rd.zero_()
        lib.mmada_set_option(b"gemm_config", -1)
        lib.mmada_set_option(b"gemm_short_tiles", 1)
        lib.mmada_set_option(b"gemm_silu_lut", 1)
    assert not errors, f"{len(errors)} violations:\n" + "\n".join(errors[:12])


_INT = {}


def _int_case(M, N, K):
    """Integer operands, their exact pre-activation and a residual at the accumulator's magnitude: computed once per shape, read-only."""
    if (M, N, K) not in _INT:
        A, W = gemm_int_operands(M, N, K)
        pre = gemm_pre(A, W)
        _INT[(M, N, K)] = (A, W, pre, gemm_resid(pre, M, N + 16))
    return _INT[(M, N, K)]


# ------------------------------------------------------------------------------------------------------------------ EPI_STORE
@pytest.mark.parametrize("M,N,K", [(77, 204, 64), (8, 256, 128), (8, 256, 192), (328, 520, 256), (648, 512, 384), (632, 264, 640),
                                   (328, 256, 16512)])
def test_store_is_exact(M, N, K):
    """bf16(acc) of integer operands.  (77, 204, 64): M, N not multiples of 8 — 16-wave kernels only — and one K-tile (a pipeline
    prologue with nothing to prefetch); (8, 256, 128 / 192): two and three K-tiles on the 2- and 3-stage 16-wave kernels, one 8-row tile;
    (328, 520, 256): the 8-phase kernel's least K (its two-tile tail only), 320 + 8 rows, 2 x 256 + 8 columns; (648, 512, 384): short row
    tiles (pitch 304), an odd count of K-tile pairs; (632, 264, 640): does not fit short tiles, ragged last column tile;
    (328, 256, 16512): K > 16384, no zero rows — the pad rows of the last row tile re-read live rows."""
    A, W, pre, _ = _int_case(M, N, K)
    _run_case(0, A, W, gemm_expected_store(pre), what=f"store ({M}, {N}, {K})")


def test_store_misaligned_c_falls_back_and_is_exact():
    """C two elements (4 bytes) off a 16-byte boundary: the 8-phase kernel's 16-byte stores cannot run, every pinned 8-phase
    configuration must report the automatic 16-wave pick (asserted in _run_case) and still return the exact bits."""
    A, W, pre, _ = _int_case(328, 520, 256)
    _run_case(0, A, W, gemm_expected_store(pre), c_offset=2, what="store, C + 2 elements")


@pytest.mark.parametrize("M,N,K,stride,shift", [(328, 520, 256, 37, 11), (77, 204, 64, 5, 3)])
def test_store_onehot_routes_k_and_n(M, N, K, stride, shift):
    """A[m, pi(m)] = 1: the output is W[n, pi(m)] itself, arbitrary mantissas — which k and which n every element reads."""
    A, pi = gemm_onehot(M, K, stride, shift)
    W = gemm_random_w(N, K)
    _run_case(0, A, W, W[:, pi].t().contiguous(), what=f"one-hot ({M}, {N}, {K})")


# ------------------------------------------------------------------------------------------------------------------ EPI_RESID
RESID_SHAPES = [(328, 520, 256), (648, 512, 384), (632, 264, 640)]
OWNERS = [(1, 0), (2, 0), (2, 1), (4, 0), (4, 1), (4, 2), (4, 3), (8, 0), (8, 3), (8, 7)]


def test_resid_ragged_one_k_tile():
    """(77, 204, 64) with the residual on every row: the 16-wave epilogue's element guards with a residual read behind them."""
    A, W, pre, resid = _int_case(77, 204, 64)
    _run_case(1, A, W, gemm_expected_resid(pre, resid), resid=resid, ldr=resid.shape[1], what="resid (77, 204, 64)")


@pytest.mark.parametrize("mod,rank", OWNERS)
@pytest.mark.parametrize("M,N,K", RESID_SHAPES)
def test_resid_ownership_and_rounding_order(M, N, K, mod, rank):
    """bf16(resid + bf16(acc)) on the fragment rows rank `rank` of `mod` owns, bf16(acc) — finite — on the others, whose residual rows
    hold NaN: a rank reads 1 / tp of the stream and nothing else (kernels.h: GemmArgs::resid_mod).  The three shapes reach the
    row-by-row residual path of the 320-row tiles (FM = 10), short row tiles with a residual, and the batched path with ragged tiles."""
    A, W, pre, resid = _int_case(M, N, K)
    poisoned = gemm_poison_resid(resid, gemm_resid_rows(M)[gemm_owner(M, mod, rank)])
    exp = gemm_expected_resid(pre, poisoned, mod, rank)
    assert bool(torch.isfinite(exp.float()).all())
    _run_case(1, A, W, exp, resid=poisoned, ldr=resid.shape[1], mod=mod, rank=rank, what=f"resid ({M}, {N}, {K}) rank {rank} of {mod}")


@pytest.mark.parametrize("M,N,K", RESID_SHAPES)
def test_resid_publish_keeps_the_bits(M, N, K):
    """publish = 1 (the system-scope release behind the stores of a tensor-parallel partial sum) changes no value."""
    A, W, pre, resid = _int_case(M, N, K)
    _run_case(1, A, W, gemm_expected_resid(pre, resid), resid=resid, ldr=resid.shape[1], publish=1, what=f"resid + publish ({M}, {N}, {K})")


@pytest.mark.parametrize("mod,rank", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("B,rwin,rlp,rbeg", [(3, 136, 200, 32), (2, 72, 168, 64)])
def test_resid_row_window(B, rwin, rlp, rbeg, mod, rank):
    """Compact rows b * rwin + i read the residual of full-layout row b * rlp + rbeg + i; every residual row outside the windows — and
    every row inside that the rank does not own — holds NaN.  M = 408 is one full row tile plus 88 rows; N = 264, K = 256."""
    M, N, K = B * rwin, 264, 256
    A, W, pre, _ = _int_case(M, N, K)
    resid = gemm_resid(pre, B * rlp, N + 16, seed=rwin)
    poisoned = gemm_poison_resid(resid, gemm_resid_rows(M, rwin, rlp, rbeg)[gemm_owner(M, mod, rank)])
    exp = gemm_expected_resid(pre, poisoned, mod, rank, rwin, rlp, rbeg)
    assert bool(torch.isfinite(exp.float()).all())
    _run_case(1, A, W, exp, resid=poisoned, ldr=N + 16, mod=mod, rank=rank, rwin=rwin, rlp=rlp, rbeg=rbeg,
              what=f"resid window {B} x {rwin} of {rlp} from {rbeg}, rank {rank} of {mod}")


# ----------------------------------------------------------------------------------------------------------------- EPI_SWIGLU
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("lut", [1, 0])
@pytest.mark.parametrize("M,N,K,stride,shift", [(77, 64, 64, 5, 3), (328, 576, 256, 37, 11), (648, 1088, 384, 53, 7)])
def test_swiglu_is_exact(M, N, K, stride, shift, lut, mixed):
    """bf16(silu_bf16(gate) * up) with one-hot A, so gate and up are weight entries: gates from the safe set (helpers.silu_safe_set:
    the table's whole domain, minus the few values whose SiLU lies within 2^-16 of a rounding midpoint), so that every wave reads the
    table when it is on; `mixed` puts 0 and +-32 into some gate columns, whose waves must evaluate.  Ragged row tiles, a 64-column
    last tile, two and five column tiles; N / 2 output columns, ldc = N / 2 + 8."""
    extras = None
    if mixed:
        cand = torch.tensor([0.0, 32.0, -32.0], dtype=torch.bfloat16)
        extras = cand[silu_margin_ok(cand)[0]]          # silu(-32) is held to its own margin, and dropped if it fails
        assert extras.numel() >= 2
    G, U = swiglu_weights(N, K, extras=extras)
    A, pi = gemm_onehot(M, K, stride, shift)
    _run_case(2, A, swiglu_pack(G, U), swiglu_expected(G, U, pi), silu_lut=lut, pads=(8,),
              what=f"swiglu ({M}, {N}, {K}) table {'on' if lut else 'off'}{', evaluating values mixed in' if mixed else ''}")

