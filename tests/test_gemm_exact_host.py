"""Host side of the exact GEMM-epilogue tests (tests/test_gpu_gemm_exact.py): the operand builders, the expected values and the
verdict are checked on the CPU — the inputs can tell the defects apart, and every listed mutation of a CPU emulation of the
expected output is rejected — so that a GPU failure points at the kernel.  mmada_probe_gemm's refusals need no GPU either."""
import pytest
import torch

from helpers import (bits, gemm8_admits, gemm_exact_verdict, gemm_expected_resid, gemm_expected_store, gemm_int_operands, gemm_onehot,
                     gemm_owner, gemm_poison_resid, gemm_pre, gemm_random_w, gemm_resid, gemm_resid_rows, silu_bf16_torch, silu_margin_ok,
                     silu_safe_set, swiglu_expected, swiglu_pack, swiglu_weights)
from mmada_parallel_amd import abi

# the shapes the input conditions were measured on, and every integer-operand shape of the GPU file but the 8-row ones
CONDITION_SHAPES = [(328, 520, 384), (648, 512, 256), (77, 200, 64), (77, 204, 64), (328, 520, 256), (648, 512, 384), (632, 264, 640)]


def _adjacent_equal_share(t):
    b = bits(t)
    return max(float((b[:, 1:] == b[:, :-1]).float().mean()), float((b[1:] == b[:-1]).float().mean()))


@pytest.mark.parametrize("M,N,K", CONDITION_SHAPES)
def test_integer_operands_can_tell_the_defects_apart(M, N, K):
    A, W = gemm_int_operands(M, N, K)
    assert float(A.float().abs().max()) <= 15 and bool((A.float() == A.float().round()).all())
    pre = gemm_pre(A, W)
    # the builder's product IS the integer product
    assert torch.equal(pre, A.to(torch.int64) @ W.to(torch.int64).t())
    assert int(pre.abs().max()) < 2 ** 24 and K * 15 * 15 < 2 ** 24
    store = gemm_expected_store(pre)
    inexact = float((store.double() != pre.double()).float().mean())
    assert inexact >= 0.10, inexact                      # a wrong or missing bf16 rounding shows
    resid = gemm_resid(pre, M, N + 16)
    double = gemm_expected_resid(pre, resid)
    single = gemm_expected_resid(pre, resid, single_rounding=True)
    differ = float((bits(double) != bits(single)).float().mean())
    assert differ >= 0.05, differ                        # the rounding order bf16(resid + bf16(acc)) shows
    assert _adjacent_equal_share(store) < 0.01 and _adjacent_equal_share(double) < 0.01   # a neighbour's value shows
    print(f"({M}, {N}, {K}): {inexact:.3f} of the pre-activations are not bf16-exact, {differ:.3f} of the residual outputs tell double "
          f"from single rounding, {_adjacent_equal_share(store):.4f} of adjacent outputs are equal")


def test_expected_residual_is_one_add_and_one_rounding():
    A, W = gemm_int_operands(77, 204, 64)
    pre = gemm_pre(A, W)
    resid = gemm_resid(pre, 77, 220)
    exp = gemm_expected_resid(pre, resid)
    # the same in float64: bf16(acc) + resid is exact there (two bf16 values within 2^40 of each other), one rounding follows
    acc = gemm_expected_store(pre)
    from helpers import bf16_nearest
    assert torch.equal(exp.double(), bf16_nearest(acc.double() + resid[:, :204].double()))
    # non-owner rows are bf16(acc), whatever the residual holds there
    own = gemm_owner(77, 2, 1)
    poisoned = gemm_poison_resid(resid, gemm_resid_rows(77)[own])
    got = gemm_expected_resid(pre, poisoned, mod=2, rank=1)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got[~own], acc[~own]) and torch.equal(got[own], exp[own])
    assert own[:16].sum() == 0 and own[16:32].all() and own[64:].sum() == 0


def test_row_window_map():
    rows = gemm_resid_rows(408, 136, 200, 32)
    assert rows[0] == 32 and rows[135] == 167 and rows[136] == 232 and rows[407] == 2 * 200 + 32 + 135
    assert rows.unique().numel() == 408 and int(rows.max()) < 3 * 200
    assert torch.equal(gemm_resid_rows(5), torch.arange(5))


def test_onehot_operand_pins_k_and_n():
    for (M, N, K, s, t) in [(328, 520, 256, 37, 11), (77, 204, 64, 5, 3)]:
        A, pi = gemm_onehot(M, K, s, t)
        W = gemm_random_w(N, K)
        assert bool((A.float().sum(1) == 1).all()) and pi.unique().numel() == min(M, K)      # odd stride: every k is used
        exp = W[:, pi].t()
        assert torch.equal((A.double() @ W.double().t()), exp.double())                      # the product IS the selected entry
        assert W.unique().numel() > 1000 and (bits(W) & 0x7F).unique().numel() == 128          # arbitrary mantissas: all 128 occur
        # reading the neighbouring k, or the neighbouring n, shows on nearly every element
        assert gemm_exact_verdict(W[:, (pi + 1) % K].t(), exp)["count"] > 0.99 * M * N
        assert gemm_exact_verdict(exp.roll(1, dims=1), exp)["count"] > 0.99 * M * N


def test_silu_safe_set():
    gates, silu, n_domain = silu_safe_set()
    assert n_domain == 4864 and gates.numel() >= 0.99 * n_domain, gates.numel()
    assert float(gates.float().abs().min()) == 2.0 ** -14 and float(gates.float().abs().max()) < 32.0
    # torch's fp32 SiLU, rounded to bf16, is the float64 value's rounding on every one of them
    assert torch.equal(bits(silu_bf16_torch(gates)), bits(silu))
    # the evaluating path's values: silu(0) = 0 and silu(32) = 32 exactly; -32 is held to the margin like the rest
    extras = torch.tensor([0.0, 32.0, -32.0], dtype=torch.bfloat16)
    ok, s = silu_margin_ok(extras)
    assert bool(ok[0]) and bool(ok[1]) and s[:2].tolist() == [0.0, 32.0]
    assert torch.equal(bits(silu_bf16_torch(extras[ok])), bits(s[ok]))
    print(f"safe set: {gates.numel()} of {n_domain}; silu(-32) passes its margin: {bool(ok[2])}")


def test_swiglu_builder():
    N, K, M = 576, 256, 328
    G, U = swiglu_weights(N, K)
    W = swiglu_pack(G, U)
    assert torch.equal(W[0:16], G[0:16]) and torch.equal(W[16:32], U[0:16]) and torch.equal(W[32:48], G[16:32])
    assert torch.equal(W[N - 16:], U[N // 2 - 16:])
    A, pi = gemm_onehot(M, K, 37, 11)
    pre = (A.double() @ W.double().t()).view(M, N // 32, 2, 16)
    exp = swiglu_expected(G, U, pi)
    # the packed product, un-packed: gate and up pre-activations of output column c are G[c, pi(m)] and U[c, pi(m)]
    assert torch.equal(pre[:, :, 0].reshape(M, N // 2), G[:, pi].t().double())
    assert torch.equal(pre[:, :, 1].reshape(M, N // 2), U[:, pi].t().double())
    assert exp.shape == (M, N // 2) and bool(torch.isfinite(exp.float()).all())
    safe = set(bits(silu_safe_set()[0]).tolist())
    assert set(bits(G).flatten().tolist()) <= safe                                           # every wave takes the table path
    extras = torch.tensor([0.0, 32.0], dtype=torch.bfloat16)
    G2, _ = swiglu_weights(N, K, extras=extras)
    outside = torch.tensor([b not in safe for b in bits(G2).flatten().tolist()]).view(N // 2, K)
    per_fragment = outside.view(N // 32, 16, K).any(1).float().mean(1)                       # share of k with an untabulated gate, per 16 columns
    assert int((per_fragment == 0).sum()) >= 3 and int((per_fragment > 0.4).sum()) >= 6       # table-only and evaluating fragments, both


def _mutants(M=328, N=520, K=256):
    """(name, expected, mutated emulation) for every listed defect."""
    A, W = gemm_int_operands(M, N, K)
    pre = gemm_pre(A, W)
    store = gemm_expected_store(pre)
    out = []
    t = store.clone()
    t[16:32, 32:48] = store[16:32, 32:48].t()
    out.append(("a transposed 16 x 16 fragment", store, t))
    t = store.clone()
    t[200:216, 264:272] = store[200:216, 272:280]
    out.append(("an 8-column run shifted by 8", store, t))
    nk = K // 64
    out.append(("one K-tile dropped", store, gemm_expected_store(gemm_pre(A, W, [1] * (nk - 1) + [0]))))
    out.append(("one K-tile counted twice", store, gemm_expected_store(gemm_pre(A, W, [2] + [1] * (nk - 1)))))
    resid = gemm_resid(pre, M, N + 16)
    good = gemm_expected_resid(pre, resid, mod=4, rank=1)
    out.append(("the residual on the wrong owner's fragment rows", good, gemm_expected_resid(pre, resid, mod=4, rank=1, owner_shift=1)))
    out.append(("the residual added by every rank", good, gemm_expected_resid(pre, resid, mod=4, rank=1, every_rank=True)))
    out.append(("single instead of double rounding", good, gemm_expected_resid(pre, resid, mod=4, rank=1, single_rounding=True)))
    # the same two ownership defects against the poisoned residual the GPU test uses: NaN where the rank must not read
    own = gemm_owner(M, 4, 1)
    poisoned = gemm_poison_resid(resid, gemm_resid_rows(M)[own])
    assert torch.equal(bits(gemm_expected_resid(pre, poisoned, mod=4, rank=1)), bits(good))
    out.append(("the residual added by every rank (poisoned)", good, gemm_expected_resid(pre, poisoned, mod=4, rank=1, every_rank=True)))
    Aw, Ww = gemm_int_operands(408, 264, 256)
    prew = gemm_pre(Aw, Ww)
    residw = gemm_resid(prew, 3 * 200, 280)
    goodw = gemm_expected_resid(prew, residw, rwin=136, rlp=200, rbeg=32)
    out.append(("rbeg off by one row", goodw, gemm_expected_resid(prew, residw, rwin=136, rlp=200, rbeg=33)))
    out.append(("the row window ignored", goodw, gemm_expected_resid(prew, residw)))
    G, U = swiglu_weights(576, 256)
    _, pi = gemm_onehot(328, 256, 37, 11)
    out.append(("gate and up halves swapped", swiglu_expected(G, U, pi), swiglu_expected(G, U, pi, swapped=True)))
    return out


def test_every_listed_mutation_is_rejected():
    for name, exp, mutated in _mutants():
        assert gemm_exact_verdict(exp, exp) is None
        v = gemm_exact_verdict(mutated, exp)
        assert v is not None and v["count"] > 0, name
        m, n = v["first"]
        assert v["got"] == int(bits(mutated)[m, n]) & 0xFFFF and v["expected"] == int(bits(exp)[m, n]) & 0xFFFF and v["got"] != v["expected"]
        print(f"{name}: {v['count']} elements, first at {v['first']}: got {v['got']:#06x}, expected {v['expected']:#06x}")


def test_verdict_points_at_one_element_and_sees_one_ulp_and_the_sign_of_zero():
    exp = gemm_expected_store(gemm_pre(*gemm_int_operands(77, 204, 64)))
    one = (bits(exp).clone())
    one[40, 100] += 1                                                       # one bf16 ulp
    v = gemm_exact_verdict(one.view(torch.bfloat16), exp)
    assert v["count"] == 1 and v["first"] == (40, 100)
    z = torch.zeros(2, 2, dtype=torch.bfloat16)
    assert gemm_exact_verdict(-z, z)["count"] == 4                         # -0 is not +0


def test_gemm8_contract_restated():
    assert gemm8_admits(328, 520, 256, 528) and gemm8_admits(648, 512, 384, 536, 528)
    assert not gemm8_admits(77, 204, 64, 212) and not gemm8_admits(8, 256, 128, 264) and not gemm8_admits(8, 256, 192, 264)
    assert not gemm8_admits(328, 520, 256, 528, c_byte_offset=4) and not gemm8_admits(328, 520, 256, 524)
    assert gemm8_admits(328, 256, 16512, 264)


def test_probe_refuses_bad_arguments_without_a_gpu():
    """Every refusal names mmada_probe_gemm and comes before anything touches the device."""
    lib = abi.lib()
    ok = dict(A=0x1000, W=0x2000, C=0x3000, resid=0x4000, epi=1, M=144, N=264, K=256, ldc=272, ldr=280, resid_mod=2, resid_rank=1,
              rwin=72, rlp=168, rbeg=64, publish=0)
    bad = [dict(A=None), dict(W=None), dict(C=None), dict(epi=3), dict(epi=-1), dict(resid=None), dict(resid_mod=0), dict(resid_rank=2),
           dict(resid_rank=-1), dict(rwin=-8), dict(rwin=80), dict(rbeg=100), dict(rbeg=-8), dict(epi=2, N=96), dict(ldc=256), dict(ldr=256),
           dict(epi=2, N=320, ldc=152)]
    for change in bad:
        p = abi.MmadaGemmProbe(**{**ok, **change})
        p.ran = 7
        assert lib.mmada_probe_gemm(p, None) != 0, change
        assert b"mmada_probe_gemm" in lib.mmada_last_error(), (change, lib.mmada_last_error())
        assert p.ran == -1, change
    assert lib.mmada_probe_gemm(None, None) != 0 and b"mmada_probe_gemm" in lib.mmada_last_error()
