"""The fused QKV epilogue (csrc/gemm_epilogue.h, EPI_QKV) held to exact answers: head routing, RoPE position, the K-major V
layout and the dLLM-cache scatter, in both forms of the epilogue (16-wave kernel; 8-phase kernel with per-wave operand order).

The checkpoints of helpers.qkv_exact_checkpoint make the GEMM in front of the epilogue exact (every pre-activation is one
product by a power of two), so q, k and V are compared with what the block's own input xn prescribes: V value for value, q and k
with oracle.llada_oracle.apply_rope — at most one bf16 ulp off, on at most 1e-4 of the elements (the only legitimate difference
is a table entry: rope_table_kernel rounds an fp64 sin / cos, torch evaluates them in fp32; tests/test_qkv_host.py checks the
builder and the conditions on the CPU).  The measured shares go to the parity report (helpers.save_parity).

Measured on an MI355X: the share of differing elements is 0 ... 1.2e-5 in every layout, shape, mode and GEMM configuration (at
L = 4096: 2.9e-6 ... 5.7e-6 for q, 0 ... 2.9e-6 for k), the figures the CPU gives when the oracle's rotation is fed the kernel's
table convention.  One ulp is |got - ref| <= 2^-7 |ref| plus a floor; with a bf16 denormal step as the only floor ONE element of
the 2 097 152 of q misses it in layouts (4, 2) and (4, 1) at L = 4096, under every GEMM configuration alike: the rotation cancels
there (|ref| = 3e-7 from operands of 0.6) and one fp32 ulp of a table entry is then more than a bf16 ulp of the result.  The
floor therefore carries the reference's own fp32 error as well (helpers.qkv_rope_verdict); how many elements needed it is printed
and recorded with every share."""
import ctypes as C

import pytest
import torch

from helpers import (QKV_LAYOUTS, QKV_VOCAB, check_block_stages, qkv_assert_rope, qkv_exact_checkpoint, qkv_expected, same_values,
                     save_parity, tiny_job, vt_unpermute)
from mmada_parallel_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 4096), (2, 333), (3, 70), (1, 1)]
GEMM_CODES = (-1, 0, 1, 2, 3, 1128, 1160, 1192, 1224, 1256, 1320)
NAN_BITS = 0x7FC0

_CK, _MODELS, _SHARES = {}, {}, {}


def _ck(layout):
    if layout not in _CK:
        _CK[layout] = qkv_exact_checkpoint(*layout)
    return _CK[layout]


def _model(layout, tp_rank=0, tp_size=1):
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    key = (layout, tp_rank, tp_size)
    if key not in _MODELS:
        ck = _ck(layout)
        _MODELS[key] = LLaDAForMultiModalGeneration.from_state_dict(ck.cfg, ck.sd, device=DEV, tp_rank=tp_rank, tp_size=tp_size)
    return _MODELS[key]


def _record(section, shares):
    _SHARES.setdefault(section, {}).update(shares)
    save_parity("qkv_epilogue_share_of_elements_one_ulp_off", _SHARES)


def _ids(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, QKV_VOCAB, (B, L), generator=g)


def _tap(model, which):
    """Raw parity tap: (address, Lp, Lkv) of an intermediate of the resident plain forward."""
    from mmada_parallel_amd import abi

    p, lp, lkv = C.c_void_p(), C.c_int32(), C.c_int32()
    abi.check(model._lib.mmada_debug_buffer(model._handle, which, C.byref(p), C.byref(lp), C.byref(lkv)), "debug_buffer")
    return p.value, lp.value, lkv.value


def _view(buf, addr, shape):
    """bf16 view of `shape` at device address `addr` inside the uint8 tensor `buf`."""
    n = 2
    for v in shape:
        n *= v
    off = addr - buf.data_ptr()
    assert 0 <= off and off + n <= buf.numel()
    return buf[off:off + n].view(torch.bfloat16).view(*shape)


def _plain(model, ids_d, nan_vt=False):
    """mmada_embed + mmada_attn_partial on layer 0; returns clones of xn [B, Lp, d], q [B, hq, Lkv, 128], k [B, hkv, Lkv, 128] and
    vT [B, hkv, 128, Lkv] in key order.  nan_vt: the vT region — whose address a forward of the same (B, L) leaves in the tap,
    carve_for depends on (B, L) only — is filled with the bf16 NaN pattern first."""
    from mmada_parallel_amd import abi

    B, L = ids_d.shape
    lib, h, st = model._lib, model._handle, abi.stream_ptr()
    model._ensure_ws(B, L)
    model._shape = (B, L)
    hkv = model.n_kv_heads // model.tp_size
    if nan_vt:
        addr, _, lkv = _tap(model, 3)
        _view(model._lanes[0].ws, addr, (B, hkv, 128, lkv)).view(torch.int16).fill_(NAN_BITS)
    abi.check(lib.mmada_embed(h, ids_d.data_ptr(), B, L, st), "embed")
    abi.check(lib.mmada_attn_partial(h, 0, st), "attn")
    Lp = (L + 7) // 8 * 8
    out = dict(xn=model.debug_buffer(0).view(B, Lp, -1).clone(), q=model.debug_buffer(1).clone(), k=model.debug_buffer(2).clone(),
               vT=model.debug_buffer(3).clone())
    torch.cuda.synchronize()
    return out


def _rmsnorm(ck, ids_d):
    """mmada_rmsnorm(wte[ids], attn_norm of block 0): [B, T, d] on the device."""
    from mmada_parallel_amd import abi

    B, T = ids_d.shape
    d = ck.base["d_model"]
    x = ck.sd["model.transformer.wte.weight"].to(DEV)[ids_d].contiguous()
    w = ck.sd["model.transformer.blocks.0.attn_norm.weight"].to(DEV).contiguous()
    out = torch.empty_like(x)
    abi.check(abi.lib().mmada_rmsnorm(x.data_ptr(), w.data_ptr(), out.data_ptr(), B * T, d, ck.base["rms_norm_eps"], abi.stream_ptr()),
              "rmsnorm")
    torch.cuda.synchronize()
    return out


def _plain_expected(ck, xn, L, dev="cpu"):
    B = xn.shape[0]
    pos = torch.arange(L).repeat(B, 1)
    return [t.to(dev) for t in qkv_expected(ck, xn[:, :L].cpu(), pos, pos)]


def _check_plain(tag, got, exp, L, heads=None, record=None):
    """The conditions on a plain forward's q, k, vT (heads: this rank's (q slice, kv slice) of the expectation) and on the pad
    region: vT columns >= L exactly zero, k rows in [L, Lp) finite."""
    q, k, v, tq, tk = exp
    if heads is not None:
        q, k, v, tq, tk = q[:, heads[0]], k[:, heads[1]], v[:, heads[1]], tq[:, heads[0]], tk[:, heads[1]]
    Lp = (L + 7) // 8 * 8
    qkv_assert_rope(f"{tag} q", got["q"][:, :, :L], q, tq, record)
    qkv_assert_rope(f"{tag} k", got["k"][:, :, :L], k, tk, record)
    assert same_values(got["vT"][..., :L].transpose(2, 3), v), f"{tag}: V differs from xn[:, col] * scale"
    assert int(torch.count_nonzero(got["vT"][..., L:])) == 0, f"{tag}: vT columns >= L are not zero"
    assert bool(torch.isfinite(got["k"][:, :, L:Lp].float()).all()), f"{tag}: k pad rows are not finite"


# ------------------------------------------------------------------------------------------------------ plain forward
@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("layout", QKV_LAYOUTS)
def test_plain_forward_qkv_is_exact(layout, B, L):
    ck, model = _ck(layout), _model(layout)
    ids_d = _ids(B, L, 11 * B + L).to(DEV)
    _plain(model, ids_d)                               # leaves the vT address of this (B, L) in the tap
    got = _plain(model, ids_d, nan_vt=True)
    # the block's input is mmada_rmsnorm of the embedded rows, bit for bit (the fused embedding runs the same row routine), and
    # zero on the pad rows
    assert torch.equal(got["xn"][:, :L], _rmsnorm(ck, ids_d))
    assert int(torch.count_nonzero(got["xn"][:, L:])) == 0
    shares = {}
    _check_plain(f"{layout} B={B} L={L}", got, _plain_expected(ck, got["xn"], L, DEV), L, record=shares)
    _record("plain", shares)


@pytest.mark.parametrize("B,L", [(2, 333), (1, 4096)])
@pytest.mark.parametrize("layout", QKV_LAYOUTS)
def test_every_gemm_configuration_writes_the_same_exact_qkv(layout, B, L):
    """Every tile configuration of both GEMM kernels (and the 320-row one with full-height row tiles): the conditions hold under
    each, and q, k over rows < L and the whole vT are bit-identical across them."""
    from mmada_parallel_amd import abi

    ck, model, lib = _ck(layout), _model(layout), abi.lib()
    ids_d = _ids(B, L, 7 * B + L).to(DEV)
    exp = _plain_expected(ck, _plain(model, ids_d)["xn"], L, DEV)
    outs, shares = {}, {}
    try:
        for code in GEMM_CODES:
            abi.check(lib.mmada_set_option(b"gemm_config", code), "set_option")
            outs[code] = _plain(model, ids_d, nan_vt=True)
        abi.check(lib.mmada_set_option(b"gemm_config", 0), "set_option")
        abi.check(lib.mmada_set_option(b"gemm_short_tiles", 0), "set_option")
        outs["0, full-height row tiles"] = _plain(model, ids_d, nan_vt=True)
    finally:
        lib.mmada_set_option(b"gemm_config", -1)
        lib.mmada_set_option(b"gemm_short_tiles", 1)
    first = outs[-1]
    for code, got in outs.items():
        _check_plain(f"{layout} B={B} L={L} gemm_config {code}", got, exp, L, record=shares)
        for name, rows in (("q", L), ("k", L), ("vT", None)):
            a, b = (got[name], first[name]) if rows is None else (got[name][:, :, :rows], first[name][:, :, :rows])
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"configuration {code}: {name} differs from the planner's pick"
    _record("gemm_configurations", shares)


@pytest.mark.parametrize("layout", [(4, 2), (4, 4)])
def test_tensor_parallel_ranks_write_their_slice(layout):
    """tp_size = 2 handles without any exchange: each rank's q, k and vT are exactly its heads of the expectation.  Rank r of
    (4, 2) owns two q heads and one kv head — its fused projection is the mixed K / V tile again."""
    ck = _ck(layout)
    B, L = 2, 333
    ids_d = _ids(B, L, 5).to(DEV)
    H, Hkv = layout
    shares = {}
    exp = None
    for r in range(2):
        model = _model(layout, r, 2)
        _plain(model, ids_d)
        got = _plain(model, ids_d, nan_vt=True)
        assert got["q"].shape[1] == H // 2 and got["k"].shape[1] == Hkv // 2
        assert torch.equal(got["xn"][:, :L], _rmsnorm(ck, ids_d))
        if exp is None:
            exp = _plain_expected(ck, got["xn"], L, DEV)
        heads = (slice(r * H // 2, (r + 1) * H // 2), slice(r * Hkv // 2, (r + 1) * Hkv // 2))
        _check_plain(f"{layout} tp=2 rank {r}", got, exp, L, heads=heads, record=shares)
    _record("tensor_parallel_slices", shares)


# ---------------------------------------------------------------------------------------------------------- cache step
CACHE_L = 200
# 13 positions per sequence (not a multiple of 8: the compact stream has pad rows).  Sequence 0: both ends and both sides of the
# 32-key block boundaries at 32 and 64; sequence 1: other positions, position 0 NOT among them (a pad row that were written at
# a clamped position would show there)
CACHE_POS = [[0, 1, 31, 32, 33, 63, 64, 100, 127, 128, 170, 198, 199], [3, 30, 31, 32, 65, 95, 96, 97, 130, 159, 160, 161, 199]]


def _slot_kv(model, cat):
    """Clones of layer 0's K [B, hkv, Lkv, 128] and vT [B, hkv, 128, Lkv] (key order) of the slot's memory (csrc/cache.hip,
    csrc/handle.h: K at the slot's base, vT after kv_bytes, in vt_key_pos order)."""
    ent = model._cache[cat]
    B, L = ent.shape
    hkv, Lkv = model.n_kv_heads // model.tp_size, (L + 63) // 64 * 64
    base = (ent.mem.data_ptr() + 255) // 256 * 256
    kv_bytes = (B * hkv * Lkv * 128 * 2 + 255) // 256 * 256
    torch.cuda.synchronize()
    return (_view(ent.mem, base, (B, hkv, Lkv, 128)).clone(), vt_unpermute(_view(ent.mem, base + kv_bytes, (B, hkv, 128, Lkv))).clone())


def _cache_inputs(B):
    L = CACHE_L
    ids0 = _ids(B, L, 21)
    ids1 = (ids0 + 1 + _ids(B, L, 22) % (QKV_VOCAB - 1)) % QKV_VOCAB        # differs from ids0 at EVERY position
    assert bool((ids0 != ids1).all())
    pos = torch.tensor(CACHE_POS[:B])
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[torch.arange(B)[:, None], pos] = True
    return ids0, ids1, pos, mask


@pytest.mark.parametrize("enable", [True, False])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("layout", [(2, 2), (4, 2)])
def test_cache_step_scatters_k_and_v_and_rotates_q(layout, B, enable):
    ck, model = _ck(layout), _model(layout)
    L, Lp = CACHE_L, (CACHE_L + 7) // 8 * 8
    ids0, ids1, pos, mask = _cache_inputs(B)
    Tc = pos.shape[1]
    assert Tc % 8 != 0 and L % 64 != 0
    allpos = torch.arange(L).repeat(B, 1)
    shares = {}
    tag = f"{layout} B={B} caching={enable}"
    try:
        model.caching(enable)
        _plain(model, ids0.to(DEV))                          # a plain forward of the same (B, L): its q address is the step's
        q_addr = _tap(model, 1)[0]
        # ---- prime: the slot holds ids0's keys / values at every position ----
        model.forward_cached(ids0.to(DEV), cat="c")
        k0, v0 = _slot_kv(model, "c")
        _, ek0, ev0, _, tk0 = qkv_expected(ck, _rmsnorm(ck, ids0.to(DEV)).cpu(), allpos, allpos)
        qkv_assert_rope(f"{tag} prime k", k0[:, :, :L].cpu(), ek0, tk0, shares)
        assert same_values(v0[..., :L].transpose(2, 3).cpu(), ev0)
        assert int(torch.count_nonzero(v0[..., L:])) == 0 and int(torch.count_nonzero(k0[:, :, L:])) == 0
        # ---- compute-mask step ----
        model.forward_cached(ids1.to(DEV), to_compute_mask=mask, cat="c")
        k1, v1 = _slot_kv(model, "c")
        Tq = (Tc + 63) // 64 * 64
        qc = _view(model._lanes[0].ws, q_addr, (B, layout[0], Tq, 128))[:, :, :Tc].cpu()
        xn_c = _rmsnorm(ck, ids1[mask].view(B, Tc).to(DEV)).cpu()
        pos_q = pos if enable else torch.arange(L - Tc, L).repeat(B, 1)     # the reference's fallback: the LAST Tc positions
        eq, ek, ev, tq, tk = qkv_expected(ck, xn_c, pos_q, pos)
        bi = torch.arange(B)[:, None]
        # masked positions: ids1's values, rotated at the token's sequence position
        qkv_assert_rope(f"{tag} step k", k1.cpu()[bi, :, pos].transpose(1, 2), ek, tk, shares)
        assert same_values(v1.cpu()[bi, :, :, pos].permute(0, 2, 1, 3), ev), f"{tag}: V at the masked positions"
        qkv_assert_rope(f"{tag} step q", qc, eq, tq, shares)
        # everything else — unmasked positions, the rows and columns >= L — is what the prime left, bit for bit: nothing of a
        # pad row of the compact stream (13 -> 16 rows) is written anywhere
        keep = torch.ones(B, k1.shape[2], dtype=torch.bool)
        keep[bi, pos] = False
        for b in range(B):
            kb = keep[b].to(DEV)
            assert torch.equal(k1[b][:, kb].view(torch.int16), k0[b][:, kb].view(torch.int16)), f"{tag}: K outside the mask changed"
            assert torch.equal(v1[b][:, :, kb].view(torch.int16), v0[b][:, :, kb].view(torch.int16)), f"{tag}: vT outside the mask changed"
        assert int(torch.count_nonzero(v1[..., L:])) == 0
        assert not same_values(k1[:, :, :Lp], k0[:, :, :Lp])                 # the step did write
    finally:
        model.caching(False)
    _record("cache_step", shares)


def test_mask_step_on_a_fresh_slot_keeps_never_computed_positions_at_zero():
    layout, B = (4, 2), 2
    ck, model = _ck(layout), _model(layout)
    L = CACHE_L
    _, ids1, pos, mask = _cache_inputs(B)
    Tc = pos.shape[1]
    shares = {}
    try:
        model.caching(True)
        model.forward_cached(ids1.to(DEV), to_compute_mask=mask, cat="fresh")
        k1, v1 = _slot_kv(model, "fresh")
        _, ek, ev, _, tk = qkv_expected(ck, _rmsnorm(ck, ids1[mask].view(B, Tc).to(DEV)).cpu(), pos, pos)
        bi = torch.arange(B)[:, None]
        qkv_assert_rope("fresh slot k", k1.cpu()[bi, :, pos].transpose(1, 2), ek, tk, shares)
        assert same_values(v1.cpu()[bi, :, :, pos].permute(0, 2, 1, 3), ev)
        keep = torch.ones(B, k1.shape[2], dtype=torch.bool)
        keep[bi, pos] = False
        for b in range(B):
            kb = keep[b].to(DEV)
            assert int(torch.count_nonzero(k1[b][:, kb].view(torch.int16))) == 0
            assert int(torch.count_nonzero(v1[b][:, :, kb].view(torch.int16))) == 0
    finally:
        model.caching(False)
    _record("cache_fresh_slot", shares)


# -------------------------------------------------------------------------------- grouped heads through the whole block
@pytest.mark.parametrize("layout", [(4, 2), (4, 1)])
def test_block_stages_vs_oracle_with_grouped_heads(layout):
    """The stage-by-stage comparison of tests/test_gpu_model.py::test_block_stages_vs_oracle, at its tolerances and on its ids
    (the tolerances were set on that job's sequences), on an ordinary random checkpoint — CFG_TINY widened to four heads, the same
    seed — with n_kv_heads != n_heads ((4, 1) spelled multi_query_attention=True)."""
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    H, Hkv = layout
    base = dict(synth.CFG_TINY, d_model=128 * H, n_heads=H, n_kv_heads=Hkv)
    sd = synth.synthetic_state_dict(base, seed=0)
    cfg = synth.full_config(base)
    if Hkv == 1:
        cfg.update(n_kv_heads=None, multi_query_attention=True)
    model = LLaDAForMultiModalGeneration.from_state_dict(cfg, sd, device=DEV)
    assert model.n_kv_heads == Hkv
    ids = tiny_job()["input_ids"].repeat(2, 1)
    ids[1, :8] = torch.arange(100, 108)
    check_block_stages(model, base, sd, ids)
