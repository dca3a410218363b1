"""Host side of the exact QKV-epilogue tests (tests/test_gpu_qkv.py): the checkpoint builder, its expectation and the
un-permutation of the K-major V tap are checked on the CPU against the oracle, so that a GPU failure points at the kernel."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from helpers import (QKV_LAYOUTS, QKV_SCALES, qkv_exact_checkpoint, qkv_expected, qkv_pre, qkv_rope_verdict, same_values, vt_key_pos,
                     vt_unpermute)
from mmada_parallel_amd import model as model_mod
from oracle import llada_oracle as lo


def _xn(ck, B, T, seed=3):
    """A block input as the device produces it: RMSNorm of embedded ids with the checkpoint's attn_norm."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, ck.base["vocab_size"], (B, T), generator=g)
    x = F.embedding(ids, ck.sd["model.transformer.wte.weight"])
    return x, lo.rms_norm(x, ck.sd["model.transformer.blocks.0.attn_norm.weight"], ck.base["rms_norm_eps"])


def test_vt_key_pos_is_a_permutation_of_every_32_key_block():
    pos = [vt_key_pos(l) for l in range(256)]
    assert sorted(pos) == list(range(256))
    for l in range(256):
        assert pos[l] // 32 == l // 32 and pos[l] % 4 == l % 4
    # the chunk order the attention kernel reads: position chunk j holds key chunk [0, 4, 1, 5, 2, 6, 3, 7][j]
    assert [pos.index(4 * j) // 4 for j in range(8)] == [0, 4, 1, 5, 2, 6, 3, 7]


@pytest.mark.parametrize("tp", [1, 2])
def test_debug_buffer_undoes_vt_key_pos(tp):
    """model.debug_buffer(3) on a stand-in library whose V tap is a CPU buffer written in vt_key_pos storage order: every key
    below 256 comes back at its own index, for every (batch, head, feature) row."""
    B, L, Lkv, H, Hkv = 2, 250, 256, 4, 2
    hkv = Hkv // tp
    # distinct bf16 bit patterns (all finite): key index in the low byte, the (batch, head, feature) row above it
    row = torch.arange(B * hkv * 128, dtype=torch.int32).view(B, hkv, 128, 1)
    want = (torch.arange(Lkv, dtype=torch.int32) + 256 * (row % 64 + 1)).to(torch.int16).view(torch.bfloat16)
    stored = torch.empty_like(want)
    for l in range(Lkv):
        stored[..., vt_key_pos(l)] = want[..., l]
    ws = stored.contiguous().view(torch.uint8).reshape(-1)

    def tap(handle, which, p, lp, lkv):
        p._obj.value, lp._obj.value, lkv._obj.value = ws.data_ptr(), (L + 7) // 8 * 8, Lkv
        return 0

    m = object.__new__(model_mod.LLaDAForMultiModalGeneration)
    m._lib = SimpleNamespace(mmada_debug_buffer=tap)
    m._handle = C.c_void_p()
    m._lanes = [model_mod._Lane(m._handle, ws)]
    m._resident = model_mod._Resident((B, L))
    m.config = SimpleNamespace(d_model=128 * H, n_heads=H)
    m.mlp_hidden, m.tp_size, m.n_kv_heads = 512, tp, Hkv
    got = m.debug_buffer(3)
    assert got.shape == (B, hkv, 128, Lkv)
    assert torch.equal(got, want)
    assert torch.equal(vt_unpermute(stored), want)                          # the tests' own restatement agrees


@pytest.mark.parametrize("layout", QKV_LAYOUTS)
def test_effective_n_kv_heads_of_the_layouts(layout):
    ck = qkv_exact_checkpoint(*layout)
    cfg = model_mod.LLaDAConfigLite(**ck.cfg)
    assert (cfg.n_heads, model_mod.effective_n_kv_heads(cfg)) == layout
    assert cfg.d_model == 128 * layout[0]
    if layout == (4, 1):
        assert cfg.n_kv_heads is None and cfg.multi_query_attention is True


@pytest.mark.parametrize("layout", QKV_LAYOUTS)
def test_builder_projections_are_exact_in_the_oracles_bf16_linear(layout):
    ck = qkv_exact_checkpoint(*layout)
    d = ck.base["d_model"]
    _, xn = _xn(ck, 2, 333)
    assert xn.unique().numel() > 1000                                        # xn covers many bf16 values
    for name, heads in (("q", layout[0]), ("k", layout[1]), ("v", layout[1])):
        w = ck.sd[f"model.transformer.blocks.0.{name}_proj.weight"]
        assert w.shape == (128 * heads, d) and bool(((w != 0).sum(1) == 1).all())
        assert set(w[w != 0].float().tolist()) <= set(QKV_SCALES)
        col, _ = ck.maps[name]
        assert col.unique().numel() == col.numel()                           # no two rows pull the same column
        lin = F.linear(xn, w).view(2, 333, heads, 128).transpose(1, 2)
        assert same_values(lin, qkv_pre(ck, xn, name))
        # and in fp64: the bf16 result IS the product, no rounding took place
        assert torch.equal(lin.double(), (xn.double() @ w.double().t()).view(2, 333, heads, 128).transpose(1, 2))


@pytest.mark.parametrize("layout", QKV_LAYOUTS)
def test_builder_expectation_equals_q_k_v_inside_block_forward(layout, monkeypatch):
    ck = qkv_exact_checkpoint(*layout)
    H, Hkv = layout
    B, T = 2, 333
    x, xn = _xn(ck, B, T)
    seen = {}
    sdpa = F.scaled_dot_product_attention

    def spy(q, k, v, **kw):
        seen.update(q=q, k=k, v=v)
        return sdpa(q, k, v, **kw)

    monkeypatch.setattr(lo.F, "scaled_dot_product_attention", spy)
    sin, cos = lo.rope_tables(T, 128, ck.base["rope_theta"])
    lo.block_forward(x, lo.layer_weights(ck.sd, 0), H, Hkv, ck.base["rms_norm_eps"], sin, cos)
    pos = torch.arange(T).repeat(B, 1)
    q, k, v, _, _ = qkv_expected(ck, xn, pos, pos)
    rep = H // Hkv
    assert same_values(seen["q"], q)
    assert same_values(seen["k"], k.repeat_interleave(rep, dim=1)) and same_values(seen["v"], v.repeat_interleave(rep, dim=1))


def test_a_neighbouring_position_or_head_fails_the_conditions():
    """The conditions of tests/test_gpu_qkv.py are sharp: an expectation built one position, one head, one rotary partner or one
    sign off fails them against the true one (position 0 rotates by nothing and is left out of the shifted comparison)."""
    ck = qkv_exact_checkpoint(4, 2)
    B, T = 2, 333
    _, xn = _xn(ck, B, T)
    pos = torch.arange(T).repeat(B, 1)
    q, k, v, tq, tk = qkv_expected(ck, xn, pos, pos)
    assert qkv_rope_verdict(q, q, tq) == (True, 0.0, 0)
    q1, k1 = qkv_expected(ck, xn, pos + 1, pos + 1)[:2]
    for good, bad, pre in ((q, q1, tq), (k, k1, tk), (q, q.roll(1, dims=1), tq), (k, k.roll(1, dims=1), tk), (q, q.roll(64, dims=-1), tq),
                           (q, -q, tq)):
        within, share, _ = qkv_rope_verdict(bad, good, pre)
        # (a step of one position moves the slow half of the rotary pairs by less than a bf16 ulp: about half of the elements)
        assert not within and share > 0.25, share
    assert not same_values(v, v.roll(1, dims=1)) and not same_values(v, v.roll(1, dims=2))
    # a single wrong element is enough for V, and a single element two ulps off is enough for q
    v2 = v.clone()
    v2[1, 1, 200, 5] += 1.0
    assert not same_values(v, v2)
    q2 = q.clone()
    q2[1, 3, 300, 100] *= 1.0 + 2.0 ** -6
    assert not qkv_rope_verdict(q2, q, tq)[0]
    # the fp32 floor only matters where the rotation cancels: it stays below a bf16 ulp of the result on all but a few elements
    floor = 2.0 ** -22 * (tq.float().abs() + tq.float().abs().roll(64, dims=-1))
    assert float((floor > 2.0 ** -8 * q.float().abs()).float().mean()) < 1e-3
