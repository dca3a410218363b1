"""Host side of the attention tests (tests/test_gpu_attention.py): the input builders and the three verdicts of helpers.py are
checked on the CPU, so that a GPU failure points at the kernel.  Each verdict must accept an fp32 emulation of the kernel's
arithmetic (csrc/attention.hip: 64-key tiles, fp32 scores, a running maximum that a 16-row group raises only when one of its
rows exceeds it by more than 2^4, P rounded to bf16 before P·V, one bf16 rounding of the result) and must reject the mutation it
exists for, applied to that emulation.  A pad key counted in l is rejected twice: by verdict B under the q = 0 inputs, and by
verdict C under the negative-score inputs (B's exact expectation needs uniform weights, so there the bound is the judge)."""
import pytest
import torch

from helpers import (ATT_E_CAP, ATT_GAP, ATT_KINDS, ATT_PLAN_GROUPS, ATT_SHAPES, att_counting_inputs, att_counting_verdict,
                     att_general_inputs, att_general_verdict, att_groups_per_workgroup, att_onehot_expected, att_onehot_gap,
                     att_onehot_inputs, att_reference, bf16_nearest, bits)

SMALL = [(2, 2, 2, 65), (1, 4, 2, 129), (3, 2, 1, 333)]
SCALE_LOG2E = torch.tensor(0.08838834764831845 * 1.4426950408889634, dtype=torch.float32)
DEFER_LOG2 = 4.0


def emulate(q, k, v):
    """attn16_wave in fp32 on the CPU: q [B, H, L, 128], k, v [B, Hkv, Lk, 128] -> [B, L, H * 128] bf16.  Lk may differ from L (the
    mutations add or drop a key)."""
    B, H, L, _ = q.shape
    rep, Lk = H // k.shape[1], k.shape[2]
    G = (L + 15) // 16
    out = torch.empty(B, H, L, 128, dtype=torch.bfloat16)
    for b in range(B):
        for h in range(H):
            qf = q[b, h].float()
            qf = torch.cat([qf, qf[-1:].expand(G * 16 - L, 128)]).view(G, 16, 128)      # the kernel clamps the row index
            kf, vf = k[b, h // rep].float(), v[b, h // rep].float()
            m = torch.full((G, 16), -1e30)
            l, o = torch.zeros(G, 16), torch.zeros(G, 16, 128)
            for t0 in range(0, Lk, 64):
                s = qf @ kf[t0:t0 + 64].t()
                mx = s.amax(-1) * SCALE_LOG2E
                raised = ((mx - m) > DEFER_LOG2).any(-1, keepdim=True)                  # the group's vote
                m_new = torch.where(raised, torch.maximum(m, mx), m)
                alpha = torch.exp2(m - m_new)
                p = torch.exp2(s * SCALE_LOG2E - m_new[..., None])
                l = l * alpha + p.sum(-1)
                o = o * alpha[..., None] + p.to(torch.bfloat16).float() @ vf[t0:t0 + 64]
                m = m_new
            out[b, h] = (o / l[..., None]).view(G * 16, 128)[:L].to(torch.bfloat16)
    return out.transpose(1, 2).reshape(B, L, H * 128)


def test_bf16_nearest_is_torchs_rounding():
    x = torch.cat([torch.randn(4096, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 37.0,
                   torch.tensor([0.0, 1.0, 1.00390625, 1.01171875, -255.5, 3.0e-3])])      # two ties among them
    assert torch.equal(bf16_nearest(x), x.float().to(torch.bfloat16).double())


def test_shapes_reach_their_launch_plans():
    from mmada_parallel_amd import abi

    for (B, H, Hkv, L), want in ATT_PLAN_GROUPS.items():
        lo, hi = att_groups_per_workgroup(abi.lib(), B, H, L)
        assert want[0] <= lo <= hi <= want[1], (B, H, Hkv, L, lo, hi)


@pytest.mark.parametrize("B,H,Hkv,L", ATT_SHAPES)
def test_onehot_construction_reaches_its_gap_and_selects_v(B, H, Hkv, L):
    q, k, v, pi = att_onehot_inputs(B, H, Hkv, L)
    assert att_onehot_gap(q, k, pi) >= max(ATT_GAP, 150.0)
    for t in (q, k, v):
        assert bool(torch.isfinite(t.float()).all())
    assert bool((v.float() != 0).all())
    want = att_onehot_expected(v, pi)
    if B * H * L * L > 1 << 24:        # the fp64 reference of the first and the last (batch, head) pair only: a second per case
        rep, sel = H // Hkv, [(0, 0), (B - 1, H - 1)]
        q = torch.stack([q[b, h] for b, h in sel])[:, None]
        k, v = (torch.stack([t[b, h // rep] for b, h in sel])[:, None] for t in (k, v))
        want = torch.stack([want[b, :, h * 128:(h + 1) * 128] for b, h in sel])
    ref = att_reference(q, k, v)[0]
    assert torch.equal(bits(ref.float().to(torch.bfloat16)), bits(want))


@pytest.mark.parametrize("perm", ["random", "identity", "reversal"])
@pytest.mark.parametrize("B,H,Hkv,L", SMALL)
def test_verdict_a_accepts_the_emulation_and_rejects_the_neighbouring_batch(B, H, Hkv, L, perm):
    q, k, v, pi = att_onehot_inputs(B, H, Hkv, L, perm)
    want = att_onehot_expected(v, pi)
    got = emulate(q, k, v)
    assert torch.equal(bits(got), bits(want))
    if B > 1:
        assert not torch.equal(bits(got.roll(1, dims=0)), bits(want))
    # the K of another (batch, kv head) does not select: its sign vector differs
    if Hkv > 1:
        assert not torch.equal(bits(emulate(q, k.roll(1, dims=1), v)), bits(want))


def _one_pad_key(k, v):
    """One zero key with a zero V row behind the last: what the kernel would see if its -inf selection let key L through."""
    z = torch.zeros_like(k[:, :, :1])
    return torch.cat([k, z], dim=2), torch.cat([v, z], dim=2)


@pytest.mark.parametrize("B,H,Hkv,L", [(1, 2, 1, 64)] + SMALL)
def test_verdict_b_accepts_the_emulation_and_rejects_a_counted_pad_key(B, H, Hkv, L):
    q, k, v = att_counting_inputs(B, H, Hkv, L)
    assert att_counting_verdict(emulate(q, k, v), v, H) == 0
    assert att_counting_verdict(emulate(q, *_one_pad_key(k, v)), v, H) > 0
    assert att_counting_verdict(emulate(q, k[:, :, :-1], v[:, :, :-1]), v, H) > 0                     # a missed key
    twice = torch.cat([v, v[:, :, :1]], dim=2)
    assert att_counting_verdict(emulate(q, torch.cat([k, k[:, :, :1]], dim=2), twice), v, H) > 0      # a doubled key


@pytest.mark.parametrize("kind", ATT_KINDS)
@pytest.mark.parametrize("B,H,Hkv,L", SMALL)
def test_verdict_c_accepts_the_emulation_and_rejects_its_mutations(B, H, Hkv, L, kind):
    q, k, v = att_general_inputs(kind, B, H, Hkv, L)
    ref, A, E = att_reference(q, k, v)
    assert float(E.max()) <= ATT_E_CAP
    ratio = att_general_verdict(emulate(q, k, v), ref, A, E)
    print(f"{kind} {(B, H, Hkv, L)}: emulation err / bound {ratio:.3f}")
    assert ratio <= 1.0
    # two V rows swapped inside the last 32-key block (where every kind has weight)
    j0, j1 = L - 2, L - 6
    assert j0 // 32 == j1 // 32
    vs = v.clone()
    vs[:, :, [j0, j1]] = v[:, :, [j1, j0]]
    assert att_general_verdict(emulate(q, k, vs), ref, A, E) > 1.0
    assert att_general_verdict(emulate(q, k[:, :, :-1], v[:, :, :-1]), ref, A, E) > 1.0               # the last key dropped
    if Hkv > 1:                                                  # kv head 0's K under the query heads of kv head 1
        kw = k.clone()
        kw[:, 1] = k[:, 0]
        assert att_general_verdict(emulate(q, kw, v), ref, A, E) > 1.0
    if kind == "negative":                                       # a zero pad key (score 0 against -45) owns every row
        assert att_general_verdict(emulate(q, *_one_pad_key(k, v)), ref, A, E) > 1.0
    assert att_general_verdict(torch.full_like(ref, float("nan")), ref, A, E) == float("inf")


@pytest.mark.parametrize("kind", ATT_KINDS)
@pytest.mark.parametrize("B,H,Hkv,L", ATT_SHAPES[-2:])
def test_general_inputs_keep_the_score_error_under_its_cap_at_the_largest_shapes(B, H, Hkv, L, kind):
    q, k, _ = att_general_inputs(kind, B, H, Hkv, L)
    worst = 0.0
    for b in range(B):
        dots = q[b].float().abs() @ k[b].float().abs().repeat_interleave(H // Hkv, dim=0).transpose(1, 2)
        worst = max(worst, float(dots.max()))
    assert 2.0 ** -17 * worst / 128 ** 0.5 <= ATT_E_CAP, worst
