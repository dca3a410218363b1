"""The attention kernel (csrc/attention.hip) held to exact answers and to a derived per-element bound, against the caller's own
q, k, v — not against another run of the same kernel.  tests/test_attention_host.py checks the builders and the verdicts on
the CPU: each accepts an fp32 emulation of the kernel's arithmetic and rejects the mutation it exists for.

A. Routing, bit for bit.  helpers.att_onehot_inputs makes the soft-max exactly one-hot (the matching key leads by 179 or more in
   the log2 domain), so out[b, i, h] must be the bits of v[b, h's kv head, pi(i)]: a wrong key order inside vT, tile offset, ring
   stage, swizzle, head map, batch offset, grid map or store permutation returns another row's bits.
B. Every key once, pad keys never.  q = 0 and integer v: out = bf16(sum_j v[j] / L) up to the rounding of the reciprocal
   (helpers.att_counting_verdict); a counted pad key divides by L + 1, a missed or doubled key changes the sum.
C. General weights.  |got - ref| <= u A + u |ref| + 2 E (A + |ref|) per element against the fp64 soft-max attention of the bf16
   inputs, ref = P V, A = P |V|, u = 2^-8, E the row's worst-case fp32 score error (derived at helpers.att_general_verdict), on
   five kinds of input (helpers.att_general_inputs).
D. The forward's own calls through the parity taps: plain (pad query rows computed and finite) and a dLLM-cache step (13 compact
   queries per sequence against the slot's 200 keys), under condition C.

mmada_sdpa runs with its workspace filled with the bf16 NaN pattern, an output prefilled with NaN and 16 sentinel rows behind
it: nothing of the fill may reach the output, every row must be written, nothing behind the last row.

Measured on an MI355X: A and B hold on every shape, permutation and form.  The largest |got - ref| / bound of condition C over
the shapes from L = 63 on (parity report, section attention_err_over_bound; with a single key the output is v itself, 0):
normal 0.25 ... 0.47, peaked 0.54 ... 0.79, spike 0.41 ... 0.44, negative 0.47 ... 0.62, ascending 0.31 ... 0.68 — the figures of
the CPU emulation to three digits where both ran (ascending at (2, 2, 2, 65): 0.681 and 0.6808); through the taps 0.21 ... 0.35
for the plain forward and 0.22 ... 0.26 for the cache step (q and k of a random checkpoint are small there: E below 2e-5).  No
defect of the kernel was found."""
import ctypes as C

import pytest
import torch

from helpers import (ATT_E_CAP, ATT_GAP, ATT_KINDS, ATT_PLAN_GROUPS, ATT_SHAPES, QKV_MAX_SEQ, QKV_VOCAB, att_counting_exact,
                     att_counting_inputs, att_counting_verdict, att_general_inputs, att_general_verdict, att_groups_per_workgroup,
                     att_onehot_expected, att_onehot_gap, att_onehot_inputs, att_reference, save_parity, vt_unpermute)
from mmada_parallel_amd import abi, synth
from test_gpu_qkv import CACHE_L, _cache_inputs, _ids, _slot_kv, _tap, _view

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC0
SENTINEL_BITS = 0x5A3C        # a finite bf16 pattern (1.3e16)
WS_BYTES = 64 << 20           # the largest shape needs 38 MiB
FORWARD_LAYOUTS = [(2, 2), (4, 1)]

_RATIOS, _MODELS = {}, {}


@pytest.fixture(scope="module")
def sdpa():
    """sdpa(q, k, v) -> out [B, L, H * 128] of mmada_sdpa on a handle of its own (as tests/test_gpu_kernels.py builds one), under
    the NaN-filled workspace and the guarded output described above."""
    lib = abi.lib()
    c = abi.MmadaCfg(d_model=256, n_layers=1, n_heads=2, n_kv_heads=2, head_dim=128, mlp_hidden=512, vocab=134656, max_seq=1024,
                     rms_eps=1e-5, rope_theta=500000.0, tp_rank=0, tp_size=1, mask_token_id=synth.MASK,
                     text_vocab_size=synth.TEXT_VOCAB, codebook_size=synth.CODEBOOK, reserved=0)
    h = C.c_void_p()
    abi.check(lib.mmada_create(C.byref(c), None, C.byref(h)), "create")
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) // 256 * 256
    abi.check(lib.mmada_set_workspace(h, base, ws.numel() - 256), "set_workspace")

    def run(q, k, v):
        B, H, L, _ = q.shape
        Hkv = k.shape[1]
        qd, kd, vd = (t.to(DEV).contiguous() for t in (q, k, v))
        ws.view(torch.int16).fill_(NAN_BITS)
        out = torch.empty(B * L + 16, H * 128, dtype=torch.bfloat16, device=DEV)
        out[:B * L].view(torch.int16).fill_(NAN_BITS)
        out[B * L:].view(torch.int16).fill_(SENTINEL_BITS)
        abi.check(lib.mmada_sdpa(h, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), B, H, Hkv, L, abi.stream_ptr()), "sdpa")
        torch.cuda.synchronize()
        assert bool((out[B * L:].view(torch.int16) == SENTINEL_BITS).all()), "the kernel wrote behind the last query row"
        return out[:B * L].view(B, L, H * 128)

    yield run
    lib.mmada_destroy(h)
    del ws


def _both_forms(fn):
    lib = abi.lib()
    try:
        for form in (0, 1):
            abi.check(lib.mmada_set_option(b"attention_form", form), "set_option")
            fn(form)
    finally:
        lib.mmada_set_option(b"attention_form", -1)


def test_shapes_reach_their_launch_plans():
    """A later change to the planner must not move these tests off the three-group and late-wave paths silently."""
    for (B, H, Hkv, L), want in ATT_PLAN_GROUPS.items():
        lo, hi = att_groups_per_workgroup(abi.lib(), B, H, L)
        assert want[0] <= lo <= hi <= want[1], (B, H, Hkv, L, lo, hi)


# ------------------------------------------------------------------------------------------------------------ A: routing
@pytest.mark.parametrize("B,H,Hkv,L", ATT_SHAPES)
def test_one_hot_softmax_returns_the_bits_of_the_matching_v_row(sdpa, B, H, Hkv, L):
    for perm in ("random", "identity", "reversal"):
        q, k, v, pi = att_onehot_inputs(B, H, Hkv, L, perm)
        qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
        assert att_onehot_gap(qd, kd, pi) >= ATT_GAP
        want = att_onehot_expected(vd, pi)

        def check(form):
            got = sdpa(qd, kd, vd)
            wrong = int((got.view(torch.int16) != want.view(torch.int16)).sum())
            assert wrong == 0, f"{perm} permutation, form {form}: {wrong} of {got.numel()} elements are not the bits of v[pi(i)]"

        _both_forms(check)


# ----------------------------------------------------------------------------------------------------------- B: counting
@pytest.mark.parametrize("B,H,Hkv,L", [s for s in ATT_SHAPES if s[3] % 64 != 0 or s[3] == 64])
def test_every_key_counts_once_and_pad_keys_not_at_all(sdpa, B, H, Hkv, L):
    q, k, v = att_counting_inputs(B, H, Hkv, L)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)

    def check(form):
        got = sdpa(qd, kd, vd)
        bad = att_counting_verdict(got, vd, H)
        assert bad == 0, (f"form {form}: {bad} elements are not bf16(sum_j v[j] / {L}); the last row's first eight: "
                          f"{got[-1, -1, :8].tolist()} for {att_counting_exact(vd, H)[-1, 0, :8].tolist()}")

    _both_forms(check)


# ------------------------------------------------------------------------------------------------------ C: derived bound
def _record(name, ratio, section="sdpa"):
    _RATIOS.setdefault(section, {})[name] = round(ratio, 4)
    save_parity("attention_err_over_bound", _RATIOS)


@pytest.mark.parametrize("kind", ATT_KINDS)
@pytest.mark.parametrize("B,H,Hkv,L", ATT_SHAPES)
def test_general_weights_stay_inside_the_derived_bound(sdpa, B, H, Hkv, L, kind):
    q, k, v = att_general_inputs(kind, B, H, Hkv, L, device=DEV)
    ref, A, E = att_reference(q, k, v)
    assert float(E.max()) <= ATT_E_CAP
    ratio = att_general_verdict(sdpa(q, k, v), ref, A, E)
    print(f"{kind} {(B, H, Hkv, L)}: largest |got - ref| / bound = {ratio:.4f}")
    _record(f"{kind} {(B, H, Hkv, L)}", ratio)
    assert ratio <= 1.0


# --------------------------------------------------------------------------------------------- D: the forward's own calls
def _model(layout):
    """A one-layer model on an ordinary seeded random checkpoint; (4, 1) spelled multi_query_attention=True, as a config would."""
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    if layout not in _MODELS:
        H, Hkv = layout
        base = dict(d_model=128 * H, n_heads=H, n_kv_heads=Hkv, n_layers=1, mlp_hidden_size=512, vocab_size=QKV_VOCAB,
                    embedding_size=QKV_VOCAB, rms_norm_eps=1e-5, rope_theta=500000.0, max_sequence_length=QKV_MAX_SEQ)
        cfg = synth.full_config(base)
        if layout == (4, 1):
            cfg.update(n_kv_heads=None, multi_query_attention=True)
        _MODELS[layout] = LLaDAForMultiModalGeneration.from_state_dict(cfg, synth.synthetic_state_dict(base, seed=0), device=DEV)
        assert _MODELS[layout].n_kv_heads == Hkv
    return _MODELS[layout]


def _attn_partial(model, ids_d):
    model._ensure_ws(*ids_d.shape)
    model._shape = tuple(ids_d.shape)
    st = abi.stream_ptr()
    abi.check(model._lib.mmada_embed(model._handle, ids_d.data_ptr(), ids_d.shape[0], ids_d.shape[1], st), "embed")
    abi.check(model._lib.mmada_attn_partial(model._handle, 0, st), "attn")
    torch.cuda.synchronize()


def _check_forward(name, got, q, k, v):
    ref, A, E = att_reference(q, k, v)
    ratio = att_general_verdict(got, ref, A, E)
    print(f"{name}: largest |got - ref| / bound = {ratio:.4f} (E <= {float(E.max()):.2e})")
    _record(name, ratio, "forward")
    assert ratio <= 1.0


@pytest.mark.parametrize("B,L", [(2, 333), (1, 70)])
@pytest.mark.parametrize("layout", FORWARD_LAYOUTS)
def test_plain_forward_attention_against_its_tapped_q_k_v(layout, B, L):
    model = _model(layout)
    H, Hkv = layout
    ids_d = _ids(B, L, 13 * B + L).to(DEV)
    _attn_partial(model, ids_d)                         # leaves this shape's addresses in the taps
    addr, Lp, Lkv = _tap(model, 4)
    ws = model._lanes[0].ws
    att = _view(ws, addr, (B, Lp, H * 128))
    att.view(torch.int16).fill_(NAN_BITS)
    _attn_partial(model, ids_d)
    q = _view(ws, _tap(model, 1)[0], (B, H, Lkv, 128))[:, :, :L]
    k = _view(ws, _tap(model, 2)[0], (B, Hkv, Lkv, 128))[:, :, :L]
    v = vt_unpermute(_view(ws, _tap(model, 3)[0], (B, Hkv, 128, Lkv)))[..., :L].transpose(2, 3)
    assert bool(torch.isfinite(att.float()).all()), "a row of att (pad rows L..Lp included) is not finite"
    _check_forward(f"plain {layout} B={B} L={L}", att[:, :L], q, k, v)


@pytest.mark.parametrize("layout", FORWARD_LAYOUTS)
def test_cache_step_attention_against_the_slots_keys(layout):
    """The compute-mask step of tests/test_gpu_qkv.py (13 positions of 200 per sequence, B = 2, caching on): the only call that
    reaches launch_attention with a q allocation of its own and the key count from the slot."""
    model = _model(layout)
    H, Hkv = layout
    B, L = 2, CACHE_L
    ids0, ids1, pos, mask = _cache_inputs(B)
    Tc = pos.shape[1]
    Tp, Tq = (Tc + 7) // 8 * 8, (Tc + 63) // 64 * 64
    ws_of = lambda: model._lanes[0].ws
    try:
        model.caching(True)
        _attn_partial(model, ids0.to(DEV))               # a plain forward of the same (B, L): its addresses are the step's
        q_addr, att_addr = _tap(model, 1)[0], _tap(model, 4)[0]
        model.forward_cached(ids0.to(DEV), cat="att")
        _view(ws_of(), att_addr, (B, Tp, H * 128)).view(torch.int16).fill_(NAN_BITS)
        model.forward_cached(ids1.to(DEV), to_compute_mask=mask, cat="att")
        K, vT = _slot_kv(model, "att")
        q = _view(ws_of(), q_addr, (B, H, Tq, 128))[:, :, :Tc]
        att = _view(ws_of(), att_addr, (B, Tp, H * 128))
        _check_forward(f"cache step {layout}", att[:, :Tc], q, K[:, :, :L], vT[..., :L].transpose(2, 3))
    finally:
        model.caching(False)
