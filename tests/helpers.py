"""Shared test helpers (seeded inputs identical to oracle/gen_golden.py)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mmada_parallel_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
STUB_TEXT_VOCAB, STUB_CB = 2048, 512
SAMPLER_CASES = {
    "img4": dict(text_steps=8, timesteps=4, cfg_scale=0.0, cfg_img=4.0),
    "both": dict(text_steps=12, timesteps=6, cfg_scale=2.5, cfg_img=4.0),
    "odd": dict(text_steps=7, timesteps=5, cfg_scale=2.3, cfg_img=0.0),
    "nocfg": dict(text_steps=8, timesteps=8, cfg_scale=0.0, cfg_img=0.0),
}


def tiny_job():
    return synth.synthetic_job(height=64, width=64, text_gen_length=16, prompt_len=8, uncond_prompt_len=4,
                               in_height=64, in_width=64, seed=1)


def stub_logits(seed, call_idx, B, L, V):
    g = torch.Generator().manual_seed(seed * 100003 + call_idx)
    return (torch.randn(B, L, V, generator=g) * 2.0).to(torch.bfloat16)


def from_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.bfloat16)


def bits(t):
    return t.detach().to("cpu", torch.bfloat16).contiguous().view(torch.int16)


def golden_float(name, prefer=None):
    """Float-GEMM fixtures are recorded once per host ISA class (oracle/gen_golden.py): returns (npz, same_class) where
    same_class says that the file was recorded on a CPU of THIS host's class, i.e. bit-equality with a CPU recomputation
    may be demanded.  `prefer` picks a particular recording (the GPU tests' thresholds are calibrated on one)."""
    isa = synth.host_isa()
    for cand in ([prefer] if prefer else []) + [isa, "amx_bf16", "avx512", "avx512_bf16"]:
        path = os.path.join(GOLDEN, f"{name}.{cand}.npz")
        if os.path.exists(path):
            return np.load(path), cand == isa
    raise FileNotFoundError(f"no recording of {name} under {GOLDEN}")


_SD = {}


def tiny_sd():
    if "tiny" not in _SD:
        _SD["tiny"] = synth.synthetic_state_dict(synth.CFG_TINY, seed=0)
    return _SD["tiny"]

M_CASES = {
    "m_both": dict(text_cfg=1.5, image_cfg=3.5, text_steps=8, image_steps=4, image_temperature=1.0, text_temperature=0.0),
    "m_img": dict(text_cfg=0.0, image_cfg=2.0, text_steps=7, image_steps=7, image_temperature=0.5, text_temperature=0.0),
    "m_noisy": dict(text_cfg=0.7, image_cfg=3.5, text_steps=6, image_steps=3, image_temperature=1.0, text_temperature=0.8),
}
M_SHAPE = dict(prompt=6, N=16, T=16, text_vocab=2048, CB=512, soi=2040, eoi=2041, bos=2042, mask_id=126336)

STEPWISE_CASES = {"sw_img4": dict(text_steps=10, cfg_scale=0.0, cfg_img=4.0), "sw_both": dict(text_steps=14, cfg_scale=2.5, cfg_img=4.0)}


# generate_image (A, text-to-image) stub-logit cases: tests/golden/t2i_traj.npz
T2I_CASES = {
    "g_nocfg_t0": dict(timesteps=6, temperature=0.0, cfg_scale=0.0),
    "g_cfg_t0": dict(timesteps=5, temperature=0.0, cfg_scale=3.0),
    "g_cfg_t1": dict(timesteps=4, temperature=1.0, cfg_scale=2.0),
}


def t2i_job(seed=3, P=8, U=4, side=4):
    """prompt = [P text tokens][2 tokens][side rows of (side masks + newline)][2 tokens]; code_start = P + 2."""
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(0, 1000, (P,), generator=g).tolist()
    body = []
    for _ in range(side):
        body += [synth.MASK] * side + [synth.NEW_LINE]
    prompt = torch.tensor([text + [synth.BOA, synth.BOI] + body + [synth.EOI, synth.EOA]], dtype=torch.long)
    uncon = torch.randint(0, 1000, (1, U), generator=g)
    return dict(prompt=prompt, uncon_ids=uncon, code_start=P + 2, seq_len=side * side, newline_every=side)


class ReplayRng:
    """Replays the reference's torch.rand(shape, dtype=bf16, generator=cpu_generator) draws on the CPU generator."""

    def rand(self, shape, dtype, device, generator):
        return torch.rand(tuple(shape), dtype=dtype, generator=generator).to(device)


# mmu_generate (M text sampler) stub-logit cases: tests/golden/mmu_traj.npz
MMU_CASES = {
    "mmu_plain": dict(max_new_tokens=16, steps=8, block_length=8, temperature=0.0, cfg_scale=0.0),
    "mmu_cfg": dict(max_new_tokens=12, steps=6, block_length=4, temperature=0.0, cfg_scale=1.5),
    "mmu_noisy": dict(max_new_tokens=8, steps=4, block_length=8, temperature=0.6, cfg_scale=0.0),
}
MMU_SHAPE = dict(B=2, P=7, V=2560, mask_id=126336)


# t2i_generate (M text-to-image sampler) stub-logit cases: tests/golden/m_t2i_traj.npz
M_T2I_CASES = {
    "t2i_cfg": dict(B=2, temperature=1.0, timesteps=5, guidance_scale=2.0, uncond=True, known=0),
    "t2i_plain": dict(B=1, temperature=0.7, timesteps=4, guidance_scale=0.0, uncond=False, known=3),
}
M_T2I_SHAPE = dict(P=9, N=16, resolution=6, text_vocab=2048, CB=512, mask_id=126336)


def m_t2i_job(seed, B, known):
    """[P prompt tokens][soi][N image slots][eoi]; `known` leading image slots already hold codebook tokens."""
    sh = M_T2I_SHAPE
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(0, 2000, (B, sh["P"]), generator=g)
    unc = torch.randint(0, 2000, (B, sh["P"]), generator=g)
    img = torch.full((B, sh["N"]), sh["mask_id"], dtype=torch.long)
    if known:
        img[:, :known] = torch.randint(0, sh["CB"], (B, known), generator=g) + sh["text_vocab"]
    tail = torch.cat([torch.full((B, 1), 2040), img, torch.full((B, 1), 2041)], dim=1)
    return torch.cat([prompt, tail], dim=1), torch.cat([unc, tail], dim=1)


# generate_ti2ti at temperature > 0 (README default: temperature=1.0, text_temperature=0.7): tests/golden/sampler_noisy.npz
NOISY_CASES = {
    "noisy_img": dict(text_steps=8, timesteps=4, temperature=1.0, text_temperature=0.0, cfg_scale=0.0, cfg_img=4.0),
    "noisy_both": dict(text_steps=6, timesteps=6, temperature=1.0, text_temperature=0.7, cfg_scale=2.0, cfg_img=3.0),
}


class ReplayCpuRng:
    """Draws exactly what the reference draws when it runs on CPU with a seeded CPU generator (torch.rand / randn in the
    tensor's dtype, torch.multinomial), then moves the result to the device the HIP path works on."""

    def rand(self, shape, dtype, device, generator):
        return torch.rand(tuple(shape), dtype=dtype, generator=generator).to(device)

    def randn(self, shape, dtype, device, generator):
        return torch.randn(tuple(shape), dtype=dtype, generator=generator).to(device)

    def multinomial(self, probs2d, generator):
        return torch.multinomial(probs2d.cpu(), 1, generator=generator).to(probs2d.device)


# ---- measured parity numbers (tests/test_gpu_parity_depth.py, test_gpu_fullsize.py) -> gpurun_out/r06_parity.json (copied to profiles/ after a full suite run) ----
PARITY_REPORT = os.path.join(ROOT, "gpurun_out", "r06_parity.json")


def save_parity(section, payload):
    import json

    os.makedirs(os.path.dirname(PARITY_REPORT), exist_ok=True)
    data = {}
    if os.path.exists(PARITY_REPORT):
        try:
            with open(PARITY_REPORT) as f:
                data = json.load(f)
        except Exception:
            data = {}
    data[section] = payload
    with open(PARITY_REPORT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def host_threads():
    """Oracle matmuls on the physical cores, not on every hyper-thread (oversubscription made round 1's CPU numbers 3x slow)."""
    n = os.cpu_count() or 8
    torch.set_num_threads(max(1, n if n <= 64 else n // 2))


# painting mode (the output image span starts partly known): tests/golden/paint_traj.npz
PAINT_CASES = {
    "inpaint_img4": ("inpainting", dict(text_steps=8, timesteps=4, cfg_scale=0.0, cfg_img=4.0)),
    "outpaint_both": ("outpainting", dict(text_steps=10, timesteps=5, cfg_scale=2.5, cfg_img=4.0)),
}
TINY_JOB_KW = dict(height=64, width=64, text_gen_length=16, prompt_len=8, uncond_prompt_len=4, in_height=64, in_width=64, seed=1)


def paint_job(kind):
    return synth.paint_job(kind, codebook_size=STUB_CB, text_vocab=STUB_TEXT_VOCAB, **TINY_JOB_KW)


# remasking='random' (text positions ranked by a uniform draw from the GLOBAL RNG): tests/golden/random_traj.npz
RANDOM_CASES = {
    "rand_img4": dict(text_steps=8, timesteps=4, cfg_scale=0.0, cfg_img=4.0, temperature=0.0, text_temperature=0.0),
    "rand_both": dict(text_steps=9, timesteps=3, cfg_scale=2.0, cfg_img=4.0, temperature=0.0, text_temperature=0.0),
}
RANDOM_SEED = 4321


# edge cases of generate_ti2ti (tests/golden/edge_traj.npz): name -> (job tweak, uncon_text given, uncon_image given, kwargs)
EDGE_CASES = {
    # CFG scales > 0 but no unconditional prompts: the reference substitutes ZERO logits for both branches (:275-278)
    "cfg_without_uncond": ("plain", False, False, dict(text_steps=6, timesteps=3, cfg_scale=1.5, cfg_img=4.0)),
    # only the image branch has an unconditional prompt: both forwards still run (:243), the text one on the plain ids
    "only_uncon_image": ("plain", False, True, dict(text_steps=6, timesteps=3, cfg_scale=2.0, cfg_img=3.0)),
    # the text span is already complete: no text step ever runs (:183), image steps still do
    "text_done": ("text_done", True, True, dict(text_steps=5, timesteps=5, cfg_scale=0.0, cfg_img=4.0)),
    # more image steps requested than steps exist: linspace repeats indices, `step in list` runs each once
    "more_timesteps_than_steps": ("plain", True, True, dict(text_steps=4, timesteps=9, cfg_scale=0.0, cfg_img=4.0)),
    # a single step: the image step coincides with the only text step, ratio = 1 -> one cell left masked
    "single_step": ("plain", True, True, dict(text_steps=1, timesteps=1, cfg_scale=0.0, cfg_img=4.0)),
}


def edge_job(name):
    tweak, ut, ui, kw = EDGE_CASES[name]
    job = tiny_job()
    if tweak == "text_done":
        g = torch.Generator().manual_seed(77)
        ids = job["input_ids"].clone()
        ids[0, job["text_start"]:job["text_end"]] = torch.randint(0, 1000, (job["text_end"] - job["text_start"],), generator=g)
        job["input_ids"] = ids
    if not ut:
        job["uncon_text"] = None
    if not ui:
        job["uncon_image"] = None
    return job, kw


class FakeVq:
    """CPU stand-in with the surface utils/image_utils.py touches: latents = 2x2 mean of the red channel, index = its
    value quantised to 0..63 (so token arithmetic and mask geometry can be checked without a GPU)."""

    def __init__(self):
        self.config = SimpleNamespace(block_out_channels=[1, 1], latent_channels=1)
        self.device = torch.device("cpu")

    def encode(self, x):
        return SimpleNamespace(latents=torch.nn.functional.avg_pool2d(x[:, :1], 2))

    def quantize(self, latents):
        return None, None, (None, None, (latents.reshape(-1) * 63).round().long())

    def decode(self, codes, force_not_quantize=False, shape=None):
        assert force_not_quantize and tuple(shape) == (codes.shape[0], codes.shape[1], codes.shape[2], 1)
        g = codes.float() / 63.0 * 1.2 - 0.1                               # leaves [0, 1] on both sides: the clip matters
        x = torch.stack([g, 1.0 - g, g * g], 1)
        return SimpleNamespace(sample=torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest"))


# utils/image_utils.py against the reference's own functions (tests/golden/image_utils_tokens.npz)
PAINT_UTIL_CASES = {
    "inpaint": dict(mask_h_ratio=0.5, mask_w_ratio=0.25, mask_mode="inpainting"),
    "outpaint": dict(mask_h_ratio=0.5, mask_w_ratio=0.25, mask_mode="outpainting"),
    "inpaint_dilated": dict(mask_h_ratio=0.4, mask_w_ratio=0.3, dilate_latent_k=1, mask_mode="inpainting"),
    "inpaint_nearest": dict(mask_h_ratio=0.37, mask_w_ratio=0.21, downsample_mode="nearest", mask_mode="inpainting"),
    "outpaint_bilinear": dict(mask_h_ratio=0.55, mask_w_ratio=0.45, downsample_mode="bilinear", gray_value=90, mask_mode="outpainting"),
}


def paint_util_image():
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, size=(36, 70, 3), dtype=np.uint8)       # resized to 36 x 70 -> multiples of 2: unchanged size


# ---- in-process tensor-parallel rank groups (tests/test_gpu_tp.py, tests/test_gpu_parity_depth.py) ----
_TP_STREAMS = []


def tp_group(cfg_base, sd, tp, max_rows, dev="cuda:0", transport="pull", exchange_cus=0):
    """The ranks of a tensor-parallel group as separate handles of ONE process, each on its own stream, connected with
    connect_local_group (tests/test_gpu_tp.py explains why this is the multi-device code path unchanged)."""
    from mmada_parallel_amd import LLaDAForMultiModalGeneration
    from mmada_parallel_amd.tp_link import connect_local_group

    cfg = synth.full_config(cfg_base)
    ranks = connect_local_group([LLaDAForMultiModalGeneration.from_state_dict(cfg, sd, device=dev, tp_rank=r, tp_size=tp)
                                 for r in range(tp)], max_rows, transport=transport, exchange_cus=exchange_cus)
    # One pool of compute streams for every group this process ever builds: a rank's wait kernel spins until its peers'
    # launches run, so no two live streams may share a hardware queue (GPU_MAX_HW_QUEUES, tests/conftest.py) — fresh
    # streams per group would walk through the queues and end up doubling up (seen as hand-off timeouts, status.error).
    while len(_TP_STREAMS) < tp:
        _TP_STREAMS.append(torch.cuda.Stream(device=dev))
    return ranks, _TP_STREAMS[:tp]


def tp_each(ranks, streams, fn):
    """fn(rank_model) enqueued for every rank on its own stream; NO host sync until all are enqueued."""
    out = []
    cur = torch.cuda.current_stream()
    for m, s in zip(ranks, streams):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            out.append(fn(m))
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    return out


# ---- block 0, stage by stage, against the oracle (tests/test_gpu_model.py, tests/test_gpu_qkv.py) ----
def relerr(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item(), \
           ((got - ref).abs().mean() / ref.abs().mean().clamp_min(1e-30)).item()


def check_block_stages(model, cfg, sd, ids):
    """Every intermediate of block 0 (RMSNorm, q/k after RoPE, V, SDPA output, residual adds, SiLU-gated hidden) of `model`
    against the oracle's value of the same tensor; errors are relative to each tensor's own magnitude, so a wrong branch
    cannot hide behind the (much larger) residual stream.  cfg: the checkpoint's base config (d_model, n_heads, rms_norm_eps,
    rope_theta); the number of kv heads is the model's (grouped heads are expanded as the reference does, :666-669)."""
    import torch.nn.functional as F
    from mmada_parallel_amd import abi
    from oracle import llada_oracle as lo

    dev = model.device
    B, L = ids.shape
    H, Hkv, hd, eps = cfg["n_heads"], model.n_kv_heads, 128, cfg["rms_norm_eps"]
    w = lo.layer_weights(sd, 0)
    x0 = F.embedding(ids, sd["model.transformer.wte.weight"])
    xn = lo.rms_norm(x0, w["attn_norm"], eps)
    q = F.linear(xn, w["q_proj"]).view(B, L, H, hd).transpose(1, 2)
    k = F.linear(xn, w["k_proj"]).view(B, L, Hkv, hd).transpose(1, 2)
    v = F.linear(xn, w["v_proj"]).view(B, L, Hkv, hd).transpose(1, 2)
    sin, cos = lo.rope_tables(L, hd, cfg["rope_theta"])
    q, k = lo.apply_rope(q, sin, cos), lo.apply_rope(k, sin, cos)
    ke, ve = (k, v) if Hkv == H else (k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1))
    att = F.scaled_dot_product_attention(q, ke, ve).transpose(1, 2).contiguous().view(B, L, H * hd)
    x1 = x0 + F.linear(att, w["attn_out"])
    n2 = lo.rms_norm(x1, w["ff_norm"], eps)
    hmid = F.silu(F.linear(n2, w["ff_proj"])) * F.linear(n2, w["up_proj"])
    x2 = x1 + F.linear(hmid, w["ff_out"])

    lib, h = model._lib, model._handle
    ids_d = ids.to(dev)
    model._ensure_ws(B, L)
    model._shape = (B, L)
    st = abi.stream_ptr()
    abi.check(lib.mmada_embed(h, ids_d.data_ptr(), B, L, st), "embed")
    e_x0 = relerr(model.hidden_state(), x0)
    abi.check(lib.mmada_attn_partial(h, 0, st), "attn")
    Lp = (L + 7) // 8 * 8
    got = {
        "xn": model.debug_buffer(0).view(B, Lp, -1)[:, :L],
        "q": model.debug_buffer(1)[:, :, :L],
        "k": model.debug_buffer(2)[:, :, :L],
        "v": model.debug_buffer(3)[:, :, :, :L].transpose(2, 3),
        "att": model.debug_buffer(4).view(B, Lp, -1)[:, :L],
        "x1": model.hidden_state(),
    }
    got = {k_: v_.clone() for k_, v_ in got.items()}
    abi.check(lib.mmada_mlp_partial(h, 0, st), "mlp")
    got["n2"] = model.debug_buffer(0).view(B, Lp, -1)[:, :L].clone()
    got["h"] = model.debug_buffer(5).view(B, Lp, -1)[:, :L].clone()
    got["x2"] = model.hidden_state()
    ref = {"xn": xn, "q": q, "k": k, "v": v, "att": att, "x1": x1, "n2": n2, "h": hmid, "x2": x2}
    report = {"x0": e_x0}
    for name in ref:
        report[name] = relerr(got[name], ref[name])
    print("stage errors (max/maxabs, mean/meanabs):", {k_: (f"{a:.2e}", f"{b:.2e}") for k_, (a, b) in report.items()})
    assert report["x0"][0] == 0.0
    # the branch deltas, not just the stream: attention and MLP contributions themselves
    report["d_attn"] = relerr(got["x1"].float().cpu() - x0.float(), x1.float() - x0.float())
    report["d_mlp"] = relerr(got["x2"].float().cpu() - got["x1"].float().cpu(), x2.float() - x1.float())
    print("branch deltas:", report["d_attn"], report["d_mlp"])
    for name, (emax, emean) in report.items():
        # bf16 storage everywhere: a few ulps (2^-8) of the tensor's magnitude; deltas are differences of bf16 values
        lim_max, lim_mean = (0.25, 0.05) if name.startswith("d_") else (2.0 ** -5, 2.0 ** -8)
        assert emax < lim_max and emean < lim_mean, f"{name}: {emax:.3e} {emean:.3e}"
    return report


# ---- the QKV epilogue, exactly (tests/test_gpu_qkv.py, tests/test_qkv_host.py) ----
# (n_heads, n_kv_heads): today's layout; grouped heads; multi_query_attention=True; a K head and the V head in ONE 256-column tile
# (the fused projection has 3 + 1 + 1 heads of 128 columns: K is columns 384..511, V 512..639)
QKV_LAYOUTS = [(2, 2), (4, 2), (4, 1), (3, 1)]
QKV_VOCAB, QKV_MAX_SEQ = 1024, 4096
QKV_SCALES = (0.5, 1.0, 2.0, -0.5, -1.0, -2.0)
QKV_DIFF_CAP = 1e-4          # share of q / k elements that may differ from the oracle at all (each by one bf16 ulp at most)
BF16_DENORMAL_STEP = 2.0 ** -133


def qkv_exact_checkpoint(n_heads, n_kv_heads, seed=0):
    """A one-layer checkpoint with d_model = 128 * n_heads whose q / k / v projections are EXACT: every row of q_proj, k_proj and
    v_proj has one non-zero entry, a power of two from QKV_SCALES, in a column drawn from a seeded random map (no two rows of a
    projection pull the same column), so each pre-activation is one product xn[col] * 2^e — the same bf16 value in the MFMA and
    in the oracle's bf16 F.linear.  Everything else is the usual seeded random checkpoint, except wte ~ N(0, 1).

    Returns a namespace: cfg (what the model class takes; (4, 1) is spelled multi_query_attention=True as a config would),
    base (the same with n_kv_heads explicit: what synth and the oracle take), sd, maps {'q' | 'k' | 'v': (column, scale)}."""
    d, kv = 128 * n_heads, 128 * n_kv_heads
    base = dict(d_model=d, n_heads=n_heads, n_kv_heads=n_kv_heads, n_layers=1, mlp_hidden_size=512, vocab_size=QKV_VOCAB,
                embedding_size=QKV_VOCAB, rms_norm_eps=1e-5, rope_theta=500000.0, max_sequence_length=QKV_MAX_SEQ)
    sd = synth.synthetic_state_dict(base, seed=seed)
    g = torch.Generator().manual_seed(7919 * seed + 16 * n_heads + n_kv_heads)
    p = "model.transformer."
    sd[p + "wte.weight"] = torch.randn(QKV_VOCAB, d, generator=g).to(torch.bfloat16)
    maps = {}
    for name, rows in (("q", d), ("k", kv), ("v", kv)):
        col = torch.randperm(d, generator=g)[:rows]
        scale = torch.tensor(QKV_SCALES)[torch.randint(0, len(QKV_SCALES), (rows,), generator=g)]
        w = torch.zeros(rows, d)
        w[torch.arange(rows), col] = scale
        sd[f"{p}blocks.0.{name}_proj.weight"] = w.to(torch.bfloat16)
        maps[name] = (col, scale)
    cfg = synth.full_config(base)
    if (n_heads, n_kv_heads) == (4, 1):
        cfg.update(n_kv_heads=None, multi_query_attention=True)
    return SimpleNamespace(cfg=cfg, base=base, sd=sd, maps=maps, n_heads=n_heads, n_kv_heads=n_kv_heads)


_ROPE = {}


def qkv_rope_rows(pos, theta=500000.0):
    """(sin, cos) [B, 1, T, 128] of the oracle's fp32 tables at the rotary positions pos [B, T]."""
    from oracle import llada_oracle as lo

    if theta not in _ROPE:
        _ROPE[theta] = lo.rope_tables(QKV_MAX_SEQ, 128, theta)
    sin, cos = _ROPE[theta]
    return sin[0, 0][pos][:, None], cos[0, 0][pos][:, None]


def qkv_pre(ck, xn, name):
    """The exact pre-activation of projection `name` ('q' | 'k' | 'v') for xn [B, T, d] bf16: [B, heads, T, 128] bf16."""
    col, scale = ck.maps[name]
    B, T, _ = xn.shape
    t = (xn.float()[:, :, col] * scale).to(torch.bfloat16)       # one product by a power of two: exact
    return t.view(B, T, col.numel() // 128, 128).transpose(1, 2).contiguous()


def qkv_expected(ck, xn, pos_q, pos_k):
    """What the QKV epilogue must write for the block input xn [B, T, d] (bf16, CPU): q rotated at pos_q [B, T], k rotated at
    pos_k [B, T] — oracle.llada_oracle.apply_rope, the reference's fp32 arithmetic — and V as it is.  Returns (q, k, v, tq, tk),
    [B, heads, T, 128] each; tq, tk are the un-rotated q and k (the operands of the rotation: qkv_rope_verdict's floor)."""
    from oracle import llada_oracle as lo

    theta = ck.base["rope_theta"]
    tq, tk = qkv_pre(ck, xn, "q"), qkv_pre(ck, xn, "k")
    q = lo.apply_rope(tq, *qkv_rope_rows(pos_q, theta))
    k = lo.apply_rope(tk, *qkv_rope_rows(pos_k, theta))
    return q, k, qkv_pre(ck, xn, "v"), tq, tk


def same_values(a, b):
    """Equal as VALUES (+0 == -0; a NaN equals nothing)."""
    return bool((a.float() == b.float()).all())


def qkv_rope_verdict(got, ref, pre):
    """The conditions on a rotated tensor against the oracle's `ref`; `pre` is the un-rotated tensor.  Returns (every element
    within one bf16 ulp of the oracle, the share of elements that differ at all, the number of elements that needed the floor).

    One ulp: |got - ref| <= 2^-7 |ref| + floor.  The floor is the reference's OWN fp32 error, which a bf16 ulp of the result does
    not cover where the rotation cancels: an output is fl(t1 * c) -+ fl(t2 * s) in fp32 (t1, t2: the element and its rotary
    partner, c, s: table entries), torch's fp32 sin / cos is within one fp32 ulp of the correctly rounded value
    rope_table_kernel stores, so each product may move by 2^-23 |t| for the table entry plus two roundings of 2^-24 |t|:
    floor = 2^-22 (|t1| + |t2|), plus one bf16 denormal step.  With |ref| below 2^-15 of the operands that exceeds a bf16 ulp of
    ref: measured, 1 element of 2 097 152 (q of layout (4, 2) at L = 4096: ref 2.98e-7, got 3.28e-7 from operands -0.586 and
    0.719, the cosine one fp32 ulp apart), reproduced on the CPU with the kernel's table convention.  Anywhere else the floor is
    2^-14 of a bf16 ulp."""
    g, r, t = got.float(), ref.float(), pre.float().abs()
    diff = (g - r).abs()
    rel = 2.0 ** -7 * r.abs() + BF16_DENORMAL_STEP
    floor = 2.0 ** -22 * (t + t.roll(64, dims=-1))
    within = bool((diff <= rel + floor).all())
    return within, float((diff > 0).float().mean()), int((diff > rel).sum())


def qkv_assert_rope(name, got, ref, pre, record=None):
    within, share, floored = qkv_rope_verdict(got, ref, pre)
    print(f"{name}: share of elements that differ from the oracle {share:.3e} (cap {QKV_DIFF_CAP:.0e}), all within one ulp: {within}"
          f" ({floored} of {got.numel()} under cancellation, by the fp32 floor)")
    if record is not None:
        record[name] = {"share_differing": share, "elements": got.numel(), "within_by_fp32_floor_only": floored}
    assert within, f"{name}: an element is more than one bf16 ulp from the oracle"
    assert share <= QKV_DIFF_CAP, f"{name}: {share:.3e} of the elements differ from the oracle"


def vt_key_pos(l):
    """csrc/common.h vt_key_pos restated: storage position of key l inside the K-major V buffer."""
    c = (l >> 2) & 7
    return (l & ~28) | ((c & 3) << 3) | ((c >> 2) << 2)


def vt_unpermute(t):
    """[..., Lkv] in vt_key_pos storage order -> key order."""
    idx = torch.tensor([vt_key_pos(l) for l in range(t.shape[-1])], device=t.device)
    return t[..., idx]


# ---- the attention kernel: exact routing and a derived per-element bound (tests/test_gpu_attention.py, tests/test_attention_host.py) ----
# (B, n_heads, n_kv_heads, L): the smallest shapes that reach each branch of csrc/attention.hip — one key, just under / exactly /
# just over one 64-key tile, 3 and 4 key tiles (the vT ring of three wraps), a pair-major grid with a ragged last group, the
# XCD grid with 6-7 groups per workgroup (late waves carry a group), 17-18 groups (3 early + 2 late per SIMD, a 1 + 3 split of
# the DMA pieces) and 23-24 groups (3 + 3)
ATT_SHAPES = [(1, 1, 1, 1), (1, 2, 2, 63), (1, 2, 1, 64), (2, 2, 2, 65), (1, 4, 2, 129), (1, 2, 2, 193), (3, 2, 1, 333), (8, 8, 2, 400),
              (2, 32, 8, 1100), (2, 32, 8, 1530)]
# the range the groups of 16 query rows per workgroup must stay in, under the launch plan, for the above to hold
ATT_PLAN_GROUPS = {(1, 1, 1, 1): (1, 1), (8, 8, 2, 400): (6, 7), (2, 32, 8, 1100): (17, 18), (2, 32, 8, 1530): (23, 24)}
ATT_KINDS = ("normal", "peaked", "spike", "negative", "ascending")
ATT_U = 2.0 ** -8            # the unit of the bound: one bf16 ulp, relative
ATT_E_CAP = 2.0 ** -11       # the inputs keep the fp32 score error below this (natural-log units)
ATT_GAP = 64.0               # least lead of the matching key's score, log2 domain, in the one-hot construction
ATT_CODE_SCALE = 8.0
ATT_LOG2_SCALE = 1.4426950408889634 / 128 ** 0.5    # a dot product -> the kernel's log2-domain score


def att_groups_per_workgroup(lib, B, H, L):
    """(smallest, largest) number of 16-row query groups a workgroup of attn16_kernel carries under the library's launch plan."""
    groups = (L + 15) // 16
    chunks = lib.mmada_attention_plan(B * H, groups, L)
    return groups // chunks, -(-groups // chunks)


def att_code(L):
    """[L, 128] code words of +-1: the bits of the key index (as many as L - 1 needs, at least one), the whole set repeated as
    often as fits into 128 features, the remaining features 0.  Two indices differ in at least `repeats` features."""
    nbits = max(1, (L - 1).bit_length())
    rep = 128 // nbits
    b = ((torch.arange(L)[:, None] >> torch.arange(nbits)) & 1).float() * 2.0 - 1.0
    code = torch.zeros(L, 128)
    code[:, :nbits * rep] = b.repeat(1, rep)
    return code


def att_random_finite_bf16(shape, g):
    """Random finite bf16 values over many binades: random sign, random 7-bit mantissa, exponent 2^-20 ... 2^20 (no
    zero — the kernel's +0 accumulator cannot return a -0 — and nothing whose sum over a row could overflow fp32)."""
    sign = torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0
    man = 1.0 + torch.randint(0, 128, shape, generator=g).float() / 128.0
    return (sign * man * torch.exp2(torch.randint(-20, 21, shape, generator=g).float())).to(torch.bfloat16)


def att_onehot_inputs(B, H, Hkv, L, perm="random", seed=0):
    """Inputs whose soft-max is exactly one-hot: k[b, g, j] = c * code(j) * s[b, g], q[b, h, i] = c * code(pi[b, h, i]) * s[b, h's kv
    head] with a random sign vector s per (batch, kv head) — so the K of another head or batch does not match — and a permutation
    pi per (batch, q head): 'random' (a fresh one each), 'identity' or 'reversal'.  v: att_random_finite_bf16.
    Query i's score of key pi(i) is c^2 * (features used); any other key loses 2 c^2 per differing feature, at least
    2 * 64 * repeats * log2(e) / sqrt(128) = 179 in the log2 domain at L <= 2048 (11 bits x 11 repeats), more at smaller L:
    past ATT_GAP, and past 150, so exp2(-gap) — every other key's p, and the factor alpha that rescales what a row gathered
    before its matching key arrived — is exactly 0 in fp32.  p of the matching key is 1, or 1 + a few 2^-24 |score| if the
    compiler contracts s * scale - m into an fma; l and 1 / l then differ from 1 by that much and v * (1 / l) still rounds to v.
    Returns q [B, H, L, 128], k, v [B, Hkv, L, 128] (bf16, CPU) and pi [B, H, L]."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * L + 31 * H + B)
    code = att_code(L) * ATT_CODE_SCALE
    if perm == "random":
        pi = torch.stack([torch.randperm(L, generator=g) for _ in range(B * H)]).view(B, H, L)
    else:
        one = torch.arange(L) if perm == "identity" else torch.arange(L - 1, -1, -1)
        pi = one.expand(B, H, L).contiguous()
    s = torch.randint(0, 2, (B, Hkv, 1, 128), generator=g).float() * 2.0 - 1.0
    k = (code * s).to(torch.bfloat16)
    q = (code[pi] * s.repeat_interleave(H // Hkv, dim=1)).to(torch.bfloat16)
    return q, k, att_random_finite_bf16((B, Hkv, L, 128), g), pi


def att_onehot_gap(q, k, pi):
    """The least lead, in the log2 domain, of the score of key pi(i) over every other key of query i (inf with a single key)."""
    B, H, L, _ = q.shape
    rep = H // k.shape[1]
    gap = float("inf")
    for b in range(B):
        s = q[b].float() @ k[b].float().repeat_interleave(rep, dim=0).transpose(1, 2)      # integers below 2^24: exact
        idx = pi[b].to(s.device)[..., None]
        match = s.gather(2, idx)
        if L > 1:
            gap = min(gap, float((match - s.scatter(2, idx, float("-inf")).amax(2, keepdim=True)).min()) * ATT_LOG2_SCALE)
    return gap


def att_onehot_expected(v, pi):
    """What the one-hot construction must return, in the kernel's output layout [B, L, H * 128]: v[b, h's kv head, pi[b, h, i]]."""
    B, H, L = pi.shape
    ve = v.repeat_interleave(H // v.shape[1], dim=1)
    return ve.gather(2, pi.to(v.device)[..., None].expand(B, H, L, 128)).transpose(1, 2).reshape(B, L, H * 128)


def att_counting_inputs(B, H, Hkv, L, seed=0):
    """q = 0: every score is 0, every p exactly 1, l = L; v holds integers of [-8, 8], so the numerator is exact in fp32 in any
    order.  k is random (it must not matter)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * L + 31 * H + B + 1)
    k = torch.randn(B, Hkv, L, 128, generator=g).to(torch.bfloat16)
    v = torch.randint(-8, 9, (B, Hkv, L, 128), generator=g).to(torch.bfloat16)
    return torch.zeros(B, H, L, 128, dtype=torch.bfloat16), k, v


def bf16_nearest(x):
    """fp64 -> the nearest bf16 value (ties to even), kept in fp64; for 0 and magnitudes in bf16's normal range.  Integer
    arithmetic on the bit pattern (45 of the 52 mantissa bits go), so the CPU and the device give the same answer."""
    i = x.contiguous().view(torch.int64)
    i = (i + ((1 << 44) - 1) + ((i >> 45) & 1)) & ~((1 << 45) - 1)
    return i.view(torch.float64)


def att_counting_exact(v, H):
    """sum_j v[j] / L in fp64 (one rounding, of the quotient), [B, 1, H * 128]: every query row of a sequence gets the same."""
    B, Hkv, L, _ = v.shape
    return (v.double().sum(2) / L).repeat_interleave(H // Hkv, dim=1).view(B, 1, H * 128)


def att_counting_verdict(got, v, H):
    """The number of elements of got [B, L, H * 128] that are NOT the bf16 rounding of some number within relative 2^-21 of the exact
    sum_j v[j] / L (the kernel's only inexact steps are the reciprocal of l = L and one product: 2^-23 + 2^-24 with a one-ulp
    reciprocal): got must equal bf16(exact), or bf16 of either end of that interval where exact lies that close to a boundary."""
    exact = att_counting_exact(v, H)
    g = got.double()
    ok = (g == bf16_nearest(exact)) | (g == bf16_nearest(exact * (1.0 - 2.0 ** -21))) | (g == bf16_nearest(exact * (1.0 + 2.0 ** -21)))
    return int((~ok).sum())


def att_general_inputs(kind, B, H, Hkv, L, seed=0, device="cpu"):
    """q [B, H, L, 128], k, v [B, Hkv, L, 128] (bf16, on `device`) for condition C:
    'normal'    q, k, v ~ N(0, 1): a diffuse soft-max;
    'peaked'    q scaled by 3: single keys carry a row;
    'spike'     k[b, g, L // 2] scaled by 6: the running maximum jumps mid-sequence (the rescale branch);
    'negative'  q + 2, k - 2: every real score is near -45, a zero pad key (score 0) would own the row;
    'ascending' kv head 0 and its query heads: k[j] = 3 j / (L - 1) + N(0, 1/16), q = 1 + N(0, 1/100) — the score climbs by 49 in the
                log2 domain from the first key to the last, so the maximum rises on every tile; the other heads as 'normal'.
    E <= ATT_E_CAP asks for max_ij sum_f |q_if| |k_jf| <= 2^6 sqrt(128) = 724.  'spike' and 'negative' come within a few per cent
    of that at the largest shapes (the largest of 10^8 such sums), on either side of it depending on the draw: where the
    largest sum exceeds 0.98 of the cap, q as a whole is scaled down to put it there (the most for 'spike' at L = 1100: by 0.945)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * L + 31 * H + B + 2 + ATT_KINDS.index(kind))
    q = torch.randn(B, H, L, 128, generator=g)
    k = torch.randn(B, Hkv, L, 128, generator=g)
    v = torch.randn(B, Hkv, L, 128, generator=g)
    if kind == "peaked":
        q *= 3.0
    elif kind == "spike":
        k[:, :, L // 2] *= 6.0
    elif kind == "negative":
        q += 2.0
        k -= 2.0
    elif kind == "ascending":
        ramp = 3.0 * torch.arange(L).float() / max(L - 1, 1)
        k[:, 0] = 0.25 * k[:, 0] + ramp[:, None]
        q[:, :H // Hkv] = 0.1 * q[:, :H // Hkv] + 1.0
    q, k, v = q.to(device), k.to(device), v.to(device)
    worst = max(float((q[b].abs() @ k[b].abs().repeat_interleave(H // Hkv, dim=0).transpose(1, 2)).max()) for b in range(B))
    cap = 0.98 * ATT_E_CAP * 2.0 ** 17 * 128 ** 0.5          # 0.98: rounding q and k to bf16 may add 2^-8 of the sum
    if worst > cap:
        q *= cap / worst
    return q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)


def att_reference(q, k, v):
    """fp64 soft-max attention of the bf16 inputs q [B, H, Lq, 128], k, v [B, Hkv, Lk, 128], on their device, one kv head at a time.
    Returns, in the kernel's output layout [B, Lq, H * 128] (fp64): ref = P V, A = P |V| and E, the row's worst-case fp32 score
    error in natural-log units (att_general_verdict)."""
    B, H, Lq, _ = q.shape
    Hkv = k.shape[1]
    rep = H // Hkv
    ref = torch.empty(B, H, Lq, 128, dtype=torch.float64, device=q.device)
    A, E = torch.empty_like(ref), torch.empty_like(ref)
    for b in range(B):
        for g in range(Hkv):
            qd, kd, vd = q[b, g * rep:(g + 1) * rep].double(), k[b, g].double(), v[b, g].double()
            p = torch.softmax(qd @ kd.t() / 128 ** 0.5, dim=-1)
            ref[b, g * rep:(g + 1) * rep] = p @ vd
            A[b, g * rep:(g + 1) * rep] = p @ vd.abs()
            E[b, g * rep:(g + 1) * rep] = 2.0 ** -17 / 128 ** 0.5 * (qd.abs() @ kd.abs().t()).amax(-1, keepdim=True)
    return tuple(t.transpose(1, 2).reshape(B, Lq, H * 128) for t in (ref, A, E))


def att_general_verdict(got, ref, A, E):
    """max over the elements of |got - ref| / bound (at most 1 passes; a NaN gives inf), bound = u A + u |ref| + 2 E (A + |ref|).

    The kernel computes out = bf16(sum_j bf16(p_j) v_j / sum_j p_j) with p_j = exp2(fl(s_j) * scale - m) and everything but the two
    roundings named in fp32; ref = sum_j P_j v_j with the exact weights P.
      * Rounding p_j to bf16 moves it by at most 2^-9 p_j (round to nearest, 8 significant bits), the numerator by 2^-9 sum_j p_j
        |v_j| and the output by 2^-9 A; rounding the result moves it by 2^-9 |out|.  The bound allows u = 2^-8 for each, twice
        that: the other half covers every fp32 step that is not in E — the P V and l accumulations (at most (Lk + 4) 2^-24 <
        2^-12 relative to A and |ref| at Lk < 4092), the product with the scale, exp2 (2^-22) and the reciprocal.
      * The deferred maximum subtracts an m up to DEFER_LOG2 = 4 below the row's maximum, the same for every key of the row:
        p and l grow by a common factor of at most 2^4 before the rounding, relative errors are unchanged.
      * fl(s_j), the MFMA's fp32 accumulation of 128 exact products, is off by at most 127 * 2^-24 * sum_f |q_f| |k_jf| < 2^-17
        sum_f |q_f| |k_jf|; in natural-log units (divided by sqrt(128)) that is at most E for every key of the row, E = 2^-17
        max_j (sum_f |q_f| |k_jf|) / sqrt(128).  Each p_j is then off by a factor within exp(+-E): the numerator moves by (e^E -
        1) A, the denominator's relative change moves the quotient by (e^E - 1) |ref|; with E <= 2^-11 e^E - 1 < 1.001 E, and
        the bound's 2 E (A + |ref|) allows twice the sum."""
    r = ref.abs()
    bound = (ATT_U + 2.0 * E) * (A + r)
    ratio = (got.double() - ref).abs() / bound.clamp_min(1e-300)
    return float(torch.nan_to_num(ratio, nan=float("inf")).max())


# ---- the GEMM epilogues STORE / RESID / SWIGLU, exactly (tests/test_gpu_gemm_exact.py, tests/test_gemm_exact_host.py) ----
# Every expected value is integer arithmetic or ONE IEEE operation plus torch's fp32 -> bf16 cast (which
# test_f2bf_matches_torch_on_every_bit_pattern ties to the device's conversion): independent of libm and of accumulation order.
GEMM_CONFIGS = (-1, 0, 1, 2, 3, 1128, 1160, 1192, 1224, 1256, 1320)     # "gemm_config": automatic, the 8-phase tiles, 1000 + BM
GEMM_BM16 = (128, 160, 192, 224, 256, 320)
GEMM_CANARY = 0x7FA5                                                    # a bf16 NaN whose payload no kernel produces


def gemm8_admits(M, N, K, ldc, ldr=None, c_byte_offset=0):
    """csrc/gemm8.hip gemm8_supports restated for K-contiguous operands and 16-byte aligned allocations: may the 8-phase kernel run?"""
    return (K % 128 == 0 and K >= 256 and M % 8 == 0 and N % 8 == 0 and M >= 8 and N >= 8 and ldc % 8 == 0
            and (ldr is None or ldr % 8 == 0) and c_byte_offset % 16 == 0)


def gemm_int_operands(M, N, K, seed=0):
    """A [M, K], W [N, K] (bf16, CPU): seeded random integers of [-7, 7], or [-15, 15] at K = 64 (so that a single K-tile's sums still leave
    bf16's 8 bits).  Every product and partial sum is an integer below K * 225 < 2^24: the fp32 accumulator is exact in any order."""
    amp = 15 if K <= 64 else 7
    assert K * amp * amp < 2 ** 24
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
    A = torch.randint(-amp, amp + 1, (M, K), generator=g).to(torch.bfloat16)
    W = torch.randint(-amp, amp + 1, (N, K), generator=g).to(torch.bfloat16)
    return A, W


def gemm_pre(A, W, k_tiles=None):
    """The exact pre-activation A @ W.T of integer operands as int64 (float64 products and sums of integers below 2^53: exact).
    k_tiles: weights per 64-wide K-tile (the mutations: 0 drops a tile, 2 counts it twice); None: every tile once."""
    a, w = A.double(), W.double()
    if k_tiles is not None:
        a = a * torch.tensor(k_tiles, dtype=torch.float64).repeat_interleave(64)[None, :]
    return (a @ w.t()).to(torch.int64)


def gemm_expected_store(pre):
    """bf16(acc): the integer as fp32 (exact below 2^24), then torch's cast."""
    assert int(pre.abs().max()) < 2 ** 24
    return pre.float().to(torch.bfloat16)


def gemm_resid_rows(M, rwin=0, rlp=0, rbeg=0):
    """Residual row of output row m: m, or with a row window b * rlp + rbeg + i for the compact row m = b * rwin + i."""
    m = torch.arange(M)
    if not rwin:
        return m
    b = m // rwin
    return b * rlp + rbeg + (m - b * rwin)


def gemm_owner(M, mod, rank, shift=0):
    """[M] bool: does rank `rank` of `mod` add the residual of row m?  Fragment row m >> 4 belongs to rank (m >> 4) % mod.
    shift != 0 is the mutation 'the wrong owner's fragment rows'."""
    return (((torch.arange(M) >> 4) + shift) % mod) == rank


def gemm_resid(pre, rows, ldr, seed=0):
    """[rows, ldr] random bf16 ~ N(0, std(acc)): arbitrary mantissas at the magnitude of the accumulator."""
    g = torch.Generator().manual_seed(seed + 17)
    return (torch.randn(rows, ldr, generator=g) * float(pre.double().std())).to(torch.bfloat16)


def gemm_poison_resid(resid, keep_rows):
    """A copy of resid with every row NOT in keep_rows filled with NaN: what a rank must never read."""
    out = torch.full_like(resid, float("nan"))
    out[keep_rows] = resid[keep_rows]
    return out


def gemm_expected_resid(pre, resid, mod=1, rank=0, rwin=0, rlp=0, rbeg=0, owner_shift=0, every_rank=False, single_rounding=False):
    """bf16(resid + bf16(acc)) on the rows the rank owns, bf16(acc) elsewhere: one IEEE fp32 add and one rounding per element.
    The keyword mutations restate the defects the tests must catch."""
    M, N = pre.shape
    acc = gemm_expected_store(pre)
    own = torch.ones(M, dtype=torch.bool) if every_rank else gemm_owner(M, mod, rank, owner_shift)
    r = resid[gemm_resid_rows(M, rwin, rlp, rbeg), :N].float()
    summed = (r + (pre.float() if single_rounding else acc.float())).to(torch.bfloat16)
    return torch.where(own[:, None], summed, acc)


def gemm_onehot(M, K, stride, shift):
    """A [M, K] bf16 with A[m, pi(m)] = 1, pi(m) = (m * stride + shift) % K, stride odd: the pre-activation is W[n, pi(m)] exactly, for
    arbitrary mantissas of W — which k and which n every output reads.  Returns (A, pi)."""
    assert stride % 2 == 1
    pi = (torch.arange(M) * stride + shift) % K
    A = torch.zeros(M, K, dtype=torch.bfloat16)
    A[torch.arange(M), pi] = 1.0
    return A, pi


def gemm_random_w(N, K, seed=0):
    """[N, K] random normal bf16, finite and nonzero (0 * Inf would poison a whole output row)."""
    g = torch.Generator().manual_seed(seed + 29)
    W = torch.randn(N, K, generator=g).to(torch.bfloat16)
    assert bool(torch.isfinite(W.float()).all()) and bool((W.float() != 0).all())
    return W


def silu_margin_ok(vals):
    """For bf16 gate values: (ok, silu) — silu = the bf16 nearest to the float64 g / (1 + exp(-g)); ok where that float64 value lies
    further than 2^-16 (relative) from a bf16 rounding midpoint.  The device evaluates g / (1.0f + expf(-g)): a few-ulp expf, one
    add, one IEEE division, about 2^-21 relative in all — 1/32 of the margin, so bf16(silu) is the same for ANY correct fp32
    evaluation (and for the table, which silu_lut_kernel fills with that function)."""
    g = vals.double()
    s = g / (1.0 + torch.exp(-g))
    mant, _ = torch.frexp(s.abs())                 # [0.5, 1)
    scaled = mant * 256.0                          # [128, 256): bf16's 8 significant bits are the integer part
    frac = scaled - torch.floor(scaled)
    ok = ((frac - 0.5).abs() / scaled > 2.0 ** -16) | (s == 0)
    return ok, bf16_nearest(s).to(torch.bfloat16)


_SILU_SAFE = {}


def silu_safe_set():
    """(gates, silu, n_domain): the bf16 values with |g| in [2^-14, 2^5) — the whole domain of the SwiGLU epilogue's table
    (gemm_epilogue.h: SiluLut), 4 864 values — that pass silu_margin_ok, and their bf16 SiLU."""
    if not _SILU_SAFE:
        key = torch.arange(19 * 128, dtype=torch.int32) + (113 << 7)
        dom = torch.cat([key, key | 0x8000]).to(torch.int16).view(torch.bfloat16)
        ok, s = silu_margin_ok(dom)
        _SILU_SAFE["v"] = (dom[ok], s[ok], dom.numel())
    return _SILU_SAFE["v"]


def silu_bf16_torch(x):
    """F.silu on a bf16 tensor the way the reference runs it: fp32 inside, rounded to bf16."""
    return torch.nn.functional.silu(x.float()).to(torch.bfloat16)


def swiglu_weights(N, K, seed=0, extras=None):
    """Gate rows G [N / 2, K] drawn from the safe set and up rows U [N / 2, K] ~ N(0, 1) (bf16).  extras: gate values outside the table's
    domain mixed into half of the entries of every 24th gate column (two whole 16-row fragments at least, so some waves of every
    tile configuration take the evaluating path while the others read the table)."""
    g = torch.Generator().manual_seed(1000003 * seed + 31 * N + K + 41)
    safe = silu_safe_set()[0]
    G = safe[torch.randint(0, safe.numel(), (N // 2, K), generator=g)]
    U = torch.randn(N // 2, K, generator=g).to(torch.bfloat16)
    if extras is not None:
        cols = torch.arange(5, N // 2, 24)
        pick = extras[torch.randint(0, extras.numel(), (cols.numel(), K), generator=g)]
        mix = torch.rand(cols.numel(), K, generator=g) < 0.5
        G[cols] = torch.where(mix, pick, G[cols])
    return G, U


def swiglu_pack(G, U):
    """W [N, K] in the library's packed gate/up row order (pack_gate_up): groups of 32 rows = [16 gate rows | the matching 16 up rows]."""
    n2, K = G.shape
    W = torch.empty(2 * n2, K, dtype=torch.bfloat16)
    Wv = W.view(n2 // 16, 2, 16, K)
    Wv[:, 0] = G.view(n2 // 16, 16, K)
    Wv[:, 1] = U.view(n2 // 16, 16, K)
    return W


def swiglu_expected(G, U, pi, swapped=False):
    """[M, N / 2]: bf16(silu_bf16(gate) * up) with gate = G[c, pi(m)], up = U[c, pi(m)] — the one-hot operand's pre-activations: one
    exact fp32 product of two bf16 values and one rounding.  swapped: the mutation 'gate and up halves exchanged'."""
    gate, up = G[:, pi].t(), U[:, pi].t()
    if swapped:
        gate, up = up, gate
    return (silu_bf16_torch(gate).float() * up.float()).to(torch.bfloat16)


def gemm_exact_verdict(got, exp):
    """None if got and exp (bf16, same shape) hold the same BITS; else the first wrong element, both bit patterns and the count."""
    g, e = bits(got), bits(exp)
    bad = g != e
    count = int(bad.sum())
    if count == 0:
        return None
    m, n = (int(i) for i in bad.nonzero()[0])
    return dict(count=count, first=(m, n), got=int(g[m, n]) & 0xFFFF, expected=int(e[m, n]) & 0xFFFF)
