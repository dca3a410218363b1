"""MI355X-native `interleave_generate` — the MMaDA-Parallel-M sampler
(MMaDA-Parallel-M/models/modeling_mmada.py:117-248, models/sampling.py:31-36) on the same HIP kernels.

Differences from the A sampler that matter: cond and uncond run as ONE batch-2 forward every step;
text logits are CFG-combined (cond + text_cfg*(uncond-cond)); image logits are (1+cfg)*cond - cfg*uncond; the image
token is ALWAYS drawn with torch.multinomial; the re-mask uses Gumbel noise and a cut-off compare; no newline tokens
inside the image span; the returned image ids are the last image step's samples.

The random draws go through an `rng` object (default: torch's own RNG calls, in the reference's order) so that parity
tests can replay the reference's draws.

Opt-in, `image_sampler="device"` / `text_sampler="device"` with `sampler_seed`: the draws run inside the kernels
(mmada_image_sample_m, mmada_image_commit_m_sampled, mmada_text_draw_cfg) on the counter-based generator of
csrc/sample_noise.h, and a step can then replay as one hipGraph (`graph=True`); see interleave_generate.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch

from .. import abi
from ..model import LLaDAForMultiModalGeneration
from .parallel_generator import check_tp_exchange, mask_len_schedule
from .sampler_options import IMAGE_COUNTER0, check_samplers, seed_u64
from .step_graph import StepGraphs


def cosine_schedule(t):
    """models/sampling.py:39-40."""
    return torch.cos(t * math.pi * 0.5)


def get_num_transfer_tokens(mask_index: torch.Tensor, steps: int) -> torch.Tensor:
    """modeling_mmada.py:63-81: base + remainder schedule (differs from the A sampler's)."""
    mask_num = mask_index.sum(dim=1, keepdim=True)
    base = mask_num // steps
    remainder = mask_num % steps
    out = torch.zeros(mask_num.size(0), steps, dtype=torch.int64) + base
    for i in range(mask_num.size(0)):
        out[i, :remainder[i]] += 1
    return out


class TorchRng:
    """The reference's random draws, call for call (device RNG)."""

    def text_gumbel_argmax(self, text_logits: torch.Tensor, temperature: float) -> torch.Tensor:
        # add_gumbel_noise (:49-60) + argmax (:182), float64
        l64 = text_logits.to(torch.float64)
        noise = torch.rand_like(l64, dtype=torch.float64)
        return torch.argmax(l64.exp() / ((-torch.log(noise)) ** temperature), dim=-1)

    def rand_f64(self, shape, device) -> torch.Tensor:
        return torch.rand(tuple(shape), dtype=torch.float64, device=device)  # torch.rand_like(logits, dtype=float64)

    def multinomial(self, probs2d: torch.Tensor, generator) -> torch.Tensor:
        return torch.multinomial(probs2d, 1, generator=generator)[:, 0]  # :220-222

    def uniform_like(self, t: torch.Tensor, generator) -> torch.Tensor:
        return torch.zeros_like(t).uniform_(0, 1, generator=generator)  # sampling.py:15-16


def _log(t, eps=1e-20):
    return torch.log(t.clamp(min=eps))  # sampling.py:11-12


@torch.no_grad()
def interleave_generate(
    model,
    input_ids: torch.LongTensor = None,
    uncond_input_ids: torch.LongTensor = None,
    text_cfg: float = 0.0,
    image_cfg: float = 3.5,
    noise_schedule: Callable = cosine_schedule,
    text_steps: int = 100,
    image_steps: int = 100,
    reserved_token_mapping: Dict = None,
    generator: torch.Generator = None,
    config=None,
    remasking="low_confidence",
    text_temperature: float = 0.0,
    image_temperature: float = 1.0,
    rng=None,
    trace: Optional[list] = None,
    image_sampler: str = "torch",
    text_sampler: str = "torch",
    sampler_seed: Optional[int] = None,
    graph: Optional[bool] = None,
    **kwargs,
):
    """Returns (image ids [1, num_vq_tokens], text ids [1, max_seq_length]) like the reference.

    ONE loop for every sampler setting: the launches of a step run over buffers that all exist before the loop, so that a step
    takes no argument that changes from step to step (k, mask_len and the re-mask temperature are copied per step into device [1]
    buffers).  A sampler left at "torch" draws from `rng` in the reference's order, on those buffers.

    `image_sampler="device"` (opt-in; the default "torch" is the reference's path, draw for draw): an image step is
    mmada_head_rows, mmada_image_sample_m (col0 = len(tokenizer)) and mmada_image_commit_m_sampled.  Neither the [N, codebook]
    probabilities nor any torch random tensor exists and `rng` / `generator` are never called for it.  The token is a Gumbel-max draw
    at temperature 1 over the CFG-combined bf16 logits — it samples their soft-max evaluated in fp32, where the reference's
    multinomial samples the bf16-rounded probabilities — and the re-mask noise is a counter-based Gumbel value per image position,
    both keyed by `sampler_seed` (required) and a counter that starts at 1 << 62 per call and advances by 1 per image step.  The
    re-mask temperature image_temperature * (1 - (i + 1) / text_steps) is host double arithmetic as on the torch path, cast to fp32.
    One rank, or a tensor-parallel group on the library's pull / copy transport (every rank runs the same call with the same seed).

    `text_sampler="device"` (opt-in; needs text_temperature > 0): the text draw is mmada_text_draw_cfg on the cond / uncond halves of
    the text logits — a Gumbel-max draw in fp32 from soft-max(combined / text_temperature) instead of the reference's float64
    exp(l) / (-log u)^T on a [T, V] float64 copy — keyed by `sampler_seed` and a counter that starts at 0 and advances by 1 per step.
    The draws of neither sampler reproduce torch's RNG stream.

    `graph` (None = env MMADA_GRAPH=1): replay each kind of step — text-only, image step — as ONE hipGraph (step_graph.StepGraphs):
    the first step of a kind runs eagerly, the second is captured, the rest replay, bit-identical to the eager run.  Only when
    image_sampler == "device" and (text_temperature == 0 or text_sampler == "device") and trace is None and the forward issues no
    host-side collective; otherwise the run is eager."""
    if not isinstance(model, LLaDAForMultiModalGeneration):
        raise TypeError("interleave_generate (MI355X) needs mmada_parallel_amd.LLaDAForMultiModalGeneration")
    if remasking != "low_confidence":
        raise NotImplementedError(remasking)
    if not (text_cfg or image_cfg):
        raise ValueError("text_cfg and image_cfg cannot be both 0")  # modeling_mmada.py:176-177
    dev_img, dev_text = check_samplers(model, image_sampler, text_sampler, sampler_seed, text_temperature=text_temperature)
    rng = rng or TorchRng()
    lib, h, device = model._lib, model._handle, model.device
    uni_prompting = kwargs.get("uni_prompting", None)
    tok = uni_prompting.text_tokenizer
    text_vocab = len(tok)
    mask_id = int(model.config.get("mask_token_id", 126336))
    N = config.model.mmada.num_vq_tokens
    CB = config.model.mmada.codebook_size
    T = config.dataset.preprocessing.max_seq_length
    V = model.vocab

    input_ids = input_ids.to(device).unsqueeze(0)
    uncond_input_ids = uncond_input_ids.to(device).unsqueeze(0)
    P = input_ids.shape[1]

    def full(n, v):
        return torch.full((1, n), v, dtype=torch.long, device=device)

    out_ids = torch.cat([full(1, reserved_token_mapping['<|soi|>']), full(N, mask_id),
                         full(1, reserved_token_mapping['<|eoi|>']), full(1, tok.bos_token_id), full(T - 1, mask_id)], dim=1)
    L = P + out_ids.shape[1]
    if uncond_input_ids.shape[1] != P:
        raise ValueError("cond and uncond prompts must have equal length (the reference batches them, :171)")
    text_start, img_start = L - T, P + 1
    # cond and uncond as ONE fixed [2, L] batch: row 0 IS the running combined_input_ids (:144), row 1 = the uncond prompt + a copy of
    # row 0's tail, refreshed every step (:166-169)
    both = torch.cat([torch.cat([input_ids, out_ids], dim=1), torch.cat([uncond_input_ids, out_ids], dim=1)], dim=0).contiguous()
    ids = both[0:1]

    num_transfer = get_num_transfer_tokens((ids[:, text_start:] == mask_id).cpu(), text_steps)
    img_steps = set(torch.linspace(text_steps // 4, text_steps - 1, image_steps).round().int().tolist())
    temps = [image_temperature * (1.0 - 1.0 * (s + 1) / text_steps) for s in range(text_steps)]   # host double
    k_dev = num_transfer.t().contiguous().to(device=device, dtype=torch.int32)
    mlen_dev = torch.tensor(mask_len_schedule(N, text_steps, noise_schedule), dtype=torch.int32, device=device)
    pos_map = torch.arange(img_start, img_start + N, dtype=torch.int32, device=device)
    ar = torch.arange(text_start, L, dtype=torch.int32, device=device)
    text_rows = torch.cat([ar, ar + L])                       # cond rows then uncond rows (batch-major)
    img_rows = torch.cat([pos_map, pos_map + L])
    scratch = torch.empty(T * 16, dtype=torch.uint8, device=device)
    argmax = torch.empty((1, N), dtype=torch.int32, device=device)
    pmax = torch.empty((1, N), dtype=torch.bfloat16, device=device)
    model._ensure_ws(2, L)   # before the first step: a workspace that grew later would leave a captured graph pointing at freed memory
    tl = torch.empty((2 * T, V), dtype=torch.bfloat16, device=device)                   # [2T, V]: cond rows, uncond rows
    il = torch.empty((2 * N, CB), dtype=torch.bfloat16, device=device) if img_steps else None
    x0 = torch.zeros(T, dtype=torch.int32, device=device) if text_temperature != 0 else None
    k_cur = torch.zeros(1, dtype=torch.int32, device=device)
    mlen_cur = torch.zeros(1, dtype=torch.int32, device=device)
    seed64 = seed_u64(sampler_seed) if dev_img or dev_text else None
    if dev_text:
        text_counter = torch.zeros(1, dtype=torch.int64, device=device)          # advanced by mmada_text_draw_cfg
    if dev_img:
        img_counter = torch.full((1,), IMAGE_COUNTER0, dtype=torch.int64, device=device)   # advanced by mmada_image_commit_m_sampled
        temp_dev = torch.tensor(temps, dtype=torch.float32, device=device)
        temp_cur = torch.zeros(1, dtype=torch.float32, device=device)
        drawn = torch.empty((1, N), dtype=torch.int32, device=device)
        p_sel = torch.empty((1, N), dtype=torch.bfloat16, device=device)
        sampled = torch.empty((1, N), dtype=torch.int32, device=device)
    sampled_ids = None

    def step_body(i, is_img):
        nonlocal sampled_ids
        both[1, P:].copy_(both[0, P:])
        if trace is not None:
            trace.append(both.cpu().clone())
        # rows read this step: the text span, plus the image span on image steps (the last block computes only those)
        model.forward_body(both, consumed=(img_start if is_img else text_start, L))   # one batch-2 forward (:171)
        st = abi.stream_ptr()
        model.head_rows(text_rows, 0, V, out=tl)
        if is_img:
            model.head_rows(img_rows, text_vocab, text_vocab + CB, out=il)
        if text_temperature != 0 and dev_text:
            abi.check(lib.mmada_text_draw_cfg(h, tl[:T].data_ptr(), tl[T:].data_ptr(), float(text_cfg), 1, T, V, V,
                                              float(text_temperature), seed64, text_counter.data_ptr(), x0.data_ptr(), st),
                      "mmada_text_draw_cfg")
        elif text_temperature != 0:
            comb = tl[:T] + text_cfg * (tl[T:] - tl[:T])         # :173 on the text rows, bf16 tensor ops
            x0.copy_(rng.text_gumbel_argmax(comb.view(1, T, V), text_temperature).view(T))
        abi.check(lib.mmada_text_select_cfg(h, tl[:T].data_ptr(), tl[T:].data_ptr(), float(text_cfg), abi.ptr(x0), 1, T, V, V,
                                            ids.data_ptr(), L, text_start, k_cur.data_ptr(), scratch.data_ptr(), st),
                  "mmada_text_select_cfg")
        if is_img and dev_img:
            abi.check(lib.mmada_image_sample_m(h, il[:N].data_ptr(), il[N:].data_ptr(), 1, N, CB, float(image_cfg), text_vocab, seed64,
                                               img_counter.data_ptr(), drawn.data_ptr(), p_sel.data_ptr(), None, None, st),
                      "mmada_image_sample_m")
            abi.check(lib.mmada_image_commit_m_sampled(h, ids.data_ptr(), 1, L, pos_map.data_ptr(), N, drawn.data_ptr(),
                                                       p_sel.data_ptr(), temp_cur.data_ptr(), seed64, img_counter.data_ptr(),
                                                       mlen_cur.data_ptr(), text_vocab, sampled.data_ptr(), st),
                      "mmada_image_commit_m_sampled")
        elif is_img:   # the reference's draws (:216-241)
            probs = torch.empty((N, CB), dtype=torch.bfloat16, device=device)
            abi.check(lib.mmada_image_probs_m(h, il[:N].data_ptr(), il[N:].data_ptr(), 1, N, CB, float(image_cfg), probs.data_ptr(),
                                              argmax.data_ptr(), pmax.data_ptr(), st), "mmada_image_probs_m")
            cur = ids[:, img_start:img_start + N]
            unknown = cur == mask_id
            sampled_ids = torch.where(unknown, rng.multinomial(probs, generator).view(1, N), cur - text_vocab)   # :224-225
            p = torch.gather(probs.view(1, N, CB), -1, sampled_ids[..., None]).squeeze(-1)
            p = torch.where(unknown, p, torch.finfo(p.dtype).max).contiguous()                # :233
            gumbel = (-_log(-_log(rng.uniform_like(p, generator)))).contiguous()              # sampling.py:15-17
            s32 = sampled_ids.to(torch.int32).contiguous()
            abi.check(lib.mmada_image_commit_m(h, ids.data_ptr(), 1, L, pos_map.data_ptr(), N, s32.data_ptr(), p.data_ptr(),
                                               gumbel.data_ptr(), float(temps[i]), mlen_cur.data_ptr(), text_vocab, st),
                      "mmada_image_commit_m")

    # a replayed step would otherwise replay torch's draws
    with StepGraphs(model, graph, dev_img and (text_temperature == 0 or dev_text) and trace is None) as sg:
        with sg.stream():
            for i in range(text_steps):
                is_img = i in img_steps
                k_cur.copy_(k_dev[i])
                mlen_cur.copy_(mlen_dev[i:i + 1])
                if dev_img:
                    temp_cur.copy_(temp_dev[i:i + 1])
                sg.step(is_img, lambda: step_body(i, is_img), nodes_key=("interleave", is_img))
        sg.join()   # whoever consumes the ids sees the finished run
    check_tp_exchange(model)   # tensor parallel: a timed-out hand-off raises instead of returning void tokens
    if dev_img and img_steps:
        sampled_ids = sampled.long()
    return sampled_ids, ids[:, text_start:]
