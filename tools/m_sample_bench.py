#!/usr/bin/env python
"""An M image step's sampling two ways, after the LM head has written the cond / uncond [N, 8192] codebook logits, timed with
device events, interleaved in one process on one GPU:

  (a) torch    mmada_image_probs_m with the [N, 8192] bf16 probabilities + torch.multinomial + gather + uniform_ and two logs +
               mmada_image_commit_m (temperature by value): what interleave_generate(image_sampler="torch") runs per image step
  (b) device   mmada_image_sample_m + mmada_image_commit_m_sampled: the draw and the re-mask noise inside the kernels, no
               probabilities

and then, at 8B width on synthetic weights, the step time of interleave_generate(image_sampler="device") eager against graph=True
(each step kind replayed as one hipGraph).

    python tools/m_sample_bench.py [--rounds 12] [--reps 64] [--layers 32] [--text-steps 32] [--out profiles/m_sample_bench.txt]

Part one runs at N = 1024 image positions, codebook 8192, image_cfg = 3.5.  Each round times (a) and (b) once, in an order that
alternates from round to round; medians and the min-max spread over the rounds are reported, the per-round ratio (b)/(a), and the
peak device memory each adds while it runs (torch's allocator).  The two draw from different random streams (and (b) samples the
fp32 soft-max, (a) its bf16 rounding), so their tokens are not compared; what they share — arg-max and its probability — is
checked bit for bit before the timing.  Part two runs the whole sampler (N = 1024, max_seq_length 256, a 64-token prompt) twice per
mode, alternating, after one warm-up run of each, and checks that both modes return the same ids."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmada_parallel_amd import LLaDAForMultiModalGeneration, abi, synth  # noqa: E402
from mmada_parallel_amd.generators.interleave_generator import interleave_generate  # noqa: E402


def peak_added(fn, dev):
    """Bytes torch's allocator holds at its peak while fn() runs, above what it held before."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def _log(t, eps=1e-20):
    return torch.log(t.clamp(min=eps))


def image_step(args, dev, lines):
    seed = 20261020
    lib = abi.lib()
    cfg = abi.MmadaCfg(d_model=256, n_layers=1, n_heads=2, n_kv_heads=2, head_dim=128, mlp_hidden=512, vocab=134656, max_seq=1024,
                       rms_eps=1e-5, rope_theta=500000.0, tp_rank=0, tp_size=1, mask_token_id=synth.MASK,
                       text_vocab_size=synth.TEXT_VOCAB, codebook_size=synth.CODEBOOK, reserved=0)
    h = C.c_void_p()
    abi.check(lib.mmada_create(C.byref(cfg), None, C.byref(h)), "mmada_create")   # the sampler entry points only read its cfg
    CB, N, image_cfg, temp, mlen_v, B = synth.CODEBOOK, 1024, 3.5, 0.6, 400, 1
    L = N + 64
    g = torch.Generator().manual_seed(6)
    cond = (torch.randn(N, CB, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    unc = (cond.float().cpu() + torch.randn(N, CB, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    pos = torch.arange(32, 32 + N, dtype=torch.int32, device=dev)
    ids0 = torch.randint(0, 1000, (B, L), generator=g).to(dev)
    ids0[:, 32:32 + N] = synth.MASK
    ids = ids0.clone()
    mlen = torch.tensor([mlen_v], dtype=torch.int32, device=dev)
    argmax = torch.empty((B, N), dtype=torch.int32, device=dev)
    pmax = torch.empty((B, N), dtype=torch.bfloat16, device=dev)
    counter = torch.full((1,), 1 << 62, dtype=torch.int64, device=dev)
    temp_dev = torch.tensor([temp], dtype=torch.float32, device=dev)
    sampled = torch.empty((B, N), dtype=torch.int32, device=dev)
    p_sel = torch.empty((B, N), dtype=torch.bfloat16, device=dev)
    probs = torch.empty((N, CB), dtype=torch.bfloat16, device=dev)

    def run_a():   # generators/interleave_generator.py, the image step of the torch path
        st = abi.stream_ptr()
        abi.check(lib.mmada_image_probs_m(h, cond.data_ptr(), unc.data_ptr(), B, N, CB, image_cfg, probs.data_ptr(), argmax.data_ptr(),
                                          pmax.data_ptr(), st), "mmada_image_probs_m")
        drawn = torch.multinomial(probs, 1)[:, 0].view(B, N)
        cur = ids[:, 32:32 + N]
        unknown = cur == synth.MASK
        s64 = torch.where(unknown, drawn, cur - synth.TEXT_VOCAB)
        p = torch.gather(probs.view(B, N, CB), -1, s64[..., None]).squeeze(-1)
        p = torch.where(unknown, p, torch.finfo(p.dtype).max).contiguous()
        gumbel = (-_log(-_log(torch.zeros_like(p).uniform_(0, 1)))).contiguous()
        s32 = s64.to(torch.int32).contiguous()
        abi.check(lib.mmada_image_commit_m(h, ids.data_ptr(), B, L, pos.data_ptr(), N, s32.data_ptr(), p.data_ptr(), gumbel.data_ptr(),
                                           temp, mlen.data_ptr(), synth.TEXT_VOCAB, st), "mmada_image_commit_m")

    def run_b():
        st = abi.stream_ptr()
        abi.check(lib.mmada_image_sample_m(h, cond.data_ptr(), unc.data_ptr(), B, N, CB, image_cfg, synth.TEXT_VOCAB, seed,
                                           counter.data_ptr(), sampled.data_ptr(), p_sel.data_ptr(), None, None, st), "mmada_image_sample_m")
        abi.check(lib.mmada_image_commit_m_sampled(h, ids.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p_sel.data_ptr(),
                                                   temp_dev.data_ptr(), seed, counter.data_ptr(), mlen.data_ptr(), synth.TEXT_VOCAB, None,
                                                   st), "mmada_image_commit_m_sampled")

    fns = {"a": run_a, "b": run_b}
    # what the two share is the same bits: arg-max and its probability, and p_sel is (a)'s probability of (b)'s token
    am_b, pm_b = torch.empty_like(argmax), torch.empty_like(pmax)
    run_a()
    abi.check(lib.mmada_image_sample_m(h, cond.data_ptr(), unc.data_ptr(), B, N, CB, image_cfg, synth.TEXT_VOCAB, seed, counter.data_ptr(),
                                       sampled.data_ptr(), p_sel.data_ptr(), am_b.data_ptr(), pm_b.data_ptr(), abi.stream_ptr()),
              "mmada_image_sample_m")
    torch.cuda.synchronize()
    assert torch.equal(am_b, argmax) and torch.equal(pm_b.view(torch.int16), pmax.view(torch.int16))
    assert torch.equal(p_sel.view(torch.int16), probs.gather(-1, sampled.view(N, 1).long()).view(B, N).view(torch.int16))
    for f in fns.values():   # warm-up of every timed shape
        ids.copy_(ids0)
        f()
    torch.cuda.synchronize()
    probs = None             # (a)'s peak counts its probabilities too

    def run_a_alloc():
        nonlocal probs
        probs = torch.empty((N, CB), dtype=torch.bfloat16, device=dev)
        run_a()

    ids.copy_(ids0)
    mem_a = peak_added(run_a_alloc, dev)
    ids.copy_(ids0)
    mem_b = peak_added(run_b, dev)
    times = {n: [] for n in fns}
    order = ["a", "b"]
    for r in range(args.rounds):
        for n in order[r % 2:] + order[:r % 2]:
            ids.copy_(ids0)          # outside the timed window; a step's cost does not depend on how many positions are known
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fns[n]()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) / args.reps)
    med = {n: statistics.median(v) for n, v in times.items()}
    ba = [b / a for a, b in zip(times["a"], times["b"])]
    lines.append(f"image step: N = {N} image positions, codebook {CB}, image_cfg {image_cfg}, re-mask temperature {temp}, mask_len {mlen_v}, "
                 f"{args.rounds} rounds x {args.reps} steps, device events, ms per step; arg-max, its probability and p_sel of (b) "
                 f"bit-identical to mmada_image_probs_m")
    names = {"a": "(a) image_probs_m + multinomial + gather + uniform_/logs + image_commit_m", "b": "(b) mmada_image_sample_m + mmada_image_commit_m_sampled"}
    for n in order:
        lines.append(f"  {names[n]:74s} median {med[n]:8.4f}  min {min(times[n]):8.4f}  max {max(times[n]):8.4f}")
    lines.append(f"  (b) / (a): median of rounds {statistics.median(ba):.4f}  min {min(ba):.4f}  max {max(ba):.4f}")
    lines.append(f"  peak memory added: (a) {mem_a / 2**20:.2f} MiB of torch tensors (bf16 probabilities {N * CB * 2 / 2**20:.1f} MiB, "
                 f"multinomial's temporaries, the draws);  (b) {mem_b / 2**20:.3f} MiB")
    lib.mmada_destroy(h)


class Tok:
    bos_token_id = 126080

    def __len__(self):
        return synth.TEXT_VOCAB


def whole_sampler(args, dev, lines):
    cfg = dict(synth.CFG_8B, n_layers=args.layers)
    sd = synth.synthetic_state_dict(cfg, seed=0, device=dev)
    model = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, max_batch=2)
    del sd
    N, T, P = 1024, 256, 64
    g = torch.Generator().manual_seed(3)
    inp, unc = torch.randint(0, 120000, (P,), generator=g), torch.randint(0, 120000, (P,), generator=g)
    config = SimpleNamespace(model=SimpleNamespace(mmada=SimpleNamespace(num_vq_tokens=N, codebook_size=synth.CODEBOOK)),
                             dataset=SimpleNamespace(preprocessing=SimpleNamespace(max_seq_length=T)))

    def run(graph):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = interleave_generate(model, inp, unc, text_cfg=2.5, image_cfg=3.5, text_steps=args.text_steps, image_steps=args.text_steps,
                                  reserved_token_mapping={"<|soi|>": synth.BOI, "<|eoi|>": synth.EOI}, config=config, text_temperature=0.7,
                                  uni_prompting=SimpleNamespace(text_tokenizer=Tok()), image_sampler="device", text_sampler="device",
                                  sampler_seed=7, graph=graph)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.text_steps, out

    outs = {graph: run(graph)[1] for graph in (False, True)}    # warm-up of both modes
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1]), "graph replay changed the ids"
    times = {False: [], True: []}
    for r in range(2):
        for graph in ((False, True) if r % 2 == 0 else (True, False)):
            times[graph].append(run(graph)[0])
    L = P + N + T + 2
    lines.append(f"interleave_generate at 8B width ({args.layers} blocks, synthetic weights), one batch-2 forward of L = {L} per step, "
                 f"{args.text_steps} steps ({len(set(torch.linspace(args.text_steps // 4, args.text_steps - 1, args.text_steps).round().int().tolist()))} "
                 f"image steps), both samplers on the device, text_temperature 0.7, wall time per step over the whole call, ms; "
                 f"the two modes return the same ids")
    for graph, name in ((False, "eager"), (True, "graph=True")):
        lines.append(f"  {name:12s} runs {', '.join(f'{t:.3f}' for t in times[graph])}  best {min(times[graph]):.3f}")
    lines.append(f"  graph / eager (best of each): {min(times[True]) / min(times[False]):.4f}; nodes per captured step kind "
                 f"{ {k[1]: v for k, v in model.graph_nodes.items() if k[0] == 'interleave'} } (key: image step)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=64, help="image steps per timed window")
    ap.add_argument("--layers", type=int, default=32, help="denoiser blocks of the 8B-width model of part two (0: skip part two)")
    ap.add_argument("--text-steps", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m_sample_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("m_sample_bench: needs a GPU (a CPU run measures nothing)")
    dev = "cuda:0"
    lines = [f"m_sample_bench: {torch.cuda.get_device_name(0)}"]
    image_step(args, dev, lines)
    if args.layers:
        whole_sampler(args, dev, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
