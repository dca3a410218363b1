#!/usr/bin/env python
"""generate_image's and mmu_generate's sampling two ways — the torch path (image_sampler / text_sampler = "torch", the reference's
draws) against the device path — interleaved in one process on one GPU.  No threshold is set anywhere: the torch side of each
comparison is the baseline and the figures are reported as measured.

  (a) the sampling of ONE generate_image step after the LM head has written the cond / uncond [N, 8192] codebook logits (N = 1024,
      cfg on), device events:
        torch    mmada_image_probs_m with the [N, 8192] bf16 probabilities, the bf16 CFG combine, torch.rand + two logs over [N, 8192],
                 divide, add, argmax, gather, torch.rand + two logs over [1, N], three scatters, mmada_image_commit_g
        device   mmada_image_sample_g + mmada_image_commit_g_sampled
  (b) a whole generate_image(image_sampler="device") call at 8B width on synthetic weights, eager against graph=True (the step
      replayed as one hipGraph), wall time per step, and the node count of the captured step
  (c) a whole mmu_generate call at temperature > 0 at 8B width, P + max_new_tokens = 1600, block_length 128, torch path against
      device path, without and with guidance, wall time per step
  (d) the peak of torch's allocator that each of the above adds while it runs

    python tools/t2i_mmu_sample_bench.py [--rounds 12] [--reps 64] [--layers 32] [--timesteps 8] [--mmu-steps 8]
                                         [--out profiles/t2i_mmu_sample_bench.txt]

Part (a): each round times both once, in an order that alternates from round to round; medians and the min-max spread over the
rounds, and the per-round ratio.  Every repetition of either starts from the all-masked ids (a 9 KB copy inside the window, the same
for both), so the torch path's row count is N every time.  The two draw from different random streams, so their tokens are not
compared; p_sel of the device draw is checked against the torch path's probabilities before the timing.  Parts (b) and (c) run
each mode twice, alternating, after one warm-up run of each; the eager and the replayed run of (b) must return the same ids
without guidance (with guidance the ids that differ are counted, between the two modes and between two eager runs)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmada_parallel_amd import LLaDAForMultiModalGeneration, abi, synth  # noqa: E402
from mmada_parallel_amd.generators.image_generation_generator import _gumbel, generate_image  # noqa: E402
from mmada_parallel_amd.generators.mmu_generator import mmu_generate  # noqa: E402


def peak_added(fn, dev):
    """Bytes torch's allocator holds at its peak while fn() runs, above what it held before."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def image_step(args, dev, lines):
    seed = 20261020
    lib = abi.lib()
    cfg = abi.MmadaCfg(d_model=256, n_layers=1, n_heads=2, n_kv_heads=2, head_dim=128, mlp_hidden=512, vocab=134656, max_seq=1024,
                       rms_eps=1e-5, rope_theta=500000.0, tp_rank=0, tp_size=1, mask_token_id=synth.MASK,
                       text_vocab_size=synth.TEXT_VOCAB, codebook_size=synth.CODEBOOK, reserved=0)
    h = C.c_void_p()
    abi.check(lib.mmada_create(C.byref(cfg), None, C.byref(h)), "mmada_create")   # the sampler entry points only read its cfg
    CB, N, cfg_scale, temp, keep_v, off = synth.CODEBOOK, 1024, 3.5, 1.0, 400, synth.TEXT_VOCAB
    L = N + 64
    g = torch.Generator().manual_seed(6)
    cond = (torch.randn(N, CB, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    unc = (cond.float().cpu() + torch.randn(N, CB, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    pos = torch.arange(32, 32 + N, dtype=torch.int32, device=dev)
    ids0 = torch.randint(0, 1000, (1, L), generator=g).to(dev)
    ids0[:, 32:32 + N] = synth.MASK
    ids = ids0.clone()
    masked = torch.ones(N, dtype=torch.bool, device=dev)       # what the torch path computed before the head ran
    keep = torch.tensor([keep_v], dtype=torch.int32, device=dev)
    argmax = torch.empty((1, N), dtype=torch.int32, device=dev)
    pmax = torch.empty((1, N), dtype=torch.bfloat16, device=dev)
    counter = torch.full((1,), 1 << 62, dtype=torch.int64, device=dev)
    sampled = torch.empty((1, N), dtype=torch.int32, device=dev)
    p_sel = torch.empty((1, N), dtype=torch.bfloat16, device=dev)
    probs = torch.empty((N, CB), dtype=torch.bfloat16, device=dev)

    def run_a():   # generators/image_generation_generator.py, the torch path after the head, all N slots unknown
        ids.copy_(ids0)
        st = abi.stream_ptr()
        abi.check(lib.mmada_image_probs_m(h, cond.data_ptr(), unc.data_ptr(), 1, N, CB, cfg_scale, probs.data_ptr(), argmax.data_ptr(),
                                          pmax.data_ptr(), st), "mmada_image_probs_m")
        logits = (1 + cfg_scale) * cond - cfg_scale * unc
        gum = _gumbel(torch.rand(logits.shape, dtype=logits.dtype, device=dev))
        s = (logits / temp + gum).argmax(dim=-1)
        conf = probs.gather(-1, s.unsqueeze(-1)).squeeze(-1)
        gm = _gumbel(torch.rand((1, N), dtype=torch.bfloat16, device=dev))
        s_full = torch.zeros((1, N), dtype=torch.int32, device=dev)
        p_full = torch.zeros((1, N), dtype=torch.bfloat16, device=dev)
        g_full = torch.zeros((1, N), dtype=torch.bfloat16, device=dev)
        s_full[0, masked] = s.to(torch.int32)
        p_full[0, masked] = conf
        g_full[0, masked] = gm[0]
        abi.check(lib.mmada_image_commit_g(h, ids.data_ptr(), 1, L, pos.data_ptr(), N, s_full.data_ptr(), p_full.data_ptr(),
                                           g_full.data_ptr(), temp, keep.data_ptr(), off, st), "mmada_image_commit_g")

    def run_b():
        ids.copy_(ids0)
        st = abi.stream_ptr()
        abi.check(lib.mmada_image_sample_g(h, cond.data_ptr(), unc.data_ptr(), 1, N, CB, cfg_scale, temp, off, seed, counter.data_ptr(),
                                           sampled.data_ptr(), p_sel.data_ptr(), None, None, st), "mmada_image_sample_g")
        abi.check(lib.mmada_image_commit_g_sampled(h, ids.data_ptr(), 1, L, pos.data_ptr(), N, sampled.data_ptr(), p_sel.data_ptr(), temp,
                                                   seed, counter.data_ptr(), keep.data_ptr(), off, st), "mmada_image_commit_g_sampled")

    fns = {"a": run_a, "b": run_b}
    run_a()
    run_b()
    torch.cuda.synchronize()
    assert torch.equal(p_sel.view(torch.int16), probs.gather(-1, sampled.view(N, 1).long()).view(1, N).view(torch.int16))
    for f in fns.values():   # warm-up of every timed shape
        f()
    torch.cuda.synchronize()
    probs = None             # (a)'s peak counts its probabilities too

    def run_a_alloc():
        nonlocal probs
        probs = torch.empty((N, CB), dtype=torch.bfloat16, device=dev)
        run_a()

    mem_a = peak_added(run_a_alloc, dev)
    mem_b = peak_added(run_b, dev)
    times = {n: [] for n in fns}
    order = ["a", "b"]
    for r in range(args.rounds):
        for n in order[r % 2:] + order[:r % 2]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fns[n]()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) / args.reps)
    med = {n: statistics.median(v) for n, v in times.items()}
    ba = [b / a for a, b in zip(times["a"], times["b"])]
    lines.append(f"(a) generate_image, the sampling of one step after the head: N = {N} slots (all unknown), codebook {CB}, cfg_scale {cfg_scale}, "
                 f"temperature {temp}, keep_n {keep_v}, {args.rounds} rounds x {args.reps} steps, device events, ms per step; p_sel of the "
                 f"device draw bit-identical to mmada_image_probs_m's probability of its token")
    names = {"a": "torch: image_probs_m + combine + rand/logs + argmax + gather + scatters + image_commit_g",
             "b": "device: mmada_image_sample_g + mmada_image_commit_g_sampled"}
    for n in order:
        lines.append(f"  {names[n]:90s} median {med[n]:8.4f}  min {min(times[n]):8.4f}  max {max(times[n]):8.4f}")
    lines.append(f"  device / torch: median of rounds {statistics.median(ba):.4f}  min {min(ba):.4f}  max {max(ba):.4f}")
    lines.append(f"(d) peak memory added by one such step: torch {mem_a / 2**20:.2f} MiB (bf16 probabilities {N * CB * 2 / 2**20:.1f} MiB, the "
                 f"combined logits, the noise and their temporaries);  device {mem_b / 2**20:.3f} MiB")
    lib.mmada_destroy(h)


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps, out


def alternate(modes, run, steps):
    """One warm-up run of each mode, then two timed runs of each, alternating.  Returns ({mode: [ms per step]}, {mode: output})."""
    outs = {m: run(m) for m in modes}
    times = {m: [] for m in modes}
    for r in range(2):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            times[m].append(timed(lambda: run(m), steps)[0])
    return times, outs


def image_job(N=1024, every=32, P=64, U=16):
    g = torch.Generator().manual_seed(3)
    body = []
    for _ in range(N // every):
        body += [synth.MASK] * every + [synth.NEW_LINE]
    prompt = torch.tensor([torch.randint(0, 120000, (P,), generator=g).tolist() + [synth.BOA, synth.BOI] + body + [synth.EOI, synth.EOA]])
    return dict(prompt=prompt, uncon_ids=torch.randint(0, 120000, (1, U), generator=g), code_start=P + 2, seq_len=N, newline_every=every)


def whole_generate_image(args, model, dev, lines):
    job = image_job()
    kw = dict(seq_len=job["seq_len"], newline_every=job["newline_every"], uncon_ids=job["uncon_ids"], code_start=job["code_start"],
              timesteps=args.timesteps, temperature=1.0, cfg_scale=3.5, image_sampler="device", sampler_seed=7)

    def run(graph):
        return generate_image(model, job["prompt"], graph=graph, **kw)

    # bit-identity of the replay is checked where the forward itself repeats: without guidance (one sequence length per step).  With
    # guidance a step alternates two lengths, and at this width a forward's logits depend on what the previous forward of ANOTHER
    # length left in the workspace (two eager runs differ as well), so there the differing ids are counted, not asserted on.
    plain = {graph: generate_image(model, job["prompt"], graph=graph, **dict(kw, cfg_scale=0.0)) for graph in (False, True, False)}
    assert torch.equal(plain[False], plain[True]), "graph replay changed the ids"
    times, outs = alternate([False, True], run, args.timesteps)
    again = run(False)
    diff_replay, diff_eager = int((outs[False] != outs[True]).sum()), int((outs[False] != again).sum())
    mem = {graph: peak_added(lambda: run(graph), dev) for graph in (False, True)}
    mem_torch = peak_added(lambda: generate_image(model, job["prompt"], **dict(kw, image_sampler="torch", sampler_seed=None)), dev)
    L = job["prompt"].shape[1]
    lines.append(f"(b) generate_image(image_sampler='device') at 8B width ({args.layers} blocks, synthetic weights): {job['seq_len']} slots, "
                 f"a cond forward of L = {L} and an uncond forward of L = {L - job['code_start'] + 2 + job['uncon_ids'].shape[1]} per step, "
                 f"{args.timesteps} timesteps, cfg_scale 3.5, temperature 1, wall time per step over the whole call, ms.  Without guidance "
                 f"the two modes return the same ids; with it {diff_replay} of {job['seq_len']} ids differ between the eager and the "
                 f"replayed run and {diff_eager} between two eager runs (the forward does not repeat after a forward of another length)")
    for graph, name in ((False, "eager"), (True, "graph=True")):
        lines.append(f"  {name:12s} runs {', '.join(f'{t:.3f}' for t in times[graph])}  best {min(times[graph]):.3f}")
    lines.append(f"  graph / eager (best of each): {min(times[True]) / min(times[False]):.4f}; nodes of the captured step "
                 f"{model.graph_nodes.get(('generate_image',))}")
    lines.append(f"(d) peak memory added by the call: eager {mem[False] / 2**20:.1f} MiB, graph=True {mem[True] / 2**20:.1f} MiB, "
                 f"image_sampler='torch' {mem_torch / 2**20:.1f} MiB")


def whole_mmu(args, model, dev, lines):
    P, new, BL, temp = 1088, 512, 128, 0.7
    idx = torch.randint(0, 120000, (1, P), generator=torch.Generator().manual_seed(4))
    lines.append(f"(c) mmu_generate at 8B width ({args.layers} blocks, synthetic weights): B = 1, P = {P}, max_new_tokens {new} (L = {P + new}), "
                 f"block_length {BL}, {args.mmu_steps} steps, temperature {temp}, wall time per step over the whole call, ms")
    for cfg_scale in (0.0, 1.5):
        def run(sampler):
            return mmu_generate(model, idx, max_new_tokens=new, steps=args.mmu_steps, block_length=BL, temperature=temp, cfg_scale=cfg_scale,
                                text_sampler=sampler, sampler_seed=7 if sampler == "device" else None)

        times, _ = alternate(["torch", "device"], run, args.mmu_steps)
        mem = {m: peak_added(lambda: run(m), dev) for m in ("torch", "device")}
        lines.append(f"  cfg_scale {cfg_scale} ({'one batch-2 forward' if cfg_scale else 'one forward'} per step)")
        for m in ("torch", "device"):
            lines.append(f"    text_sampler={m!r:9s} runs {', '.join(f'{t:.3f}' for t in times[m])}  best {min(times[m]):.3f};  (d) peak memory added "
                         f"{mem[m] / 2**20:.1f} MiB")
        lines.append(f"    device / torch (best of each): {min(times['device']) / min(times['torch']):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=64, help="image steps per timed window of part (a)")
    ap.add_argument("--layers", type=int, default=32, help="denoiser blocks of the 8B-width model of parts (b), (c) (0: skip them)")
    ap.add_argument("--timesteps", type=int, default=8, help="timesteps of generate_image in part (b)")
    ap.add_argument("--mmu-steps", type=int, default=8, help="steps of mmu_generate in part (c), a multiple of 4 (the blocks)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t2i_mmu_sample_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("t2i_mmu_sample_bench: needs a GPU (a CPU run measures nothing)")
    dev = "cuda:0"
    lines = [f"t2i_mmu_sample_bench: {torch.cuda.get_device_name(0)}"]
    image_step(args, dev, lines)
    if args.layers:
        cfg = dict(synth.CFG_8B, n_layers=args.layers)
        sd = synth.synthetic_state_dict(cfg, seed=0, device=dev)
        model = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, max_batch=2)
        del sd
        whole_generate_image(args, model, dev, lines)
        whole_mmu(args, model, dev, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
