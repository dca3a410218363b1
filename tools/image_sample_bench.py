#!/usr/bin/env python
"""An image step's sampling at temperature > 0 two ways, after the LM head has written the [B*N, 8192] codebook logits, timed with
device events, interleaved in one process on one GPU:

  (a) torch    mmada_image_probs with the [B*N, 8192] bf16 probabilities + torch.multinomial + gather + torch.randn +
               mmada_image_commit (temperature by value): what generate_ti2ti(image_sampler="torch") runs per image step
  (b) device   mmada_image_sample + mmada_image_commit_sampled: the draw and the re-mask noise inside the kernels, no probabilities

    python tools/image_sample_bench.py [--rounds 12] [--reps 64] [--out profiles/image_sample_bench.txt]

at B*N = 1024 and 2048 rows (B sequences of N = 1024 image positions), codebook 8192, cfg_img = 4 with an unconditional image
branch.  Each round times (a) and (b) once, in an order that alternates from round to round; medians and the min-max spread over
the rounds are reported, the per-round ratio (b)/(a), and the peak device memory each adds while it runs (torch's allocator).
The two draw from different random streams (and (b) samples the fp32 soft-max, (a) its bf16 rounding), so their tokens are not
compared; what they share — arg-max and its probability — is checked bit for bit before the timing."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmada_parallel_amd import abi, synth  # noqa: E402


def peak_added(fn, dev):
    """Bytes torch's allocator holds at its peak while fn() runs, above what it held before."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=64, help="image steps per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_sample_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("image_sample_bench: needs a GPU (a CPU run measures nothing)")
    dev, seed = "cuda:0", 20261020
    lib = abi.lib()
    cfg = abi.MmadaCfg(d_model=256, n_layers=1, n_heads=2, n_kv_heads=2, head_dim=128, mlp_hidden=512, vocab=134656, max_seq=1024,
                       rms_eps=1e-5, rope_theta=500000.0, tp_rank=0, tp_size=1, mask_token_id=synth.MASK,
                       text_vocab_size=synth.TEXT_VOCAB, codebook_size=synth.CODEBOOK, reserved=0)
    h = C.c_void_p()
    abi.check(lib.mmada_create(C.byref(cfg), None, C.byref(h)), "mmada_create")   # the sampler entry points only read its cfg
    CB, N, cfg_img, temp, mlen_v = synth.CODEBOOK, 1024, 4.0, 0.6, 400
    lines = [f"image_sample_bench: {torch.cuda.get_device_name(0)}, codebook {CB}, N = {N} image positions per sequence, cfg_img {cfg_img}, "
             f"re-mask temperature {temp}, mask_len {mlen_v}, {args.rounds} rounds x {args.reps} steps, device events, ms per step"]
    for B in (1, 2):
        R, L = B * N, N + 64
        g = torch.Generator().manual_seed(5 + B)
        cond = (torch.randn(R, CB, generator=g) * 1.5).to(torch.bfloat16).to(dev)
        ui = (cond.float().cpu() + torch.randn(R, CB, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        pos = torch.arange(32, 32 + N, dtype=torch.int32, device=dev)
        ids0 = torch.randint(0, 1000, (B, L), generator=g).to(dev)
        ids0[:, 32:32 + N] = synth.MASK
        ids = ids0.clone()
        mlen = torch.tensor([mlen_v], dtype=torch.int32, device=dev)
        argmax = torch.empty((B, N), dtype=torch.int32, device=dev)
        pmax = torch.empty((B, N), dtype=torch.bfloat16, device=dev)
        noise = torch.zeros((B, N), dtype=torch.bfloat16, device=dev)
        counter = torch.full((1,), 1 << 62, dtype=torch.int64, device=dev)
        temp_dev = torch.tensor([temp], dtype=torch.float32, device=dev)
        sampled = torch.empty((B, N), dtype=torch.int32, device=dev)
        p_sel = torch.empty((B, N), dtype=torch.bfloat16, device=dev)
        probs = torch.empty((R, CB), dtype=torch.bfloat16, device=dev)

        def run_a():
            st = abi.stream_ptr()
            abi.check(lib.mmada_image_probs(h, cond.data_ptr(), None, ui.data_ptr(), B, N, CB, 0.0, cfg_img, probs.data_ptr(),
                                            argmax.data_ptr(), pmax.data_ptr(), st), "mmada_image_probs")
            s64 = torch.multinomial(probs, 1)
            p = torch.gather(probs, -1, s64).view(B, N).contiguous()
            s32 = s64.view(B, N).to(torch.int32).contiguous()
            noise.copy_(torch.randn((B, N), dtype=torch.bfloat16, device=dev))
            abi.check(lib.mmada_image_commit(h, ids.data_ptr(), B, L, pos.data_ptr(), N, s32.data_ptr(), p.data_ptr(), noise.data_ptr(),
                                             temp, mlen.data_ptr(), synth.TEXT_VOCAB, CB, st), "mmada_image_commit")

        def run_b():
            st = abi.stream_ptr()
            abi.check(lib.mmada_image_sample(h, cond.data_ptr(), None, ui.data_ptr(), B, N, CB, 0.0, cfg_img, synth.TEXT_VOCAB, seed,
                                             counter.data_ptr(), sampled.data_ptr(), p_sel.data_ptr(), None, None, st), "mmada_image_sample")
            abi.check(lib.mmada_image_commit_sampled(h, ids.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p_sel.data_ptr(),
                                                     temp_dev.data_ptr(), seed, counter.data_ptr(), mlen.data_ptr(), synth.TEXT_VOCAB, CB,
                                                     st), "mmada_image_commit_sampled")

        fns = {"a": run_a, "b": run_b}
        # what the two share is the same bits: arg-max and its probability, and p_sel is (a)'s probability of (b)'s token
        am_b, pm_b = torch.empty_like(argmax), torch.empty_like(pmax)
        run_a()
        abi.check(lib.mmada_image_sample(h, cond.data_ptr(), None, ui.data_ptr(), B, N, CB, 0.0, cfg_img, synth.TEXT_VOCAB, seed,
                                         counter.data_ptr(), sampled.data_ptr(), p_sel.data_ptr(), am_b.data_ptr(), pm_b.data_ptr(),
                                         abi.stream_ptr()), "mmada_image_sample")
        torch.cuda.synchronize()
        assert torch.equal(am_b, argmax) and torch.equal(pm_b.view(torch.int16), pmax.view(torch.int16))
        assert torch.equal(p_sel.view(torch.int16), probs.gather(-1, sampled.view(R, 1).long()).view(B, N).view(torch.int16))
        for f in fns.values():   # warm-up of every timed shape
            f()
        torch.cuda.synchronize()
        probs = None             # (a)'s peak counts its probabilities too

        def run_a_alloc():
            nonlocal probs
            probs = torch.empty((R, CB), dtype=torch.bfloat16, device=dev)
            run_a()

        mem_a, mem_b = peak_added(run_a_alloc, dev), peak_added(run_b, dev)
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
        lines.append(f"B*N = {R} (B = {B}); arg-max, its probability and p_sel of (b) bit-identical to mmada_image_probs")
        names = {"a": "(a) image_probs + multinomial + gather + randn + image_commit", "b": "(b) mmada_image_sample + mmada_image_commit_sampled"}
        for n in order:
            lines.append(f"  {names[n]:62s} median {med[n]:8.4f}  min {min(times[n]):8.4f}  max {max(times[n]):8.4f}")
        lines.append(f"  (b) / (a): median of rounds {statistics.median(ba):.4f}  min {min(ba):.4f}  max {max(ba):.4f}")
        lines.append(f"  peak memory added: (a) {mem_a / 2**20:.2f} MiB of torch tensors (bf16 probabilities {R * CB * 2 / 2**20:.1f} MiB, "
                     f"multinomial's temporaries, the draws);  (b) {mem_b / 2**20:.3f} MiB")
        del probs
    lib.mmada_destroy(h)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
