#!/usr/bin/env python
"""Three ways to score R rows against the full vocabulary on the 8B-width head (d = 4096, V = 134 656), timed with device
events, interleaved in one process on one GPU:

  (a) head      mmada_head_rows over the whole vocabulary: [R, V] bf16 logits are written               (no score yet)
  (b) torch     (a) + torch log_softmax(float) + gather on those logits: the only way to score before mmada_head_logprobs
  (c) fused     mmada_head_logprobs: row statistics in the GEMM epilogue + the record-joining kernel; no logits

    python tools/score_bench.py [--rounds 12] [--out profiles/score_bench.txt]

Each round times (a), (b), (c) once, in an order that rotates from round to round; medians and the min-max spread over the
rounds are reported, plus the per-round ratio (c)/(a).  Weights are synthetic (synth.synthetic_state_dict, one block)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmada_parallel_amd import LLaDAForMultiModalGeneration, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg = dict(synth.CFG_8B, n_layers=1)
    sd = synth.synthetic_state_dict(cfg, seed=3, device=dev)
    model = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, max_batch=2)
    del sd
    V = model.vocab
    lines = [f"score_bench: {torch.cuda.get_device_name(0)}, d = {cfg['d_model']}, V = {V}, {args.rounds} rounds x {args.reps} calls, "
             "device events, ms per call"]
    for B in (1, 2):
        L = 2438
        R = B * L
        g = torch.Generator().manual_seed(5 + B)
        ids = torch.randint(0, 126000, (B, L), generator=g).to(dev)
        targets = torch.randint(0, V, (R,), generator=g).to(dev)
        rows = torch.arange(R, dtype=torch.int32, device=dev)
        model.forward_body(ids)
        logits = torch.empty((R, V), dtype=torch.bfloat16, device=dev)

        def run_a():
            model.head_rows(rows, 0, V, out=logits)

        def run_b():
            model.head_rows(rows, 0, V, out=logits)
            return torch.log_softmax(logits.float(), -1).gather(1, targets[:, None])[:, 0]

        def run_c():
            return model.token_logprobs(rows, targets)

        fns = {"a": run_a, "b": run_b, "c": run_c}
        # the results agree (faster and different is not faster)
        ref, got = run_b(), run_c()
        torch.cuda.synchronize()
        worst = float((ref - got).abs().max())
        for f in fns.values():   # warm-up of every timed shape
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        order = ["a", "b", "c"]
        for r in range(args.rounds):
            for k in order[r % 3:] + order[:r % 3]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fns[k]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        ratio = [c / a for a, c in zip(times["a"], times["c"])]
        lines.append(f"R = {R} (B = {B}, L = {L}); max |fused - torch| log-probability {worst:.2e}")
        names = {"a": "(a) head_rows, full vocabulary", "b": "(b) (a) + torch log_softmax + gather", "c": "(c) mmada_head_logprobs (fused)"}
        for k in order:
            lines.append(f"  {names[k]:40s} median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}")
        lines.append(f"  (c) / (a): median of rounds {statistics.median(ratio):.4f}  min {min(ratio):.4f}  max {max(ratio):.4f};   "
                     f"(c) / (b): {med['c'] / med['b']:.4f}")
        flops = 2.0 * R * V * cfg["d_model"]
        lines.append(f"  head GEMM {flops / 1e12:.2f} TFLOP: (a) {flops / med['a'] / 1e9:.0f} TFLOP/s, (c) {flops / med['c'] / 1e9:.0f} TFLOP/s "
                     "(whole call over the GEMM's operations)")
        del logits
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
