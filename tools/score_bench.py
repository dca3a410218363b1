#!/usr/bin/env python
"""Three ways to score R rows against the full vocabulary on the 8B-width head (d = 4096, V = 134 656), timed with device
events, interleaved in one process on one GPU:

  (a) head      mmada_head_rows over the whole vocabulary: [R, V] bf16 logits are written               (no score yet)
  (b) torch     (a) + torch log_softmax(float) + gather on those logits: the only way to score before mmada_head_logprobs
  (c) fused     mmada_head_logprobs: row statistics in the GEMM epilogue + the record-joining kernel; no logits

    python tools/score_bench.py [--rounds 12] [--out profiles/score_bench.txt]

Each round times (a), (b), (c) once, in an order that rotates from round to round; medians and the min-max spread over the
rounds are reported, plus the per-round ratio (c)/(a).  Weights are synthetic (synth.synthetic_state_dict, one block).

    python tools/score_bench.py --tp 2 [--out profiles/score_tp_bench.txt]

--tp k: a FUNCTIONAL rig, not a scaling measurement.  The k ranks of a tensor-parallel group are handles of this process on ONE
device (tp_link.connect_local_group, pull transport): they share its compute units and no link is involved.  Timed, interleaved:

  (c)  fused, one rank     mmada_head_logprobs on a plain TP = 1 model
  (t)  fused, k ranks      the vocabulary-parallel call on every rank of the group, all enqueued before the window closes: the
                           SUMMED device time of the k ranks (k tile-range GEMMs + k hand-offs per round + k joins of every row)
  (h)  one TP rank, torch  head_rows + torch log_softmax + gather on rank 0 of the group (what a TP rank could do before)

(t) / (c) is what the split and the k joins cost on top of the one-rank call; on k devices each rank's share runs in parallel.

    python tools/score_bench.py --tp 2 --topk 8 | --sample [--out profiles/heads_tp_bench.txt]

--tp k with --topk K or --sample: the same rig and the same three rows for the vocabulary-parallel top-k head (top_logprobs) or
draw (sample_tokens at temperature 0.7): (c) the one-rank call, (t) the call on every rank of the group, (h) head_rows on one
rank + torch.topk / logsumexp, or + the generator's add_gumbel_noise and an arg-max.  The lines are APPENDED to --out.

    python tools/score_bench.py --topk 8 [--out profiles/topk_bench.txt]

--topk K: the K likeliest columns of every row and the row's lse, three ways, timed the same way (interleaved, device events):

  (a) torch     mmada_head_rows over the whole vocabulary + torch.topk(K) + torch.logsumexp on those logits (as fp32)
  (c) fused     mmada_head_logprobs: the plain row-statistics head (one target per row, no top-k) — what (d) adds its work to
  (d) top-k     mmada_head_topk: the same GEMM whose epilogue also keeps every tile's eight best + the key-joining kernel

and the peak device memory (a) and (d) add while they run (torch's allocator; for (d) plus the library's record buffer).

    python tools/score_bench.py --sample [--out profiles/sample_bench.txt]

--sample: a text step's draw at text_temperature 0.7 over R = 256 and R = 1024 rows, three ways, timed the same way:

  (a) torch     mmada_head_rows over the whole vocabulary + the generator's add_gumbel_noise (a second [R, V] tensor and five
                elementwise passes) + mmada_text_select: what generate_ti2ti(text_sampler="torch") runs per text step
  (b) fused     mmada_head_logprobs: the plain row-statistics head — what (c) adds its work to
  (c) sample    mmada_head_sample: the same GEMM whose epilogue also draws (Philox4x32-10, two logarithms per logit)

and the peak device memory (a) adds while it runs against the record buffer (c) works in."""
import argparse
import os
import statistics
import sys

if not os.environ.get("GPU_MAX_HW_QUEUES", "").isdigit() or int(os.environ["GPU_MAX_HW_QUEUES"]) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"   # --tp: every rank's compute and exchange stream needs a hardware queue of its own

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mmada_parallel_amd import LLaDAForMultiModalGeneration, synth  # noqa: E402


def tp_rig(cfg, sd, k, max_rows, dev):
    """The k ranks of a tensor-parallel group as handles of this process, one stream each, pull transport."""
    from mmada_parallel_amd.tp_link import connect_local_group

    ranks = [LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, tp_rank=r, tp_size=k, max_batch=2)
             for r in range(k)]
    return connect_local_group(ranks, max_rows), [torch.cuda.Stream(device=dev) for _ in range(k)]


def on_every_rank(ranks, streams, fn):
    """fn(rank) enqueued on every rank's stream, joined to the current stream; no host synchronisation."""
    cur = torch.cuda.current_stream()
    out = []
    for m, s in zip(ranks, streams):
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            out.append(fn(m))
    for s in streams:
        cur.wait_stream(s)
    return out


def main_tp(args):
    dev, k = "cuda:0", args.tp
    cfg = dict(synth.CFG_8B, n_layers=1)
    sd = synth.synthetic_state_dict(cfg, seed=3, device=dev)
    L = 2438
    plain = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, max_batch=2)
    ranks, streams = tp_rig(cfg, sd, k, 2 * ((L + 7) // 8 * 8), dev)
    del sd
    V = plain.vocab
    head = f"top-k {args.topk}" if args.topk else "sample (T = 0.7)" if args.sample else "score"
    lines = [f"score_bench --tp {k} [{head}]: FUNCTIONAL RIG: {k} ranks as handles of one process on ONE {torch.cuda.get_device_name(0)} (pull transport, "
             f"no link involved); d = {cfg['d_model']}, V = {V}, {args.rounds} rounds x {args.reps} calls, device events, ms per call"]
    for B in (1, 2):
        R = B * L
        g = torch.Generator().manual_seed(5 + B)
        ids = torch.randint(0, 126000, (B, L), generator=g).to(dev)
        targets = torch.randint(0, V, (R,), generator=g).to(dev)
        rows = torch.arange(R, dtype=torch.int32, device=dev)
        plain.forward_body(ids)
        on_every_rank(ranks, streams, lambda m: m.forward_body(ids))
        torch.cuda.synchronize()
        logits = torch.empty((R, V), dtype=torch.bfloat16, device=dev)

        if args.topk:       # the result compared below: the log-probability of the likeliest column
            from_call = lambda m: m.top_logprobs(rows, args.topk)[1][:, 0]   # noqa: E731

            def run_h():
                ranks[0].head_rows(rows, 0, V, out=logits)
                lf = logits.float()
                return torch.topk(lf, args.topk, dim=1).values[:, 0] - torch.logsumexp(lf, 1)
        elif args.sample:   # the drawn ids (the torch draw is another stream of noise: nothing to compare)
            from mmada_parallel_amd.generators.parallel_generator import add_gumbel_noise

            for m in [plain] + ranks:
                m.sample_counter.zero_()   # (created here, outside the timed windows)
            torch.cuda.synchronize()
            from_call = lambda m: m.sample_tokens(rows, 0.7, seed=1234)[0]   # noqa: E731

            def run_h():
                ranks[0].head_rows(rows, 0, V, out=logits)
                return add_gumbel_noise(logits, temperature=0.7).argmax(1)
        else:
            from_call = lambda m: m.token_logprobs(rows, targets)   # noqa: E731

            def run_h():
                ranks[0].head_rows(rows, 0, V, out=logits)
                return torch.log_softmax(logits.float(), -1).gather(1, targets[:, None])[:, 0]

        def run_c():
            return from_call(plain)

        def run_t():
            return on_every_rank(ranks, streams, from_call)

        fns = {"c": run_c, "t": run_t, "h": run_h}
        got, ref = run_t(), run_h()
        torch.cuda.synchronize()
        assert all(torch.equal(x, got[0]) for x in got), "the ranks disagree"
        if args.sample:
            ref = got[0]
        for m in ranks:
            assert m.comm_status()["error"] == 0, m.comm_status()
        worst = float((ref - got[0]).abs().max())
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        times = {n: [] for n in fns}
        order = ["c", "t", "h"]
        for r in range(args.rounds):
            for n in order[r % 3:] + order[:r % 3]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fns[n]()
                e1.record()
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) / args.reps)
        for m in ranks:
            assert m.comm_status()["error"] == 0, m.comm_status()
        med = {n: statistics.median(v) for n, v in times.items()}
        ratio = [t / c for c, t in zip(times["c"], times["t"])]
        lines.append(f"R = {R} (B = {B}, L = {L}); ranks bit-identical" + ("" if args.sample else
                     f"; max |fused TP - torch on the same rank's logits| log-probability {worst:.2e}"))
        names = {"c": "(c) fused, one rank (TP = 1 model)", "t": f"(t) fused, {k} ranks, summed device time", "h": "(h) one TP rank: head_rows + torch"}
        for n in order:
            lines.append(f"  {names[n]:42s} median {med[n]:8.3f}  min {min(times[n]):8.3f}  max {max(times[n]):8.3f}")
        lines.append(f"  (t) / (c): median of rounds {statistics.median(ratio):.4f}  min {min(ratio):.4f}  max {max(ratio):.4f};   "
                     f"(t) / {k} / (h): {med['t'] / k / med['h']:.4f} (a rank's share against what it could do before)")
        del logits
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.topk or args.sample else "w") as f:
        f.write(text + "\n")


def peak_added(fn, dev):
    """Bytes torch's allocator holds at its peak while fn() runs, above what it held before."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated(dev) - before
    del out
    return grew


def main_topk(args):
    from mmada_parallel_amd import abi

    dev, K = "cuda:0", args.topk
    cfg = dict(synth.CFG_8B, n_layers=1)
    sd = synth.synthetic_state_dict(cfg, seed=3, device=dev)
    model = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, max_batch=2)
    del sd
    V = model.vocab
    lines = [f"score_bench --topk {K}: {torch.cuda.get_device_name(0)}, d = {cfg['d_model']}, V = {V}, {args.rounds} rounds x {args.reps} calls, "
             "device events, ms per call"]
    for B in (1, 2):
        L = 2438
        R = B * L
        g = torch.Generator().manual_seed(5 + B)
        ids = torch.randint(0, 126000, (B, L), generator=g).to(dev)
        targets = torch.randint(0, V, (R,), generator=g).to(dev)
        rows = torch.arange(R, dtype=torch.int32, device=dev)
        model.forward_body(ids)

        def run_a():
            lf = model.head_rows(rows, 0, V).float()
            v, i = torch.topk(lf, K, dim=1)
            return i, v, torch.logsumexp(lf, 1)

        def run_c():
            return model.token_logprobs(rows, targets)

        def run_d():
            return model.top_logprobs(rows, K)

        fns = {"a": run_a, "c": run_c, "d": run_d}
        # the results agree: the same logits, the same lse to fp32 rounding (torch.topk leaves the order of ties to the build)
        (ia, va, la), (idd, lpd, lsd) = run_a(), run_d()
        torch.cuda.synchronize()
        assert float((va - (lpd + lsd[:, None])).abs().max()) < 1e-4   # logprob + lse is the logit again, to fp32 rounding
        same_ids = float((ia == idd).float().mean())
        worst = float((la - lsd).abs().max())
        del ia, va, la, idd, lpd, lsd
        for f in fns.values():   # warm-up of every timed shape
            f()
        torch.cuda.synchronize()
        mem_a, mem_d = peak_added(run_a, dev), peak_added(run_d, dev)
        own = abi.lib().mmada_score_buffer_bytes(model._handle)
        times = {k: [] for k in fns}
        order = ["a", "c", "d"]
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
        da = [d / a for a, d in zip(times["a"], times["d"])]
        dc = [d / c for c, d in zip(times["c"], times["d"])]
        lines.append(f"R = {R} (B = {B}, L = {L}); ids equal to torch.topk's on {100 * same_ids:.3f} % of the entries (ties: torch's order is "
                     f"unspecified); max |lse - torch.logsumexp| {worst:.2e}")
        names = {"a": f"(a) head_rows + torch.topk({K}) + logsumexp", "c": "(c) mmada_head_logprobs (fused, no top-k)", "d": "(d) mmada_head_topk"}
        for k in order:
            lines.append(f"  {names[k]:44s} median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}")
        lines.append(f"  (d) / (a): median of rounds {statistics.median(da):.4f}  min {min(da):.4f}  max {max(da):.4f};   "
                     f"(d) / (c): median of rounds {statistics.median(dc):.4f}  min {min(dc):.4f}  max {max(dc):.4f}")
        lines.append(f"  peak memory added: (a) {mem_a / 2**20:.1f} MiB (bf16 logits {R * V * 2 / 2**20:.1f} MiB + torch's fp32 temporaries);  "
                     f"(d) {mem_d / 2**20:.3f} MiB of torch tensors + {own / 2**20:.1f} MiB record buffer held by the library")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


def main_sample(args):
    from mmada_parallel_amd import abi
    from mmada_parallel_amd.generators.parallel_generator import add_gumbel_noise

    dev, temp, seed = "cuda:0", 0.7, 20261019
    cfg = dict(synth.CFG_8B, n_layers=1)
    sd = synth.synthetic_state_dict(cfg, seed=3, device=dev)
    model = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, max_batch=2)
    del sd
    lib, h, V = abi.lib(), model._handle, model.vocab
    lines = [f"score_bench --sample: {torch.cuda.get_device_name(0)}, d = {cfg['d_model']}, V = {V}, text_temperature {temp}, "
             f"{args.rounds} rounds x {args.reps} calls, device events, ms per call"]
    for R in (256, 1024):
        B, T = 1, R                                  # one sequence whose whole length is the text span, every position masked
        g = torch.Generator().manual_seed(5 + R)
        ids = torch.randint(0, 126000, (B, T), generator=g).to(dev)
        model.forward_body(ids)
        cur = torch.full((B, T), model.MASK_TOKEN, dtype=torch.long, device=dev)
        rows = torch.arange(R, dtype=torch.int32, device=dev)
        targets = torch.randint(0, V, (R,), generator=g).to(dev)
        k = torch.full((B,), 8, dtype=torch.int32, device=dev)
        scratch = torch.empty(B * T * 16, dtype=torch.uint8, device=dev)
        logits = torch.empty((R, V), dtype=torch.bfloat16, device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)

        def run_a():
            model.head_rows(rows, 0, V, out=logits)
            noisy = add_gumbel_noise(logits.view(B, T, V), temperature=temp).contiguous()
            abi.check(lib.mmada_text_select(h, logits.data_ptr(), noisy.data_ptr(), B, T, V, V, cur.data_ptr(), T, 0, k.data_ptr(),
                                            scratch.data_ptr(), abi.stream_ptr()), "mmada_text_select")

        def run_b():
            return model.token_logprobs(rows, targets)

        def run_c():
            return model.sample_tokens(rows, temp, seed=seed, counter=counter)

        fns = {"a": run_a, "b": run_b, "c": run_c}
        # (c) agrees with the scoring head: its log-probabilities are those of its own draws, its lse the same bits
        ids_c, lp_c, lse_c = run_c()
        lp_b, lse_b, _, _ = model.token_logprobs(rows, ids_c.long(), return_stats=True)
        torch.cuda.synchronize()
        assert torch.equal(lp_c, lp_b) and torch.equal(lse_c, lse_b)
        for f in fns.values():   # warm-up of every timed shape
            f()
        torch.cuda.synchronize()
        logits = None            # (a)'s peak counts its logits too
        def run_a_alloc():
            nonlocal logits
            logits = torch.empty((R, V), dtype=torch.bfloat16, device=dev)
            run_a()
        mem_a, mem_c = peak_added(run_a_alloc, dev), peak_added(run_c, dev)
        own = lib.mmada_score_buffer_bytes(h)
        times = {n: [] for n in fns}
        order = ["a", "b", "c"]
        assert args.reps * 8 <= R                    # (a) commits 8 positions per call: a window never runs out of masked ones
        for r in range(args.rounds):
            for n in order[r % 3:] + order[:r % 3]:
                cur.fill_(model.MASK_TOKEN)          # outside the timed window: re-masking is no part of a text step
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fns[n]()
                e1.record()
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) / args.reps)
        med = {n: statistics.median(v) for n, v in times.items()}
        ca = [c / a for a, c in zip(times["a"], times["c"])]
        cb = [c / b for b, c in zip(times["b"], times["c"])]
        lines.append(f"R = {R}; log-probabilities and lse of (c) bit-identical to mmada_head_logprobs on its draws")
        names = {"a": "(a) head_rows + add_gumbel_noise + mmada_text_select", "b": "(b) mmada_head_logprobs (fused, no draw)", "c": "(c) mmada_head_sample"}
        for n in order:
            lines.append(f"  {names[n]:54s} median {med[n]:8.3f}  min {min(times[n]):8.3f}  max {max(times[n]):8.3f}")
        lines.append(f"  (c) / (a): median of rounds {statistics.median(ca):.4f}  min {min(ca):.4f}  max {max(ca):.4f};   "
                     f"(c) / (b): median of rounds {statistics.median(cb):.4f}  min {min(cb):.4f}  max {max(cb):.4f}")
        lines.append(f"  peak memory added: (a) {mem_a / 2**20:.1f} MiB of torch tensors (bf16 logits {R * V * 2 / 2**20:.1f} MiB, the noise and its "
                     f"temporaries);  (c) {mem_c / 2**20:.3f} MiB of torch tensors + {own / 2**20:.2f} MiB record buffer held by the library")
        del logits
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed window")
    ap.add_argument("--tp", type=int, default=0, help="k > 1: the functional tensor-parallel rig (k ranks on one device)")
    ap.add_argument("--topk", type=int, default=0, help="K in 1..8: top-k three ways (torch on the logits, the plain fused head, mmada_head_topk)")
    ap.add_argument("--sample", action="store_true", help="a text step's draw three ways (torch noise on the logits, the plain fused head, "
                                                          "mmada_head_sample)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "heads_tp_bench.txt" if args.tp and (args.topk or args.sample) else
                                "score_tp_bench.txt" if args.tp else "topk_bench.txt" if args.topk else
                                "sample_bench.txt" if args.sample else "score_bench.txt")
    if args.topk and not 1 <= args.topk <= 8:
        ap.error("--topk takes K in 1..8")
    if args.sample and args.topk:
        ap.error("--sample takes no --topk")
    if args.tp:
        if args.tp not in (2, 4, 8):
            ap.error("--tp must be 2, 4 or 8")
        return main_tp(args)
    if args.sample:
        return main_sample(args)
    if args.topk:
        return main_topk(args)
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
