#!/usr/bin/env python
"""The exposed fraction f of the tensor-parallel exchange, MEASURED on one GPU against an emulated link.

Rank 0 of TP = n with the weak-scaling batch of bench.py --gpus n (n jobs of 2438 tokens), 8B-width blocks, alone on one GPU —
the set-up of tools/tp_compute_probe.py — timed per block in
    mode 3  the no-exchange diagnostic: a rank's compute and owner-side kernels, nothing for the transfers;
    mode 5  the emulated link: the same, plus a one-wave timed wait of bytes / rate where each half of every exchange would move
            its bytes (same stream, same dependencies; csrc/tp_comm.hip).
mode 5 - mode 3 is the exchange time the schedule leaves exposed; over the requested wait it is f, the one unmeasured quantity of
the scaling table.  Rates 76 000 and 153 000 MB/s per link and direction, MMADA_TP_CHUNKS 1, 2, 4 and 8 (--chunks): 1 and 2 cut the rows
into chunks around a whole-batch attention, 4 and 8 run the batch's sequences as independent chains (csrc/tp_plan.h chunk_plan_of).
After every rank count a summary compares each count with chunks = 2 OF THE SAME RUN: t3 (the compute-side price of smaller GEMMs
and per-chain attention launches) and t5 (what a forward costs with the link in it).

The emulated link has a FIXED rate and NO contention: no remote-load latency, no hand-off between ranks, no CU taken by a pull
kernel, no link shared between transfers.  f is a property of the schedule on this GPU; it says nothing about what xGMI delivers.

The peers rank 0 is connected to are stand-ins (one tiny block each, tp_rank j of n): mmada_comm_connect_local wants a handle per
rank, and modes 3 and 5 touch no peer memory.  No other mode is ever run on this group.
Timing: device events around ONE forward_body on a side stream, the modes alternating, `reps` repetitions, medians; each timed
forward is enqueued behind a few large GEMMs so that the host's launch rate is not in the figure.
    python tools/tp_emulated_probe.py [--layers 4] [--reps 7] [--tp 2,4,8] [--chunks 1,2,4,8] >> profiles/tp_emulated.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mmada_parallel_amd import LLaDAForMultiModalGeneration, abi, synth, tp as tp_plan  # noqa: E402
from mmada_parallel_amd.tp_link import (MODE_EMULATE, MODE_NO_EXCHANGE, connect_local_group, emulate_mbps_in_use,  # noqa: E402
                                        set_emulate_mbps)

RATES = (76000, 153000)
STAND_IN = dict(d_model=1024, n_heads=8, n_kv_heads=8, n_layers=1, mlp_hidden_size=2048, vocab_size=1024, embedding_size=1024,
                rms_norm_eps=1e-5, rope_theta=500000.0, max_sequence_length=1024)


def rank0_and_stand_ins(cfg, sd, tp, dev):
    """[rank 0 of TP = tp at full width, tp - 1 stand-in peers]"""
    rank0 = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(cfg), sd, device=dev, tp_rank=0, tp_size=tp, max_batch=tp)
    small = synth.synthetic_state_dict(STAND_IN, seed=1, device=dev)
    return [rank0] + [LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(STAND_IN), small, device=dev, tp_rank=j, tp_size=tp)
                      for j in range(1, tp)]


def connect(group, rows, chunks):
    """Connect the group with comms cut into `chunks` row chunks (MMADA_TP_CHUNKS is read by mmada_comm_create) and leave rank 0 in
    mode 3: from here on only modes 3 and 5 run, and the peers' buffers are never addressed."""
    os.environ["MMADA_TP_CHUNKS"] = str(chunks)
    connect_local_group(group, rows)
    group[0]._set_mode(MODE_NO_EXCHANGE)
    return group[0]


def timed(model, ids, stream, mode_rates, reps, blocker):
    """{(mode, mbps): [ms per forward] * reps}, the variants alternating inside every repetition."""
    lib = model._lib
    a, c, n = blocker
    out = {k: [] for k in mode_rates}
    with torch.cuda.stream(stream):
        for mode, mbps in mode_rates:               # warm-up: every variant once
            set_emulate_mbps(lib, mbps)
            model._set_mode(mode)
            model.forward_body(ids)
        torch.cuda.synchronize()
        for _ in range(reps):
            for key in mode_rates:
                set_emulate_mbps(lib, key[1])
                model._set_mode(key[0])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(3):
                    abi.check(lib.mmada_gemm_bt(a.data_ptr(), a.data_ptr(), c.data_ptr(), n, n, n, abi.stream_ptr()), "gemm")
                e0.record()
                model.forward_body(ids)
                e1.record()
                torch.cuda.synchronize()
                out[key].append(e0.elapsed_time(e1))
    return out


def wait_of(waits, layers):
    """ms of requested wait per block"""
    return sum(waits) * 1e-6 / layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tp", default="2,4,8")
    ap.add_argument("--chunks", default="1,2,4,8", help="MMADA_TP_CHUNKS values to create the comms under")
    args = ap.parse_args()
    dev = "cuda:0"
    layers = args.layers
    cfg = dict(synth.CFG_8B, n_layers=layers)
    d = cfg["d_model"]
    job = synth.synthetic_job(512, 512, text_gen_length=256, prompt_len=64, uncond_prompt_len=24, seed=1)
    L = job["input_ids"].shape[1]
    n = 8192
    blocker = (torch.randn(n, n, device=dev).to(torch.bfloat16), torch.empty(n, n, dtype=torch.bfloat16, device=dev), n)
    stream = torch.cuda.Stream(device=dev)
    rate_before = emulate_mbps_in_use()
    print(f"emulated link, rank 0 of TP = n alone, weak-scaling batch B = n, L = {L}, {layers} blocks of 8B width, {args.reps} interleaved "
          f"repetitions (medians); per block: t3 = mode 3, t5 = mode 5, wait = requested, exposed = t5 - t3, f = exposed / wait", flush=True)
    try:
        for tp in (int(t) for t in args.tp.split(",")):
            sd = synth.synthetic_state_dict(cfg, seed=0, device=dev)
            ids = job["input_ids"].repeat(tp, 1).to(dev)
            Lp = (L + 7) // 8 * 8
            M = tp * Lp
            summary = {}
            group = rank0_and_stand_ins(cfg, sd, tp, dev)
            del sd
            for chunks in (int(c) for c in args.chunks.split(",")):
                model = connect(group, M, chunks)
                variants = [(MODE_NO_EXCHANGE, RATES[0])] + [(MODE_EMULATE, r) for r in RATES]
                ts = timed(model, ids, stream, variants, args.reps, blocker)
                assert model.comm_status()["error"] == 0
                t3 = ts[variants[0]]
                m3 = statistics.median(t3) / layers
                for r in RATES:
                    t5 = ts[(MODE_EMULATE, r)]
                    m5 = statistics.median(t5) / layers
                    waits = tp_plan.forward_link_waits_ns(M, d, tp, layers, r, chunks, batch=(tp, Lp))
                    summary[(chunks, r)] = (m3, m5, (m5 - m3) / wait_of(waits, layers))
                    wait = wait_of(waits, layers)
                    print(f"TP={tp} B={tp} chunks={chunks} {r} MB/s: t3 {m3:.3f} ms/block (min {min(t3) / layers:.3f} max {max(t3) / layers:.3f})  "
                          f"t5 {m5:.3f} (min {min(t5) / layers:.3f} max {max(t5) / layers:.3f})  wait {wait:.3f} ({len(waits) // layers} x "
                          f"{max(waits) * 1e-3:.1f} us)  exposed {m5 - m3:.3f}  f = {(m5 - m3) / wait:.3f}", flush=True)
                for m in group:
                    m.disconnect_tp()
            for (chunks, r), (m3, m5, f) in summary.items():   # against chunks = 2 of this run
                if chunks != 2 and (2, r) in summary:
                    b3, b5, bf = summary[(2, r)]
                    print(f"TP={tp} B={tp} {r} MB/s chunks={chunks} against chunks=2: t3 {m3:.3f} / {b3:.3f} = {m3 / b3:.3f}  "
                          f"t5 {m5:.3f} / {b5:.3f} = {m5 / b5:.3f}  f {f:.3f} against {bf:.3f}", flush=True)
            del model, group
            torch.cuda.empty_cache()
    finally:
        set_emulate_mbps(abi.lib(), rate_before)


if __name__ == "__main__":
    main()
