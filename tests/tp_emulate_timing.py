"""The timed half of tests/test_gpu_tp_emulate.py: forwards of one rank of a tiny TP = 2 group in mode 3 (no exchange) and mode 5
(emulated link) between device events.  Run as a program it measures in a process of its own and prints one JSON line.

Why a process of its own: device-event timings of a 0.2 ms forward need a runtime nothing else has used.  Inside the process that
has run the whole GPU suite, forwards of BOTH modes — mode 3 is code from before mode 5 existed — read 8.5 ms (mode 3) and 10.4 ms
(mode 5) too long in a fixed pattern over the alternating repetitions: mode-3 repetitions 1, 3 and 5 in each of three whole-suite
runs (8.67 - 8.96 ms instead of 0.21 - 0.23 ms), mode-5 repetitions 2 and 4, or 2, in two of them (12.3 - 12.5 ms instead of
1.85 ms) — stalled: m3 . . m5 m3 . . m5 m3 . — while the same code in a fresh process, or behind tests/test_gpu_tp.py alone, never
did (six runs).  A fixed period is no neighbour's doing; what in the long-lived process causes it is not known."""
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest  # noqa: F401  (GPU_MAX_HW_QUEUES before the runtime starts, as for the tests)

import torch

from helpers import tiny_job, tiny_sd, tp_group
from mmada_parallel_amd import abi, synth, tp as tp_plan
from mmada_parallel_amd.tp_link import MODE_EMULATE, MODE_NO_EXCHANGE, emulate_mbps_in_use, set_emulate_mbps

DEV = "cuda:0"
TP = 2
D, NL = synth.CFG_TINY["d_model"], synth.CFG_TINY["n_layers"]
WAIT_NS = 200_000          # what one wait of the one-chunk forward should last in the timing tests


def fixture_ids():
    ids = tiny_job()["input_ids"].repeat(3, 1).to(DEV)
    ids[1, :6] = torch.arange(50, 56, device=DEV)
    ids[2, :4] = torch.arange(7, 11, device=DEV)
    return ids


def many_rows_ids():
    return ((torch.arange(128 * 128, device=DEV) * 7 + 3) % 1000).view(128, 128)


def rows_of(ids):
    B, L = ids.shape
    return B * ((L + 7) // 8 * 8)


def group_with_chunks(chunks, tp=TP, rows=None):
    """A connected pull group whose comms were created under MMADA_TP_CHUNKS=chunks (the library reads it at mmada_comm_create),
    sized for `rows` stream rows (default: the fixture ids')."""
    before = os.environ.get("MMADA_TP_CHUNKS")
    os.environ["MMADA_TP_CHUNKS"] = str(chunks)
    try:
        return tp_group(synth.CFG_TINY, tiny_sd(), tp, rows or rows_of(fixture_ids()))
    finally:
        if before is None:
            del os.environ["MMADA_TP_CHUNKS"]
        else:
            os.environ["MMADA_TP_CHUNKS"] = before


def timed_forwards(m, stream, ids, reps=5):
    """{3: [ms] * reps, 5: [ms] * reps}: one forward_body of rank `m` alone between device events, the two modes alternating.
    A tiny forward is enqueued more slowly than the device runs it, and in mode 5 the host would catch up during the first wait:
    so every timed forward is enqueued while the stream is still busy with a few large GEMMs of the library, and both modes are
    measured device-bound."""
    lib = m._lib
    n = 6144
    a = torch.randn(n, n, device=DEV).to(torch.bfloat16)
    c = torch.empty(n, n, dtype=torch.bfloat16, device=DEV)
    out = {MODE_NO_EXCHANGE: [], MODE_EMULATE: []}
    with torch.cuda.stream(stream):
        for mode in out:                       # warm-up of both modes
            m._set_mode(mode)
            m.forward_body(ids)
        torch.cuda.synchronize()
        for _ in range(reps):
            for mode, ts in out.items():
                m._set_mode(mode)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(6):
                    abi.check(lib.mmada_gemm_bt(a.data_ptr(), a.data_ptr(), c.data_ptr(), n, n, n, abi.stream_ptr()), "gemm")
                e0.record()
                m.forward_body(ids)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
    return out


def measured(ids, chunk_counts):
    """{"mbps", "rows", "1": [t3 reps, t5 reps, requested wait per forward in ms], "2": ...}: everything at ONE rate — the rate that
    makes a wait of the one-chunk forward over `ids` WAIT_NS long."""
    M = rows_of(ids)
    mbps = max(1, round((M + TP - 1) // TP * D * 2 * 1000 / WAIT_NS))
    assert abs(tp_plan.link_wait_ns(M, D, TP, mbps) - WAIT_NS) < 0.02 * WAIT_NS
    lib = abi.lib()
    rate = emulate_mbps_in_use()
    out = {"mbps": mbps, "rows": M}
    try:
        set_emulate_mbps(lib, mbps)
        for chunks in chunk_counts:
            ranks, streams = group_with_chunks(chunks, rows=M)
            try:
                t = timed_forwards(ranks[0], streams[0], ids)
                assert ranks[0].comm_status()["error"] == 0
            finally:
                for m in ranks:
                    m.disconnect_tp()
            want_ms = sum(tp_plan.forward_link_waits_ns(M, D, TP, NL, mbps, chunks)) * 1e-6
            assert abs(want_ms - 4 * NL * WAIT_NS * 1e-6) < 0.02 * want_ms      # 2 blocks x 2 exchanges x 2 phases x 200 us in all
            out[str(chunks)] = [t[MODE_NO_EXCHANGE], t[MODE_EMULATE], want_ms]
    finally:
        set_emulate_mbps(lib, rate)
    return out


if __name__ == "__main__":
    result = {"fixture": measured(fixture_ids(), (1,)), "many_rows": measured(many_rows_ids(), (1, 2))}
    torch.cuda.synchronize()
    print("TIMINGS " + json.dumps(result), flush=True)
