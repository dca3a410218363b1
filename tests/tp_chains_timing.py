"""The timed half of tests/test_gpu_tp_chains.py: forwards of rank 0 of a tiny TP = 2 group in mode 3 (no exchange) and mode 5
(emulated link) between device events, the comm created under MMADA_TP_CHUNKS = 1, 2, 4 and 8.  Run as a program it measures in a
process of its own — for the reason tests/tp_emulate_timing.py records — and prints one JSON line.

Also the home of group_with(), the group builder of the chain tests (any rank count, configuration and transport)."""
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest  # noqa: F401  (GPU_MAX_HW_QUEUES before the runtime starts, as for the tests)

import torch

from helpers import tiny_sd, tp_group
from mmada_parallel_amd import abi, synth, tp as tp_plan
from mmada_parallel_amd.tp_link import MODE_EMULATE, MODE_NO_EXCHANGE, emulate_mbps_in_use, set_emulate_mbps
from tp_emulate_timing import D, DEV, NL, TP, WAIT_NS, timed_forwards

# The shape of the timing test, picked by measurement on an MI355X (tests/test_gpu_tp_chains.py records the figures): 256
# sequences of 128 tokens of the tiny model, 32 768 stream rows — a chain of a quarter of them is 8 192 rows, whose kernels last
# well above their dispatch.
SEQS, LEN = 256, 128
COUNTS = (1, 2, 4, 8)


def chain_ids(seqs=SEQS, length=LEN):
    return ((torch.arange(seqs * length, device=DEV) * 7 + 3) % 1000).view(seqs, length)


def group_with(chunks, tp=TP, rows=0, cfg=None, sd=None, transport="pull"):
    """A connected group whose comms were created under MMADA_TP_CHUNKS=chunks (the library reads it at mmada_comm_create)."""
    before = os.environ.get("MMADA_TP_CHUNKS")
    os.environ["MMADA_TP_CHUNKS"] = str(chunks)
    try:
        return tp_group(cfg or synth.CFG_TINY, sd if sd is not None else tiny_sd(), tp, rows, transport=transport)
    finally:
        if before is None:
            del os.environ["MMADA_TP_CHUNKS"]
        else:
            os.environ["MMADA_TP_CHUNKS"] = before


def measured(ids, counts=COUNTS):
    """{"mbps", "rows", "batch", "<count>": [t3 reps, t5 reps, requested wait per forward in ms, chunks of the plan]}: everything at
    ONE rate — the rate that makes a wait of the one-chunk forward over `ids` WAIT_NS long."""
    B, L = ids.shape
    Lp = (L + 7) // 8 * 8
    M = B * Lp
    mbps = max(1, round((M + TP - 1) // TP * D * 2 * 1000 / WAIT_NS))
    lib = abi.lib()
    rate = emulate_mbps_in_use()
    out = {"mbps": mbps, "rows": M, "batch": B}
    try:
        set_emulate_mbps(lib, mbps)
        for count in counts:
            ranks, streams = group_with(count, rows=M)
            try:
                assert ranks[0]._link.chunks == count
                t = timed_forwards(ranks[0], streams[0], ids)
                assert ranks[0].comm_status()["error"] == 0
            finally:
                for m in ranks:
                    m.disconnect_tp()
            waits = tp_plan.forward_link_waits_ns(M, D, TP, NL, mbps, count, batch=(B, Lp))
            out[str(count)] = [t[MODE_NO_EXCHANGE], t[MODE_EMULATE], sum(waits) * 1e-6, len(waits) // (4 * NL)]
    finally:
        set_emulate_mbps(lib, rate)
    return out


if __name__ == "__main__":
    shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(SEQS, LEN)]
    result = {f"{b}x{length}": measured(chain_ids(b, length)) for b, length in shapes}
    torch.cuda.synchronize()
    print("TIMINGS " + json.dumps(result), flush=True)
