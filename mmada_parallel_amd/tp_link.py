"""The tensor-parallel link of a model: connection, self-test, status and measurement probes of the library's exchange
(csrc/tp_comm.hip), as a mix-in of LLaDAForMultiModalGeneration.  tp.py holds the shard plan as index arithmetic; this module
is the host code that connects ranks.  The link's state lives in ONE record, `model._link`; `model._comm_in_library`,
`model.tp_collective` and `model._comm_rows` are views of it.  Nothing needs to write it from outside: a rank group of one process
is made with connect_local_group(), a group of processes with model.init_tp_comm(), either is ended with model.disconnect_tp().
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch

from . import abi

# the modes of mmada_comm_set_mode / mmada_comm_status (include/mmada_mi355x.h) and what comm_status() calls them
MODE_NONE, MODE_PULL, MODE_RCCL, MODE_NO_EXCHANGE, MODE_COPY = 0, 1, 2, 3, 4
MODE_NAMES = {MODE_NONE: "none", MODE_PULL: "pull", MODE_RCCL: "rccl", MODE_NO_EXCHANGE: "no-exchange diagnostic", MODE_COPY: "copy"}
MODE_OF = {name: mode for mode, name in MODE_NAMES.items()}
# The emulated link: the no-exchange data path with a timed wait where each transfer would sit (timing only, values void).  It has
# tables of its own: MODE_NAMES / MODE_OF are the five modes tests/test_lanes_and_link_host.py pins entry for entry.  mode_name()
# and mode_of() look through both, and comm_status() / set_transport() go through them.
MODE_EMULATE = 5
DIAGNOSTIC_NAMES = {MODE_EMULATE: "emulate"}
DIAGNOSTIC_OF = {name: mode for mode, name in DIAGNOSTIC_NAMES.items()}
HOST_ALL_REDUCE = "host all-reduce (torch.distributed)"
_emulate_mbps = None   # what set_emulate_mbps() last gave the library (the switch is process-wide and has no getter)


def mode_name(mode: int) -> str:
    """What comm_status() calls a mode of mmada_comm_status."""
    return DIAGNOSTIC_NAMES[mode] if mode in DIAGNOSTIC_NAMES else MODE_NAMES[mode]


def mode_of(name: str) -> int:
    """The mode of mmada_comm_set_mode behind a name of comm_status() / set_transport()."""
    return DIAGNOSTIC_OF[name] if name in DIAGNOSTIC_OF else MODE_OF[name]


def emulate_mbps_in_use() -> int:
    """The emulated link's rate in use: the last set_emulate_mbps(), else MMADA_TP_EMULATE_MBPS, else 76000 (as the library)."""
    if _emulate_mbps is not None:
        return _emulate_mbps
    try:
        env = int(os.environ.get("MMADA_TP_EMULATE_MBPS", "0"))
    except ValueError:
        env = 0
    from .tp import DEFAULT_EMULATE_MBPS
    return env if env >= 1 else DEFAULT_EMULATE_MBPS


def set_emulate_mbps(lib, mbps: int) -> None:
    """mmada_set_option("tp_emulate_mbps", mbps): MB/s per link and direction, an integer >= 1 (the library refuses anything else)."""
    global _emulate_mbps
    abi.check(lib.mmada_set_option(b"tp_emulate_mbps", int(mbps)), "mmada_set_option(tp_emulate_mbps)")
    _emulate_mbps = int(mbps)


@dataclass
class TpLink:
    connected: bool = False          # the exchange runs inside the library (model._comm_in_library)
    rows: int = 0                    # stream rows the comm was created for
    transport: Optional[str] = None  # model.tp_collective: "pull" / "copy" / "rccl" / HOST_ALL_REDUCE, None before any connect
    rccl_also: bool = False          # a second, RCCL communicator exists beside a mapped transport (MMADA_TP_PROBE_RCCL)
    chunks: int = 2                  # chunk count the comm was created with: 1, 2, 4 or 8 (MMADA_TP_CHUNKS at mmada_comm_create;
                                     # 4 and 8 run sequence chains where tp.runs_chains says so, else the plan of 2)


def _chunks_at_create() -> int:
    """What mmada_comm_create makes of MMADA_TP_CHUNKS right now: 1, 2 (the default), 4 or 8 (tp.normalise_chunks)."""
    from .tp import normalise_chunks

    try:
        return normalise_chunks(int(os.environ.get("MMADA_TP_CHUNKS", "2")))
    except ValueError:
        return 1   # atoi() of a non-number is 0


def connect_local_group(ranks, max_rows: int, transport: str = "pull", exchange_cus: int = 0):
    """Connect `ranks` — models of THIS process with tp_rank 0..n-1 — into one group whose exchange runs inside the library, sized
    for `max_rows` stream rows (B * L padded to 8).  transport: "pull" (mmada_comm_connect_local), "copy" (the same mapped buffers,
    bytes moved by the copy engines) or, for a one-rank group only, "rccl" (RCCL refuses two ranks on one device).  exchange_cus:
    mmada_comm_set_partition.  No self-test runs and nothing synchronises.  Returns `ranks`."""
    if transport not in ("pull", "copy", "rccl") or (transport == "rccl" and len(ranks) != 1):
        raise ValueError(f"connect_local_group: transport {transport!r} for {len(ranks)} rank(s) of one process")
    lib = ranks[0]._lib
    for m in ranks:
        abi.check(lib.mmada_comm_create(m._handle, max_rows, None), "mmada_comm_create")
        m._link = TpLink(rows=max_rows, chunks=_chunks_at_create())
    arr = (C.c_void_p * len(ranks))(*[m._handle.value for m in ranks])
    for m in ranks:
        if transport == "rccl":
            if not m._connect_rccl():
                raise abi.MmadaError("mmada_comm_connect_rccl failed: " + (lib.mmada_last_error() or b"").decode())
        else:
            abi.check(lib.mmada_comm_connect_local(m._handle, arr), "mmada_comm_connect_local")
        m._link.connected, m._link.transport = True, "rccl" if transport == "rccl" else "pull"
        if transport == "copy":
            m.set_transport("copy")
        if exchange_cus:
            m.set_exchange_partition(exchange_cus)
    return ranks


def _link_field(name):
    """A model attribute that lives in the link record.  Product code only reads it; a test double that skips __init__ or drives the
    C ABI by hand may still assign it, and then gets a record of its own."""
    return property(lambda self: getattr(self._link, name),
                    lambda self, value: setattr(self.__dict__.setdefault("_link", TpLink()), name, value))


class TpLinkMixin:
    """The tensor-parallel side of LLaDAForMultiModalGeneration, whose __init__ sets `_link = TpLink()`.  Uses the model's _lib,
    _handle, config, tp_rank / tp_size, device, _ensure_ws, _stream_view, debug_buffer, forward_body and the _shape setter."""

    connect_local_group = staticmethod(connect_local_group)
    _comm_in_library, _comm_rows, tp_collective = _link_field("connected"), _link_field("rows"), _link_field("transport")

    def _part_view(self, rows: int) -> torch.Tensor:
        """Zero-copy torch view (__cuda_array_interface__) of the library-owned buffer of this rank's partial sums."""
        ptr, d = self._lib.mmada_comm_part_ptr(self._handle), self.config.d_model
        mem = SimpleNamespace(__cuda_array_interface__={"shape": (rows * d,), "typestr": "<u2", "data": (ptr, False), "version": 2})
        return torch.as_tensor(mem, device=self.device).view(torch.bfloat16).view(rows, d)

    def _set_mode(self, mode: int) -> None:
        abi.check(self._lib.mmada_comm_set_mode(self._handle, mode), "mmada_comm_set_mode")

    def set_transport(self, name: str) -> None:
        """Move the forward's exchange to another CONNECTED transport ("pull" <-> "copy" share their mapped buffers), or to
        "emulate": the emulated link on top of whichever transport is connected (timing only, the forward's values are void; the
        rate is set_emulate_mbps).  The link record keeps naming the connected transport under it, so
        set_transport(model.tp_collective) ends the emulation."""
        self._set_mode(mode_of(name))
        if name not in DIAGNOSTIC_OF:
            self._link.transport = name

    def set_exchange_partition(self, exchange_cus: int) -> None:
        """Give the exchange stream `exchange_cus` CUs of its own (0: none) — mmada_comm_set_partition."""
        abi.check(self._lib.mmada_comm_set_partition(self._handle, int(exchange_cus)), "mmada_comm_set_partition")

    def disconnect_tp(self) -> None:
        """End the link made by init_tp_comm() / connect_local_group(): mmada_comm_destroy; the model is unconnected again."""
        self._lib.mmada_comm_destroy(self._handle)
        self._link = TpLink()

    def comm_status(self):
        mode, err, fine = C.c_int(), C.c_int(), C.c_int()
        abi.check(self._lib.mmada_comm_status(self._handle, C.byref(mode), C.byref(err), C.byref(fine), abi.stream_ptr()),
                  "mmada_comm_status")
        return {"mode": mode_name(mode.value), "error": err.value, "finegrained_counters": bool(fine.value & 1),
                "finegrained_buffers": bool(fine.value & 2)}

    def comm_selftest(self, iters: int = 3, L: int = 96, wait: bool = True):
        """`iters` exchanges over a small carve with known partials (different data every round, so a stale cache line
        cannot pass): every row of the all-gathered, normalised result must equal the locally computed expectation bit for
        bit.  Every rank must call it; returns this rank's verdict.  wait=False: only enqueue, and return the comparison's verdict
        as a device tensor — for the ranks of ONE process, where nothing may synchronise before every rank has enqueued."""
        d, tp, r = self.config.d_model, self.tp_size, self.tp_rank
        B = 2
        ids = (torch.arange(B * L, device=self.device).view(B, L) * 7 + 3) % 1000
        Lp = (L + 7) // 8 * 8
        M = B * Lp
        self._ensure_ws(B, L)
        w = torch.ones(d, dtype=torch.bfloat16, device=self.device)
        part = self._part_view(M)
        st = abi.stream_ptr()
        ok = torch.ones((), dtype=torch.bool, device=self.device)
        col = torch.arange(d, device=self.device, dtype=torch.float32)[None, :]
        row = torch.arange(M, device=self.device, dtype=torch.float32)[:, None]
        for it in range(iters):
            abi.check(self._lib.mmada_embed(self._handle, ids.data_ptr(), B, L, st), "mmada_embed")
            self._shape = (B, L)
            x0 = self._stream_view().view(M, d).clone()

            def pat(rank):  # small integers: exact in bf16, different per rank / row / column / round
                return (((row * 3 + col * 5 + rank * 11 + it * 17) % 13) - 6.0) * (rank + 1)

            part.copy_(pat(r).to(torch.bfloat16))
            abi.check(self._lib.mmada_comm_exchange(self._handle, w.data_ptr(), st), "mmada_comm_exchange")
            total = sum(pat(j).to(torch.bfloat16).float() for j in range(tp))
            x_new = (x0.float() + total.to(torch.bfloat16).float()).to(torch.bfloat16)
            want = torch.empty_like(x_new)
            abi.check(self._lib.mmada_rmsnorm(x_new.data_ptr(), w.data_ptr(), want.data_ptr(), M, d,
                                              float(self.config.ref("rms_norm_eps")), st), "mmada_rmsnorm")
            got = self.debug_buffer(0).view(-1, d)[:M]
            ok = ok & (got == want).all()
        return ok if not wait else bool(ok) and self.comm_status()["error"] == 0

    def _connect_rccl(self, broadcast=None) -> bool:
        """The RCCL connect sequence: unique id on rank 0 -> `broadcast(blob)` hands rank 0's to every rank (None: a one-rank
        group) -> mmada_comm_connect_rccl, which leaves the mode at RCCL.  A rank 0 that cannot make the id hands out None, so
        every rank returns False instead of waiting for it."""
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so").encode()
        uid = C.create_string_buffer(128)
        made = self.tp_rank != 0 or self._lib.mmada_comm_unique_id(uid, path) == 0
        blob = uid.raw if made else None
        if broadcast is not None:
            blob = broadcast(blob)
        return blob is not None and self._lib.mmada_comm_connect_rccl(self._handle, blob, path) == 0

    def init_tp_comm(self, max_batch: int, max_len: int, group=None, transport: str = "auto") -> str:
        """Connect the library's tensor-parallel exchange over the ranks of `group` (a torch.distributed group: control
        plane only — handles / unique id are exchanged as objects; the data path never goes through torch).
        transport: "pull" (mapped peer buffers, hipIpc), "copy" (the same mapped buffers, bytes moved by the copy engines),
        "rccl", or "auto" = pull if it connects AND passes the self-test on every rank, else RCCL, else the host-issued
        all-reduce of the segment API.  Returns what is in use.  MMADA_TP_EXCHANGE_CUS=n (a multiple of 8) additionally gives
        the exchange stream n CUs of its own and masks the compute stream to the rest (mmada_comm_set_partition)."""
        import torch.distributed as dist

        lib = self._lib
        rows = max_batch * ((max_len + 7) // 8 * 8)
        nb = lib.mmada_comm_export_bytes()
        buf = C.create_string_buffer(nb)
        exported = lib.mmada_comm_create(self._handle, rows, buf) == 0
        if not exported:
            abi.check(lib.mmada_comm_create(self._handle, rows, None), "mmada_comm_create")
        link = self._link = TpLink(rows=rows, chunks=_chunks_at_create())

        def all_agree(flag: bool) -> bool:
            got = [None] * self.tp_size
            dist.all_gather_object(got, bool(flag), group=group)
            return all(got)

        def broadcast(blob):
            box = [blob]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            return box[0]

        chosen = None
        if transport in ("auto", "pull", "copy"):
            blobs = [None] * self.tp_size
            dist.all_gather_object(blobs, buf.raw if exported else None, group=group)
            ok = exported and all(b is not None for b in blobs)
            if ok:
                ok = lib.mmada_comm_connect_ipc(self._handle, b"".join(blobs)) == 0
            ok = all_agree(ok)
            if ok and transport == "copy":
                ok = all_agree(lib.mmada_comm_set_mode(self._handle, MODE_COPY) == 0)
            if ok:
                link.connected = True
                lib.mmada_comm_set_timeout(self._handle, 3.0)   # a transport that cannot work is abandoned quickly
                ok = all_agree(self.comm_selftest())
                lib.mmada_comm_set_timeout(self._handle, 0.0)   # back to MMADA_TP_TIMEOUT_S; clears a sticky error
            if ok:
                chosen = "copy" if transport == "copy" else "pull"
            elif transport in ("pull", "copy"):
                raise abi.MmadaError("tensor-parallel pull transport failed to connect or failed its self-test: "
                                     + (lib.mmada_last_error() or b"").decode())
        if chosen is None and transport in ("auto", "rccl"):
            # one rank per device: RCCL refuses two ranks on one GPU
            if all_agree(dist.get_backend(group) == "nccl") and all_agree(self._connect_rccl(broadcast)):
                link.connected = True
                if all_agree(self.comm_selftest()):
                    chosen = "rccl"
            if chosen is None and transport == "rccl":
                raise abi.MmadaError("tensor-parallel RCCL transport failed: " + (lib.mmada_last_error() or b"").decode())
        if chosen is None:
            self.disconnect_tp()
            link, chosen = self._link, HOST_ALL_REDUCE
        if chosen in ("pull", "copy") and os.environ.get("MMADA_TP_PROBE_RCCL", "0") == "1":
            # OPT-IN (bench.py sets it): one rank per device over RCCL as well, so that collective_probe() can time BOTH
            # transports.  A production start does not pay a second communicator (init time, memory, one more thing that
            # can fail or hang at start-up).
            if all_agree(dist.get_backend(group) == "nccl"):
                ok = False
                try:
                    ok = self._connect_rccl(broadcast)
                finally:
                    lib.mmada_comm_set_mode(self._handle, MODE_OF[chosen])   # the forward keeps its transport
                link.rccl_also = all_agree(ok)
        link.transport = chosen
        cus = int(os.environ.get("MMADA_TP_EXCHANGE_CUS", "0") or 0)
        if cus and link.connected:
            self.set_exchange_partition(cus)
        return chosen

    def _time_exchanges(self, w: torch.Tensor, iters: int) -> float:
        """ms per exchange in the current mode: 3 warm-up exchanges, synchronise, `iters` timed exchanges, synchronise."""
        def run(n):
            for _ in range(n):
                abi.check(self._lib.mmada_comm_exchange(self._handle, w.data_ptr(), abi.stream_ptr()), "mmada_comm_exchange")
            torch.cuda.synchronize()

        run(3)
        t0 = time.perf_counter()
        run(iters)
        return (time.perf_counter() - t0) / iters * 1e3

    def collective_probe(self, L: int, B: int = 1, iters: int = 10):
        """Outside any timed region: one exchange (reduce-scatter + RMSNorm + all-gather of B*L rows x d bf16) timed alone,
        so a scaling run also records what the fabric delivered for the message size the forward uses."""
        if not self._comm_in_library:
            return None
        ids = torch.zeros((B, L), dtype=torch.long, device=self.device)
        self._ensure_ws(B, L)
        abi.check(self._lib.mmada_embed(self._handle, ids.data_ptr(), B, L, abi.stream_ptr()), "mmada_embed")
        w = torch.ones(self.config.d_model, dtype=torch.bfloat16, device=self.device)
        nbytes = B * ((L + 7) // 8 * 8) * self.config.d_model * 2
        tp, in_use = self.tp_size, self.tp_collective

        def timed():
            ms = self._time_exchanges(w, iters)
            return {"ms": ms, "busbw_GBps": 2.0 * (tp - 1) / tp * nbytes / (ms * 1e-3) / 1e9}

        out = {"transport": in_use, "rows": B * L, "bytes": nbytes, **timed(), "exchanges_per_forward": 2 * self.config.n_layers,
               "status": self.comm_status()}
        # the other data path over the same mapped buffers, for comparison: OPT-IN (MMADA_TP_PROBE_COPY=1) — it exercises a
        # transport the run did not select; a first multi-GPU session should ask for it explicitly
        if in_use in ("pull", "copy") and os.environ.get("MMADA_TP_PROBE_COPY", "0") == "1":
            other = "copy" if in_use == "pull" else "pull"
            # a comparison only: a data path that fails HERE (first contact with real multi-GPU hardware) must not take the
            # benchmark line of the transport in use with it — record the error and go on
            err_in_use = out["status"]["error"]   # what the transport IN USE left behind: recorded above, never erased below
            try:
                self._set_mode(MODE_OF[other])
                out[other] = {**timed(), "error_flag": self.comm_status()["error"]}
                ok = int(out[other]["error_flag"] == 0)
            except Exception as e:   # noqa: BLE001
                out[other] = {"error": str(e)[:300]}
                ok = 0
            finally:
                self._set_mode(MODE_OF[in_use])
                if err_in_use == 0:   # only a flag the COMPARISON raised is cleared; an earlier one stays for bench.py to report
                    self._lib.mmada_comm_set_timeout(self._handle, 0.0)
            # a rank that failed stopped issuing exchanges while its peers went on: agree on the outcome before anything else
            # uses the group (the comparison's figure is only meaningful when every rank completed it)
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                flag = torch.tensor([ok], dtype=torch.int32, device=self.device)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                out[other]["all_ranks_ok"] = bool(int(flag.item()))
        if self._link.rccl_also and in_use in ("pull", "copy"):   # the same exchange over RCCL, for comparison
            self._set_mode(MODE_RCCL)
            try:
                out["rccl"] = timed()
            finally:
                self._set_mode(MODE_OF[in_use])
        return out

    def rccl_nranks(self) -> int:
        """Ranks of the RCCL communicator the LIBRARY created (ncclCommCount), 0 when it holds none."""
        return int(self._lib.mmada_comm_rccl_nranks(self._handle)) if self._link.connected or self._link.rccl_also else 0

    def emulated_wait_ns_per_forward(self, B: int, L: int, mbps: int) -> int:
        """The waits the emulated link is asked for over one forward of a (B, L) batch on this model's group at `mbps`, summed
        (tp.forward_link_waits_ns with the chunks the library cuts for this batch shape: the link record's `chunks`; the emulated
        link is never the RCCL transport, so a count of 4 or 8 means sequence chains once B >= 2)."""
        from . import tp as tp_plan

        Lp = (L + 7) // 8 * 8
        return sum(tp_plan.forward_link_waits_ns(B * Lp, self.config.d_model, self.tp_size, self.config.n_layers, int(mbps),
                                                 self._link.chunks, batch=(B, Lp)))

    def exchange_exposure_probe(self, input_ids: torch.Tensor, reps: int = 3, emulate_mbps: Optional[int] = None):
        """Outside any timed region: wall time of one tensor-parallel forward with its exchanges and of the same forward
        with the library's "no exchange" diagnostic (MODE_NO_EXCHANGE: identical GEMM / attention / owner-side kernels,
        no peer traffic, no hand-off; the values are wrong, only the time is used).  The difference is what the exchanges
        cost the forward AFTER the overlap of its chunk plan: the exposed exchange time.  Every rank must call it.

        emulate_mbps: instead of the real transport, time the EMULATED link at that rate (MODE_EMULATE: a timed wait of bytes /
        rate where each transfer would sit, no peer traffic — so one rank alone can call it).  The result then also holds
        emulated_link_mbps, emulated_wait_ms_per_forward (the sum of the requested waits) and exposed_fraction = exposed ms /
        that sum: the share of a fixed-rate, contention-free link's time the schedule fails to hide.  The mode and the rate in
        use before the call are restored."""
        if not self._comm_in_library or self.tp_size == 1:
            return None
        import torch.distributed as dist

        emulated = emulate_mbps is not None
        real_mode = mode_of(self.comm_status()["mode"]) if emulated else MODE_OF[self.tp_collective]
        mbps_before = emulate_mbps_in_use() if emulated else None

        def timed(mode):
            self._set_mode(mode)
            ts = []
            try:
                for i in range(reps + 1):
                    if dist.is_initialized():
                        dist.barrier()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    self.forward_body(input_ids)
                    torch.cuda.synchronize()
                    if i:   # the first call of a mode is a warm-up
                        ts.append((time.perf_counter() - t0) * 1e3)
            finally:
                self._set_mode(real_mode)
            return sorted(ts)[len(ts) // 2]

        if emulated:
            try:
                set_emulate_mbps(self._lib, emulate_mbps)
                with_x = timed(MODE_EMULATE)
                without = timed(MODE_NO_EXCHANGE)
                with_x2 = timed(MODE_EMULATE)
            finally:
                set_emulate_mbps(self._lib, mbps_before)
            ms = min(with_x, with_x2)
            wait_ms = self.emulated_wait_ns_per_forward(int(input_ids.shape[0]), int(input_ids.shape[1]), emulate_mbps) * 1e-6
            return {"forward_ms_with_exchange": ms, "forward_ms_no_exchange_diagnostic": without,
                    "exposed_exchange_ms_per_forward": ms - without, "exchanges_per_forward": 2 * self.config.n_layers,
                    "batch": int(input_ids.shape[0]), "emulated_link_mbps": int(emulate_mbps),
                    "emulated_wait_ms_per_forward": wait_ms, "exposed_fraction": (ms - without) / wait_ms,
                    "what": "median wall time of a synchronised forward_body, mmada_comm_set_mode(5) (the emulated link: a "
                    "timed wait of bytes / rate where each transfer would sit; fixed rate, no contention) vs mmada_comm_set_mode(3)"}
        with_x = timed(real_mode)
        without = timed(MODE_NO_EXCHANGE)
        with_x2 = timed(real_mode)
        ms = min(with_x, with_x2)
        return {"forward_ms_with_exchange": ms, "forward_ms_no_exchange_diagnostic": without,
                "exposed_exchange_ms_per_forward": ms - without, "exchanges_per_forward": 2 * self.config.n_layers,
                "batch": int(input_ids.shape[0]), "what": "median wall time of a synchronised forward_body, real transport vs "
                "mmada_comm_set_mode(3) (owner-side kernels on the rank's own partials only, no peer traffic)"}

    def vocab_parallel_head(self) -> bool:
        """True when the text step can run on vocabulary slices of the LM head (library transport connected)."""
        return self._comm_in_library and os.environ.get("MMADA_TP_REPLICATED_HEAD") != "1"

    def graph_capturable(self) -> bool:
        """True when forward_body / head_rows issue only stream launches (no host-side collective): the sampler may then
        capture a whole denoise step into one hipGraph (mmada_graph_*)."""
        # RCCL's reduce-scatter / all-gather would be captured on a forked stream; whether every call it makes is
        # capturable has never been exercised with more than one rank, so only the pull transport (plain kernels and
        # device-memory counters) qualifies under tensor parallelism
        return self.tp_size == 1 or (self._comm_in_library and self.tp_collective in ("pull", "copy")
                                     and self._lib.mmada_comm_partition(self._handle) == 0)   # a CU mask does not survive capture
