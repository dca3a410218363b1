"""The emulated link (mmada_comm_set_mode 5, csrc/tp_comm.hip): the data path of the no-exchange diagnostic (mode 3) plus one timed
wait where each half of an exchange would move bytes.  Exact: mode 5 computes mode 3's bits and leaves no state behind.  Timed: the
waits are really on the forward's dependency chain, and cutting the rows into two chunks never adds to what they cost.

Rank groups are handles of ONE process (helpers.tp_group).  Modes 3 and 5 hand nothing off, so for the timings one rank runs alone;
the timings are taken by tests/tp_emulate_timing.py in a process of its own, once for both timing tests."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import pytest
import torch

from helpers import tiny_sd, tp_each
from mmada_parallel_amd import abi, synth, tp as tp_plan
from mmada_parallel_amd.tp_link import MODE_EMULATE, MODE_NO_EXCHANGE, MODE_PULL, connect_local_group, set_emulate_mbps, emulate_mbps_in_use
from tp_emulate_timing import D, DEV, NL, TP, fixture_ids, group_with_chunks, rows_of

pytestmark = pytest.mark.gpu
os.environ.setdefault("MMADA_TP_TIMEOUT_S", "8")


def set_mode(ranks, mode):
    for m in ranks:
        m._set_mode(mode)


def state_in_mode(ranks, streams, ids):
    """After a forward in mode 3 or 5 on every rank: each rank's normalised buffer as it stands, then — the transport switched back
    to pull, which the parity tap needs and which touches no state — the residual stream gathered from its owners (hidden_state())."""
    tp_each(ranks, streams, lambda m: m.forward_body(ids))
    xn = [m.debug_buffer(0).clone() for m in ranks]
    set_mode(ranks, MODE_PULL)
    hid = tp_each(ranks, streams, lambda m: m.hidden_state())
    return xn, hid


@pytest.mark.parametrize("chunks", [1, 2])
def test_mode_5_computes_the_bits_of_mode_3_and_leaves_no_state(chunks):
    ids = fixture_ids()
    assert len(tp_plan.chunk_slices(rows_of(ids), TP, chunks)) == chunks
    ranks, streams = group_with_chunks(chunks)
    rate = emulate_mbps_in_use()
    try:
        set_emulate_mbps(ranks[0]._lib, 2000)      # waits of some tens of microseconds: long enough to matter, short enough to be quick
        tp_each(ranks, streams, lambda m: m.forward_body(ids))
        pull = tp_each(ranks, streams, lambda m: m.hidden_state())
        assert torch.equal(pull[0], pull[1])
        set_mode(ranks, MODE_NO_EXCHANGE)
        xn3, hid3 = state_in_mode(ranks, streams, ids)
        for m in ranks:
            m.set_transport("emulate")
            assert m.comm_status()["mode"] == "emulate" and m.tp_collective == "pull"
        xn5, hid5 = state_in_mode(ranks, streams, ids)
        for r in range(TP):
            assert torch.equal(hid5[r], hid3[r]), f"rank {r}, {chunks} chunk(s): {int((hid5[r] != hid3[r]).sum())} stream elements differ"
            assert torch.equal(xn5[r], xn3[r]), f"rank {r}, {chunks} chunk(s): the normalised rows differ"
        assert not torch.equal(hid3[0], pull[0]), "the diagnostic's values are those of a rank's own partials, not the sum's"
        # back on pull (state_in_mode left it there): the bits of the pull forward from before
        tp_each(ranks, streams, lambda m: m.forward_body(ids))
        again = tp_each(ranks, streams, lambda m: m.hidden_state())
        for r in range(TP):
            assert torch.equal(again[r], pull[r]), f"rank {r}: the pull forward after the emulation computes other bits"
            status = ranks[r].comm_status()
            assert status["mode"] == "pull" and status["error"] == 0, status
    finally:
        set_emulate_mbps(ranks[0]._lib, rate)
        for m in ranks:
            m.disconnect_tp()


def test_mode_5_on_a_single_rank_group_equals_mode_3():
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    lib = abi.lib()
    ids = fixture_ids()
    m = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(synth.CFG_TINY), tiny_sd(), device=DEV, tp_rank=0, tp_size=1)
    abi.check(lib.mmada_set_option(b"tp_allow_single_rank", 1), "set_option")
    rate = emulate_mbps_in_use()
    try:
        set_emulate_mbps(lib, 2000)
        connect_local_group([m], rows_of(ids))
        m.forward_body(ids)
        pull = m.hidden_state().clone()
        got = {}
        for mode in (MODE_NO_EXCHANGE, MODE_EMULATE):
            m._set_mode(mode)
            m.forward_body(ids)
            xn = m.debug_buffer(0).clone()
            m._set_mode(MODE_PULL)
            got[mode] = (xn, m.hidden_state().clone())
        assert torch.equal(got[MODE_EMULATE][0], got[MODE_NO_EXCHANGE][0]) and torch.equal(got[MODE_EMULATE][1], got[MODE_NO_EXCHANGE][1])
        assert torch.equal(got[MODE_EMULATE][1], pull), "one rank: its own partial is the whole sum"
        assert m.comm_status()["error"] == 0
    finally:
        set_emulate_mbps(lib, rate)
        lib.mmada_set_option(b"tp_allow_single_rank", 0)
        m.disconnect_tp()


# ---- timing -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def timings():
    """What tests/tp_emulate_timing.py measures, in a process of its own (its docstring says why), once for both timing tests:
    {"fixture": ..., "many_rows": ...}, each {"mbps", "rows", "<chunks>": [t3 reps, t5 reps, requested wait in ms]}."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tp_emulate_timing.py")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [script]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("TIMINGS ")]
    assert p.returncode == 0 and len(lines) == 1, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    return json.loads(lines[0][len("TIMINGS "):])


def exposed(timings, chunks):
    t3, t5, want = timings[str(chunks)]
    return statistics.median(t5) - statistics.median(t3), want


def test_the_waits_are_on_the_one_chunk_forwards_dependency_chain(timings):
    """One chunk: GEMM -> exchange -> GEMM is a single chain, every wait lies on it, so the forward grows by at least the summed
    requested waits.  0.98: the event timer and the device's wall clock are different clock domains.  On the fixture ids (216 rows):
    the compute between the waits is a few microseconds per kernel, so nothing but the waits separates the two modes.
    Measured on an MI355X: ratio 1.010 - 1.012 in four runs (an excess of 16 - 19 us: 2.2 us of dispatch per wait kernel)."""
    timings = timings["fixture"]
    t3, t5, want = timings["1"]
    got, _ = exposed(timings, 1)
    print(f"one chunk, {timings['rows']} rows at {timings['mbps']} MB/s: mode 3 {t3} ms, mode 5 {t5} ms; t5 - t3 = {got:.4f} ms for "
          f"{want:.4f} ms of requested waits: ratio {got / want:.4f}, excess {1e3 * (got - want):.1f} us, f = {got / want:.3f}")
    assert len(t3) == 5 and len(t5) == 5 and timings["rows"] == rows_of(fixture_ids())
    assert got >= 0.98 * want


def test_two_chunks_never_add_to_the_exposed_time(timings):
    """The same rate, the rows cut in two: twice as many waits of half the length on the one exchange stream — the same link time in
    all — and the second chunk's GEMM free to run under the first chunk's exchange.  What the forward grows by may shrink or stay,
    never grow, beyond the run-to-run spread (max - min of the five mode-3 repetitions of the two-chunk forward).

    The shape: the statement is about transfer time hidden under a chunk's GEMMs, so it needs GEMMs whose time grows with their rows.
    On the 216 rows of the fixture ids every kernel lasts as long as its dispatch whatever its rows: halving the rows hides nothing,
    and the eight extra wait kernels cost their 2.2 us of dispatch each (measured there: two chunks expose 10 - 18 us MORE, against
    a spread of 9 - 25 us — a coin toss, and no defect: a real transfer kernel pays the same dispatch).  128 sequences of 128
    tokens, 16 384 rows of the same tiny model, is where a kernel lasts about 40 us (1.04 ms per mode-3 forward of 26 kernels):
    ten times what the extra launches cost.  Measured there: two chunks expose 57 and 64 us LESS than one (spread 87 and 163 us);
    at 32 768 rows 151 - 206 us less."""
    timings = timings["many_rows"]
    one, want1 = exposed(timings, 1)
    two, want2 = exposed(timings, 2)
    t3 = timings["2"][0]
    spread = max(t3) - min(t3)
    assert abs(want2 - want1) < 1e-3 * want1 and len(t3) == 5 and timings["rows"] == 128 * 128
    print(f"{timings['rows']} rows at {timings['mbps']} MB/s: one chunk exposes {one:.4f} ms (f = {one / want1:.3f}), two chunks "
          f"{two:.4f} ms (f = {two / want2:.3f}); mode-3 spread of the two-chunk forward {1e3 * spread:.1f} us; "
          f"mode 3 {timings['1'][0]} / {t3} ms")
    assert two <= one + spread


def test_exposure_probe_at_an_emulated_rate_reports_f_and_restores_mode_and_rate():
    ids = fixture_ids()
    M = rows_of(ids)
    ranks, _ = group_with_chunks(1)
    m = ranks[0]
    rate = emulate_mbps_in_use()
    try:
        set_emulate_mbps(m._lib, 2000)
        out = m.exchange_exposure_probe(ids, reps=2, emulate_mbps=276)       # one rank alone: modes 3 and 5 hand nothing off
        assert set(out) == {"forward_ms_with_exchange", "forward_ms_no_exchange_diagnostic", "exposed_exchange_ms_per_forward",
                            "exchanges_per_forward", "batch", "what", "emulated_link_mbps", "emulated_wait_ms_per_forward", "exposed_fraction"}
        want_ms = sum(tp_plan.forward_link_waits_ns(M, D, TP, NL, 276, 1)) * 1e-6
        assert out["emulated_link_mbps"] == 276 and out["emulated_wait_ms_per_forward"] == pytest.approx(want_ms, rel=1e-12)
        assert out["exchanges_per_forward"] == 2 * NL and out["batch"] == 3
        assert out["forward_ms_with_exchange"] >= want_ms                    # a synchronised forward cannot end before its waits
        assert out["exposed_fraction"] == pytest.approx(out["exposed_exchange_ms_per_forward"] / want_ms, rel=1e-12)
        print(f"probe: {out}")
        assert m.comm_status()["mode"] == "pull" and m.tp_collective == "pull" and emulate_mbps_in_use() == 2000
    finally:
        set_emulate_mbps(m._lib, rate)
        for r in ranks:
            r.disconnect_tp()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_cap_and_refusals():
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    lib = abi.lib()
    ids = fixture_ids()
    M = rows_of(ids)
    ranks, streams = group_with_chunks(1)
    m = ranks[0]
    rate = emulate_mbps_in_use()
    try:
        with torch.cuda.stream(streams[0]):
            m._set_mode(MODE_NO_EXCHANGE)
            m.forward_body(ids)
            usual = (m.debug_buffer(0).clone(), m._stream_view().clone())
            # 1 MB/s: one wait of ceil(M / 2) * 256 * 2 bytes = that many microseconds, beyond the cap of 20 ms
            assert tp_plan.link_wait_ns(M, D, TP, 1) > tp_plan.LINK_WAIT_CAP_NS
            set_emulate_mbps(lib, 1)
            m._set_mode(MODE_EMULATE)
            with pytest.raises(abi.MmadaError, match=r"exceeds the cap of 20000000 ns \(20 ms\)"):
                m.forward_body(ids)
            assert b"cap" in lib.mmada_last_error()
            w = torch.ones(D, dtype=torch.bfloat16, device=DEV)
            assert lib.mmada_comm_exchange(m._handle, w.data_ptr(), abi.stream_ptr()) != 0 and b"cap" in lib.mmada_last_error()
            # nothing was enqueued: the next mode-3 forward gives its usual bits, no error flag
            m._set_mode(MODE_NO_EXCHANGE)
            m.forward_body(ids)
            torch.cuda.synchronize()
            assert torch.equal(m.debug_buffer(0), usual[0]) and torch.equal(m._stream_view(), usual[1])
            assert m.comm_status()["error"] == 0
            # the scoring head refuses mode 5 in the words it uses for mode 3
            rows = torch.arange(8, dtype=torch.int32, device=DEV)
            words = {}
            set_emulate_mbps(lib, 2000)
            for mode in (MODE_NO_EXCHANGE, MODE_EMULATE):
                m._set_mode(mode)
                m.forward_body(ids)
                with pytest.raises(abi.MmadaError) as err:
                    m.token_logprobs(rows, torch.zeros(8, dtype=torch.long, device=DEV))
                words[mode] = str(err.value)
            assert words[MODE_EMULATE] == words[MODE_NO_EXCHANGE] and "no tensor-parallel transport connected" in words[MODE_EMULATE]
            m._set_mode(MODE_PULL)
        # a comm that was created and never connected takes neither diagnostic
        lone = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(synth.CFG_TINY), tiny_sd(), device=DEV, tp_rank=0, tp_size=TP)
        abi.check(lib.mmada_comm_create(lone._handle, M, None), "mmada_comm_create")
        try:
            for mode in (MODE_NO_EXCHANGE, MODE_EMULATE):
                assert lib.mmada_comm_set_mode(lone._handle, mode) != 0
                assert b"connect a transport" in lib.mmada_last_error()
            assert lib.mmada_comm_set_mode(lone._handle, 6) != 0
        finally:
            lib.mmada_comm_destroy(lone._handle)
    finally:
        set_emulate_mbps(lib, rate)
        for r in ranks:
            r.disconnect_tp()


# ---- graph ------------------------------------------------------------------------------------------------------------------
def test_a_captured_mode_5_forward_replays_mode_3s_bits():
    lib = abi.lib()
    ids = fixture_ids()
    other = (ids + 3) % 1000
    M = rows_of(ids)
    ranks, streams = group_with_chunks(2)
    m = ranks[0]
    rate = emulate_mbps_in_use()
    try:
        if not m.graph_capturable():
            pytest.skip("forward_body is not capturable on this group (graph_capturable())")
        set_emulate_mbps(lib, 2000)
        own = tp_plan.owned_rows(M, 0, TP, 2)

        def state():
            torch.cuda.synchronize()
            x = m._stream_view().view(M, D)
            return m.debug_buffer(0).clone(), torch.cat([x[r0:r1] for r0, r1 in own]).clone()

        with torch.cuda.stream(streams[0]):
            m._set_mode(MODE_NO_EXCHANGE)
            m.forward_body(ids)
            want = state()
            m._set_mode(MODE_EMULATE)
            m.forward_body(ids)                       # eager once: workspace and carve in place before the capture
            abi.check(lib.mmada_graph_begin(abi.stream_ptr()), "graph_begin")
            try:
                m.forward_body(ids)
            except Exception:
                lib.mmada_graph_abort(abi.stream_ptr())
                raise
            gr = C.c_void_p()
            abi.check(lib.mmada_graph_end(abi.stream_ptr(), C.byref(gr)), "graph_end")
            try:
                m._set_mode(MODE_NO_EXCHANGE)
                m.forward_body(other)                 # other values in every buffer the replay writes
                assert not torch.equal(state()[1], want[1])
                for _ in range(2):
                    abi.check(lib.mmada_graph_launch(gr, abi.stream_ptr()), "graph_launch")
                got = state()
            finally:
                lib.mmada_graph_destroy(gr)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert m.comm_status()["error"] == 0
    finally:
        set_emulate_mbps(lib, rate)
        for r in ranks:
            r.disconnect_tp()
