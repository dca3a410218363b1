"""Host side of the emulated link (mmada_comm_set_mode 5; no GPU): the wait arithmetic of tp.link_wait_ns against values worked out
by hand, the sum over a forward, the mode tables of tp_link, the sampler's refusal, and the "tp_emulate_mbps" switch of a built
library."""
import ctypes as C
import os

import pytest

from mmada_parallel_amd import abi, tp, tp_link
from mmada_parallel_amd import build as lib_build
from mmada_parallel_amd.generators.parallel_generator import check_tp_exchange
from mmada_parallel_amd.model import LLaDAForMultiModalGeneration, _Lane, _Resident


def test_link_wait_ns_against_hand_computed_values():
    # 2440 rows over 8 ranks: ceil(2440 / 8) = 305 rows x 4096 x 2 B = 2 498 560 B; at 76 000 MB/s = 76 000 B/us that is
    # 32.8757... us -> 32 876 ns (rounded up)
    assert 305 * 4096 * 2 == 2_498_560
    assert tp.link_wait_ns(2440, 4096, 8, 76000) == 32_876
    # twice the rate: 2 498 560 000 / 153 000 = 16 330.45... -> 16 331 ns
    assert tp.link_wait_ns(2440, 4096, 8, 153000) == 16_331
    # the weak-scaling batch of TP = 8 (8 x 2440 rows): every link carries 2440 rows = 19 988 480 B -> 263 006.3... -> 263 007 ns
    assert tp.link_wait_ns(8 * 2440, 4096, 8, 76000) == 263_007
    # a slice smaller than tp: 3 rows over 8 ranks still moves one whole row, 256 x 2 = 512 B; at 1 MB/s = 1 B/us: 512 us
    assert tp.link_wait_ns(3, 256, 8, 1) == 512_000
    assert tp.link_wait_ns(1, 256, 2, 1000) == 512           # 512 B at 1000 B/us = 0.512 us exactly
    assert tp.link_wait_ns(0, 256, 2, 1000) == 0
    # tp = 1: every row, 40 x 256 x 2 = 20 480 B at 76 000 MB/s = 269.47... -> 270 ns
    assert tp.link_wait_ns(40, 256, 1, 76000) == 270
    for bad in ((-1, 256, 2, 1), (8, 0, 2, 1), (8, 256, 0, 1), (8, 256, 2, 0)):
        with pytest.raises(ValueError):
            tp.link_wait_ns(*bad)
    assert tp.LINK_WAIT_CAP_NS == 20_000_000 and tp.DEFAULT_EMULATE_MBPS == 76000


def test_forward_link_waits_follow_the_row_chunks():
    # 96 rows, tp = 2: two chunks of 48 rows (tp.chunk_slices), each 24 x 256 x 2 = 12 288 B = 12 288 ns at 1000 MB/s; two phases per
    # chunk, two exchanges per block, two blocks: 16 waits
    assert [(m0, m1) for m0, m1, _ in tp.chunk_slices(96, 2, 2)] == [(0, 48), (48, 96)]
    assert tp.forward_link_waits_ns(96, 256, 2, 2, 1000, n_chunks=2) == [12_288] * 16
    # one chunk: 48 x 256 x 2 = 24 576 ns, 8 waits — the same bytes in all
    assert tp.forward_link_waits_ns(96, 256, 2, 2, 1000, n_chunks=1) == [24_576] * 8
    # 40 rows are below the two-chunk threshold (4 * 8 * tp = 64) whatever is asked for
    assert tp.forward_link_waits_ns(40, 256, 2, 1, 1000, n_chunks=2) == [20 * 512] * 4
    # an uneven cut: 104 rows, tp = 2: first chunk ceil(52 / 16) * 16 = 64 rows, second 40
    assert tp.forward_link_waits_ns(104, 256, 2, 1, 1000, n_chunks=2) == [32 * 512, 32 * 512, 20 * 512, 20 * 512] * 2


def test_mode_tables_name_the_emulated_link():
    assert tp_link.MODE_EMULATE == 5
    assert tp_link.DIAGNOSTIC_NAMES == {5: "emulate"} and tp_link.DIAGNOSTIC_OF == {"emulate": 5}
    assert tp_link.mode_name(5) == "emulate" and tp_link.mode_of("emulate") == 5
    # the five modes that were there keep their names, through the same two functions
    for mode, name in ((0, "none"), (1, "pull"), (2, "rccl"), (3, "no-exchange diagnostic"), (4, "copy")):
        assert tp_link.mode_name(mode) == name and tp_link.mode_of(name) == mode
    assert not set(tp_link.DIAGNOSTIC_NAMES) & set(tp_link.MODE_NAMES) and not set(tp_link.DIAGNOSTIC_OF) & set(tp_link.MODE_OF)
    with pytest.raises(KeyError):
        tp_link.mode_name(6)
    with pytest.raises(KeyError):
        tp_link.mode_of("emulated")


class StatusLib:
    """mmada_comm_status of a library whose comm is in `mode`, and a recorder of mmada_comm_set_mode."""

    def __init__(self, mode):
        self.mode, self.calls = mode, []

    def mmada_comm_status(self, handle, mode, err, fine, stream):
        mode._obj.value, err._obj.value, fine._obj.value = self.mode, 0, 1
        return 0

    def mmada_comm_set_mode(self, handle, mode):
        self.calls.append(("set_mode", mode))
        self.mode = mode
        return 0


def bare_model(lib):
    m = object.__new__(LLaDAForMultiModalGeneration)   # the constructor needs a GPU
    m._lib, m._handle = lib, C.c_void_p()
    m._lanes, m._resident, m._link = [_Lane(m._handle)], _Resident(), tp_link.TpLink(connected=True, rows=64, transport="pull")
    return m


def test_the_sampler_refuses_the_emulated_link_and_set_transport_reaches_it(monkeypatch):
    monkeypatch.setattr(abi, "stream_ptr", lambda: 0)
    m = bare_model(StatusLib(tp_link.MODE_PULL))
    check_tp_exchange(m)
    m.set_transport("emulate")
    assert m._lib.calls == [("set_mode", 5)]
    assert m.tp_collective == "pull"                     # the record keeps the connected transport under the emulation
    assert m.comm_status() == {"mode": "emulate", "error": 0, "finegrained_counters": True, "finegrained_buffers": False}
    with pytest.raises(abi.MmadaError, match="tokens are void"):
        check_tp_exchange(m)
    m.set_transport(m.tp_collective)
    assert m._lib.calls[-1] == ("set_mode", 1) and m.comm_status()["mode"] == "pull"
    check_tp_exchange(m)


def test_emulated_wait_per_forward_uses_the_chunk_count_the_comm_was_created_with(monkeypatch):
    from types import SimpleNamespace

    m = bare_model(None)
    m.config, m.tp_size = SimpleNamespace(d_model=256, n_layers=2), 2
    assert m._link.chunks == 2
    assert m.emulated_wait_ns_per_forward(1, 93, 1000) == 16 * 12_288          # 93 -> 96 stream rows
    assert m.emulated_wait_ns_per_forward(2, 48, 1000) == 16 * 12_288
    m._link.chunks = 1
    monkeypatch.setenv("MMADA_TP_CHUNKS", "2")                                 # what the environment says LATER does not matter
    assert m.emulated_wait_ns_per_forward(1, 93, 1000) == 8 * 24_576
    # the record takes the count at the moment the comm is created, as the library does
    for env, chunks in (("2", 2), ("1", 1), ("0", 1), ("3", 2)):
        monkeypatch.setenv("MMADA_TP_CHUNKS", env)
        assert tp_link._chunks_at_create() == chunks
    monkeypatch.delenv("MMADA_TP_CHUNKS")
    assert tp_link._chunks_at_create() == 2 and tp_link.TpLink().chunks == 2


@pytest.mark.skipif(not os.path.exists(lib_build.LIB_PATH), reason="the library is not built")
def test_the_rate_option_is_known_and_refuses_values_below_one():
    lib = abi.lib()
    before = tp_link.emulate_mbps_in_use()
    try:
        abi.check(lib.mmada_set_option(b"tp_emulate_mbps", 153000), "set_option")
        abi.check(lib.mmada_set_option(b"tp_emulate_mbps", 1), "set_option")
        for bad in (0, -1, -76000):
            assert lib.mmada_set_option(b"tp_emulate_mbps", bad) != 0
            assert b"tp_emulate_mbps" in lib.mmada_last_error() and b">= 1" in lib.mmada_last_error()
        tp_link.set_emulate_mbps(lib, 42)
        assert tp_link.emulate_mbps_in_use() == 42
        with pytest.raises(abi.MmadaError):
            tp_link.set_emulate_mbps(lib, 0)
        assert tp_link.emulate_mbps_in_use() == 42          # a refused value is not recorded
    finally:
        tp_link.set_emulate_mbps(lib, before)
