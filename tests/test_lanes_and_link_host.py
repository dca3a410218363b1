"""Host side of the model's activation lanes and of its tensor-parallel link (no GPU): how a batch-major row list is split over the
two lanes of a micro-batched forward (model.lane_calls and the two ways to find the cut), the records behind _shape / _split /
_ws_bytes, and the names of the transport modes (tp_link).  Every expected value is spelled out by hand."""
import ctypes as C

import pytest
import torch

from mmada_parallel_amd import abi, tp_link
from mmada_parallel_amd.generators.parallel_generator import check_tp_exchange
from mmada_parallel_amd.model import LLaDAForMultiModalGeneration, _Lane, _Resident, counted_cut, equal_cut, lane_calls

H = ("lane 0", "lane 1")


def plain(calls):
    return [(h, lo, hi, None if r is None else r.tolist()) for h, lo, hi, r in calls]


# (B, L, B0), batch-major rows with the SAME count per sequence -> cut, lane 0's rows, lane 1's rows counted from its own batch
EQUAL = [
    ((2, 5, 1), [1, 3, 6, 8], 2, [1, 3], [1, 3]),
    ((3, 5, 2), [0, 4, 5, 9, 10, 14], 4, [0, 4, 5, 9], [0, 4]),
    ((4, 8, 2), [2, 3, 7, 10, 11, 15, 18, 19, 23, 26, 27, 31], 6, [2, 3, 7, 10, 11, 15], [2, 3, 7, 10, 11, 15]),
]
# the same with a different count per sequence (what a labelled-row list looks like), including a lane that gets no row
UNEQUAL = [
    ((2, 5, 1), [0, 1, 2, 3, 4, 7], 5, [0, 1, 2, 3, 4], [2]),
    ((3, 5, 2), [0, 1, 2, 3, 4, 5, 8, 10, 13], 7, [0, 1, 2, 3, 4, 5, 8], [0, 3]),
    ((4, 8, 2), [1, 9, 12, 15, 16, 24, 25, 31], 4, [1, 9, 12, 15], [0, 8, 9, 15]),
    ((3, 5, 2), [2, 7, 9], 3, [2, 7, 9], []),
    ((4, 8, 2), [17, 30], 0, [], [1, 14]),
]


@pytest.mark.parametrize("shape,rows,cut,rows0,rows1", EQUAL)
def test_equal_counts_split_by_arithmetic(shape, rows, cut, rows0, rows1):
    B, L, B0 = shape
    t = torch.tensor(rows, dtype=torch.int32)
    assert equal_cut(len(rows), B, B0) == cut          # head_rows: host integers only
    assert counted_cut(t, B0 * L) == cut               # token_logprobs counts and finds the same place
    assert plain(lane_calls(H, len(rows), cut, t, B0 * L)) == [("lane 0", 0, cut, rows0), ("lane 1", cut, len(rows), rows1)]


@pytest.mark.parametrize("shape,rows,cut,rows0,rows1", UNEQUAL)
def test_unequal_counts_split_by_counting(shape, rows, cut, rows0, rows1):
    B, L, B0 = shape
    t = torch.tensor(rows, dtype=torch.int32)
    assert counted_cut(t, B0 * L) == cut
    calls = lane_calls(H, len(rows), cut, t, B0 * L)
    assert plain(calls) == [("lane 0", 0, cut, rows0), ("lane 1", cut, len(rows), rows1)]
    assert all(r.dtype == torch.int32 and r.is_contiguous() for _, _, _, r in calls)


def test_refusals():
    with pytest.raises(ValueError, match="batch-major"):
        counted_cut(torch.tensor([12, 0, 3], dtype=torch.int32), 2 * 5)      # (3, 5, 2): a row of lane 1 in front
    with pytest.raises(ValueError, match="batch-major"):
        counted_cut(torch.tensor([0, 9, 8, 3], dtype=torch.int32), 1 * 8)
    with pytest.raises(ValueError, match="equal row count per batch element"):
        equal_cut(5, 2, 1)
    with pytest.raises(ValueError, match="equal row count per batch element"):
        equal_cut(7, 3, 2)


def test_one_lane_passes_the_rows_through_and_sequences_split_like_rows():
    t = torch.tensor([4, 0, 9], dtype=torch.int32)     # any order: nothing is split
    (h, lo, hi, r), = lane_calls(H, 3, None, t)
    assert (h, lo, hi) == ("lane 0", 0, 3) and r is t, "the single-lane path makes no tensor"
    assert lane_calls(H, 3, 2) == [("lane 0", 0, 2, None), ("lane 1", 2, 3, None)]      # hidden_state: the items are sequences
    assert lane_calls(H, 3, None) == [("lane 0", 0, 3, None)]


def bare_model(lib=None):
    m = object.__new__(LLaDAForMultiModalGeneration)   # the constructor needs a GPU
    m._lib, m._handle = lib, C.c_void_p()
    m._lanes, m._resident, m._link = [_Lane(m._handle)], _Resident(), tp_link.TpLink()
    return m


def test_resident_forward_and_lane_records_behind_the_old_names():
    m = bare_model()
    assert m._shape is None and m._split is None and m._ws_bytes == [0]
    m._resident = _Resident((3, 5), 2, (1, 4))
    assert m._shape == (3, 5) and m._split == 2
    rows = torch.tensor([0, 4, 5, 9, 10, 14], dtype=torch.int32)
    h0 = m._handle
    m._lanes.append(_Lane("clone", ws_bytes=64))
    assert m._ws_bytes == [0, 64] and m._lane_handle(0) is h0 and m._lane_handle(1) == "clone"
    assert plain(m._lane_calls(6, 4, rows)) == [(h0, 0, 4, [0, 4, 5, 9]), ("clone", 4, 6, [0, 4])]
    m._shape = (2, 7)                                   # a caller that drove mmada_embed itself: a plain forward in lane 0
    assert m._resident == _Resident((2, 7), None, None)
    m._split = 1
    assert m._resident == _Resident((2, 7), 1, None)
    assert not m._comm_in_library and m.tp_collective is None and 0 == m._comm_rows
    assert not m.vocab_parallel_head()


def test_mode_names_round_trip_and_match_the_header():
    assert (tp_link.MODE_NONE, tp_link.MODE_PULL, tp_link.MODE_RCCL, tp_link.MODE_NO_EXCHANGE, tp_link.MODE_COPY) == (0, 1, 2, 3, 4)
    assert tp_link.MODE_NAMES == {0: "none", 1: "pull", 2: "rccl", 3: "no-exchange diagnostic", 4: "copy"}
    assert all(tp_link.MODE_OF[name] == mode for mode, name in tp_link.MODE_NAMES.items()) and len(tp_link.MODE_OF) == 5
    assert all(tp_link.MODE_NAMES[mode] == name for name, mode in tp_link.MODE_OF.items())


class StatusLib:
    """mmada_comm_status of a library whose comm is in `mode`, and a recorder of mmada_comm_set_mode / destroy."""

    def __init__(self, mode):
        self.mode, self.calls = mode, []

    def mmada_comm_status(self, handle, mode, err, fine, stream):
        mode._obj.value, err._obj.value, fine._obj.value = self.mode, 0, 1
        return 0

    def mmada_comm_set_mode(self, handle, mode):
        self.calls.append(("set_mode", mode))
        self.mode = mode
        return 0

    def mmada_comm_destroy(self, handle):
        self.calls.append("destroy")
        return 0


@pytest.mark.parametrize("mode,name", [(0, "none"), (1, "pull"), (2, "rccl"), (3, "no-exchange diagnostic"), (4, "copy")])
def test_comm_status_mode_strings(monkeypatch, mode, name):
    monkeypatch.setattr(abi, "stream_ptr", lambda: 0)
    m = bare_model(StatusLib(mode))
    assert m.comm_status() == {"mode": name, "error": 0, "finegrained_counters": True, "finegrained_buffers": False}


def test_the_sampler_refuses_the_no_exchange_diagnostic_by_its_name(monkeypatch):
    monkeypatch.setattr(abi, "stream_ptr", lambda: 0)
    m = bare_model(StatusLib(tp_link.MODE_PULL))
    check_tp_exchange(m)                                 # unconnected: nothing to check
    m._link = tp_link.TpLink(connected=True, rows=64, transport="pull")
    check_tp_exchange(m)
    m._lib.mode = tp_link.MODE_NO_EXCHANGE
    assert m.comm_status()["mode"] == "no-exchange diagnostic"
    with pytest.raises(abi.MmadaError, match="no-exchange diagnostic"):
        check_tp_exchange(m)


def test_set_transport_and_disconnect_keep_the_link_record_in_step():
    m = bare_model(StatusLib(tp_link.MODE_PULL))
    m._link = tp_link.TpLink(connected=True, rows=64, transport="pull")
    m.set_transport("copy")
    assert m._lib.calls == [("set_mode", 4)] and m.tp_collective == "copy" and m._comm_in_library and 64 == m._comm_rows
    m.disconnect_tp()
    assert m._lib.calls[-1] == "destroy" and m._link == tp_link.TpLink()
    assert not m._comm_in_library and m.tp_collective is None and not m.vocab_parallel_head()
