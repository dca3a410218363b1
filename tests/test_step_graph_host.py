"""generators/step_graph.StepGraphs on the host (no GPU): a stub model, a stub library that records every mmada_graph_* call, and
torch's stream functions replaced by recorders.  Every assertion is on the exact sequence of calls."""
import contextlib

import pytest
import torch

from mmada_parallel_amd import abi
from mmada_parallel_amd.generators.step_graph import StepGraphs

STREAM = 0x5EED   # what the patched abi.stream_ptr returns


class StubLib:
    def __init__(self, log):
        self.log, self.made = log, 0

    def mmada_graph_begin(self, st):
        self.log.append(("begin", st))
        return 0

    def mmada_graph_end(self, st, out):
        self.made += 1
        out._obj.value = 0x1000 + self.made     # the handle of the graph made: 0x1001, 0x1002, ...
        self.log.append(("end", st, out._obj.value))
        return 0

    def mmada_graph_abort(self, st):
        self.log.append(("abort", st))
        return 0

    def mmada_graph_num_nodes(self, g):
        return 10 * (g.value - 0x1000)

    def mmada_graph_launch(self, g, st):
        self.log.append(("launch", g.value, st))
        return 0

    def mmada_graph_destroy(self, g):
        self.log.append(("destroy", g.value))
        return 0


class StubModel:
    device = "stub-device"

    def __init__(self, log, capturable=True):
        self._lib, self._ws_epoch, self.graph_replays, self.graph_nodes, self.capturable = StubLib(log), 3, 0, {}, capturable

    def graph_capturable(self):
        return self.capturable


class StubStream:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_stream(self, other):
        self.log.append(("wait", self.name, other.name))


@pytest.fixture
def log(monkeypatch):
    """The call log; torch.cuda.Stream / stream / current_stream and abi.stream_ptr record into it."""
    log = []

    def stream_ctx(s):
        log.append(("stream", s.name))
        return contextlib.nullcontext()

    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: log.append(("Stream", device)) or StubStream(log, "side"))
    monkeypatch.setattr(torch.cuda, "stream", stream_ctx)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: StubStream(log, "caller"))
    monkeypatch.setattr(abi, "stream_ptr", lambda: STREAM)
    monkeypatch.delenv("MMADA_GRAPH", raising=False)
    return log


def drive(sg, log, keys, nodes_key=lambda k: ("kind", k)):
    for i, k in enumerate(keys):
        sg.step(k, lambda: log.append(("body", i, k)), nodes_key=nodes_key(k))


def test_capture_and_replay(log):
    model = StubModel(log)
    with StepGraphs(model, True, True) as sg:
        assert sg.on and log == [("Stream", "stub-device"), ("wait", "side", "caller")]
        with sg.stream():
            drive(sg, log, "aaababb")
        sg.join()
        inside = list(log)
    A, B = 0x1001, 0x1002
    assert inside[2:] == [
        ("stream", "side"),
        ("body", 0, "a"),                                                                    # first of its kind: eager
        ("begin", STREAM), ("body", 1, "a"), ("end", STREAM, A), ("launch", A, STREAM),      # second: captured, launched once
        ("launch", A, STREAM),                                                               # from then on: its graph
        ("body", 3, "b"),
        ("launch", A, STREAM),
        ("begin", STREAM), ("body", 5, "b"), ("end", STREAM, B), ("launch", B, STREAM),
        ("launch", B, STREAM),
        ("wait", "caller", "side"),
    ]
    assert [e[1] for e in log if e[0] == "body"] == [0, 1, 3, 5]
    assert model.graph_replays == sum(e[0] == "launch" for e in log) == 5
    assert model.graph_nodes == {("kind", "a"): 10, ("kind", "b"): 20}
    assert log[len(inside):] == [("destroy", A), ("destroy", B)], "leaving the block destroys each held graph exactly once"


def test_nodes_are_recorded_under_the_key_itself_when_no_other_is_given(log):
    model = StubModel(log)
    with StepGraphs(model, True, True) as sg:
        drive(sg, log, [(True, False)] * 2 + [False] * 2, nodes_key=lambda k: None)
    assert model.graph_nodes == {(True, False): 10, False: 20}


def test_a_workspace_that_moved_drops_every_graph_before_the_next_step(log):
    model = StubModel(log)
    with StepGraphs(model, True, True) as sg:
        drive(sg, log, "aabb")
        del log[:]
        model._ws_epoch += 1
        drive(sg, log, "aaab")
        moved = list(log)
    A, B, A2 = 0x1001, 0x1002, 0x1003
    assert moved == [
        ("destroy", A), ("destroy", B),                                                      # before anything of the next step
        ("body", 0, "a"),                                                                    # eager again
        ("begin", STREAM), ("body", 1, "a"), ("end", STREAM, A2), ("launch", A2, STREAM),    # recaptured
        ("launch", A2, STREAM),
        ("body", 3, "b"),                                                                    # the other kind starts over too
    ]
    assert log[len(moved):] == [("destroy", A2)]
    assert sum(e == ("destroy", A) for e in log) == sum(e == ("destroy", B) for e in log) == 1


def test_a_body_that_raises_during_capture_aborts_the_capture(log):
    model = StubModel(log)

    def body():
        log.append(("body",))
        if len([e for e in log if e == ("body",)]) == 4:
            raise RuntimeError("in the capture of b")

    with pytest.raises(RuntimeError, match="in the capture of b"):
        with StepGraphs(model, True, True) as sg:
            for k in "aabb":
                sg.step(k, body)
    A = 0x1001
    assert log[2:] == [("body",), ("begin", STREAM), ("body",), ("end", STREAM, A), ("launch", A, STREAM), ("body",),
                       ("begin", STREAM), ("body",), ("abort", STREAM), ("destroy", A)]
    assert model.graph_replays == 1 and model.graph_nodes == {"a": 10}


@pytest.mark.parametrize("graph,eligible,capturable,env", [(False, True, True, "1"), (True, False, True, "1"), (True, True, False, "1"),
                                                           (None, True, True, None), (None, True, True, "0")])
def test_off_only_calls_the_body(log, monkeypatch, graph, eligible, capturable, env):
    if env is not None:
        monkeypatch.setenv("MMADA_GRAPH", env)
    model = StubModel(log, capturable)
    with StepGraphs(model, graph, eligible) as sg:
        assert not sg.on
        with sg.stream():
            drive(sg, log, "aaab")
        sg.join()
        sg.fork()
    assert log == [("body", i, k) for i, k in enumerate("aaab")], "no stream function, no library call"
    assert model.graph_replays == 0 and model.graph_nodes == {}


def test_graph_none_follows_the_environment(log, monkeypatch):
    monkeypatch.setenv("MMADA_GRAPH", "1")
    with StepGraphs(StubModel(log), None, True) as sg:
        assert sg.on
        drive(sg, log, "aa")
    assert [e[0] for e in log] == ["Stream", "wait", "body", "begin", "body", "end", "launch", "destroy"]


def test_fork_and_join_are_the_two_hand_offs(log):
    with StepGraphs(StubModel(log), True, True) as sg:
        del log[:]
        sg.join()
        sg.fork()
    assert log == [("wait", "caller", "side"), ("wait", "side", "caller")]
