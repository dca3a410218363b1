"""hipGraph replay of a sampler's steps, for every generator that has it (generate_ti2ti, interleave_generate, generate_image).

A step whose launches are a fixed sequence over fixed buffers is run eagerly the first time its kind is met (first calls set
attributes / carve), captured the second time (mmada_graph_*) and replayed from then on.  The generators keep their own concerns:
which buffers exist before the loop, the per-step copies of k / mask_len / temperature into them, when a run is eligible, and
the step body.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch

from .. import abi


class StepGraphs:
    """with StepGraphs(model, graph, eligible) as sg: ... sg.step(kind, body) per step, under `with sg.stream()`.

    `graph` None = env MMADA_GRAPH=1.  On only if `eligible` (the caller's rule: a replayed step must not replay torch's draws) and
    the forward issues no host-side collective (model.graph_capturable()); off, step() just calls body() and no stream is made.
    The legacy default stream cannot be captured, so the steps run on a side stream: ordered after the caller's on entry and by
    fork(), and the caller's after it by join() — once around the loop, or around every hand-over of the ids to a consumer.
    Leaving the block, by an exception or a closed generator too, destroys every graph held."""

    def __init__(self, model, graph, eligible):
        if graph is None:
            graph = os.environ.get("MMADA_GRAPH") == "1"
        self.model, self.lib = model, model._lib
        self.on = bool(graph) and bool(eligible) and model.graph_capturable()
        self.side = torch.cuda.Stream(device=model.device) if self.on else None
        self.graphs, self.seen = {}, set()
        self.ws_epoch = model._ws_epoch

    def __enter__(self):
        self.fork()
        return self

    def __exit__(self, *exc):
        self._drop()

    def _drop(self):
        for g in self.graphs.values():
            self.lib.mmada_graph_destroy(g)
        self.graphs.clear()
        self.seen.clear()

    def stream(self):
        return torch.cuda.stream(self.side) if self.on else contextlib.nullcontext()

    def fork(self):
        """The side stream continues after what the caller's stream has queued."""
        if self.on:
            self.side.wait_stream(torch.cuda.current_stream(self.model.device))

    def join(self):
        """Whoever consumes the ids on the caller's stream sees the finished steps."""
        if self.on:
            torch.cuda.current_stream(self.model.device).wait_stream(self.side)

    def step(self, key, body, nodes_key=None):
        """Run one step of kind `key`: body() eagerly, captured, or its graph.  model.graph_replays counts every graph launch, the
        captured step's own included; model.graph_nodes[nodes_key or key] is the captured step's node count."""
        if not self.on:
            body()
            return
        model, lib = self.model, self.lib
        if model._ws_epoch != self.ws_epoch:
            self._drop()   # the workspace moved after all (a foreign forward in between): captured pointers are stale
            self.ws_epoch = model._ws_epoch
        if key not in self.graphs:
            if key not in self.seen:
                self.seen.add(key)
                body()
                return
            st = abi.stream_ptr()
            abi.check(lib.mmada_graph_begin(st), "mmada_graph_begin")
            try:
                body()
            except Exception:
                lib.mmada_graph_abort(st)
                raise
            g = C.c_void_p()
            abi.check(lib.mmada_graph_end(st, C.byref(g)), "mmada_graph_end")
            self.graphs[key] = g
            model.graph_nodes[key if nodes_key is None else nodes_key] = lib.mmada_graph_num_nodes(g)
        abi.check(lib.mmada_graph_launch(self.graphs[key], abi.stream_ptr()), "mmada_graph_launch")
        model.graph_replays += 1
