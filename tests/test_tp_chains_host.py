"""Host side of the sequence-chain plan of the tensor-parallel forward (no GPU): what MMADA_TP_CHUNKS is kept as, the library's
plan (chunk_plan_of in csrc/tp_plan.h, the header the forward itself includes, compiled here into a small host program) against its
mirror tp.chunk_plan over the whole grid, the properties the schedule rests on, and the emulated link's requested waits under a
chain plan."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from helpers import ROOT
from mmada_parallel_amd import tp, tp_link

MODES = (1, 2, 3, 4, 5)                       # pull, RCCL, no-exchange diagnostic, copy, emulated link
BATCHES = (1, 2, 3, 4, 5, 8, 16)
LPS = (8, 48, 64, 2440)
SIZES = (1, 2, 4, 8)
COUNTS = (1, 2, 4, 8)
CSRC = os.path.join(ROOT, "mmada_parallel_amd", "csrc")
# reads "B Lp tp rank chunks mode cached" lines, prints "n" and per chunk "m0 m1 slice r0 r1 b0 b1" as the library's header plans them
PLAN_MAIN = r"""
#include <cstdio>
#include "tp_plan.h"
int main() {
    int B, Lp, tp, rank, chunks, mode, cached;
    while (std::scanf("%d %d %d %d %d %d %d", &B, &Lp, &tp, &rank, &chunks, &mode, &cached) == 7) {
        const ChunkPlan p = chunk_plan_of(B * Lp, B, Lp, tp, rank, chunks, mode, cached != 0);
        std::printf("%d %d", p.n, (int)p.chains);
        for (int k = 0; k < p.n; ++k)
            std::printf(" %d %d %d %d %d %d %d", p.sl[k].m0, p.sl[k].m1, p.sl[k].slice, p.sl[k].r0, p.sl[k].r1, p.b0[k], p.b1[k]);
        std::printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_plans(tmp_path_factory):
    """plans(queries) -> [(chains, [(m0, m1, slice, r0, r1, b0, b1)])] from csrc/tp_plan.h, one run of the compiled program."""
    work = tmp_path_factory.mktemp("tp_plan")
    src, exe = os.path.join(work, "plan_main.cpp"), os.path.join(work, "plan_main")
    with open(src, "w") as f:
        f.write(PLAN_MAIN)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]

    def plans(queries):
        text = "".join(" ".join(str(int(v)) for v in q) + "\n" for q in queries)
        run = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = []
        for line in run.stdout.splitlines():
            v = [int(x) for x in line.split()]
            assert 1 <= v[0] <= tp.TP_CHUNKS_MAX and len(v) == 2 + 7 * v[0]
            out.append((bool(v[1]), [tuple(v[2 + 7 * k:9 + 7 * k]) for k in range(v[0])]))
        assert len(out) == len(queries)
        return out

    return plans


def test_the_mapping_of_mmada_tp_chunks(monkeypatch):
    table = {-3: 1, 0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 4, 7: 4, 8: 8, 9: 8, 64: 8}
    for value, kept in table.items():
        assert tp.normalise_chunks(value) == kept
        monkeypatch.setenv("MMADA_TP_CHUNKS", str(value))
        assert tp_link._chunks_at_create() == kept, value
    monkeypatch.setenv("MMADA_TP_CHUNKS", "four")        # atoi() of a non-number is 0
    assert tp_link._chunks_at_create() == 1
    monkeypatch.delenv("MMADA_TP_CHUNKS")
    assert tp_link._chunks_at_create() == 2 and tp_link.TpLink().chunks == 2
    assert tp.TP_CHUNKS_MAX == 8


def test_the_library_plan_equals_its_mirror_over_the_grid(header_plans):
    grid = [(B, Lp, size, rank, chunks, mode, cached) for B in BATCHES for Lp in LPS for size in SIZES for rank in range(size)
            for chunks in COUNTS for mode in MODES for cached in (False, True)]
    assert len(grid) == 7 * 4 * (1 + 2 + 4 + 8) * 4 * 5 * 2
    for q, (chains, got) in zip(grid, header_plans(grid)):
        B, Lp, size, rank, chunks, mode, cached = q
        assert got == tp.chunk_plan(*q), q
        assert chains == tp.runs_chains(chunks, (B, Lp), rccl=mode == tp.MODE_RCCL, cached=cached), q
    # the header normalises a raw value the way mmada_comm_create does
    raws = ((0, 1), (3, 2), (5, 4), (7, 4), (9, 8), (100, 8))
    got = header_plans([(16, 64, 2, 1, v, 1, 0) for pair in raws for v in pair])
    for i, (raw, kept) in enumerate(raws):
        assert got[2 * i] == got[2 * i + 1] and got[2 * i][1] == tp.chunk_plan(16, 64, 2, 1, raw) == tp.chunk_plan(16, 64, 2, 1, kept)


def test_properties_of_a_chain_plan():
    for B in BATCHES:
        for Lp in LPS:
            for size in SIZES:
                for count in (4, 8):
                    for mode in (1, 3, 4, 5):
                        if B < 2:
                            continue
                        M = B * Lp
                        assert tp.runs_chains(count, (B, Lp), rccl=False, cached=False)
                        plans = [tp.chunk_plan(B, Lp, size, r, count, mode) for r in range(size)]
                        n = len(plans[0])
                        assert n == min(count, B)
                        seqs = []
                        for k in range(n):
                            m0, m1, sl, _, _, b0, b1 = plans[0][k]
                            # whole sequences [k B / n, (k + 1) B / n), rows [b0 Lp, b1 Lp): every boundary a multiple of Lp
                            assert (b0, b1) == (k * B // n, (k + 1) * B // n) and (m0, m1) == (b0 * Lp, b1 * Lp)
                            assert sl == max(8, ((m1 - m0 + size - 1) // size + 7) // 8 * 8) and sl % 8 == 0
                            seqs.append(b1 - b0)
                            # the owners partition the chain, in rank order; every rank sees the same chain
                            at = m0
                            for r in range(size):
                                assert plans[r][k][:3] == (m0, m1, sl) and plans[r][k][5:] == (b0, b1)
                                r0, r1 = plans[r][k][3:5]
                                assert r0 == at and r0 <= r1 <= m1 and (r1 - r0 == sl or r1 == m1)
                                at = r1
                            assert at == m1
                        # the chains tile [0, M); sizes differ by at most one sequence
                        assert plans[0][0][0] == 0 and plans[0][-1][1] == M
                        assert all(a[1] == b[0] for a, b in zip(plans[0], plans[0][1:]))
                        assert sum(seqs) == B and max(seqs) - min(seqs) <= 1 and min(seqs) >= 1
                        # chunk_slices / owned_rows with the batch shape are the same plan
                        assert tp.chunk_slices(M, size, count, batch=(B, Lp)) == [p[:3] for p in plans[0]]
                        for r in range(size):
                            assert tp.owned_rows(M, r, size, count, batch=(B, Lp)) == [p[3:5] for p in plans[r]]
    # the cases the GPU tests run: B = 5 at a count of 4 (sequences 1, 1, 1, 2), B = 3 at a count of 8, an empty trailing owner
    assert [p[5:] for p in tp.chunk_plan(5, 64, 2, 0, 4)] == [(0, 1), (1, 2), (2, 3), (3, 5)]
    assert [p[:2] for p in tp.chunk_plan(3, 64, 2, 0, 8)] == [(0, 64), (64, 128), (128, 192)]
    assert [tp.chunk_plan(4, 48, 4, r, 4)[1][2:5] for r in range(4)] == [(16, 48, 64), (16, 64, 80), (16, 80, 96), (16, 96, 96)]


def test_every_other_case_is_todays_plan_exactly():
    """RCCL, a cached forward, B = 1 and counts <= 2 return today's chunk_slices numbers; so does chunk_slices without a batch shape."""
    def todays(M, size, nch):       # tp.chunk_slices as it stood before the chain plan
        unit = 8 * size
        if nch >= 2 and M >= 4 * unit:
            first = (M // 2 + unit - 1) // unit * unit
            bounds = [(0, min(first, M)), (min(first, M), M)]
        else:
            bounds = [(0, M)]
        return [(m0, m1, max(8, ((m1 - m0 + size - 1) // size + 7) // 8 * 8)) for m0, m1 in bounds]

    for B in BATCHES:
        for Lp in LPS:
            for size in SIZES:
                M = B * Lp
                for count in COUNTS:
                    for mode in MODES:
                        for cached in (False, True):
                            if count >= 4 and B >= 2 and mode != 2 and not cached:
                                continue
                            for rank in range(size):
                                want = [(m0, m1, sl, min(m1, m0 + rank * sl), min(m1, m0 + (rank + 1) * sl), 0, B)
                                        for m0, m1, sl in todays(M, size, count)]
                                assert tp.chunk_plan(B, Lp, size, rank, count, mode, cached) == want, (B, Lp, size, rank, count, mode, cached)
                    assert tp.chunk_slices(M, size, count) == todays(M, size, count)
                    assert tp.chunk_slices(M, size, count, batch=(B, Lp), rccl=True) == todays(M, size, count)
                    assert tp.chunk_slices(M, size, count, batch=(B, Lp), cached=True) == todays(M, size, count)
    with pytest.raises(ValueError):
        tp.chunk_slices(100, 2, 4, batch=(2, 48))


def test_a_chain_plan_asks_the_link_for_the_time_of_one_chunk():
    """The chains cut the rows, not the bytes: the requested waits of a chain plan sum to the one-chunk forward's, up to the rounding
    of every wait (each is rounded up to a whole nanosecond, and to a whole row per rank: ceil(rows / tp))."""
    for B, Lp, size, d, layers, mbps in ((8, 2440, 8, 4096, 4, 76000), (4, 64, 2, 256, 2, 2000), (5, 64, 2, 256, 2, 1000),
                                         (4, 48, 4, 512, 1, 153000), (3, 64, 2, 256, 2, 276), (16, 8, 8, 256, 1, 1000)):
        M = B * Lp
        one = tp.forward_link_waits_ns(M, d, size, layers, mbps, 1)
        for count in (4, 8):
            waits = tp.forward_link_waits_ns(M, d, size, layers, mbps, count, batch=(B, Lp))
            n = min(count, B)
            assert len(waits) == 4 * layers * n and len(one) == 4 * layers
            # per wait: at most size - 1 rows of rounding up to whole rows per rank, and one nanosecond
            slack = len(waits) * ((size - 1) * d * 2 * 1000 / mbps + 1)
            assert sum(one) - len(one) <= sum(waits) <= sum(one) + slack, (B, Lp, size, count, sum(waits), sum(one))
            # the order is the launch order: per exchange chain 0 .. n - 1, two phases each
            per = [tp.link_wait_ns(m1 - m0, d, size, mbps) for m0, m1, _ in tp.chunk_slices(M, size, count, batch=(B, Lp)) for _ in (0, 1)]
            assert waits == per * (2 * layers)
    # rows that divide evenly: exactly the one-chunk time, as for two chunks
    assert sum(tp.forward_link_waits_ns(4 * 64, 256, 2, 2, 1000, 4, batch=(4, 64))) == sum(tp.forward_link_waits_ns(4 * 64, 256, 2, 2, 1000, 1)) \
        == sum(tp.forward_link_waits_ns(4 * 64, 256, 2, 2, 1000, 2))
    assert tp.forward_link_waits_ns(4 * 64, 256, 2, 1, 1000, 4, batch=(4, 64)) == [32 * 512] * 16
    # without the batch shape, on RCCL or through a cache slot a count of 4 is the plan of 2
    two = tp.forward_link_waits_ns(256, 256, 2, 1, 1000, 2)
    assert tp.forward_link_waits_ns(256, 256, 2, 1, 1000, 4) == two
    assert tp.forward_link_waits_ns(256, 256, 2, 1, 1000, 4, batch=(4, 64), rccl=True) == two
    assert tp.forward_link_waits_ns(256, 256, 2, 1, 1000, 4, batch=(1, 256)) == two


def test_the_model_passes_its_batch_shape_to_the_wait_arithmetic():
    from types import SimpleNamespace

    from mmada_parallel_amd.model import LLaDAForMultiModalGeneration, _Lane, _Resident

    m = object.__new__(LLaDAForMultiModalGeneration)   # the constructor needs a GPU
    m._lib, m._handle = None, C.c_void_p()
    m._lanes, m._resident, m._link = [_Lane(m._handle)], _Resident(), tp_link.TpLink(connected=True, rows=256, transport="pull", chunks=4)
    m.config, m.tp_size = SimpleNamespace(d_model=256, n_layers=2), 2
    assert m.emulated_wait_ns_per_forward(4, 61, 1000) == sum(tp.forward_link_waits_ns(256, 256, 2, 2, 1000, 4, batch=(4, 64))) == 32 * 32 * 512
    assert m.emulated_wait_ns_per_forward(1, 256, 1000) == sum(tp.forward_link_waits_ns(256, 256, 2, 2, 1000, 2))   # B = 1: the plan of 2


def test_the_assertions_on_at_most_two_chunks_still_hold():
    """Copied from tests/test_tp_emulate_host.py and tests/test_tp_gloo.py: nothing about one and two chunks has moved."""
    assert [(m0, m1) for m0, m1, _ in tp.chunk_slices(96, 2, 2)] == [(0, 48), (48, 96)]
    assert tp.forward_link_waits_ns(96, 256, 2, 2, 1000, n_chunks=2) == [12_288] * 16
    assert tp.forward_link_waits_ns(96, 256, 2, 2, 1000, n_chunks=1) == [24_576] * 8
    assert tp.forward_link_waits_ns(40, 256, 2, 1, 1000, n_chunks=2) == [20 * 512] * 4
    assert tp.forward_link_waits_ns(104, 256, 2, 1, 1000, n_chunks=2) == [32 * 512, 32 * 512, 20 * 512, 20 * 512] * 2
    assert len(tp.chunk_slices(40, 2)) == 1 and len(tp.chunk_slices(96, 2)) == 2
    for size in (2, 4, 8):
        for M in (8, 72, 216, 2440, 4880, 19520, 39040):
            for nch in (1, 2):
                seen = [0] * M
                plan = tp.chunk_slices(M, size, nch)
                for k, (m0, m1, sl) in enumerate(plan):
                    assert sl % 8 == 0 and size * sl >= m1 - m0 and size * sl <= (m1 - m0) + 8 * size
                    if k < len(plan) - 1:
                        assert (m1 - m0) == size * sl   # only the last chunk is padded
                for r in range(size):
                    for r0, r1 in tp.owned_rows(M, r, size, nch):
                        for i in range(r0, r1):
                            seen[i] += 1
                assert all(v == 1 for v in seen), (size, M, nch)
    for M in (8, 24, 96, 2440, 4880):
        for nch in (1, 2):
            sl = tp.chunk_slices(M, 1, nch)
            assert sl[0][0] == 0 and sl[-1][1] == M and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
            assert [(m0, m1) for m0, m1, _ in sl] == tp.owned_rows(M, 0, 1, nch), "the one rank owns every row"
