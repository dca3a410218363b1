"""Top-k on the GPU: mmada_head_topk / model.top_logprobs (the EPI_ROWTOPK epilogue of the head GEMM and rowtopk_combine_kernel)
against a STABLE descending sort of the repo's own logits (head_rows) — the tie rule: logit descending, then column ascending —
and against the scoring head (token_logprobs) on the same rows.  Everything is exact: no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from mmada_parallel_amd import abi, synth
from mmada_parallel_amd.abi import MmadaError
from test_gpu_score import head8b, tiny_model   # noqa: F401  (the same fixtures: the tiny model, one 8B-width block + full head)
from test_gpu_score_tp import single_rank_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = synth.CFG_TINY["vocab_size"]
Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
KMAX = 8


def raw_topk(model, rows, k, c0, c1):
    """The library call itself (one lane): ids, the logits as fp32, lse."""
    R = rows.numel()
    ids = torch.full((R, k), -7, dtype=torch.int32, device=DEV)
    logit = torch.full((R, k), -7.0, dtype=torch.float32, device=DEV)
    lse = torch.full((R,), -7.0, dtype=torch.float32, device=DEV)
    abi.check(abi.lib().mmada_head_topk(model._handle, rows.data_ptr(), R, c0, c1, k, ids.data_ptr(), logit.data_ptr(), lse.data_ptr(),
                                        abi.stream_ptr()), "mmada_head_topk")
    return ids, logit, lse


def sorted_reference(model, rows, c0, c1):
    """First min(8, width) columns of the stable descending sort of the logits, and the scoring head's statistics of the rows."""
    logits = model.head_rows(rows, c0, c1).float()
    v, i = torch.sort(logits, dim=1, descending=True, stable=True)
    n = min(KMAX, c1 - c0)
    _, lse, arg, mx = model.token_logprobs(rows, torch.full((rows.numel(),), -1, device=DEV), c0, c1, return_stats=True)
    return (i[:, :n] + c0).int().contiguous(), v[:, :n].contiguous(), lse, arg, mx


def check_topk(model, rows, k, c0=0, c1=None, ref=None, what=""):
    c1 = model.vocab if c1 is None else c1
    want_ids, want_logit, lse_ref, arg, mx = ref if ref is not None else sorted_reference(model, rows, c0, c1)
    ids, logit, lse = raw_topk(model, rows, k, c0, c1)
    ids2, lp, lse2 = model.top_logprobs(rows, k, c0, c1)
    torch.cuda.synchronize()
    bad = int((ids != want_ids[:, :k]).any(1).sum())
    print(f"{what}: R={rows.numel()} k={k} cols [{c0},{c1}): rows with a wrong id {bad}, wrong logit "
          f"{int((logit != want_logit[:, :k]).any(1).sum())}, wrong lse {int((lse != lse_ref).sum())}")
    assert torch.equal(ids, want_ids[:, :k]), f"{what}: ids"
    assert torch.equal(logit, want_logit[:, :k]), f"{what}: logits"
    assert torch.equal(lse, lse_ref), f"{what}: lse is not the scoring head's"
    assert torch.equal(ids[:, 0], arg) and torch.equal(logit[:, 0], mx), f"{what}: entry 0 is not argmax / max"
    assert torch.equal(ids2, ids) and torch.equal(lse2, lse) and torch.equal(lp, logit - lse[:, None]), f"{what}: top_logprobs"
    for j in range(k):
        assert torch.equal(lp[:, j], model.token_logprobs(rows, ids[:, j].long(), c0, c1)), f"{what}: log-probability of entry {j}"
    return ids, logit, lse


def tiny_rows(R, B, L):
    return torch.arange(B * L, dtype=torch.int32, device=DEV)[:R] if R > 1 else torch.tensor([77], dtype=torch.int32, device=DEV)


def test_tiny_model_row_counts_and_k(tiny_model):
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    tiny_model.forward_body(ids)
    for R in (1, 5, 61, B * L):       # R = 1, not a multiple of 8, every row
        rows = tiny_rows(R, B, L)
        ref = sorted_reference(tiny_model, rows, 0, V)
        for k in (1, 2, 8):
            check_topk(tiny_model, rows, k, ref=ref, what=f"tiny R={R}")


RANGES = [
    (40, 48, 8),                       # width 8, k = 8: every column is returned, no empty key may surface
    (24, 40, 8),                       # width 16: all winners within a few lanes of one wave column
    (128, 192, 8),                     # width 64: one wave column
    (512, 512 + 259, 8),               # odd: the 16-wave kernel, the last tile holds three columns
    (512 + 256, 512 + 259, 3),         # ... and a range that IS three columns
    (1000, 1000 + 1237, 8),            # odd and multi-tile
    (synth.TEXT_VOCAB, synth.TEXT_VOCAB + synth.CODEBOOK, 8),
    (0, V, 8),                         # the whole vocabulary: 526 tiles
]


@pytest.mark.parametrize("c0, c1, k", RANGES)
def test_tiny_model_column_ranges(tiny_model, c0, c1, k):
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    assert V == 526 * 256
    tiny_model.forward_body(ids)
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    got, _, _ = check_topk(tiny_model, rows, k, c0, c1, what="tiny range")
    assert int(got.min()) >= c0 and int(got.max()) < c1
    if k == c1 - c0:                   # every column exactly once
        assert torch.equal(got.sort(1).values, torch.arange(c0, c1, dtype=torch.int32, device=DEV).expand(B * L, k))


def test_tiny_model_windowed_forward(tiny_model):
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    tiny_model.forward_body(ids, consumed=(20, 50))
    try:
        wrows = (torch.arange(B)[:, None] * L + torch.arange(20, 50)[None, :]).flatten().int().to(DEV)
        check_topk(tiny_model, wrows, 8, what="tiny windowed")
        check_topk(tiny_model, wrows, 2, 1000, 1000 + 1237, what="tiny windowed, odd range")
    finally:
        tiny_model.forward_body(ids)


def test_8b_head_all_configurations_ties_graph_and_memory(head8b):
    model = head8b
    lib = abi.lib()
    g = torch.Generator().manual_seed(11)
    L = 700                                       # not a multiple of any tile height (320 / 256 / 160 / 192 / 128)
    ids = torch.randint(0, 126000, (1, L), generator=g).to(DEV)
    model.forward_body(ids)
    rows = torch.arange(L, dtype=torch.int32, device=DEV)
    ref = sorted_reference(model, rows, 0, model.vocab)          # once, under the planner's pick
    first = None
    try:
        for code in (-1, 0, 1, 2, 3, 1128, 1192, 1256, 1320, 1160):
            abi.check(lib.mmada_set_option(b"gemm_config", code), "set_option")
            got = raw_topk(model, rows, 8, 0, model.vocab)
            torch.cuda.synchronize()
            first = got if first is None else first
            for a, b, w, name in zip(got, first, (ref[0], ref[1], ref[2]), ("ids", "logits", "lse")):
                assert torch.equal(a, b), f"gemm_config {code}: {name} differ from the planner's pick"
                assert torch.equal(a, w), f"gemm_config {code}: {name} differ from the sorted logits / the scoring head"
    finally:
        lib.mmada_set_option(b"gemm_config", -1)
    check_topk(model, rows, 8, ref=ref, what="8B head")

    # memory: the record buffer is 48 bytes per row and tile + 4 per row, and torch allocates the outputs only
    own = lib.mmada_score_buffer_bytes(model._handle)
    assert 0 < own <= (L + 7) // 8 * 8 * (526 * 48 + 4), own
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    out = model.top_logprobs(rows, 8)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated(DEV) - before
    print(f"top-k at R={L}: torch peak +{grew} B, library record buffer {own} B (logits would be {L * model.vocab * 2} B)")
    assert grew < L * model.vocab * 2 // 10 and lib.mmada_score_buffer_bytes(model._handle) == own
    del out

    # planted ties: two rows of the resident stream are set to ZERO -> every logit of the row is 0, a tie across all column tiles,
    # waves and lanes: the first k columns win, in a sub-range too
    view = model._stream_view().view(-1, model.config.d_model)
    view[5].zero_(); view[333].zero_()
    try:
        tied, tl, _ = check_topk(model, rows, 8, what="8B head planted ties")
        assert tied[5].tolist() == list(range(8)) and tied[333].tolist() == list(range(8)) and bool((tl[5] == 0).all())
        tied, _, _ = check_topk(model, rows, 8, 4096 + 8, 4096 + 8 + 2048, what="8B head planted ties, range")
        assert tied[5].tolist() == list(range(4104, 4112)) and tied[333].tolist() == list(range(4104, 4112))
    finally:
        model.forward_body(ids)

    # replay from a captured graph: same bits as the eager call
    eager = raw_topk(model, rows, 8, 0, model.vocab)
    outs = [torch.full_like(e, -7) for e in eager]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        abi.check(lib.mmada_graph_begin(abi.stream_ptr()), "graph_begin")
        rc = lib.mmada_head_topk(model._handle, rows.data_ptr(), L, 0, model.vocab, 8, outs[0].data_ptr(), outs[1].data_ptr(),
                                 outs[2].data_ptr(), abi.stream_ptr())
        if rc:
            lib.mmada_graph_abort(abi.stream_ptr())
        abi.check(rc, "mmada_head_topk under capture")
        gr = C.c_void_p()
        abi.check(lib.mmada_graph_end(abi.stream_ptr(), C.byref(gr)), "graph_end")
        for _ in range(2):
            abi.check(lib.mmada_graph_launch(gr, abi.stream_ptr()), "graph_launch")
        side.synchronize()
        lib.mmada_graph_destroy(gr)
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)


def test_tensor_parallel_handle_is_refused(tiny_model):
    from helpers import tiny_sd

    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    with single_rank_group(synth.CFG_TINY, tiny_sd(), "pull", B * ((L + 7) // 8 * 8)) as m:
        m.forward_body(ids)
        rows = torch.arange(8, dtype=torch.int32, device=DEV)
        with pytest.raises(MmadaError, match="one rank"):
            raw_topk(m, rows, 2, 0, V)
        assert b"vocabulary-parallel" in abi.lib().mmada_last_error()
        with pytest.raises(NotImplementedError, match="one rank"):
            m.top_logprobs(rows, 2)
        assert m.comm_status()["error"] == 0
