"""What the library keeps resident between calls, through direct C-ABI calls on the model's lane handle: a refused call leaves
the resident forward as it was, a call that clobbers the workspace leaves none for ANY reader, and a windowed forward only
serves its window.  (The rule is written once, on `Resident` in csrc/handle.h.)"""
import ctypes as C

import pytest
import torch

from helpers import tiny_sd
from mmada_parallel_amd import abi, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tiny_model():
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    return LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(synth.CFG_TINY), tiny_sd(), device=DEV)


def _st():
    return abi.stream_ptr()


def _forward(model, ids):
    B, L = ids.shape
    model._ensure_ws(B, L)
    abi.check(abi.lib().mmada_forward_body(model._lane_handle(0), ids.data_ptr(), B, L, _st()), "mmada_forward_body")


def _head_rows(model, rows, col_begin, col_end):
    out = torch.zeros((rows.numel(), col_end - col_begin), dtype=torch.bfloat16, device=DEV)
    abi.check(abi.lib().mmada_head_rows(model._lane_handle(0), rows.data_ptr(), rows.numel(), col_begin, col_end, out.data_ptr(),
                                        _st()), "mmada_head_rows")
    return out


def _refused(status, text):
    msg = abi.lib().mmada_last_error().decode()
    assert status != 0 and text in msg, (status, msg)


@pytest.fixture(scope="module")
def plain(tiny_model):
    """(ids, every row index, logits [L, vocab]) of the script's first sequence after a plain forward; never modified."""
    ids = synth.dllm_cache_script()[0][1].to(DEV).contiguous()
    rows = torch.arange(ids.numel(), dtype=torch.int32, device=DEV)
    abi.check(abi.lib().mmada_set_consumed_rows(tiny_model._lane_handle(0), 0, 0), "mmada_set_consumed_rows")
    _forward(tiny_model, ids)
    return ids, rows, _head_rows(tiny_model, rows, 0, tiny_model.vocab)


def _readers_refuse(model, rows):
    """mmada_head_rows, mmada_head_logprobs, mmada_read_stream and mmada_debug_buffer: each must say 'no forward resident'."""
    lib, h, R, V = abi.lib(), model._lane_handle(0), rows.numel(), model.vocab
    out = torch.zeros((R, 64), dtype=torch.bfloat16, device=DEV)
    _refused(lib.mmada_head_rows(h, rows.data_ptr(), R, 0, 64, out.data_ptr(), _st()), "mmada_head_rows: no forward resident")
    targets = torch.zeros(R, dtype=torch.long, device=DEV)
    lp = torch.zeros(R, dtype=torch.float32, device=DEV)
    _refused(lib.mmada_head_logprobs(h, rows.data_ptr(), R, 0, V, targets.data_ptr(), lp.data_ptr(), None, None, None, _st()),
             "mmada_head_logprobs: no forward resident")
    stream = torch.zeros((R, model.config.d_model), dtype=torch.bfloat16, device=DEV)
    _refused(lib.mmada_read_stream(h, stream.data_ptr(), _st()), "mmada_read_stream: no forward resident")
    p, lpad, lkv = C.c_void_p(), C.c_int32(), C.c_int32()
    _refused(lib.mmada_debug_buffer(h, 0, C.byref(p), C.byref(lpad), C.byref(lkv)), "mmada_debug_buffer: no forward resident")


def test_a_refused_call_keeps_the_resident_forward(tiny_model, plain):
    """Three calls that fail before they write to the workspace; the head then reads the same bits as before them."""
    ids, rows, want = plain
    lib, h, V = abi.lib(), tiny_model._lane_handle(0), tiny_model.vocab
    B, L = ids.shape
    _forward(tiny_model, ids)
    first = _head_rows(tiny_model, rows, 0, V)
    assert torch.equal(first, want)
    tiny_model.empty_cache()   # no slot is bound now
    _refused(lib.mmada_forward_cached(h, 15, ids.data_ptr(), None, B, L, L, 1, _st()), "is not bound")
    too_long = torch.zeros((1, tiny_model.max_seq + 1), dtype=torch.long, device=DEV)
    _refused(lib.mmada_forward_body(h, too_long.data_ptr(), 1, tiny_model.max_seq + 1, _st()), "exceeds max_seq")
    out = torch.zeros((rows.numel(), 1), dtype=torch.bfloat16, device=DEV)
    _refused(lib.mmada_head_rows(h, rows.data_ptr(), rows.numel(), V, V + 1, out.data_ptr(), _st()), "bad column range")
    assert torch.equal(_head_rows(tiny_model, rows, 0, V), first)


def test_sdpa_clears_the_resident_forward_for_every_reader(tiny_model, plain):
    ids, rows, _ = plain
    _forward(tiny_model, ids)
    B, H, L = 1, 2, 16
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, H, L, 128, generator=g).to(torch.bfloat16).to(DEV) for _ in range(3))
    out = torch.zeros((B, L, H * 128), dtype=torch.bfloat16, device=DEV)
    abi.check(abi.lib().mmada_sdpa(tiny_model._lane_handle(0), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, H, L,
                                   _st()), "mmada_sdpa")
    _readers_refuse(tiny_model, rows)


def test_a_cached_forward_clears_it_and_the_slot_serves_the_same_logits(tiny_model, plain):
    ids, rows, want = plain
    lib, h, V = abi.lib(), tiny_model._lane_handle(0), tiny_model.vocab
    B, L = ids.shape
    _forward(tiny_model, ids)
    tiny_model.empty_cache()
    slot = tiny_model._cache_slot("resident", B, L, rebind_ok=True).idx
    abi.check(lib.mmada_forward_cached(h, slot, ids.data_ptr(), None, B, L, L, 1, _st()), "mmada_forward_cached")   # prime call
    _readers_refuse(tiny_model, rows)
    got = torch.zeros_like(want)
    abi.check(lib.mmada_cache_head_rows(h, slot, rows.data_ptr(), rows.numel(), 0, V, got.data_ptr(), _st()), "mmada_cache_head_rows")
    assert torch.equal(got, want)
    # the script's second entry: a compute-mask step on changed ids runs on the compact stream of the masked tokens; afterwards
    # no reader may see that stream either, and the slot serves the untouched rows unchanged and the computed rows anew
    _, ids1, m1 = synth.dllm_cache_script()[1]
    Tc = int(m1.sum())
    pos = m1.nonzero()[:, 1].view(B, Tc).to(torch.int32).to(DEV).contiguous()
    ids_c = ids1[m1].view(B, Tc).to(DEV).contiguous()
    _forward(tiny_model, ids)   # a plain forward is resident again before the step
    abi.check(lib.mmada_forward_cached(h, slot, ids_c.data_ptr(), pos.data_ptr(), B, L, Tc, 1, _st()), "mmada_forward_cached")
    _readers_refuse(tiny_model, rows)
    step = torch.zeros_like(want)
    abi.check(lib.mmada_cache_head_rows(h, slot, rows.data_ptr(), rows.numel(), 0, V, step.data_ptr(), _st()), "mmada_cache_head_rows")
    keep, comp = (~m1[0]).to(DEV), m1[0].to(DEV)
    assert torch.equal(step[keep], want[keep])
    assert torch.isfinite(step[comp].float()).all() and not torch.equal(step[comp], want[comp])
    tiny_model.empty_cache()


def test_a_windowed_forward_only_serves_its_window(tiny_model, plain):
    """mmada_read_stream names the rows the compact stream holds: the window start rounded down to the 32-query wave granule, its
    end rounded up to 8 rows (include/mmada_mi355x.h, mmada_set_consumed_rows).  The rows inside the window equal the unwindowed
    forward's; tests/test_gpu_model.py::test_consumed_row_window_is_bit_identical_on_the_consumed_rows asserts the same through
    the model for more windows and B = 2."""
    ids, rows, want = plain
    lib, h, V = abi.lib(), tiny_model._lane_handle(0), tiny_model.vocab
    lo, hi = 37, 60
    abi.check(lib.mmada_set_consumed_rows(h, lo, hi), "mmada_set_consumed_rows")
    try:
        _forward(tiny_model, ids)
        stream = torch.zeros((ids.numel(), tiny_model.config.d_model), dtype=torch.bfloat16, device=DEV)
        _refused(lib.mmada_read_stream(h, stream.data_ptr(), _st()), f"rows [{lo & ~31},{(hi + 7) & ~7})")
        assert torch.equal(_head_rows(tiny_model, rows[lo:hi].contiguous(), 0, V), want[lo:hi])
    finally:
        abi.check(lib.mmada_set_consumed_rows(h, 0, 0), "mmada_set_consumed_rows")
