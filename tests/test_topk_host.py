"""The top-k head, host side (no GPU): the C ABI of mmada_head_topk, its argument errors, and the order key the kernels sort by
(csrc/kernels.h: topk_order, reached through mmada_topk_order_key)."""
import fnmatch
import os
import re

import pytest
import torch

from helpers import ROOT
from mmada_parallel_amd import abi
from mmada_parallel_amd.model import TOPK_MAX


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmada_mi355x.h")).read(), flags=re.S)


def test_head_topk_is_declared_exported_and_bound():
    header = header_text()
    export_map = open(os.path.join(ROOT, "mmada_parallel_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:\s*([^;]+);", export_map).group(1).split()
    for sym, nargs in (("mmada_head_topk", 10), ("mmada_topk_order_key", 1)):
        decl = re.search(r"\b" + sym + r"\s*\(([^)]*)\)", header)
        assert decl and len(decl.group(1).split(",")) == nargs
        assert any(fnmatch.fnmatch(sym, p) for p in patterns)
        assert len(abi.SIGNATURES[sym][1]) == nargs
        assert hasattr(abi.lib(), sym)
    m = re.search(r"#define\s+MMADA_TOPK_MAX\s+(\d+)", header)
    assert m and int(m.group(1)) == TOPK_MAX == 8


@pytest.mark.parametrize("k, c0, c1, message", [
    (1, 0, 8, b"no forward resident"),            # a null handle
    (0, 0, 8, b"k=0"),
    (TOPK_MAX + 1, 0, 64, b"k=9"),
    (8, 100, 107, b"exceeds the column range"),   # k greater than the range width
])
def test_argument_errors_without_a_gpu(k, c0, c1, message):
    lib = abi.lib()
    assert lib.mmada_head_topk(None, None, 1, c0, c1, k, None, None, None, None) != 0
    assert message in lib.mmada_last_error(), lib.mmada_last_error()


def test_order_key_is_monotone_over_every_finite_bf16():
    """Sorted by the key, the 65 280 finite bf16 patterns are in ascending float order; the only two patterns that share a key are
    -0.0 and +0.0, which compare equal as floats.  That is torch's order too: its (stable) sort compares values, -0.0 == +0.0, so
    the lower index comes first whichever zero it holds — checked below on a row that holds both."""
    lib = abi.lib()
    bits = [b for b in range(1 << 16) if (b & 0x7f80) != 0x7f80]
    assert len(bits) == 65280
    keys = [lib.mmada_topk_order_key(b) for b in bits]
    assert all(0 < k < (1 << 16) for k in keys)
    vals = torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).double()
    order = sorted(range(len(bits)), key=lambda i: keys[i])
    v, ks = vals[order], [keys[i] for i in order]
    for i in range(len(order) - 1):
        assert (ks[i] < ks[i + 1] and bool(v[i] < v[i + 1])) or (ks[i] == ks[i + 1] and bool(v[i] == v[i + 1]))
    assert lib.mmada_topk_order_key(0x8000) == lib.mmada_topk_order_key(0x0000)
    assert len(set(keys)) == 65279
    # -inf sits below every finite value and above the empty key 0; +inf above every finite value
    assert 0 < lib.mmada_topk_order_key(0xff80) < min(keys) and lib.mmada_topk_order_key(0x7f80) > max(keys)
    # torch on the same floats: a stable descending sort leaves -0.0 and +0.0 in index order
    row = torch.tensor([-0.0, 0.0, 1.0, 0.0, -0.0, -1.0])
    idx = torch.sort(row, descending=True, stable=True).indices.tolist()
    mine = sorted(range(6), key=lambda i: (-lib.mmada_topk_order_key(int(row[i].to(torch.bfloat16).view(torch.int16)) & 0xffff), i))
    assert idx == mine == [2, 0, 1, 3, 4, 5]


def test_tensor_parallel_models_refuse_top_logprobs():
    from test_score_host import StubScore

    m = StubScore("main")
    m.tp_size = 2
    with pytest.raises(NotImplementedError, match="one rank"):
        m.top_logprobs(torch.zeros(1), 1)
