"""Host side of the vocabulary-parallel scoring head (csrc/tp_comm.hip: tp_head_logprobs): the tile split as plain arithmetic
(tp.score_tile_slice) and the argument check of the C entry point, which keeps its signature."""
import pytest

from helpers import ROOT  # noqa: F401  (puts the repository root on sys.path)
from mmada_parallel_amd import abi, tp


@pytest.mark.parametrize("size", [1, 2, 4, 8])
@pytest.mark.parametrize("n_cols", [134656, 8192, 1237, 255, 1])
def test_tile_split_is_a_partition_in_contiguous_blocks(n_cols, size):
    ntn = -(-n_cols // 256)
    q = -(-ntn // size)
    ranges = [tp.score_tile_slice(n_cols, r, size) for r in range(size)]
    at, seen_empty = 0, False
    for r, (t0, t1) in enumerate(ranges):
        assert 0 <= t0 <= t1 <= ntn
        assert (t0, t1) == (min(ntn, r * q), min(ntn, (r + 1) * q))      # the rule of the issue, as the library applies it
        if t1 == t0:
            seen_empty = True
            continue
        assert not seen_empty, "empty ranges occur only at the tail"
        assert t0 == at, "disjoint, ascending, contiguous"
        at = t1
    assert at == ntn, "the union is [0, ceil(n / 256))"
    assert ranges[0][1] > ranges[0][0], "rank 0 always has work"


def test_split_is_in_tiles_not_in_the_text_heads_column_units():
    # 1237 columns over 2 ranks: 5 tiles -> 3 + 2 (768 + 469 columns); vocab_slice would cut at 624
    assert [tp.score_tile_slice(1237, r, 2) for r in range(2)] == [(0, 3), (3, 5)]
    assert tp.vocab_slice(1237, 0, 2) == (0, 624)
    # fewer tiles than ranks: the trailing ranks own nothing
    assert [tp.score_tile_slice(255, r, 4) for r in range(4)] == [(0, 1), (1, 1), (1, 1), (1, 1)]
    assert [tp.score_tile_slice(1237, r, 8) for r in range(8)] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (5, 5), (5, 5)]


def test_head_logprobs_still_checks_its_arguments_without_a_gpu():
    lib = abi.lib()
    assert len(abi.SIGNATURES["mmada_head_logprobs"][1]) == 11
    assert lib.mmada_head_logprobs(None, None, 1, 0, 8, None, None, None, None, None, None) != 0
    assert b"no forward resident" in lib.mmada_last_error()
