"""Scoring, host side (no GPU): the reference's loss bookkeeping on recorded per-token losses, ragged-batch padding, the return
contract of forward(labels=...) and the C ABI of mmada_head_logprobs.

tests/golden/loss_tiny.npz is a recording of the reference's forward(input_ids, labels, ...) (tools/gen_loss_golden.py)."""
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT, STUB_CB, STUB_TEXT_VOCAB, from_bits, stub_logits, tiny_job
from mmada_parallel_amd import abi
from mmada_parallel_amd.model import (ANSWER_START_TOKEN, CausalLMOutputLite, LLaDAConfigLite, LLaDAForMultiModalGeneration,
                                      loss_regions, pad_id_lists)

Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
CASES = ("main", "noas", "ign")
DT = {"bfloat16": torch.bfloat16, "float32": torch.float32}


def lists(case):
    n = Z[case + "_len"].tolist()
    return ([Z[case + "_ids"][b, :n[b]].tolist() for b in range(len(n))],
            [Z[case + "_labels"][b, :n[b]].tolist() for b in range(len(n))])


def want(case, key):
    """The recorded loss as a 0-dim tensor of the dtype the reference returned."""
    i = ("interleave", "text", "image", "text_t").index(key)
    return torch.tensor(float(Z[f"{case}_{key}"]), dtype=DT[str(Z[case + "_dtypes"][i])])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b)


class StubScore(LLaDAForMultiModalGeneration):
    """The product class on the CPU with score() / the logits served from the recording (the constructor needs a GPU)."""

    def __init__(self, case=None, vocab=STUB_TEXT_VOCAB + STUB_CB):
        self.device = torch.device("cpu")
        self.vocab, self.tp_size, self._comm_in_library = vocab, 1, False
        self.config = LLaDAConfigLite(text_vocab_size=STUB_TEXT_VOCAB, codebook_size=STUB_CB, vocab_size=vocab)
        self.case, self.scored = case, []

    def score(self, input_ids, labels):
        self.scored.append((input_ids.clone(), labels.clone()))
        return from_bits(Z[self.case + "_loss_bits"]).float()

    def forward_body(self, input_ids, consumed=None):
        self._shape = tuple(input_ids.shape)
        self._logits = stub_logits(5, 1, input_ids.shape[0], input_ids.shape[1], self.vocab)

    def head_rows(self, rows, col_begin, col_end, out=None):
        return self._logits.reshape(-1, self.vocab)[rows.long(), col_begin:col_end]

    def __del__(self):
        pass


@pytest.mark.parametrize("case", CASES)
def test_region_bookkeeping_reproduces_the_reference_bit_for_bit(case):
    loss = from_bits(Z[case + "_loss_bits"])
    ids, lab = torch.from_numpy(Z[case + "_ids"]), torch.from_numpy(Z[case + "_labels"])
    inter, text, image = loss_regions(loss, ids, lab, Z[case + "_len"].tolist())
    assert same(inter, want(case, "interleave")) and same(text, want(case, "text")) and same(image, want(case, "image"))
    inter, text, image = loss_regions(loss, ids, lab, Z[case + "_len"].tolist(), t=torch.from_numpy(Z["t"]))
    assert same(inter, want(case, "interleave")) and same(text, want(case, "text_t")) and same(image, want(case, "image"))


def test_fixture_covers_the_region_rules():
    assert Z["main_len"].tolist() == [61, 48, 61]
    assert not (Z["noas_ids"][1] == ANSWER_START_TOKEN).any() and (Z["main_ids"][1] == ANSWER_START_TOKEN).any()
    assert float(Z["noas_text"]) != float(Z["main_text"])          # the sequence without an answer start left the text loss
    assert float(Z["noas_interleave"]) == float(Z["main_interleave"])   # ... but still counts in the interleave loss
    assert (Z["ign_labels"] == -100).all()
    for key in ("interleave", "text", "image", "text_t"):
        assert float(Z["ign_" + key]) == 0.0
    assert float(Z["main_image"]) > 0 and float(Z["main_text_t"]) != float(Z["main_text"])


@pytest.mark.parametrize("case", CASES)
def test_ragged_lists_are_padded_as_recorded(case):
    ids_l, lab_l = lists(case)
    ids, lab, lengths = pad_id_lists(ids_l, lab_l)
    assert lengths == Z[case + "_len"].tolist()
    assert ids.dtype == torch.long and torch.equal(ids, torch.from_numpy(Z[case + "_ids"]))
    assert lab.dtype == torch.long and torch.equal(lab, torch.from_numpy(Z[case + "_labels"]))
    ids_t, lab_t, lengths_t = pad_id_lists(ids, lab)                # tensors pass through
    assert torch.equal(ids_t, ids) and torch.equal(lab_t, lab) and lengths_t == [ids.shape[1]] * ids.shape[0]
    with pytest.raises(ValueError):
        pad_id_lists(ids, lab[:, :-1])


@pytest.mark.parametrize("case", CASES)
def test_forward_with_labels_returns_the_reference_shapes_and_values(case):
    ids_l, lab_l = lists(case)
    m = StubScore(case)
    loss, parts = m(ids_l, labels=lab_l)                            # tuple form
    assert same(loss, want(case, "interleave")) and sorted(parts) == ["image_loss", "interleave_loss", "text_loss"]
    assert same(parts["text_loss"], want(case, "text")) and same(parts["image_loss"], want(case, "image"))
    assert same(parts["interleave_loss"], want(case, "interleave"))
    assert torch.equal(m.scored[0][0], torch.from_numpy(Z[case + "_ids"])) and torch.equal(m.scored[0][1], torch.from_numpy(Z[case + "_labels"]))
    assert not hasattr(m, "_logits"), "only return_dict=True materialises the logits"
    _, parts_t = m(ids_l, labels=lab_l, t=torch.from_numpy(Z["t"]))
    assert same(parts_t["text_loss"], want(case, "text_t"))
    scalar = m(ids_l, labels=lab_l, compute_separate_losses=False)  # scalar form
    assert same(scalar, want(case, "interleave"))
    d = m(ids_l, labels=lab_l, return_dict=True)                    # dict forms
    assert sorted(d) == ["image_loss", "interleave_loss", "labels", "logits", "loss", "text_loss"]
    assert same(d["loss"], want(case, "interleave")) and same(d["text_loss"], want(case, "text")) and same(d["image_loss"], want(case, "image"))
    B, L = Z[case + "_ids"].shape
    assert d["logits"].shape == (B, L, m.vocab) and d["logits"].dtype == torch.bfloat16
    assert torch.equal(d["labels"], torch.from_numpy(Z[case + "_labels"]))
    d = m(ids_l, labels=lab_l, return_dict=True, compute_separate_losses=False)
    assert sorted(d) == ["labels", "logits", "loss"] and same(d["loss"], want(case, "interleave"))
    # tensors are accepted too
    loss2, _ = m(torch.from_numpy(Z[case + "_ids"]), labels=torch.from_numpy(Z[case + "_labels"]))
    assert same(loss2, loss)


def test_infer_true_is_untouched():
    m = StubScore()
    ids = tiny_job()["input_ids"]
    out = m(ids, infer=True, use_cache=False)
    assert isinstance(out, CausalLMOutputLite) and out.logits.shape == (1, ids.shape[1], m.vocab)
    assert torch.equal(out.logits, stub_logits(5, 1, 1, ids.shape[1], m.vocab))
    with pytest.raises(ValueError):
        m(ids, infer=True, to_compute_mask=torch.ones_like(ids, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        m(ids, infer=False)                                          # no labels: forward(infer=True) is the logits call
    with pytest.raises(NotImplementedError):
        m(ids, labels=ids, infer=True)


def test_tensor_parallel_models_refuse_to_score():
    m = StubScore("main")
    m.tp_size = 2
    ids_l, lab_l = lists("main")
    with pytest.raises(NotImplementedError, match="vocabulary-parallel"):
        m(ids_l, labels=lab_l)
    with pytest.raises(NotImplementedError, match="vocabulary-parallel"):
        LLaDAForMultiModalGeneration.score(m, torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="vocabulary-parallel"):
        m.token_logprobs(torch.zeros(1), torch.zeros(1))


def test_head_logprobs_is_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmada_mi355x.h")).read(), flags=re.S)
    export_map = open(os.path.join(ROOT, "mmada_parallel_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:\s*([^;]+);", export_map).group(1).split()
    for sym, nargs in (("mmada_head_logprobs", 11), ("mmada_score_buffer_bytes", 1)):
        decl = re.search(r"\b" + sym + r"\s*\(([^)]*)\)", header)
        assert decl and len(decl.group(1).split(",")) == nargs
        assert any(fnmatch.fnmatch(sym, p) for p in patterns)
        assert len(abi.SIGNATURES[sym][1]) == nargs
        assert hasattr(abi.lib(), sym)
    lib = abi.lib()
    assert lib.mmada_head_logprobs(None, None, 1, 0, 8, None, None, None, None, None, None) != 0
    assert b"no forward resident" in lib.mmada_last_error()
    assert lib.mmada_score_buffer_bytes(None) == 0
