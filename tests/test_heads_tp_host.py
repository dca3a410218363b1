"""The device samplers' gate under tensor parallelism, host side (no GPU): generators/sampler_options.check_samplers and the model's
top_logprobs / sample_tokens accept a group of two or more ranks whose exchange runs in the library over a mapped transport (the
vocabulary-parallel heads of csrc/tp_heads.hip) and keep every other refusal."""
import pytest
import torch

from mmada_parallel_amd.generators.sampler_options import check_samplers
from test_score_host import StubScore


def stub(tp_size, in_library, collective):
    m = StubScore()
    m.tp_size, m._comm_in_library, m.tp_collective = tp_size, in_library, collective
    return m


DEVICE = dict(image_sampler="device", text_sampler="device", sampler_seed=1, temperature=1.0, text_temperature=0.7)


@pytest.mark.parametrize("collective", ["pull", "copy"])
@pytest.mark.parametrize("tp_size", [2, 8])
def test_a_group_on_a_mapped_transport_takes_both_device_samplers(tp_size, collective):
    m = stub(tp_size, True, collective)
    assert m.vocab_parallel_row_heads()
    assert check_samplers(m, **DEVICE) == (True, True)
    assert check_samplers(m, image_sampler="device", sampler_seed=1) == (True, False)
    with pytest.raises(ValueError, match="^text_sampler='device' needs sampler_seed$"):       # the later refusals still apply
        check_samplers(m, **dict(DEVICE, sampler_seed=None))
    with pytest.raises(ValueError, match="text_sampler='device' needs text_temperature > 0"):
        check_samplers(m, **dict(DEVICE, text_temperature=0.0))


@pytest.mark.parametrize("tp_size, in_library, collective", [(2, True, "rccl"), (2, False, "pull"), (2, False, None), (1, True, "pull"),
                                                             (1, True, "copy"), (2, True, None)])
def test_every_other_tensor_parallel_model_is_refused_in_the_old_words(tp_size, in_library, collective):
    m = stub(tp_size, in_library, collective)
    assert not m.vocab_parallel_row_heads()
    with pytest.raises(ValueError, match=r"^text_sampler='device' needs one rank \(the vocabulary-parallel draw is a follow-up\)$"):
        check_samplers(m, **DEVICE, text_rank_note="the vocabulary-parallel draw is a follow-up")
    with pytest.raises(ValueError, match=r"^image_sampler='device' needs one rank \(tensor parallelism is out of scope\)$"):
        check_samplers(m, image_sampler="device", sampler_seed=1)
    with pytest.raises(NotImplementedError, match="one rank"):
        m.top_logprobs(torch.zeros(1), 1)
    with pytest.raises(NotImplementedError, match="one rank"):
        m.sample_tokens(torch.zeros(1), 0.7, seed=1)


def test_one_rank_is_untouched():
    m = stub(1, False, None)
    assert not m.vocab_parallel_row_heads()
    assert check_samplers(m, **DEVICE) == (True, True)
