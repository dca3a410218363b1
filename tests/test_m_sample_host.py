"""The M samplers' device draws, host side (no GPU): the C ABI of mmada_image_sample_m, mmada_image_commit_m_sampled,
mmada_text_draw_cfg and mmada_sample_remask_gumbel, the re-mask Gumbel value of csrc/sample_noise.h against the Philox mirror of
test_sample_host.py, the refusals that come before the device is touched, and the generators' refusals on a stub model."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT
from mmada_parallel_amd import abi
from mmada_parallel_amd.generators.interleave_generator import interleave_generate
from mmada_parallel_amd.generators.t2i_generator import t2i_generate
from test_image_sample_host import IMAGE_COUNTER, NORMAL_KEY_XOR, SEED, mirror_normal_words
from test_sample_host import mirror_u32
from test_score_host import StubScore

NEW = {"mmada_image_sample_m": 15, "mmada_image_commit_m_sampled": 15, "mmada_text_draw_cfg": 13, "mmada_sample_remask_gumbel": 3}


def g_tol(g64):
    """The bound of tests/test_gpu_sample.py::test_g_is_accurate_for_every_value_of_u: two fp32 logarithms, each off by at most 2
    ulp, leave g = -log(-log(u)) within 2^-22 (1 + |g|) of its exact value, and the bound there is twice that, 2^-21 (1 + |g|).  Two
    evaluations that each meet the first figure — the host's logf, numpy's fp32 log, the device's — differ by at most the second."""
    return 2.0 ** -21 * (1.0 + np.abs(g64))


def test_the_four_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmada_mi355x.h")).read(), flags=re.S)
    lib = abi.lib()
    for sym, nargs in NEW.items():
        assert sym in abi.SIGNATURES and len(abi.SIGNATURES[sym][1]) == nargs, sym
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, f"{sym}: the header declares another argument count"
        assert hasattr(lib, sym), f"{sym} is not exported"
    assert abi.SIGNATURES["mmada_sample_remask_gumbel"][0] is C.c_float
    assert abi.SIGNATURES["mmada_image_sample_m"][1][8] is C.c_uint64 and abi.SIGNATURES["mmada_image_commit_m_sampled"][1][9] is C.c_uint64
    assert abi.SIGNATURES["mmada_text_draw_cfg"][1][9] is C.c_uint64 and abi.SIGNATURES["mmada_text_draw_cfg"][1][8] is C.c_float
    assert lib.mmada_abi_version() == 1


def test_remask_gumbel_is_the_gumbel_value_of_the_normal_blocks_first_word():
    """mmada_sample_remask_gumbel(seed, counter, r) = -log(-log(u(word))) in fp32 with word = mmada_sample_word(seed ^ XOR, counter,
    r, 0) — the mirror's word 0 of the block the normal value uses — within g_tol of numpy's fp32 evaluation and of float64."""
    lib = abi.lib()
    worst = 0.0
    for seed, counter, r0, n in ((SEED, IMAGE_COUNTER, 0, 1 << 12), (SEED ^ 0x55, (1 << 32) + 5, (1 << 32) - (1 << 10), 1 << 10),
                                 (0, 0, 0, 1 << 10), (2 ** 64 - 1, 2 ** 64 - 1, 12345, 1 << 10)):
        r = np.arange(r0, r0 + n, dtype=np.uint64)
        words = np.array([lib.mmada_sample_word(seed ^ NORMAL_KEY_XOR, counter, int(x), 0) for x in r], dtype=np.uint64)
        assert (words == mirror_normal_words(seed, counter, r)[0]).all(), "not word 0 of the normal value's block"
        u = np.array([lib.mmada_sample_uniform(int(w)) for w in words], dtype=np.float32)
        assert (u == mirror_u32(words)).all()
        g32 = -np.log(-np.log(u))
        assert g32.dtype == np.float32
        g64 = -np.log(-np.log(u.astype(np.float64)))
        got = np.array([lib.mmada_sample_remask_gumbel(seed, counter, int(x)) for x in r], dtype=np.float64)
        assert np.isfinite(got).all()
        ratio = max(float((np.abs(got - g32.astype(np.float64)) / g_tol(g64)).max()), float((np.abs(got - g64) / g_tol(g64)).max()))
        worst = max(worst, ratio)
    print(f"host g_remask against numpy fp32 and float64: worst |difference| / (2^-21 (1 + |g64|)) = {worst:.3f}")
    assert worst <= 1.0


def test_bad_arguments_are_refused_without_a_gpu():
    """Every refusal comes before the device is touched: the pointers below are host memory that no check reads."""
    lib = abi.lib()
    mem = (C.c_uint64 * 8)()
    p = C.addressof(mem)

    def sample(h=p, cond=p, unc=p, CB=8, col0=0, counter=p, sampled=p, p_sel=p):
        return lib.mmada_image_sample_m(h, cond, unc, 1, 4, CB, 3.5, col0, 1, counter, sampled, p_sel, None, None, None)

    def commit(h=p, ids=p, pos=p, samp=p, p_in=p, temp=p, counter=p, mlen=p):
        return lib.mmada_image_commit_m_sampled(h, ids, 1, 16, pos, 4, samp, p_in, temp, 1, counter, mlen, 100, None, None)

    def draw(h=p, cond=p, unc=p, V=8, ld=8, temperature=0.7, counter=p, x0=p):
        return lib.mmada_text_draw_cfg(h, cond, unc, 1.5, 1, 4, V, ld, temperature, 1, counter, x0, None)

    for kw in (dict(h=None), dict(cond=None), dict(unc=None), dict(counter=None), dict(sampled=None), dict(p_sel=None)):
        assert sample(**kw) != 0 and b"mmada_image_sample_m: null argument" in lib.mmada_last_error(), kw
    for cb in (0, 12, 16384 + 8):
        assert sample(CB=cb) != 0 and b"multiple of 8 and <= 16384" in lib.mmada_last_error(), cb
    assert sample(col0=-1) != 0 and b"col0=-1" in lib.mmada_last_error()
    for kw in (dict(h=None), dict(ids=None), dict(pos=None), dict(samp=None), dict(p_in=None), dict(temp=None), dict(counter=None),
               dict(mlen=None)):
        assert commit(**kw) != 0 and b"mmada_image_commit_m_sampled: null argument" in lib.mmada_last_error(), kw
    for kw in (dict(h=None), dict(cond=None), dict(unc=None), dict(counter=None), dict(x0=None)):
        assert draw(**kw) != 0 and b"mmada_text_draw_cfg: null argument" in lib.mmada_last_error(), kw
    for t in (float("inf"), float("nan"), -0.5):
        assert draw(temperature=t) != 0 and b"not a finite value >= 0" in lib.mmada_last_error(), t
    assert draw(V=9, ld=8) != 0 and draw(V=8, ld=12) != 0 and draw(V=0) != 0
    assert b"text_draw_cfg" in lib.mmada_last_error()


def test_generators_refuse_bad_sampler_arguments_on_a_stub_model():
    stub = StubScore()
    ids = torch.zeros(4, dtype=torch.long)
    for kw, match in ((dict(image_sampler="gpu", sampler_seed=1), "image_sampler='gpu'"),
                      (dict(text_sampler="gpu", sampler_seed=1), "text_sampler='gpu'"),
                      (dict(image_sampler="device"), "image_sampler='device' needs sampler_seed"),
                      (dict(text_sampler="device", text_temperature=0.7), "text_sampler='device' needs sampler_seed"),
                      (dict(text_sampler="device", sampler_seed=1, text_temperature=0.0), "text_sampler='device' needs text_temperature > 0")):
        with pytest.raises(ValueError, match=match):
            interleave_generate(stub, ids, ids, **kw)
    stub.tp_size = 2
    with pytest.raises(ValueError, match="image_sampler='device' needs one rank"):
        interleave_generate(stub, ids, ids, image_sampler="device", sampler_seed=1)
    stub.tp_size = 1
    for kw, match in ((dict(image_sampler="gpu", sampler_seed=1), "image_sampler='gpu'"),
                      (dict(image_sampler="device"), "image_sampler='device' needs sampler_seed")):
        with pytest.raises(ValueError, match=match):
            t2i_generate(stub, input_ids=ids[None], mask_token_id=int(stub.config.get("mask_token_id", 126336)), **kw)


# Every refusal of the five generators' device samplers, word for word as each generator has always raised it (the one shared check,
# generators/sampler_options.check_samplers, must keep the per-caller wordings): (keywords, tensor-parallel?, MMADA_MICROBATCH, message)
VALUE = "{}='gpu': 'torch' or 'device'"
NO_TEXT_DRAW = "text_sampler='device' needs {} > 0 (at 0 the text step is an arg-max: nothing is drawn)"
NO_IMAGE_DRAW = "image_sampler='device' needs temperature > 0 (at 0 the image step is an arg-max: nothing is drawn)"
ONE_RANK = "{}='device' needs one rank (tensor parallelism is out of scope)"
LANES = "text_sampler='device' needs a forward without micro-batched lanes (MMADA_MICROBATCH=1 splits the batch)"
SEEDLESS = "{}='device' needs sampler_seed"
DEV_TEXT, DEV_IMG = dict(text_sampler="device", sampler_seed=1), dict(image_sampler="device", sampler_seed=1)
REFUSALS = {
    "generate_ti2ti": [
        (dict(text_sampler="gpu", sampler_seed=1), False, None, VALUE.format("text_sampler")),
        (dict(image_sampler="gpu", sampler_seed=1), False, None, VALUE.format("image_sampler")),
        (dict(DEV_TEXT, text_temperature=0.0), False, None, NO_TEXT_DRAW.format("text_temperature")),
        (dict(DEV_TEXT, remasking="random"), False, None, "text_sampler='device' needs remasking == 'low_confidence'"),
        (DEV_TEXT, True, None, "text_sampler='device' needs one rank (the vocabulary-parallel draw is a follow-up)"),
        (DEV_TEXT, False, "1", LANES),
        (dict(text_sampler="device"), False, None, SEEDLESS.format("text_sampler")),
        (dict(DEV_IMG, temperature=0.0), False, None, NO_IMAGE_DRAW),
        (dict(DEV_IMG, temperature=-1.0), False, None, NO_IMAGE_DRAW),
        (DEV_IMG, True, None, ONE_RANK.format("image_sampler")),
        (dict(image_sampler="device"), False, None, SEEDLESS.format("image_sampler")),
    ],
    "interleave_generate": [
        (dict(text_sampler="gpu", sampler_seed=1), False, None, VALUE.format("text_sampler")),
        (dict(image_sampler="gpu", sampler_seed=1), False, None, VALUE.format("image_sampler")),
        (dict(DEV_TEXT, text_temperature=0.0), False, None, NO_TEXT_DRAW.format("text_temperature")),
        (dict(DEV_TEXT, text_temperature=0.7), True, None, ONE_RANK.format("text_sampler")),
        (dict(text_sampler="device", text_temperature=0.7), False, None, SEEDLESS.format("text_sampler")),
        (DEV_IMG, True, None, ONE_RANK.format("image_sampler")),
        (dict(image_sampler="device"), False, None, SEEDLESS.format("image_sampler")),
    ],
    "t2i_generate": [
        (dict(image_sampler="gpu", sampler_seed=1), False, None, VALUE.format("image_sampler")),
        (DEV_IMG, True, None, ONE_RANK.format("image_sampler")),
        (dict(image_sampler="device"), False, None, SEEDLESS.format("image_sampler")),
    ],
    "generate_image": [
        (dict(image_sampler="gpu", sampler_seed=1), False, None, VALUE.format("image_sampler")),
        (dict(DEV_IMG, temperature=0.0), False, None, NO_IMAGE_DRAW),
        (DEV_IMG, True, None, ONE_RANK.format("image_sampler")),
        (dict(image_sampler="device"), False, None, SEEDLESS.format("image_sampler")),
    ],
    "mmu_generate": [
        (dict(text_sampler="gpu", sampler_seed=1, temperature=0.7), False, None, VALUE.format("text_sampler")),
        (DEV_TEXT, False, None, NO_TEXT_DRAW.format("temperature")),
        (dict(DEV_TEXT, temperature=0.7), True, None, ONE_RANK.format("text_sampler")),
        (dict(text_sampler="device", temperature=0.7), False, None, SEEDLESS.format("text_sampler")),
        (dict(DEV_TEXT, temperature=0.7), False, "1", LANES),
    ],
}


@pytest.mark.parametrize("name", REFUSALS)
def test_each_generator_refuses_in_its_own_words(name, monkeypatch):
    from mmada_parallel_amd.generators.image_generation_generator import generate_image
    from mmada_parallel_amd.generators.mmu_generator import mmu_generate
    from mmada_parallel_amd.generators.parallel_generator import generate_ti2ti

    stub = StubScore()
    ids = torch.zeros((2, 4), dtype=torch.long)
    call = {"generate_ti2ti": lambda **kw: generate_ti2ti(stub, ids, 0, 2, 2, 2, 2, **kw),
            "interleave_generate": lambda **kw: interleave_generate(stub, ids[0], ids[0], **kw),
            "t2i_generate": lambda **kw: t2i_generate(stub, input_ids=ids, mask_token_id=int(stub.config.get("mask_token_id", 126336)), **kw),
            "generate_image": lambda **kw: generate_image(stub, ids[:1], **kw),
            "mmu_generate": lambda **kw: mmu_generate(stub, ids, max_new_tokens=8, steps=4, block_length=4, **kw)}[name]
    for kw, tensor_parallel, lanes, message in REFUSALS[name]:
        for tp_size, in_library in ((2, False), (1, True)) if tensor_parallel else ((1, False),):
            stub.tp_size, stub._comm_in_library = tp_size, in_library
            with monkeypatch.context() as mp:
                mp.delenv("MMADA_MICROBATCH", raising=False)
                if lanes:
                    mp.setenv("MMADA_MICROBATCH", lanes)
                with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
                    call(**kw)
