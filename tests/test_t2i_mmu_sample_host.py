"""generate_image's and mmu_generate's device draws, host side (no GPU): the C ABI of mmada_image_sample_g and
mmada_image_commit_g_sampled, their refusals before the device is touched, the generators' refusals on a stub model, the re-mask
noise's host mirror against the definition in csrc/sample_noise.h, and the keep schedule the GPU tests rely on."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, t2i_job
from mmada_parallel_amd import abi
from mmada_parallel_amd.generators.image_generation_generator import generate_image, keep_schedule
from mmada_parallel_amd.generators.mmu_generator import mmu_generate, mmu_generate_fast
from mmada_parallel_amd.mmada import MMadaModelLM
from test_image_sample_host import IMAGE_COUNTER, NORMAL_KEY_XOR, SEED, mirror_normal_words
from test_m_sample_host import g_tol
from test_sample_host import mirror_u32
from test_score_host import StubScore

NEW = {"mmada_image_sample_g": 16, "mmada_image_commit_g_sampled": 14}


def built_lib():
    from mmada_parallel_amd import build

    if not os.path.exists(build.LIB_PATH):
        pytest.skip("libmmada_mi355x.so is not built")
    return abi.lib()


def test_the_two_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmada_mi355x.h")).read(), flags=re.S)
    for sym, nargs in NEW.items():
        assert sym in abi.SIGNATURES and len(abi.SIGNATURES[sym][1]) == nargs, sym
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, f"{sym}: the header declares another argument count"
    assert len(re.findall(r"\bmmada_\w+\s*\(", hdr)) == len(set(re.findall(r"\b(mmada_\w+)\s*\(", hdr))) == 102
    # the version script exports by pattern: both names must fall under a global pattern of it
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "mmada_parallel_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:([^}]*?)local:", script, flags=re.S).group(1).split(";") if p.strip()]
    for sym in NEW:
        assert any(fnmatch.fnmatchcase(sym, p) for p in patterns), f"{sym} is not exported by exports.map"
    sig_s, sig_c = abi.SIGNATURES["mmada_image_sample_g"][1], abi.SIGNATURES["mmada_image_commit_g_sampled"][1]
    assert sig_s[6] is C.c_float and sig_s[7] is C.c_float and sig_s[9] is C.c_uint64       # cfg_scale, temperature, seed
    assert sig_c[8] is C.c_float and sig_c[9] is C.c_uint64                                # remask_temp by value, seed
    lib = built_lib()
    for sym in NEW:
        assert hasattr(lib, sym), f"{sym} is not exported"
    assert lib.mmada_abi_version() == 1


def test_bad_arguments_are_refused_without_a_gpu():
    """Every refusal comes before the device is touched: the pointers below are host memory that no check reads."""
    lib = built_lib()
    mem = (C.c_uint64 * 8)()
    p = C.addressof(mem)

    def sample(h=p, cond=p, unc=p, CB=8, temperature=1.0, col0=0, counter=p, sampled=p, p_sel=p):
        return lib.mmada_image_sample_g(h, cond, unc, 1, 4, CB, 3.5, temperature, col0, 1, counter, sampled, p_sel, None, None, None)

    def commit(h=p, ids=p, pos=p, samp=p, p_in=p, counter=p, keep=p):
        return lib.mmada_image_commit_g_sampled(h, ids, 1, 16, pos, 4, samp, p_in, 0.6, 1, counter, keep, 100, None)

    for kw in (dict(h=None), dict(cond=None), dict(unc=None), dict(counter=None), dict(sampled=None), dict(p_sel=None)):
        assert sample(**kw) != 0 and b"mmada_image_sample_g: null argument" in lib.mmada_last_error(), kw
    for t in (float("inf"), float("nan"), -0.5):
        assert sample(temperature=t) != 0 and b"not a finite value >= 0" in lib.mmada_last_error(), t
    for cb in (0, 12, 16384 + 8):
        assert sample(CB=cb) != 0 and b"multiple of 8 and <= 16384" in lib.mmada_last_error(), cb
    assert sample(col0=-1) != 0 and b"col0=-1" in lib.mmada_last_error()
    for kw in (dict(h=None), dict(ids=None), dict(pos=None), dict(samp=None), dict(p_in=None), dict(counter=None), dict(keep=None)):
        assert commit(**kw) != 0 and b"mmada_image_commit_g_sampled: null argument" in lib.mmada_last_error(), kw


def test_remask_gumbel_mirror_agrees_with_the_definition():
    """sample_noise.h: sample_remask_gumbel(seed, counter, r) = sample_gumbel(word 0 of the block (0, r, counter) under the key seed ^
    SAMPLE_NORMAL_KEY_XOR) — the value mmada_image_commit_g_sampled rounds to bf16.  The host mirror returns it within the bound of
    test_m_sample_host.py (two fp32 logarithms) of numpy's fp32 evaluation and of float64."""
    lib = built_lib()
    for seed, counter, rows in ((SEED, IMAGE_COUNTER, (0, 1, 2, 1023)), (77, IMAGE_COUNTER + 5, (0, 3, 4095)), (0, 0, (0, 7)),
                                (2 ** 64 - 1, (1 << 32) + 5, (12345, 2 ** 32 - 1))):
        r = np.array(rows, dtype=np.uint64)
        words = np.array([lib.mmada_sample_word(seed ^ NORMAL_KEY_XOR, counter, int(x), 0) for x in r], dtype=np.uint64)
        assert (words == mirror_normal_words(seed, counter, r)[0]).all(), "not word 0 of the re-mask block"
        u = np.array([lib.mmada_sample_uniform(int(w)) for w in words], dtype=np.float32)
        assert (u == mirror_u32(words)).all()
        g32 = (-np.log(-np.log(u))).astype(np.float64)
        g64 = -np.log(-np.log(u.astype(np.float64)))
        got = np.array([lib.mmada_sample_remask_gumbel(seed, counter, int(x)) for x in r], dtype=np.float64)
        assert np.isfinite(got).all()
        assert (np.abs(got - g32) <= g_tol(g64)).all() and (np.abs(got - g64) <= g_tol(g64)).all(), (seed, counter)


def test_keep_schedule_of_the_job_that_empties_its_mask_early():
    """The GPU test's early-emptying job: 4 slots, 8 timesteps, keep_n = floor(4 * schedule((step + 1) / 8)) floored at 1, 0 on the
    last step.  3, 3, 2, 2, 1, 1, 1, 0 is that rule under the linear schedule 1 - t (3.5, 3, 2.5, 2, 1.5, 1, 0.5), which the job
    passes as noise_schedule; under the default cosine schedule 4 * cos(pi / 2 * (step + 1) / 8) = 3.92, 3.70, 3.33, 2.83, 2.22,
    1.53, 0.78 gives 3, 3, 3, 2, 2, 1, 1, 0.  Under either, a step keeps at most unknown - 1 slots masked, so 4 slots are all
    known after four steps and the later steps have nothing to do."""
    assert keep_schedule(4, 8, lambda t: 1.0 - t) == [3, 3, 2, 2, 1, 1, 1, 0]
    assert keep_schedule(4, 8) == [3, 3, 3, 2, 2, 1, 1, 0]
    for sched in ([3, 3, 2, 2, 1, 1, 1, 0], [3, 3, 3, 2, 2, 1, 1, 0]):
        unknown = 4
        for step, keep in enumerate(sched):
            unknown = max(0, min(keep, unknown - 1))        # keep_n.clamp(0, unknown - 1) stay masked, at most
            assert step < 5 or unknown == 0


class Untouchable:
    """Stands where the library and the handle would: any use is device work."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} touched before the refusal")


def stub_model(cls=StubScore):
    stub = cls.__new__(cls)
    StubScore.__init__(stub)
    stub._lib = stub._handle = Untouchable()
    return stub


def test_generate_image_refuses_bad_sampler_arguments_on_a_stub_model():
    stub, job = stub_model(), t2i_job()
    kw = dict(seq_len=job["seq_len"], newline_every=job["newline_every"], uncon_ids=job["uncon_ids"], code_start=job["code_start"])
    for extra, match in ((dict(image_sampler="gpu", sampler_seed=1), "image_sampler='gpu'"),
                         (dict(image_sampler="device", sampler_seed=1, temperature=0.0), "image_sampler='device' needs temperature > 0"),
                         (dict(image_sampler="device", sampler_seed=1, temperature=-1.0), "image_sampler='device' needs temperature > 0"),
                         (dict(image_sampler="device"), "image_sampler='device' needs sampler_seed"),
                         (dict(image_sampler="device", graph=True), "image_sampler='device' needs sampler_seed")):
        with pytest.raises(ValueError, match=match):
            generate_image(stub, job["prompt"], **kw, **extra)
    for tp_size, in_lib in ((2, False), (1, True)):
        stub.tp_size, stub._comm_in_library = tp_size, in_lib
        with pytest.raises(ValueError, match="image_sampler='device' needs one rank"):
            generate_image(stub, job["prompt"], image_sampler="device", sampler_seed=1, **kw)


def test_mmu_generate_refuses_bad_sampler_arguments_on_a_stub_model(monkeypatch):
    class StubLM(MMadaModelLM, StubScore):
        pass

    idx = torch.zeros((2, 4), dtype=torch.long)
    kw = dict(max_new_tokens=8, steps=4, block_length=4)
    for stub in (stub_model(), stub_model(StubLM)):
        method = isinstance(stub, MMadaModelLM)     # the drop-in class forwards the keywords to the same functions
        for fn in ((stub.mmu_generate, stub.mmu_generate_fast) if method else
                   (lambda *a, **k: mmu_generate(stub, *a, **k), lambda *a, **k: mmu_generate_fast(stub, *a, **k))):
            for extra, match in ((dict(text_sampler="gpu", sampler_seed=1, temperature=0.7), "text_sampler='gpu'"),
                                 (dict(text_sampler="device", sampler_seed=1), "text_sampler='device' needs temperature > 0"),
                                 (dict(text_sampler="device", temperature=0.7), "text_sampler='device' needs sampler_seed")):
                with pytest.raises(ValueError, match=match):
                    fn(idx, **kw, **extra)
            with monkeypatch.context() as mp:
                mp.setenv("MMADA_MICROBATCH", "1")
                with pytest.raises(ValueError, match="text_sampler='device' needs a forward without micro-batched lanes"):
                    fn(idx, text_sampler="device", temperature=0.7, sampler_seed=1, **kw)
            for tp_size, in_lib in ((2, False), (1, True)):
                stub.tp_size, stub._comm_in_library = tp_size, in_lib
                with pytest.raises(ValueError, match="text_sampler='device' needs one rank"):
                    fn(idx, text_sampler="device", temperature=0.7, sampler_seed=1, **kw)
            stub.tp_size, stub._comm_in_library = 1, False
