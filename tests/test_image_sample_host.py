"""The image step's device sampler, host side (no GPU): the re-mask noise of csrc/sample_noise.h — a standard-normal value per image
position, reached through mmada_sample_normal — against float64 Box-Muller on the words of the Philox mirror of test_sample_host.py,
the distribution the SPECIFICATION gives (through the mirror), the token draw's stream at the image counter, and the C ABI of the
new entry points."""
import ctypes as C
import math
import os
import re

import numpy as np
import torch

from helpers import ROOT
from mmada_parallel_amd import abi
from test_sample_host import MASK32, mirror_u32, mirror_word, philox4x32_10

SEED = 0x0123456789abcdef
NORMAL_KEY_XOR = 0x5851F42D4C957F2D
IMAGE_COUNTER = 1 << 62          # where generate_ti2ti(image_sampler="device") starts the image counter
Z_TOL = 2.0 ** -17               # tests/test_gpu_image_sample.py::test_probe_words_and_z derives it


def mirror_normal_words(seed, counter, r):
    """(word0, word1) of the specification: Philox4x32-10 on (0, r, counter low, counter high) under the key seed ^ NORMAL_KEY_XOR."""
    key = np.uint64(seed ^ NORMAL_KEY_XOR)
    counter = np.asarray(counter, dtype=np.uint64)
    r = np.asarray(r, dtype=np.uint64)
    w = philox4x32_10((np.zeros_like(r), r, counter & MASK32, counter >> np.uint64(32)), (key & MASK32, key >> np.uint64(32)))
    return w[0], w[1]


def z_float64(w0, w1):
    """sqrt(-2 log u1) cos(2 pi u2) in float64 on the exact u."""
    u1, u2 = mirror_u32(w0).astype(np.float64), mirror_u32(w1).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def test_signatures_of_the_new_entry_points():
    new = {"mmada_image_sample": 17, "mmada_image_commit_sampled": 15, "mmada_probe_normal": 8, "mmada_sample_normal": 3}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmada_mi355x.h")).read(), flags=re.S)
    for sym, nargs in new.items():
        assert sym in abi.SIGNATURES and len(abi.SIGNATURES[sym][1]) == nargs, sym
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, f"{sym}: the header declares another argument count"
    assert abi.SIGNATURES["mmada_sample_normal"][0] is C.c_float
    assert abi.SIGNATURES["mmada_image_sample"][1][10] is C.c_uint64 and abi.SIGNATURES["mmada_image_commit_sampled"][1][9] is C.c_uint64
    assert abi.lib().mmada_abi_version() == 1


def test_bad_arguments_are_refused_without_a_gpu():
    """Every refusal comes before the device is touched: the pointers below are host memory that no check reads."""
    lib = abi.lib()
    mem = (C.c_uint64 * 8)()
    p = C.addressof(mem)

    def sample(h=p, cond=p, B=1, N=4, CB=8, col0=0, counter=p, sampled=p, p_sel=p):
        return lib.mmada_image_sample(h, cond, None, None, B, N, CB, 0.0, 0.0, col0, 1, counter, sampled, p_sel, None, None, None)

    def commit(h=p, ids=p, pos=p, samp=p, p_in=p, temp=p, counter=p, mlen=p):
        return lib.mmada_image_commit_sampled(h, ids, 1, 16, pos, 4, samp, p_in, temp, 1, counter, mlen, 100, 8, None)

    for kw in (dict(h=None), dict(cond=None), dict(counter=None), dict(sampled=None), dict(p_sel=None)):
        assert sample(**kw) != 0 and b"mmada_image_sample: null argument" in lib.mmada_last_error(), kw
    for cb in (0, -8, 12, 16384 + 8):
        assert sample(CB=cb) != 0 and b"multiple of 8 and <= 16384" in lib.mmada_last_error(), cb
    assert sample(col0=-1) != 0 and b"col0=-1" in lib.mmada_last_error()
    assert sample(col0=2 ** 31 - 4) != 0 and b"col0" in lib.mmada_last_error()       # col0 + CB passes 2^31
    assert sample(B=0) == 0 and sample(N=0) == 0 and sample(B=-1) == 0               # nothing to do, as mmada_image_probs
    for kw in (dict(h=None), dict(ids=None), dict(pos=None), dict(samp=None), dict(p_in=None), dict(temp=None), dict(counter=None),
               dict(mlen=None)):
        assert commit(**kw) != 0 and b"mmada_image_commit_sampled: null argument" in lib.mmada_last_error(), kw
    assert lib.mmada_probe_normal(1, 0, 0, 0, p, None, None, None) != 0 and b"mmada_probe_normal" in lib.mmada_last_error()
    assert lib.mmada_probe_normal(1, 0, 0, 8, None, None, None, None) != 0 and b"mmada_probe_normal" in lib.mmada_last_error()
    assert lib.mmada_probe_normal(1, 0, -1, 8, p, None, None, None) != 0


def test_sample_normal_is_box_muller_on_the_mirrors_words():
    """mmada_sample_normal — the code the kernels compile, with the host's logf / cosf — against float64 Box-Muller on the mirror's
    words under the key seed ^ NORMAL_KEY_XOR: |z - z64| <= 2^-17, on both sides of counter = 2^32 and at the image counter."""
    lib = abi.lib()
    worst = 0.0
    for seed, counter, r0, n in ((SEED, IMAGE_COUNTER, 0, 1 << 14), (SEED ^ 0x55, (1 << 32) + 5, (1 << 32) - (1 << 12), 1 << 12),
                                 (0, 0, 0, 1 << 12), (2 ** 64 - 1, 2 ** 64 - 1, 12345, 1 << 12)):
        r = np.arange(r0, r0 + n, dtype=np.uint64)
        z64 = z_float64(*mirror_normal_words(seed, counter, r))
        z = np.array([lib.mmada_sample_normal(seed, counter, int(x)) for x in r], dtype=np.float64)
        assert np.isfinite(z).all() and np.abs(z).max() <= math.sqrt(48 * math.log(2))
        worst = max(worst, float(np.abs(z - z64).max()))
    print(f"host z against float64 Box-Muller: worst |z - z64| = {worst:.3e} (limit {Z_TOL:.3e})")
    assert worst <= Z_TOL
    # another key than the token draw's: the words are not those of column block 0 of the same (seed, counter, row)
    w0, _ = mirror_normal_words(SEED, 5, np.arange(64, dtype=np.uint64))
    assert (w0 != mirror_word(SEED, 5, np.arange(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64))).all()


def test_the_specified_noise_is_normal():
    """Kolmogorov-Smirnov distance of z (float64 Box-Muller on the exact u) to the normal law, n = 2^18 rows at the image counter,
    times sqrt(n): the limit of the uniform test of test_sample_host.py.  Measured 1.2296."""
    n = 1 << 18
    z = np.sort(z_float64(*mirror_normal_words(SEED, IMAGE_COUNTER, np.arange(n, dtype=np.uint64))))
    cdf = (0.5 * (1.0 + torch.erf(torch.from_numpy(z) / math.sqrt(2.0)))).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max())) * n ** 0.5
    print(f"KS distance of z to the normal law, times sqrt(n), n = {n}: {ks:.4f}")
    assert ks < 1.95, ks


def test_the_token_draw_at_the_image_counter_samples_the_softmax():
    """float64 Gumbel-max at T = 1 over the eight logits of test_sample_host.py's chi-square test, at the first eight codebook
    columns (126356 ...: not a multiple of 4 apart from the block boundary) and the image counter: chi-square against softmax(logits),
    7 degrees of freedom, p = 1e-3.  Measured 5.15."""
    logits = np.array([2, 1.5, 1, .5, 0, -.5, -1, -3], dtype=np.float64)
    R = 65536
    row, col = np.meshgrid(np.arange(R, dtype=np.uint64), np.arange(126356, 126364, dtype=np.uint64), indexing="ij")
    u = mirror_u32(mirror_word(SEED, IMAGE_COUNTER, row, col)).astype(np.float64)
    draw = (logits[None, :] - np.log(-np.log(u))).argmax(1)
    p = np.exp(logits)
    expect = p / p.sum() * R
    chi2 = float((((np.bincount(draw, minlength=8) - expect) ** 2) / expect).sum())
    print(f"chi-square of {R} Gumbel-max draws at counter 2^62 against softmax(logits): {chi2:.2f}")
    assert chi2 < 24.32, chi2
