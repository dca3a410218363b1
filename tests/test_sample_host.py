"""The sampling head, host side (no GPU): the noise definition of csrc/sample_noise.h — Philox4x32-10 words, reached through
mmada_sample_word, against a mirror written here and Random123's known answers —, the map from a word to a uniform value, the
distribution the SPECIFICATION gives (through the mirror: a property of the definition, checked where it can be), and the C ABI
of the new entry points."""
import ctypes as C
import os
import re

import numpy as np

from helpers import ROOT
from mmada_parallel_amd import abi

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 on arrays: ctr = (c0, c1, c2, c3), key = (k0, k1), each uint64 arrays holding 32-bit values.  Returns 4 words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32   # bumped after each round
    return c0, c1, c2, c3


def mirror_word(seed, counter, row, col):
    """word(seed, counter, row, col) of the specification, on uint64 arrays."""
    seed, counter, row, col = (np.asarray(a, dtype=np.uint64) for a in (seed, counter, row, col))
    w = philox4x32_10((col >> np.uint64(2), row, counter & MASK32, counter >> np.uint64(32)), (seed & MASK32, seed >> np.uint64(32)))
    sel = (col & np.uint64(3)).astype(np.int64)
    return np.choose(sel, [np.broadcast_to(x, sel.shape) for x in w])


def mirror_u32(word):
    """u = (2 * (word >> 9) + 1) * 2^-24 evaluated in fp32, as the kernels do."""
    n = (2 * (np.asarray(word, dtype=np.uint64) >> np.uint64(9)) + 1).astype(np.uint32)
    return n.astype(np.float32) * np.float32(2.0 ** -24)


def test_known_answers_and_the_library_word_equal_the_mirror():
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    lib = abi.lib()
    for ctr, key, want in kat:
        got = tuple(int(x) for x in philox4x32_10(ctr, key))
        assert got == want, f"mirror: ctr {ctr} key {key}: {[hex(g) for g in got]}"
        # the same block through the library: counter block (col >> 2, row, counter low, counter high), key (seed low, seed high)
        if ctr[0] < (1 << 30):
            seed, counter = key[0] | (key[1] << 32), ctr[2] | (ctr[3] << 32)
            assert tuple(lib.mmada_sample_word(seed, counter, ctr[1], 4 * ctr[0] + i) for i in range(4)) == want

    rng = np.random.default_rng(20261019)
    n = 4096
    seed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    counter = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    counter[::3] &= np.uint64(0xFFFFFFFF)                 # both sides of 2^32
    counter[1::3] |= np.uint64(1 << 32)
    row = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    col = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    # groups of four tuples that differ in the low two bits of col only
    for a in (seed, counter, row):
        a[:1024] = np.repeat(a[:1024:4], 4)
    col[:1024] = (np.repeat(col[:1024:4], 4) & ~np.uint64(3)) | np.tile(np.arange(4, dtype=np.uint64), 256)
    assert int(counter.max()) >= 1 << 32 and int(counter.min()) < 1 << 32
    want = mirror_word(seed, counter, row, col)
    got = np.array([lib.mmada_sample_word(int(s), int(c), int(r), int(k)) for s, c, r, k in zip(seed, counter, row, col)], dtype=np.uint64)
    assert (got == want).all(), f"{int((got != want).sum())} of {n} words differ from the mirror"
    quad = got[:1024].reshape(-1, 4)
    assert (quad[:, 0] != quad[:, 1]).all() and (quad[:, 2] != quad[:, 3]).any()   # four different words of one block


def test_uniform_map_is_exact_and_strictly_inside_the_unit_interval():
    """The library's own map (sample_uniform of csrc/sample_noise.h through mmada_sample_uniform), and the mirror the
    distribution test uses, which must be the same function."""
    words = [0, 0xffffffff, 0x1ff, 0x200]
    lib = abi.lib()
    u = np.array([lib.mmada_sample_uniform(w) for w in words], dtype=np.float32)
    assert (u == mirror_u32(words)).all()
    rng = np.random.default_rng(7)
    more = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
    got = np.array([lib.mmada_sample_uniform(int(w)) for w in more])
    assert (got == (2 * (more >> np.uint64(9)) + 1).astype(np.float64) / 2.0 ** 24).all() and (got == mirror_u32(more)).all()
    for w, x in zip(words, u.tolist()):
        exact = (2 * (w >> 9) + 1) / 2.0 ** 24                # a 24-bit odd integer over 2^24: exact in fp32 (and in float64)
        assert x == exact and 0.0 < x < 1.0, (hex(w), x)
    assert u[0] == np.float32(2.0 ** -24) and u[1] == np.float32(1.0 - 2.0 ** -24)
    assert u[2] == u[0] and u[3] == np.float32(3 * 2.0 ** -24)    # 0x1ff: still the first bucket; 0x200: the next one
    assert 1.0 - float(u[1]) == 2.0 ** -24                     # never rounds to 1


def test_the_specified_noise_is_uniform_and_gumbel_max_samples_the_softmax():
    seed = 0x0123456789abcdef
    # Kolmogorov-Smirnov distance of u to the uniform law, n = 64 rows x 4096 columns
    row, col = np.meshgrid(np.arange(64, dtype=np.uint64), np.arange(4096, dtype=np.uint64), indexing="ij")
    u = np.sort(mirror_u32(mirror_word(seed, 0, row, col)).astype(np.float64).ravel())
    n = u.size
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max(float((i / n - u).max()), float((u - (i - 1) / n).max())) * n ** 0.5
    print(f"KS distance of u to uniform, times sqrt(n), n = {n}: {ks:.4f}")
    assert ks < 1.95, ks

    # float64 Gumbel-max over eight columns, 65 536 rows: chi-square against softmax(logits / T) (7 degrees of freedom, p = 1e-3)
    logits = np.array([2, 1.5, 1, .5, 0, -.5, -1, -3], dtype=np.float64)
    T, R = 0.7, 65536
    row, col = np.meshgrid(np.arange(R, dtype=np.uint64), np.arange(40, 48, dtype=np.uint64), indexing="ij")
    u = mirror_u32(mirror_word(seed, 5, row, col)).astype(np.float64)
    g = -np.log(-np.log(u))
    draw = (logits[None, :] + T * g).argmax(1)
    p = np.exp(logits / T)
    expect = p / p.sum() * R
    chi2 = float((((np.bincount(draw, minlength=8) - expect) ** 2) / expect).sum())
    print(f"chi-square of {R} Gumbel-max draws against softmax(logits / {T}): {chi2:.2f}")
    assert chi2 < 24.32, chi2


def test_argument_errors_and_signatures_without_a_gpu():
    lib = abi.lib()
    new = {"mmada_head_sample": 14, "mmada_text_select_sampled": 13, "mmada_sample_word": 4, "mmada_probe_gumbel": 9,
           "mmada_sample_uniform": 1}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmada_mi355x.h")).read(), flags=re.S)
    for sym, nargs in new.items():
        assert sym in abi.SIGNATURES and len(abi.SIGNATURES[sym][1]) == nargs, sym
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, f"{sym}: the header declares another argument count"
    assert abi.SIGNATURES["mmada_sample_word"][0] is C.c_uint32
    assert lib.mmada_abi_version() == 1

    def refused(rc):
        err = lib.mmada_last_error()
        return rc != 0 and (b"no forward resident" in err or b"null argument" in err)

    assert refused(lib.mmada_head_sample(None, None, 1, 0, 8, 0.7, 1, None, None, None, None, None, None, None))
    assert refused(lib.mmada_text_select_sampled(None, None, 1, 4, 0.7, 1, None, None, 8, 0, None, None, None))
    assert abi.SIGNATURES["mmada_sample_uniform"][0] is C.c_float
    assert lib.mmada_probe_gumbel(1, 0, 0, 0, 0, 8, None, None, None) != 0 and b"mmada_probe_gumbel" in lib.mmada_last_error()
