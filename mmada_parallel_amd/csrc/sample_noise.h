// sample_noise.h — the noise of the sampling head (EPI_ROWSAMPLE, mmada_head_sample): a counter-based generator, so that the
// Gumbel value of (seed, counter, row, column) is a pure function — the same in the GEMM epilogue of either accumulator layout,
// in the elementwise probe (mmada_probe_gumbel) and on the host (mmada_sample_word), whatever tile or column range asks for it.
//
//   word(seed, counter, row, col) = word (col & 3) of Philox4x32-10 [Salmon et al., SC'11; Random123]
//       counter block (col >> 2, row, counter_lo32, counter_hi32), key (seed_lo32, seed_hi32),
//       multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds, key bumped after each round
//   u = (2 * (word >> 9) + 1) * 2^-24      exact in fp32, strictly inside (0, 1), 2^23 values
//   g = -log(-log(u))                      fp32, logf twice (tests/test_gpu_sample.py holds it against float64 for every u)
//   key = x + T * g                        two roundings, no FMA: x the bf16-rounded logit as fp32
// row: index of the row inside the call; col: column in the WHOLE vocabulary.  Four consecutive columns from a multiple of 4
// share one Philox evaluation.
//
// The image step (mmada_image_sample, mmada_image_commit_sampled) draws its tokens with the same g at T = 1 and adds the re-mask
// noise, a standard-normal value per image position r = b * N + n:
//   (word0, word1) = words 0, 1 of Philox4x32-10, counter block (0, r, counter_lo32, counter_hi32), key seed ^ SAMPLE_NORMAL_KEY_XOR
//                    — another key than the token draw's, so the two streams never share a block
//   z = sqrtf(-2 logf(u(word0))) * cosf(2 pi u(word1))      fp32 Box-Muller, no FMA; |z| <= sqrt(48 ln 2) ~ 5.77
// and the commit uses z rounded to bf16 (the reference's randn is bf16: generators/parallel_generator.py:30-36).
//
// The M image step (mmada_image_sample_m, mmada_image_commit_m_sampled) draws its tokens the same way and re-masks with Gumbel
// noise (MMaDA-Parallel-M/models/sampling.py:15-17), a value per image position r = b * N + n from the SAME block as z:
//   g_remask = -log(-log(u(word0)))     word0 as above: = g(seed ^ SAMPLE_NORMAL_KEY_XOR, counter, row r, column 0)
// and the commit uses g_remask rounded to bf16 (the reference's uniform_ and its two logs are bf16 tensors).  The M text draw
// (mmada_text_draw_cfg) is sample_key over the CFG-combined logits with g(seed, counter, row b * T + t, column v).
//
// The generate_image step (mmada_image_sample_g, mmada_image_commit_g_sampled) draws its tokens with sample_key at the run's
// temperature — key = l + T * g, the row-head's key — and re-masks with the same g_remask rounded to bf16.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SN_FN __host__ __device__ inline
#else
#define SN_FN inline
#endif

SN_FN uint32_t sn_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// Philox4x32-10 on the counter block (c0, c1, c2, c3) and the key (k0, k1), in place.  The ten rounds stay a LOOP: the GEMM
// epilogues evaluate this once per fragment inside fully unrolled loops over a wave's rows, and with the rounds unrolled too that
// body passes the size up to which the compiler honours `#pragma unroll` — the row loop then stays rolled and indexes the
// accumulators by a variable, which puts them all into scratch.
SN_FN void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma clang loop unroll(disable)
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = sn_mulhi(M0, c0), lo0 = M0 * c0, hi1 = sn_mulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
}

// the four words of columns 4 * col4 .. 4 * col4 + 3 of a row
SN_FN void sample_words4(uint64_t seed, uint64_t counter, uint32_t row, uint32_t col4, uint32_t& w0, uint32_t& w1, uint32_t& w2, uint32_t& w3) {
    w0 = col4; w1 = row; w2 = (uint32_t)counter; w3 = (uint32_t)(counter >> 32);
    philox4x32_10(w0, w1, w2, w3, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// word i of a block (selects, not an indexed read)
SN_FN uint32_t sample_pick(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t i) {
    const uint32_t lo = (i & 1u) ? w1 : w0, hi = (i & 1u) ? w3 : w2;
    return (i & 2u) ? hi : lo;
}
SN_FN uint32_t sample_word(uint64_t seed, uint64_t counter, uint32_t row, uint32_t col) {
    uint32_t w0, w1, w2, w3;
    sample_words4(seed, counter, row, col >> 2, w0, w1, w2, w3);
    return sample_pick(w0, w1, w2, w3, col & 3u);
}

SN_FN float sample_uniform(uint32_t word) { return (float)(2u * (word >> 9) + 1u) * 5.9604644775390625e-08f; }

SN_FN float sample_gumbel(uint32_t word) {
#pragma clang fp contract(off)
    return -logf(-logf(sample_uniform(word)));
}

// the value the draw maximises: fadd_rn(x, fmul_rn(T, g)).  T == 0: x itself
SN_FN float sample_key(float x, float T, float g) {
#pragma clang fp contract(off)
    const float tg = T * g;
    return x + tg;
}

// the re-mask noise of image position r: its two words, and z from them
constexpr uint64_t SAMPLE_NORMAL_KEY_XOR = 0x5851F42D4C957F2Dull;
SN_FN void sample_normal_words(uint64_t seed, uint64_t counter, uint32_t r, uint32_t& w0, uint32_t& w1) {
    uint32_t w2, w3;
    sample_words4(seed ^ SAMPLE_NORMAL_KEY_XOR, counter, r, 0u, w0, w1, w2, w3);
}
SN_FN float sample_normal_of(uint32_t w0, uint32_t w1) {
#pragma clang fp contract(off)
    const float radius = sqrtf(-2.0f * logf(sample_uniform(w0)));
    const float angle = 6.28318530717958647692f * sample_uniform(w1);
    return radius * cosf(angle);
}
SN_FN float sample_normal(uint64_t seed, uint64_t counter, uint32_t r) {
    uint32_t w0, w1;
    sample_normal_words(seed, counter, r, w0, w1);
    return sample_normal_of(w0, w1);
}
// the M variant's re-mask noise of image position r: the Gumbel value of the same block's word 0
SN_FN float sample_remask_gumbel(uint64_t seed, uint64_t counter, uint32_t r) {
    uint32_t w0, w1;
    sample_normal_words(seed, counter, r, w0, w1);
    return sample_gumbel(w0);
}
