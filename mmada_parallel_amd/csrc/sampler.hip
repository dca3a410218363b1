// sampler.hip — the tensor math of generate_ti2ti (generators/parallel_generator.py) as fused row kernels.
//
// These kernels are HBM-bound (one pass over [rows, vocab] bf16 logits) and integer/tie-break exact:
//   * argmax resolves ties to the LOWEST index (torch.argmax on CPU);
//   * the re-mask selection is a STABLE ascending order (torch.sort(stable) semantics observed on CPU);
//   * every bf16 rounding point of the reference is reproduced (A.7): CFG combine per op, bf16 probabilities,
//     bf16 log-confidence.
// Transcendentals are evaluated in fp64 and rounded once to the precision the reference computes in, which makes
// the device result independent of libm flavour (the CPU oracle in oracle/sampler_oracle.c does the same).
//
// Three row kernels carry every variant as template parameters, so that each rounding point above is written once:
//   text_row_stats_kernel<mode>       plain | CFG-combined | one rank's share of the vocabulary
//   image_row_kernel<MVAR, draw>      A or M combine; no draw | Gumbel-max at T = 1 | Gumbel-max at a run-time temperature
//   image_commit_kernel<MVAR, noise>  A or M re-mask rule; noise from a tensor | from the device generator
#include "kernels.h"
#include "sample_noise.h"

namespace {

constexpr int TB = 256;

// ---------------------------------------------------------------------------------------------------------------
// Reductions over the workgroup's TB / 64 waves: the wave first, then the waves in wave order.  Every thread returns the
// result.  The LDS arrays (TB / 64 entries each) are the caller's; each reduction ends with a barrier, so they may be reused.
// ---------------------------------------------------------------------------------------------------------------
MM_DEVICE float block_max(float v, float* s_v) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
    __syncthreads();
    v = s_v[0];
#pragma unroll
    for (int w = 1; w < TB / 64; ++w) v = fmaxf(v, s_v[w]);
    __syncthreads();
    return v;
}

// fp64 sum: the order of the additions (butterfly over the wave, then wave 0, 1, 2, 3) is part of the result
MM_DEVICE double block_sum_d(double v, double* s_d) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = v;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < TB / 64; ++w) tot += s_d[w];
    __syncthreads();
    return tot;
}

// first-index arg-max: value descending, index ascending (index 0 when no thread offered a candidate)
MM_DEVICE int block_argmax(float best, int bidx, float* s_v, int* s_x, float* best_out = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
    }
    if (lane == 0) { s_v[wave] = best; s_x[wave] = bidx; }
    __syncthreads();
    best = s_v[0]; bidx = s_x[0];
#pragma unroll
    for (int w = 1; w < TB / 64; ++w)
        if (s_v[w] > best || (s_v[w] == best && s_x[w] < bidx)) { best = s_v[w]; bidx = s_x[w]; }
    __syncthreads();
    if (best_out) *best_out = best;
    return bidx == 0x7fffffff ? 0 : bidx;
}

// ---------------------------------------------------------------------------------------------------------------
// Text step part 1, one workgroup per (b, t) row (generators/parallel_generator.py:185-205).  Rows whose token is not MASK
// are skipped (conf = -inf).
//   scan      16-byte chunks of eight logits, then the V % 8 tail: the first-index arg-max of `noisy` (or of the logits) and
//             the maximum of the logits
//   sum       sum_v exp(l_v - max) in fp64 (F.softmax(text_logits.to(torch.float64)), :193)
//   result    x0 = the arg-max (or x0_in[row]: an externally sampled x0, float64 Gumbel-max at text_temperature > 0),
//             conf = exp(l_x0 - max) / sum
// TEXT_CFG, the M variant (MMaDA-Parallel-M/models/modeling_mmada.py:168-199): l = cond + text_cfg * (uncond - cond), each op
// rounded to bf16.
// TEXT_PARTIAL, the vocabulary-parallel form (tensor parallelism, text_temperature == 0): this rank holds columns [col_off,
// col_off + V) only, and `noisy` and `x0_in` do not exist.  Instead of conf / x0 it publishes {local max, global index of its
// first local maximum, sum_v exp(l_v - local max)}; csrc/tp_comm.hip combines the tp records (max of maxima, the lowest rank
// holding it = the lowest column index = torch.argmax's first index, rescaled sum) into the conf / x0 the one-rank modes write.
// The published maximum is the arg-max's own value (tracked by `>`), not the fmaxf maximum: the two can differ in the sign of a
// zero, and the ranks compare the records.
// ---------------------------------------------------------------------------------------------------------------
MM_DEVICE float text_cfg_combine(float c, float u, float s) { return bfround(c + bfround(s * bfround(u - c))); }

template <TextMode MODE>
__global__ __launch_bounds__(TB) void text_row_stats_kernel(const bf16_t* __restrict__ logits,
                                                            const bf16_t* __restrict__ noisy_in,
                                                            const bf16_t* __restrict__ unc, float text_cfg,
                                                            const int32_t* __restrict__ x0_in, int T, int V, int ld, int col_off,
                                                            const int64_t* __restrict__ ids, int L, int text_start,
                                                            int mask_id, double* __restrict__ conf_out,
                                                            int32_t* __restrict__ x0_out, TextStat* __restrict__ stat_out) {
    constexpr bool CFG = MODE == TEXT_CFG, PARTIAL = MODE == TEXT_PARTIAL;
    __shared__ float s_val[TB / 64];
    __shared__ int s_idx[TB / 64];
    __shared__ double s_sum[TB / 64];
    const int row = blockIdx.x;
    const int b = row / T, t = row - b * T;
    const int tid = threadIdx.x;
    if (ids[(size_t)b * L + text_start + t] != (int64_t)mask_id) {
        if (tid == 0) {
            if constexpr (PARTIAL) {
                stat_out[row] = TextStat{-INFINITY, 0, 0.0};
            } else {
                conf_out[row] = -INFINITY;
                x0_out[row] = 0;
            }
        }
        return;
    }
    const bf16_t* noisy = PARTIAL ? nullptr : noisy_in;
    const bf16_t* lrow = logits + (size_t)row * ld;
    const bf16_t* arow = noisy ? noisy + (size_t)row * ld : lrow;
    const bf16_t* urow = CFG ? unc + (size_t)row * ld : nullptr;
    const int nchunk = V >> 3;
    // value of logit i of the (possibly CFG-combined) row
    auto lval = [&](uint32_t cbits, uint32_t ubits) -> float {
        const float c = __uint_as_float(cbits);
        if constexpr (CFG) return text_cfg_combine(c, __uint_as_float(ubits), text_cfg);
        return c;
    };

    // scan: first-index argmax of arow, max of lrow
    float best = -INFINITY, lmax = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = tid; c < nchunk; c += TB) {
        const u32x4 lv = ((const u32x4*)lrow)[c];
        u32x4 uv = lv;
        if constexpr (CFG) uv = ((const u32x4*)urow)[c];
        u32x4 av = lv;
        if (noisy) av = ((const u32x4*)arow)[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float l0 = lval(lv[j] << 16, uv[j] << 16), l1 = lval(lv[j] & 0xffff0000u, uv[j] & 0xffff0000u);
            lmax = fmaxf(lmax, fmaxf(l0, l1));
            const float lo = noisy ? __uint_as_float(av[j] << 16) : l0;
            const float hi = noisy ? __uint_as_float(av[j] & 0xffff0000u) : l1;
            if (lo > best) { best = lo; bidx = c * 8 + 2 * j; }
            if (hi > best) { best = hi; bidx = c * 8 + 2 * j + 1; }
        }
    }
    for (int i = (nchunk << 3) + tid; i < V; i += TB) {  // tail (V % 8)
        const float l = lval((uint32_t)lrow[i] << 16, CFG ? (uint32_t)urow[i] << 16 : 0u);
        lmax = fmaxf(lmax, l);
        const float a = noisy ? bf2f(arow[i]) : l;
        if (a > best || (a == best && i < bidx)) { best = a; bidx = i; }
    }
    bidx = block_argmax(best, bidx, s_val, s_idx, &best);
    if constexpr (PARTIAL) {
        lmax = best;
    } else {
        lmax = block_max(lmax, s_val);
        if (x0_in) bidx = x0_in[row];
    }

    // sum exp(l - max) in fp64
    const double dmax = (double)lmax;
    double sum = 0.0;
    for (int c = tid; c < nchunk; c += TB) {
        const u32x4 lv = ((const u32x4*)lrow)[c];
        u32x4 uv = lv;
        if constexpr (CFG) uv = ((const u32x4*)urow)[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sum += exp((double)lval(lv[j] << 16, uv[j] << 16) - dmax);
            sum += exp((double)lval(lv[j] & 0xffff0000u, uv[j] & 0xffff0000u) - dmax);
        }
    }
    for (int i = (nchunk << 3) + tid; i < V; i += TB)
        sum += exp((double)lval((uint32_t)lrow[i] << 16, CFG ? (uint32_t)urow[i] << 16 : 0u) - dmax);
    const double tot = block_sum_d(sum, s_sum);
    if (tid != 0) return;
    if constexpr (PARTIAL) {
        stat_out[row] = TextStat{best, col_off + bidx, tot};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // published: read by the other ranks (csrc/tp_comm.hip)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        const float lsel = lval((uint32_t)lrow[bidx] << 16, CFG ? (uint32_t)urow[bidx] << 16 : 0u);
        conf_out[row] = exp((double)lsel - dmax) / tot;
        x0_out[row] = bidx;
    }
}

// Text step part 2: per batch row, unmask the k highest-confidence masked positions (:207-217).
__global__ __launch_bounds__(TB) void text_commit_kernel(const double* __restrict__ conf, const int32_t* __restrict__ x0,
                                                         int T, int64_t* __restrict__ ids, int L, int text_start,
                                                         const int32_t* __restrict__ kptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* sc = (double*)smem;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k = kptr[b];
    if (k <= 0) return;
    for (int t = tid; t < T; t += TB) sc[t] = conf[(size_t)b * T + t];
    __syncthreads();
    for (int t = tid; t < T; t += TB) {
        const double c = sc[t];
        if (!(c > -INFINITY)) continue;  // only masked positions carry a finite confidence
        int rank = 0;
        for (int j = 0; j < T; ++j) {
            const double cj = sc[j];
            rank += (cj > c) || (cj == c && j < t);
        }
        if (rank < k) ids[(size_t)b * L + text_start + t] = (int64_t)x0[(size_t)b * T + t];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Image step part 1, one workgroup per (b, n) row: combine, soft-max statistics in bf16, first-index arg-max, and (draw
// instantiations) the token (generators/parallel_generator.py:282-302, 311).  The phases:
//   1 combine  l_i into LDS, with the row maximum.
//              A (:285-289): image_logits = c; += cfg_scale * (c - ut); += cfg_img * (c - ui), every op rounded to bf16.
//              M (modeling_mmada.py:216): (1 + image_cfg) * cond - image_cfg * uncond, bf16 per op — ut = the uncond branch,
//              cfg_scale = image_cfg, cfg_img = 1 + image_cfg (host-computed).
//   2 draw     (IMAGE_DRAW_UNIT, IMAGE_DRAW_TEMPERATURE) over the logits still in LDS, a Gumbel-max:
//                sampled = first-index arg-max over i < CB of sample_key(l_i, T, g(seed, *counter, row, col0 + i))   (sample_noise.h)
//              col0: the column of codebook entry 0 in the whole vocabulary (any value >= 0).  *counter is read, never written.
//              UNIT (image_sampler="device" of the A and M steps: replaces torch.multinomial + gather, :297-302, :311 and
//              modeling_mmada.py:220-222, :229-231): T is the constant 1 and `temperature` is not read.  It samples softmax(l)
//              evaluated in fp32, NOT its bf16 rounding: the reference's multinomial samples the bf16-rounded probabilities.  Like
//              the reference (:292-302) the image logits are not divided by a temperature.
//              TEMPERATURE (generate_image with image_sampler="device": replaces gumbel_max_sample + gather,
//              generators/image_generation_generator.py:152-167): T = temperature, the key of mmada_head_sample and
//              text_draw_cfg_kernel, so the draw samples softmax(l / temperature) evaluated in fp32 (the reference's bf16
//              l / temperature + g has the same arg-max in exact arithmetic); temperature == 0: the plain first-index arg-max
//              of l, no generator runs.
//   3 sum      e_i = (float)exp((double)(l_i - max)); the row sum is accumulated in fp64 (order-independent to fp32
//              precision) and rounded once: fsum.  The statistics are those of the UNSCALED l at every temperature.
//   4 token    (draw) sampled_out, and p_sel_out = f2bf(e_sampled / fsum): the probability phase 5 has for that entry.  The
//              kernel ends here when neither argmax_out nor pmax_out is wanted.
//   5 arg-max  p_i = bf16(e_i / fsum); arg-max over the bf16 values, lowest index wins.  probs_out (IMAGE_DRAW_NONE only; null =
//              skip) receives every p_i; argmax_out / pmax_out: null = skip.
// ---------------------------------------------------------------------------------------------------------------
MM_DEVICE float cfg_combine(float c, float ut, float ui, bool use_t, bool use_i, float st, float si) {
    float l = c;
    if (use_t) l = bfround(l + bfround(st * bfround(c - ut)));
    if (use_i) l = bfround(l + bfround(si * bfround(c - ui)));
    return l;
}

MM_DEVICE float cfg_combine_m(float c, float u, float one_plus, float s) {
    return bfround(bfround(one_plus * c) - bfround(s * u));
}

template <bool MVAR, ImageDraw DRAW>
__global__ __launch_bounds__(TB) void image_row_kernel(const bf16_t* __restrict__ cond, const bf16_t* __restrict__ ut,
                                                       const bf16_t* __restrict__ ui, int CB, float cfg_scale, float cfg_img,
                                                       uint32_t col0, uint64_t seed, const uint64_t* __restrict__ counter,
                                                       float temperature, bf16_t* __restrict__ probs_out,
                                                       int32_t* __restrict__ sampled_out, bf16_t* __restrict__ p_sel_out,
                                                       int32_t* __restrict__ argmax_out, bf16_t* __restrict__ pmax_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* e = (float*)smem;  // [CB]: l_i, then e_i
    __shared__ float s_f[TB / 64];
    __shared__ double s_d[TB / 64];
    __shared__ int s_i[TB / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const bool use_t = MVAR || (cfg_scale != 0.0f && ut != nullptr), use_i = !MVAR && cfg_img != 0.0f && ui != nullptr;
    const bf16_t* crow = cond + (size_t)row * CB;
    const bf16_t* trow = use_t ? ut + (size_t)row * CB : crow;
    const bf16_t* irow = use_i ? ui + (size_t)row * CB : crow;
    const int nchunk = CB >> 3;

    // 1: combine
    float mx = -INFINITY;
    for (int c = tid; c < nchunk; c += TB) {
        const u32x4 cv = ((const u32x4*)crow)[c];
        u32x4 tv = cv, iv = cv;
        if (use_t) tv = ((const u32x4*)trow)[c];
        if (use_i) iv = ((const u32x4*)irow)[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float l0, l1;
            if constexpr (MVAR) {
                l0 = cfg_combine_m(__uint_as_float(cv[j] << 16), __uint_as_float(tv[j] << 16), cfg_img, cfg_scale);
                l1 = cfg_combine_m(__uint_as_float(cv[j] & 0xffff0000u), __uint_as_float(tv[j] & 0xffff0000u), cfg_img,
                                   cfg_scale);
            } else {
                l0 = cfg_combine(__uint_as_float(cv[j] << 16), __uint_as_float(tv[j] << 16),
                                 __uint_as_float(iv[j] << 16), use_t, use_i, cfg_scale, cfg_img);
                l1 = cfg_combine(__uint_as_float(cv[j] & 0xffff0000u), __uint_as_float(tv[j] & 0xffff0000u),
                                 __uint_as_float(iv[j] & 0xffff0000u), use_t, use_i, cfg_scale, cfg_img);
            }
            e[c * 8 + 2 * j] = l0;
            e[c * 8 + 2 * j + 1] = l1;
            mx = fmaxf(mx, fmaxf(l0, l1));
        }
    }
    mx = block_max(mx, s_f);

    // 2: the draw — one Philox block per four columns of the whole vocabulary, whatever col0 & 3 is
    int sampled = 0;
    if constexpr (DRAW != IMAGE_DRAW_NONE) {
        constexpr bool TEMP = DRAW == IMAGE_DRAW_TEMPERATURE;
        const uint64_t ctr = *counter;
        const uint32_t blk0 = col0 >> 2, nblk = ((col0 + (uint32_t)CB - 1u) >> 2) - blk0 + 1u;
        const bool noisy = !TEMP || temperature != 0.0f;
        float kbest = -INFINITY;
        int kidx = 0x7fffffff;
        for (uint32_t q = tid; q < nblk; q += TB) {
            uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
            if (noisy) sample_words4(seed, ctr, (uint32_t)row, blk0 + q, w0, w1, w2, w3);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const int i = (int)(((blk0 + q) << 2) + j - col0);  // ascends per thread -> first index kept
                if (i < 0 || i >= CB) continue;
                float key = e[i];
                if (noisy) key = sample_key(key, TEMP ? temperature : 1.0f, sample_gumbel(sample_pick(w0, w1, w2, w3, j)));
                if (key > kbest) { kbest = key; kidx = i; }
            }
        }
        sampled = block_argmax(kbest, kidx, s_f, s_i);  // its barriers also end every read of the logits in e
    }

    // 3: e_i and the fp64 row sum
    double sum = 0.0;
    for (int i = tid; i < CB; i += TB) {
        const float ev = (float)exp((double)(e[i] - mx));
        e[i] = ev;
        sum += (double)ev;
    }
    const float fsum = (float)block_sum_d(sum, s_d);

    // 4: the token
    if constexpr (DRAW != IMAGE_DRAW_NONE) {
        if (tid == 0) {
            sampled_out[row] = sampled;
            p_sel_out[row] = f2bf(e[sampled] / fsum);
        }
        if (!argmax_out && !pmax_out) return;
    }

    // 5: arg-max of the bf16 probabilities
    float best = -1.0f;
    int bidx = 0x7fffffff;
    for (int i = tid; i < CB; i += TB) {
        const bf16_t pb = f2bf(e[i] / fsum);
        if constexpr (DRAW == IMAGE_DRAW_NONE)
            if (probs_out) probs_out[(size_t)row * CB + i] = pb;
        const float p = bf2f(pb);
        if (p > best) { best = p; bidx = i; }  // i ascends per thread -> first index kept
    }
    bidx = block_argmax(best, bidx, s_f, s_i, &best);
    if (tid == 0) {
        if (argmax_out) argmax_out[row] = bidx;
        if (pmax_out) pmax_out[row] = f2bf(best < 0.f ? 0.f : best);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Image step part 2, one workgroup per batch row: keep known tokens, confidence, stable lowest-k re-mask, write back
// (generators/parallel_generator.py:221-233, 304-344; mask_by_random_topk :23-70).
//   ids        A: known ids and sampled ids are clamped to the codebook.  M (MMaDA-Parallel-M/models/sampling.py:31-36 +
//              modeling_mmada.py:225-241): no clamp.  sampled_out (M with device noise only; null = skip): the id each
//              position is committed from, unknown ? sampled_in : vq - text_vocab (the reference's sampled_ids, :224-225), taken
//              from the ids this kernel READS — the barrier before the write-back separates the two.
//   confidence selected_probs = unknown ? probs[sampled] : finfo(bf16).max  (:311-315).
//              A: log(probs + 1e-10) + temperature * noise, each op rounded to bf16 (:36); torch rounds the scalar of a bf16
//              `tensor + scalar` to bf16 first, while `scalar * tensor` multiplies in fp32.  M: log(clamp(p, 1e-20)) +
//              temperature * gumbel the same way.
//   noise      COMMIT_NOISE_TENSOR: noise[b * N + n], a randn (A, :30-33) or Gumbel (M) tensor of the caller's.  A with
//              noise == null: no noise term at all.  The temperature is the by-value temp_value.
//              COMMIT_NOISE_DEVICE: the bf16 rounding of sample_normal (A) or sample_remask_gumbel (M: replaces the uniform_
//              + two logs of sampling.py:15-17) at (seed, *counter, b * N + n) (sample_noise.h).  Every workgroup reads *counter:
//              counter_bump_kernel, the launch after this one, advances it.  The temperature is read from device memory —
//              nothing that changes from step to step is a by-value argument, so a captured step replays — unless temp_dev is
//              null (generate_image, mmada_image_commit_g_sampled): then it is temp_value, a constant of the whole run there.
//   mask_len   max(1, min(unknown - 1, floor(N * ratio))) (:318-324), then clamp(…, 0, N - 1) (:43).  keep_rule
//              (generate_image, generators/image_generation_generator.py:99-103 + utils/generation_utils.py:62): k =
//              keep_n.clamp(0, unknown - 1) with keep_n supplied as is (0 on the last step) — no floor of 1, so a step with
//              nothing unknown has k = 0 and rewrites every id with itself.
//   re-mask    A: the k lowest confidences in stable order.  M: the cut-off compare confidence < sorted[mask_len] (ties with
//              the cut-off value are NOT masked).
// ---------------------------------------------------------------------------------------------------------------
template <bool MVAR, CommitNoise NOISE>
__global__ __launch_bounds__(1024) void image_commit_kernel(int64_t* __restrict__ ids, int L,
                                                            const int32_t* __restrict__ pos_map, int N,
                                                            const int32_t* __restrict__ sampled_in,
                                                            const bf16_t* __restrict__ p_in,
                                                            const bf16_t* __restrict__ noise, float temp_value,
                                                            const float* __restrict__ temp_dev, uint64_t seed,
                                                            const uint64_t* __restrict__ counter,
                                                            const int32_t* __restrict__ mask_len_sched, int mask_id,
                                                            int text_vocab, int codebook, int32_t* __restrict__ sampled_out,
                                                            int keep_rule) {
    constexpr bool DEVICE = NOISE == COMMIT_NOISE_DEVICE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* conf = (float*)smem;          // [N] bf16-valued
    int* samp = (int*)(conf + N);        // [N]
    __shared__ int s_unknown;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_unknown = 0;
    __syncthreads();
    const float temp = DEVICE && temp_dev ? temp_dev[0] : temp_value;
    const uint64_t ctr = DEVICE ? *counter : 0;
    const bool add_noise = DEVICE || MVAR || noise != nullptr;
    int64_t* row = ids + (size_t)b * L;
    int my_unknown = 0;
    for (int n = tid; n < N; n += blockDim.x) {
        const long long tok = row[pos_map[n]];
        const bool unknown = tok == (long long)mask_id;
        long long vq = tok - text_vocab;
        if constexpr (!MVAR) vq = vq < 0 ? 0 : (vq > codebook - 1 ? codebook - 1 : vq);
        int sidx = unknown ? sampled_in[(size_t)b * N + n] : (int)vq;
        if constexpr (!MVAR) sidx = sidx < 0 ? 0 : (sidx > codebook - 1 ? codebook - 1 : sidx);
        const float p = unknown ? bf2f(p_in[(size_t)b * N + n]) : bf2f((bf16_t)0x7f7f);
        float z = 0.f;  // the bf16 noise value
        if constexpr (DEVICE)
            z = bfround(MVAR ? sample_remask_gumbel(seed, ctr, (uint32_t)(b * N + n)) : sample_normal(seed, ctr, (uint32_t)(b * N + n)));
        else if (add_noise)
            z = bf2f(noise[(size_t)b * N + n]);
        float c;
        if constexpr (MVAR)
            c = bfround((float)log((double)(p < 1e-20f ? bfround(1e-20f) : p)));  // log(t.clamp(min=1e-20)) in bf16
        else
            c = bfround((float)log((double)bfround(p + bfround(1e-10f))));
        if (add_noise) c = bfround(c + bfround(temp * z));
        if constexpr (MVAR && DEVICE)
            if (sampled_out) sampled_out[(size_t)b * N + n] = sidx;
        conf[n] = c;
        samp[n] = sidx;
        my_unknown += unknown;
    }
    if (my_unknown) atomicAdd(&s_unknown, my_unknown);
    __syncthreads();
    int k = min(s_unknown - 1, mask_len_sched[0]);
    k = keep_rule ? max(0, k) : max(1, k);
    k = max(0, min(k, N - 1));
    for (int n = tid; n < N; n += blockDim.x) {
        const float c = conf[n];
        int rank = 0;
        if constexpr (MVAR) {
            // conf < sorted[k]  <=>  at most k elements are <= conf (its own tie class sits below position k)
            for (int j = 0; j < N; ++j) rank += conf[j] <= c;
            row[pos_map[n]] = (rank <= k) ? (int64_t)mask_id : (int64_t)((long long)samp[n] + text_vocab);
        } else {
            for (int j = 0; j < N; ++j) {
                const float cj = conf[j];
                rank += (cj < c) || (cj == c && j < n);
            }
            row[pos_map[n]] = (rank < k) ? (int64_t)mask_id : (int64_t)(samp[n] + text_vocab);
        }
    }
}

// The M text draw at text_temperature > 0 (replaces add_gumbel_noise + argmax on a float64 copy of the combined logits,
// modeling_mmada.py:49-60, :182), one workgroup per (b, t) row:
//   x0 = first-index arg-max over v < V of sample_key(text_cfg_combine(c_v, u_v, text_cfg), T, g(seed, *counter, row, v))
// v: the column in the whole vocabulary, so a 16-byte chunk of eight logits takes two Philox blocks.  T == 0: the plain arg-max of
// the combined logits, no generator runs.  The reference's exp(l) / (-log u)^T in float64 has the same arg-max as l + T * g in exact
// arithmetic; this draws from softmax(comb / T) evaluated in fp32, on another stream than torch's.
__global__ __launch_bounds__(TB) void text_draw_cfg_kernel(const bf16_t* __restrict__ cond, const bf16_t* __restrict__ unc,
                                                           float text_cfg, int V, int ld, float temperature, uint64_t seed,
                                                           const uint64_t* __restrict__ counter, int32_t* __restrict__ x0_out) {
    __shared__ float s_f[TB / 64];
    __shared__ int s_i[TB / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const bf16_t* crow = cond + (size_t)row * ld;
    const bf16_t* urow = unc + (size_t)row * ld;
    const uint64_t ctr = *counter;
    const bool noisy = temperature != 0.0f;
    const int nchunk = V >> 3;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = tid; c < nchunk; c += TB) {
        const u32x4 cv = ((const u32x4*)crow)[c];
        const u32x4 uv = ((const u32x4*)urow)[c];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
            if (noisy) sample_words4(seed, ctr, (uint32_t)row, (uint32_t)(2 * c + half), w0, w1, w2, w3);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t cb = cv[2 * half + j], ub = uv[2 * half + j];
                const float l0 = text_cfg_combine(__uint_as_float(cb << 16), __uint_as_float(ub << 16), text_cfg);
                const float l1 = text_cfg_combine(__uint_as_float(cb & 0xffff0000u), __uint_as_float(ub & 0xffff0000u), text_cfg);
                const float k0 = noisy ? sample_key(l0, temperature, sample_gumbel(j ? w2 : w0)) : l0;
                const float k1 = noisy ? sample_key(l1, temperature, sample_gumbel(j ? w3 : w1)) : l1;
                const int i = c * 8 + 4 * half + 2 * j;  // ascends per thread -> first index kept
                if (k0 > best) { best = k0; bidx = i; }
                if (k1 > best) { best = k1; bidx = i + 1; }
            }
        }
    }
    for (int i = (nchunk << 3) + tid; i < V; i += TB) {  // tail (V % 8): at most one column per thread
        const float l = text_cfg_combine(bf2f(crow[i]), bf2f(urow[i]), text_cfg);
        const float k = noisy ? sample_key(l, temperature, sample_gumbel(sample_word(seed, ctr, (uint32_t)row, (uint32_t)i))) : l;
        if (k > best || (k == best && i < bidx)) { best = k; bidx = i; }
    }
    const int x0 = block_argmax(best, bidx, s_f, s_i);
    if (tid == 0) x0_out[row] = x0;
}

// *counter += 1 once every workgroup of the kernel in front has read it (one thread: the stream orders it)
__global__ void counter_bump_kernel(uint64_t* __restrict__ counter) { *counter += 1; }

// remasking == 'random' (generators/parallel_generator.py:194-198): the confidence of a masked position is a uniform draw
// instead of its soft-max probability; already-unmasked positions keep -inf (:203)
__global__ void text_random_conf_kernel(double* __restrict__ conf, const float* __restrict__ u, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && conf[i] != -INFINITY) conf[i] = (double)u[i];
}

// conf of a draw (mmada_text_select_sampled): ranking by the log-probability is ranking by the probability, and needs no exp
__global__ void text_sampled_conf_kernel(double* __restrict__ conf, const float* __restrict__ logprob, const int64_t* __restrict__ ids,
                                         int T, int L, int text_start, int mask_id, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = i / T, t = i - b * T;
    conf[i] = ids[(size_t)b * L + text_start + t] == (int64_t)mask_id ? (double)logprob[i] : -INFINITY;
}

// ---- one launch per instantiation: the only place that spells out a kernel's argument list
template <TextMode MODE>
int run_text_stats(const TextStatsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(text_row_stats_kernel<MODE>, dim3(a.B * a.T), dim3(TB), 0, s, a.logits, a.noisy, a.unc, a.text_cfg, a.x0_in,
                       a.T, a.V, a.ld, a.col_off, a.ids, a.L, a.text_start, a.mask_id, a.conf_out, a.x0_out, a.stat_out);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

template <bool MVAR, ImageDraw DRAW>
int run_image_row(const ImageRowArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((image_row_kernel<MVAR, DRAW>), dim3(a.B * a.N), dim3(TB), (size_t)a.CB * 4, s, a.cond, a.ut, a.ui, a.CB,
                       a.cfg_scale, a.cfg_img, (uint32_t)a.col0, a.seed, a.counter, a.temperature, a.probs_out, a.sampled_out,
                       a.p_sel_out, a.argmax_out, a.pmax_out);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

template <bool MVAR, CommitNoise NOISE>
int run_image_commit(const ImageCommitArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((image_commit_kernel<MVAR, NOISE>), dim3(a.B), dim3(1024), (size_t)a.N * 8, s, a.ids, a.L, a.pos_map, a.N,
                       a.sampled_in, a.p_in, a.noise, a.temp_value, a.temp_dev, a.seed, a.counter, a.mask_len_sched, a.mask_id,
                       a.text_vocab, a.codebook, a.sampled_out, a.rule == COMMIT_RULE_M_KEEP);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

// dynamic LDS above the 64 KiB default for every kernel of `kernels`
template <size_t K>
int allow_dynamic_lds(const void* const (&kernels)[K], int bytes) {
    for (const void* k : kernels) MM_CHECK_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
}

}  // namespace

int launch_text_stats(const TextStatsArgs& a, hipStream_t s) {
    const bool partial = a.mode == TEXT_PARTIAL;
    if (a.B * a.T <= 0) return 0;
    if (a.ld % 8)
        return mm_fail(partial ? "text_stats_partial: ld must be a multiple of 8" : "text_select: ld_logits must be a multiple of 8");
    return partial ? run_text_stats<TEXT_PARTIAL>(a, s) : a.mode == TEXT_CFG ? run_text_stats<TEXT_CFG>(a, s) : run_text_stats<TEXT_PLAIN>(a, s);
}

int launch_text_commit(const void* scratch, int B, int T, int64_t* ids, int L, int text_start, const int32_t* k, hipStream_t s) {
    if (T > 8192) return mm_fail("text_commit: T=%d too large", T);
    const double* conf = (const double*)scratch;
    const int32_t* x0 = (const int32_t*)((const char*)scratch + (size_t)B * T * 8);
    hipLaunchKernelGGL(text_commit_kernel, dim3(B), dim3(TB), (size_t)T * 8, s, conf, x0, T, ids, L, text_start, k);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_text_select(TextStatsArgs a, const int32_t* k, void* scratch, const float* rand_conf, hipStream_t s) {
    if (a.B <= 0 || a.T <= 0) return 0;
    if (a.T > 8192) return mm_fail("text_select: T=%d too large", a.T);
    a.conf_out = (double*)scratch;
    a.x0_out = (int32_t*)((char*)scratch + (size_t)a.B * a.T * 8);
    if (launch_text_stats(a, s)) return 1;
    if (rand_conf) {
        hipLaunchKernelGGL(text_random_conf_kernel, dim3((a.B * a.T + 255) / 256), dim3(256), 0, s, a.conf_out, rand_conf, a.B * a.T);
        MM_CHECK_HIP(hipGetLastError());
    }
    return launch_text_commit(scratch, a.B, a.T, a.ids, a.L, a.text_start, k, s);
}

int launch_image_row(const ImageRowArgs& a, hipStream_t s) {
    const bool draw = a.draw != IMAGE_DRAW_NONE, mvar = a.combine == IMAGE_COMBINE_M;
    const char* who = draw ? "image_sample" : "image_probs";
    if (!draw && a.B * a.N <= 0) return 0;  // the draw validates its arguments before it looks at the batch
    if ((draw && a.CB <= 0) || a.CB % 8 || a.CB > 16384) return mm_fail("%s: codebook=%d must be a multiple of 8 and <= 16384", who, a.CB);
    if (draw && (a.col0 < 0 || a.col0 > INT32_MAX - a.CB)) return mm_fail("image_sample: col0=%d is not a column of the vocabulary", a.col0);
    if (a.B * a.N <= 0) return 0;
    if (a.draw == IMAGE_DRAW_TEMPERATURE && !mvar) return mm_fail("image_sample: a temperature goes with the M combine only");
    static MmOncePerDevice attr_set;
    static const void* const kernels[] = {(const void*)image_row_kernel<false, IMAGE_DRAW_NONE>, (const void*)image_row_kernel<true, IMAGE_DRAW_NONE>,
                                          (const void*)image_row_kernel<false, IMAGE_DRAW_UNIT>, (const void*)image_row_kernel<true, IMAGE_DRAW_UNIT>,
                                          (const void*)image_row_kernel<true, IMAGE_DRAW_TEMPERATURE>};
    MM_ONCE_PER_DEVICE(attr_set, if (allow_dynamic_lds(kernels, 16384 * 4)) return 1);
    switch (a.draw) {
    case IMAGE_DRAW_NONE: return mvar ? run_image_row<true, IMAGE_DRAW_NONE>(a, s) : run_image_row<false, IMAGE_DRAW_NONE>(a, s);
    case IMAGE_DRAW_UNIT: return mvar ? run_image_row<true, IMAGE_DRAW_UNIT>(a, s) : run_image_row<false, IMAGE_DRAW_UNIT>(a, s);
    default: return run_image_row<true, IMAGE_DRAW_TEMPERATURE>(a, s);
    }
}

int launch_image_commit(const ImageCommitArgs& a, hipStream_t s) {
    const bool device = a.noise_from == COMMIT_NOISE_DEVICE, mvar = a.rule != COMMIT_RULE_A;
    if (a.B <= 0 || a.N <= 0) return 0;
    if (a.N > 8192) return mm_fail("%s: N=%d too large", device ? "image_commit_sampled" : "image_commit", a.N);
    if (device && (a.rule == COMMIT_RULE_M_KEEP ? a.temp_dev != nullptr : !a.temp_dev))
        return mm_fail("image_commit_sampled: the temperature is by value with the keep rule only");
    if (!device && mvar && !a.noise) return mm_fail("image_commit (M variant): the gumbel tensor is required");
    static MmOncePerDevice attr_set;  // N * 8 B of dynamic LDS + the kernel's static LDS: above the 64 KiB default near N = 8192
    static const void* const kernels[] = {(const void*)image_commit_kernel<false, COMMIT_NOISE_TENSOR>, (const void*)image_commit_kernel<true, COMMIT_NOISE_TENSOR>,
                                          (const void*)image_commit_kernel<false, COMMIT_NOISE_DEVICE>, (const void*)image_commit_kernel<true, COMMIT_NOISE_DEVICE>};
    MM_ONCE_PER_DEVICE(attr_set, if (allow_dynamic_lds(kernels, 8192 * 8)) return 1);
    if (!device) return mvar ? run_image_commit<true, COMMIT_NOISE_TENSOR>(a, s) : run_image_commit<false, COMMIT_NOISE_TENSOR>(a, s);
    if (mvar ? run_image_commit<true, COMMIT_NOISE_DEVICE>(a, s) : run_image_commit<false, COMMIT_NOISE_DEVICE>(a, s)) return 1;
    hipLaunchKernelGGL(counter_bump_kernel, dim3(1), dim3(1), 0, s, a.counter);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_text_draw_cfg(const bf16_t* cond, const bf16_t* unc, float text_cfg, int B, int T, int V, int ld, float temperature,
                         uint64_t seed, uint64_t* counter, int32_t* x0_out, hipStream_t s) {
    if (V <= 0 || V > ld || ld % 8) return mm_fail("text_draw_cfg: V=%d, ld_logits=%d: 0 < V <= ld_logits, a multiple of 8", V, ld);
    if (B <= 0 || T <= 0) return 0;
    hipLaunchKernelGGL(text_draw_cfg_kernel, dim3(B * T), dim3(TB), 0, s, cond, unc, text_cfg, V, ld, temperature, seed, counter,
                       x0_out);
    MM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(counter_bump_kernel, dim3(1), dim3(1), 0, s, counter);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_text_sampled_conf(const float* logprob, int B, int T, const int64_t* ids, int L, int text_start, int mask_id, void* scratch,
                             hipStream_t s) {
    if (B <= 0 || T <= 0) return 0;
    hipLaunchKernelGGL(text_sampled_conf_kernel, dim3((B * T + 255) / 256), dim3(256), 0, s, (double*)scratch, logprob, ids, T, L,
                       text_start, mask_id, B * T);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}
