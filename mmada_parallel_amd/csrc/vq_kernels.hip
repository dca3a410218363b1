// vq_kernels.hip — the kernels of the image tokenizers on gfx950 (MAGVITv2 of MMaDA-Parallel-M, diffusers.VQModel of the A
// variant), fp32 like the reference (MMaDA-Parallel-M/inference.py:56-59 keeps the VQ model in fp32),
// with their launchers and the kernel-level entry points.  The networks built from them are in vq_net.hip.
//   ResnetBlock / AttnBlock / Upsample / Normalize / swish   models/common_modules.py:337-357,187-211,36-40,16-24
//   LFQuantizer.get_codebook_entry / get_indices             models/modeling_magvitv2.py:208-221,201-206
// Layout: activations are NHWC fp32 ([B, H, W, C], channels contiguous), so a 3x3 convolution is an implicit GEMM
// with M = B*H*W pixels, N = Cout, K = 9*Cin whose A-tile rows are 128-byte channel runs of shifted pixels; conv
// weights are repacked once at bind time to [Cout][tap][Cin].  The 2x nearest upsample is folded into the A-tile
// addressing of the convolution that follows it, bias / residual adds into the epilogue.
// Kernels: conv_mfma_kernel (v_mfma_f32_32x32x2_f32, 128x128x32 tiles, register-prefetched LDS staging),
// conv_direct_kernel (Cin = 13: scalar-weight FMA), conv_thin_kernel (conv_out: 3 channels out), gn_stats/gn_apply (GroupNorm(32) + swish, fp64
// moments, deterministic two-level reduction), softmax_rows, transpose, lfq_nhwc / lfq_index, codebook_gather / codebook_argmin,
// nchw_to_nhwc, repack_conv.
#include <algorithm>
#include <cmath>

#include "../../include/mmada_mi355x.h"
#include "vq.h"

namespace {

// Input pixel of output pixel (oh, ow) for filter tap `tap`; false = zero padding.
//   default: stride 1, padding k/2 (Conv2d(k, 1, k//2))
//   ups:     the same on the 2x nearest-upsampled input (Upsample.forward, common_modules.py:36-40)
//   down:    Downsample.forward (common_modules.py:83-90): F.pad(x, (0,1,0,1)) then Conv2d(3, stride 2, padding 0)
MM_DEVICE bool conv_src(const ConvArgs& g, int oh, int ow, int tap, int& ih, int& iw) {
    if (g.down) {
        ih = 2 * oh + tap / 3;
        iw = 2 * ow + tap % 3;
        return ih < g.Hi && iw < g.Wi;
    }
    const int uh = oh + (g.taps == 9 ? tap / 3 - 1 : 0), uw = ow + (g.taps == 9 ? tap % 3 - 1 : 0);
    ih = uh >> g.ups;
    iw = uw >> g.ups;
    return uh >= 0 && uh < g.Ho && uw >= 0 && uw < g.Wo;
}

// ---------------------------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution on the fp32 matrix cores.  256 threads = 4 waves (2x2), wave tile 64x64 = 2x2 MFMA
// 32x32 blocks, K step 32 channels of one tap.  Global -> registers (next chunk) overlaps the MFMAs of the current
// chunk; LDS rows are padded to 36 floats so both the float4 stores and the float4 fragment reads are conflict-free.
constexpr int CBM = 128, CBN = 128, CBK = 32, CLD = CBK + 4;

__global__ __launch_bounds__(256, 2) void conv_mfma_kernel(ConvArgs g) {
    __shared__ __attribute__((aligned(16))) float As[CBM * CLD];
    __shared__ __attribute__((aligned(16))) float Bs[CBN * CLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long long m0 = (long long)blockIdx.x * CBM;
    const int n0 = blockIdx.y * CBN;
    const int lc = tid & 7, lr = tid >> 3;

    // per-thread loader rows: 4 pixel rows and 4 weight rows, 32 apart
    int pb[4], poh[4], pow_[4];
    bool pv[4];
    const float* wrow[4];
    bool wv[4];
    const int HoWo = g.Ho * g.Wo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long m = m0 + lr + 32 * i;
        pv[i] = m < g.M;
        const long long mm = pv[i] ? m : 0;
        pb[i] = (int)(mm / HoWo);
        const int r = (int)(mm - (long long)pb[i] * HoWo);
        poh[i] = r / g.Wo;
        pow_[i] = r - poh[i] * g.Wo;
        const int n = n0 + lr + 32 * i;
        wv[i] = n < g.Cout;
        wrow[i] = g.w + (size_t)(wv[i] ? n : 0) * g.taps * g.Cin + 4 * lc;
    }
    const int cchunks = g.Cin / CBK, nch = g.taps * cchunks;
    f32x4 ra[4], rb[4];
    auto gload = [&](int ch) {
        const int tap = ch / cchunks, c0 = (ch - tap * cchunks) * CBK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int ih, iw;
            const bool ok = conv_src(g, poh[i], pow_[i], tap, ih, iw) && pv[i];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *(const f32x4*)(g.in + (((size_t)pb[i] * g.Hi + ih) * g.Wi + iw) * g.Cin + c0 + 4 * lc);
            ra[i] = v;
            f32x4 wv4 = {0.f, 0.f, 0.f, 0.f};
            if (wv[i]) wv4 = *(const f32x4*)(wrow[i] + (size_t)tap * g.Cin + c0);
            rb[i] = wv4;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int frow = lane & 31, kh = lane >> 5;
    gload(0);
    for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(f32x4*)&As[(lr + 32 * i) * CLD + 4 * lc] = ra[i];
            *(f32x4*)&Bs[(lr + 32 * i) * CLD + 4 * lc] = rb[i];
        }
        __syncthreads();
        if (ch + 1 < nch) gload(ch + 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k4 = s * 8 + kh * 4;
            f32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *(const f32x4*)&As[(wm * 64 + i * 32 + frow) * CLD + k4];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *(const f32x4*)&Bs[(wn * 64 + j * 32 + frow) * CLD + k4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // D[m][n]: n = lane & 31, m = 8*(r>>2) + 4*(lane>>5) + (r&3)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long m = m0 + wm * 64 + i * 32 + 8 * (r >> 2) + 4 * kh + (r & 3);
            if (m >= g.M) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + wn * 64 + j * 32 + frow;
                if (n >= g.Cout) continue;
                float v = acc[i][j][r];
                if (g.bias) v += g.bias[n];
                if (g.resid) v += g.resid[(size_t)m * g.Cout + n];
                g.out[(size_t)m * g.Cout + n] = v;
            }
        }
}

// Direct convolution for the thin ends of the network (z_channels = 13 in, 3 / 13 out): one thread per pixel and
// CO output channels; the weight index does not depend on the lane, so the weights come through the scalar cache.
template <int CO>
__global__ __launch_bounds__(256) void conv_direct_kernel(ConvArgs g) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    const int co0 = blockIdx.y * CO;
    if (m >= g.M) return;
    const int HoWo = g.Ho * g.Wo;
    const int b = (int)(m / HoWo), r = (int)(m - (long long)b * HoWo), oh = r / g.Wo, ow = r - (r / g.Wo) * g.Wo;
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = 0.f;
    const size_t wstride = (size_t)g.taps * g.Cin;
    for (int tap = 0; tap < g.taps; ++tap) {
        int ih, iw;
        if (!conv_src(g, oh, ow, tap, ih, iw)) continue;
        const float* src = g.in + (((size_t)b * g.Hi + ih) * g.Wi + iw) * g.Cin;
        const float* wt = g.w + (size_t)co0 * wstride + (size_t)tap * g.Cin;
        for (int ci = 0; ci < g.Cin; ++ci) {
            const float x = src[ci];
#pragma unroll
            for (int c = 0; c < CO; ++c)
                if (co0 + c < g.Cout) acc[c] = fmaf(x, wt[(size_t)c * wstride + ci], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < CO; ++c) {
        const int n = co0 + c;
        if (n >= g.Cout) continue;
        float v = acc[c];
        if (g.bias) v += g.bias[n];
        if (g.nchw_out) {
            g.out[((size_t)b * g.Cout + n) * HoWo + r] = v;
        } else {
            if (g.resid) v += g.resid[(size_t)m * g.Cout + n];
            g.out[(size_t)m * g.Cout + n] = v;
        }
    }
}

// conv_out (wide in, <= 4 out): eight lanes share a pixel, each owning every 8th float4 of the channel run, so a tap
// is one coalesced 128-byte-per-pixel read; weights sit in LDS; the eight partial sums meet in a 3-step butterfly.
constexpr int THIN_CO = 4;
__global__ __launch_bounds__(256) void conv_thin_kernel(ConvArgs g) {
    extern __shared__ __attribute__((aligned(16))) float wsh[];  // [Cout][taps][Cin]
    const int tid = threadIdx.x, sub = tid & 7;
    const int wtotal = g.Cout * g.taps * g.Cin;
    for (int i = tid * 4; i < wtotal; i += 1024) *(f32x4*)&wsh[i] = *(const f32x4*)&g.w[i];
    __syncthreads();
    const long long m = (long long)blockIdx.x * 32 + (tid >> 3);
    const bool live = m < g.M;
    const long long mm = live ? m : 0;
    const int HoWo = g.Ho * g.Wo;
    const int b = (int)(mm / HoWo), r = (int)(mm - (long long)b * HoWo), oh = r / g.Wo, ow = r - (r / g.Wo) * g.Wo;
    float acc[THIN_CO] = {0.f, 0.f, 0.f, 0.f};
    const int wstride = g.taps * g.Cin;
    for (int tap = 0; tap < g.taps; ++tap) {
        int ih, iw;
        if (!conv_src(g, oh, ow, tap, ih, iw) || !live) continue;
        const float* src = g.in + (((size_t)b * g.Hi + ih) * g.Wi + iw) * g.Cin;
        for (int c = sub * 4; c < g.Cin; c += 32) {
            const f32x4 x = *(const f32x4*)(src + c);
#pragma unroll
            for (int co = 0; co < THIN_CO; ++co) {
                if (co >= g.Cout) break;
                const f32x4 w4 = *(const f32x4*)&wsh[co * wstride + tap * g.Cin + c];
                acc[co] = fmaf(x[0], w4[0], fmaf(x[1], w4[1], fmaf(x[2], w4[2], fmaf(x[3], w4[3], acc[co]))));
            }
        }
    }
#pragma unroll
    for (int co = 0; co < THIN_CO; ++co)
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) acc[co] += __shfl_xor(acc[co], o, 64);
    if (!live || sub >= g.Cout) return;
    float v = sub == 0 ? acc[0] : sub == 1 ? acc[1] : sub == 2 ? acc[2] : acc[3];
    if (g.bias) v += g.bias[sub];
    if (g.nchw_out) {
        g.out[((size_t)b * g.Cout + sub) * HoWo + r] = v;
    } else {
        if (g.resid) v += g.resid[(size_t)m * g.Cout + sub];
        g.out[(size_t)m * g.Cout + sub] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// GroupNorm(32 groups, eps 1e-6) over NHWC: pass 1 writes fp64 (sum, sum of squares) per (batch, group, pixel chunk);
// pass 2 sums the chunks in a fixed order, normalises, applies the affine and (optionally) swish.
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, double* __restrict__ partial, int HW,
                                                       int C, int nchunks) {
    __shared__ double sh_s[256], sh_q[256];
    const int C4 = C >> 2, PL = 256 / C4;
    const int tid = threadIdx.x, col = tid % C4, pl = tid / C4;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int per = (HW + nchunks - 1) / nchunks;
    const int p0 = chunk * per, p1 = min(HW, p0 + per);
    double s = 0.0, q = 0.0;
    if (pl < PL) {
        const float* base = x + (size_t)b * HW * C + 4 * col;
        for (int p = p0 + pl; p < p1; p += PL) {
            const f32x4 v = *(const f32x4*)(base + (size_t)p * C);
            s += (double)v[0] + (double)v[1] + (double)v[2] + (double)v[3];
            q += (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
        }
    }
    sh_s[tid] = s;
    sh_q[tid] = q;
    __syncthreads();
    if (tid < GN_GROUPS) {
        const int cpg4 = C4 / GN_GROUPS;
        double ts = 0.0, tq = 0.0;
        for (int l = 0; l < PL; ++l)
            for (int c = 0; c < cpg4; ++c) {
                ts += sh_s[l * C4 + tid * cpg4 + c];
                tq += sh_q[l * C4 + tid * cpg4 + c];
            }
        double* o = partial + (((size_t)b * GN_GROUPS + tid) * nchunks + chunk) * 2;
        o[0] = ts;
        o[1] = tq;
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const double* __restrict__ partial,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ out, int HW, int C, int nchunks, int swish) {
    __shared__ float sh_mean[GN_GROUPS], sh_rstd[GN_GROUPS];
    const int b = blockIdx.y, tid = threadIdx.x, C4 = C >> 2, cpg4 = C4 / GN_GROUPS;
    if (tid < GN_GROUPS) {
        const double* p = partial + ((size_t)b * GN_GROUPS + tid) * nchunks * 2;
        double s = 0.0, q = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            s += p[2 * c];
            q += p[2 * c + 1];
        }
        const double n = (double)HW * (C / GN_GROUPS);
        const double mean = s / n, var = fmax(q / n - mean * mean, 0.0);
        sh_mean[tid] = (float)mean;
        sh_rstd[tid] = (float)(1.0 / sqrt(var + 1e-6));
    }
    __syncthreads();
    const size_t total = (size_t)HW * C4;
    const float* xb = x + (size_t)b * HW * C;
    float* ob = out + (size_t)b * HW * C;
    for (size_t e = (size_t)blockIdx.x * 256 + tid; e < total; e += (size_t)gridDim.x * 256) {
        const int col = (int)(e % C4), grp = col / cpg4;
        const f32x4 v = *(const f32x4*)(xb + e * 4);
        const f32x4 ga = *(const f32x4*)(gamma + 4 * col), be = *(const f32x4*)(beta + 4 * col);
        const float mean = sh_mean[grp], rstd = sh_rstd[grp];
        f32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float t = (v[i] - mean) * rstd * ga[i] + be[i];
            if (swish) t = t / (1.0f + expf(-t));
            y[i] = t;
        }
        *(f32x4*)(ob + e * 4) = y;
    }
}

// softmax over the rows of S [rows, n] in place, after scaling (AttnBlock: w_ * c^-0.5 then softmax(dim=2))
__global__ __launch_bounds__(256) void softmax_rows_kernel(float* __restrict__ S, int n, float scale) {
    __shared__ float red[4];
    float* row = S + (size_t)blockIdx.x * n;
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 256) mx = fmaxf(mx, row[i] * scale);
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < n; i += 256) {
        const float e = expf(row[i] * scale - mx);
        row[i] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
    for (int i = tid; i < n; i += 256) row[i] *= inv;
}

// out[c][r] = in[r][c]
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int Cc) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < Cc) tile[j][tx] = in[(size_t)(r0 + j) * Cc + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < Cc && r0 + tx < R) out[(size_t)(c0 + j) * R + r0 + tx] = tile[tx][j];
}

// LFQuantizer.get_codebook_entry: bit (nbits-1-c) of the index -> +-1 in channel c; NHWC
__global__ void lfq_nhwc_kernel(const int64_t* __restrict__ idx, float* __restrict__ out, long long n, int nbits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long v = idx[i];
    for (int c = 0; c < nbits; ++c) out[i * nbits + c] = ((v >> (nbits - 1 - c)) & 1) ? 1.0f : -1.0f;
}

// LFQuantizer.get_indices (modeling_magvitv2.py:201-206) of the sign quantisation (:241-243): bit (nbits-1-c) = z_c > 0
__global__ void lfq_index_kernel(const float* __restrict__ z, int64_t* __restrict__ idx, long long n, int nbits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long v = 0;
    for (int c = 0; c < nbits; ++c) v |= (long long)(z[i * nbits + c] > 0.f) << (nbits - 1 - c);
    idx[i] = v;
}

// ---- diffusers VQModel quantizer (A variant): a learned codebook [n_embed, D] instead of the lookup-free bit code ----
// VectorQuantizer.get_codebook_entry: z_q = embedding(indices).view(B, h, w, D) — which IS the NHWC layout used here
__global__ void codebook_gather_kernel(const int64_t* __restrict__ idx, const float* __restrict__ cb, float* __restrict__ out,
                                       long long n, int D, int n_embed) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * D) return;
    const long long p = i / D;
    long long id = idx[p];
    id = id < 0 ? 0 : (id >= n_embed ? n_embed - 1 : id);  // torch would raise; keep the device safe
    out[i] = cb[id * D + (i - p * D)];
}

// VectorQuantizer.forward: min_encoding_indices = argmin_j cdist(z, E)[., j].  torch.cdist (p = 2, > 25 rows) evaluates
// sqrt(clamp_min(|z|^2 + |e_j|^2 - 2 z·e_j, 0)) through one matmul; this kernel forms the same three terms in fp32 and
// takes the FIRST index of the minimum like torch.argmin.  One workgroup per latent row, codes strided over the threads.
__global__ __launch_bounds__(256) void codebook_argmin_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                              int64_t* __restrict__ idx, int D, int n_embed) {
    extern __shared__ float zrow[];  // D floats, then 256 (dist, index) pairs
    float* sd = zrow + D;
    int* si = (int*)(sd + 256);
    const long long row = blockIdx.x;
    float xn = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) zrow[c] = z[row * D + c];
    __syncthreads();
    for (int c = 0; c < D; ++c) xn = fmaf(zrow[c], zrow[c], xn);
    float best = INFINITY;
    int bi = 0x7fffffff;
    for (int j = threadIdx.x; j < n_embed; j += 256) {
        const float* e = cb + (size_t)j * D;
        float dot = 0.f, yn = 0.f;
        for (int c = 0; c < D; ++c) {
            const float ev = e[c];
            dot = fmaf(-2.0f * zrow[c], ev, dot);
            yn = fmaf(ev, ev, yn);
        }
        const float d = sqrtf(fmaxf(dot + xn + yn, 0.f));
        if (d < best) { best = d; bi = j; }  // j ascending per thread: the first minimum is kept
    }
    sd[threadIdx.x] = best; si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const float d2 = sd[threadIdx.x + o];
            const int i2 = si[threadIdx.x + o];
            if (d2 < sd[threadIdx.x] || (d2 == sd[threadIdx.x] && i2 < si[threadIdx.x])) { sd[threadIdx.x] = d2; si[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) idx[row] = si[0];
}

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int C, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long b = i / (HW * C), r = i - b * HW * C, p = r / C;
    const int c = (int)(r - p * C);
    out[i] = in[(b * C + c) * HW + p];
}

// [Cout][Cin][k][k] (nn.Conv2d) -> [Cout][k*k][Cin]
__global__ void repack_conv_kernel(const float* __restrict__ src, float* __restrict__ dst, int co, int ci, int kk) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)co * ci * kk;
    if (i >= total) return;
    const int c = (int)(i % ci);
    const int t = (int)((i / ci) % kk);
    const size_t o = i / ((size_t)ci * kk);
    dst[i] = src[(o * ci + c) * kk + t];
}

}  // namespace

int launch_conv(const ConvArgs& g, hipStream_t s) {
    if (g.M <= 0) return 0;
    if (g.taps != 1 && g.taps != 9) return mm_fail("vq conv: taps must be 1 or 9");
    const bool mfma = (g.Cin % CBK == 0) && g.Cout > 16 && !g.nchw_out;
    if (mfma) {
        hipLaunchKernelGGL(conv_mfma_kernel, dim3((unsigned)((g.M + CBM - 1) / CBM), (g.Cout + CBN - 1) / CBN), dim3(256), 0, s, g);
    } else {
        const unsigned gx = (unsigned)((g.M + 255) / 256);
        const size_t wbytes = (size_t)g.Cout * g.taps * g.Cin * sizeof(float);
        if (g.Cout <= THIN_CO && g.Cin % 32 == 0 && wbytes <= 64 * 1024)
            hipLaunchKernelGGL(conv_thin_kernel, dim3((unsigned)((g.M + 31) / 32)), dim3(256), wbytes, s, g);
        else if (g.Cout <= 3)
            hipLaunchKernelGGL(conv_direct_kernel<3>, dim3(gx, 1), dim3(256), 0, s, g);
        else if (g.Cout <= 13)
            hipLaunchKernelGGL(conv_direct_kernel<13>, dim3(gx, 1), dim3(256), 0, s, g);
        else
            hipLaunchKernelGGL(conv_direct_kernel<16>, dim3(gx, (g.Cout + 15) / 16), dim3(256), 0, s, g);
    }
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

static int gn_chunks(int HW) { return std::max(1, std::min(GN_MAX_CHUNKS, HW / 256)); }

int launch_group_norm(const float* x, const float* gamma, const float* beta, float* out, double* partial, int B, int HW,
                      int C, int swish, hipStream_t s) {
    if (C % 128 || C > 1024) return mm_fail("vq group_norm: C=%d must be a multiple of 128 and <= 1024", C);
    const int nch = gn_chunks(HW);
    hipLaunchKernelGGL(gn_stats_kernel, dim3(nch, B), dim3(256), 0, s, x, partial, HW, C, nch);
    const size_t total = (size_t)HW * (C / 4);
    const unsigned gx = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(gx, B), dim3(256), 0, s, x, partial, gamma, beta, out, HW, C, nch, swish);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_softmax_rows(float* S, int rows, int n, float scale, hipStream_t s) {
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, s, S, n, scale);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_transpose(const float* in, float* out, int R, int Cc, hipStream_t s) {
    hipLaunchKernelGGL(transpose_kernel, dim3((Cc + 31) / 32, (R + 31) / 32), dim3(256), 0, s, in, out, R, Cc);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_gather(const int64_t* idx, const float* cb, float* out, long long n, int D, int n_embed, hipStream_t s) {
    const long long tot = n * D;
    hipLaunchKernelGGL(codebook_gather_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, idx, cb, out, n, D, n_embed);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_nearest_code(const float* z, const float* cb, int64_t* idx, long long n, int D, int n_embed, hipStream_t s) {
    const size_t lds = (size_t)D * sizeof(float) + 256 * (sizeof(float) + sizeof(int));
    hipLaunchKernelGGL(codebook_argmin_kernel, dim3((unsigned)n), dim3(256), lds, s, z, cb, idx, D, n_embed);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_lfq_entry(const int64_t* idx, float* out, long long n, int nbits, hipStream_t s) {
    hipLaunchKernelGGL(lfq_nhwc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, idx, out, n, nbits);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_lfq_index(const float* z, int64_t* idx, long long n, int nbits, hipStream_t s) {
    hipLaunchKernelGGL(lfq_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, idx, n, nbits);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_nchw_to_nhwc(const float* in, float* out, int B, int C, long long HW, hipStream_t s) {
    const long long total = (long long)B * HW * C;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, C, HW, total);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_vq_repack_conv(const float* src, float* dst, int co, int ci, int kk, hipStream_t s) {
    const size_t total = (size_t)co * ci * kk;
    hipLaunchKernelGGL(repack_conv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, co, ci, kk);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" {

/* kernel-level entry points (parity tests) */
int mmada_vq_conv2d(const float* in_nhwc, const float* w_packed, const float* bias, const float* resid, float* out,
                    int B, int Hi, int Wi, int Cin, int Cout, int ksize, int upsample, void* stream) {
    if (!in_nhwc || !w_packed || !out) return mm_fail("mmada_vq_conv2d: null argument");
    if (ksize != 1 && ksize != 3) return mm_fail("mmada_vq_conv2d: ksize must be 1 or 3");
    if (upsample < 0 && ksize != 3) return mm_fail("mmada_vq_conv2d: the stride-2 mode is 3x3 only");
    return launch_conv(conv_args(in_nhwc, w_packed, bias, resid, out, B, Hi, Wi, Cin, Cout, ksize, upsample), (hipStream_t)stream);
}

int mmada_vq_group_norm(const float* x_nhwc, const float* gamma, const float* beta, float* out, void* scratch,
                        int B, int HW, int C, int swish, void* stream) {
    if (!x_nhwc || !gamma || !beta || !out || !scratch) return mm_fail("mmada_vq_group_norm: null argument");
    return launch_group_norm(x_nhwc, gamma, beta, out, (double*)scratch, B, HW, C, swish, (hipStream_t)stream);
}

size_t mmada_vq_group_norm_scratch_bytes(int B) { return group_norm_scratch_bytes(B); }

}  // extern "C"
