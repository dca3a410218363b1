// vq.h — what the two image-tokenizer units share: vq_kernels.hip (the kernels and their launchers) and vq_net.hip (the
// networks built from them).  Private to them.
#pragma once
#include "common.h"

constexpr int GN_GROUPS = 32;
constexpr int GN_MAX_CHUNKS = 256;

struct ConvArgs {
    const float* in;     // [B, Hi, Wi, Cin]
    const float* w;      // [Cout][taps][Cin]
    const float* bias;   // [Cout] or null
    const float* resid;  // [B, Ho, Wo, Cout] or null (may alias out)
    float* out;          // [B, Ho, Wo, Cout]  (nchw_out: [B, Cout, Ho, Wo], direct kernel only)
    int B, Hi, Wi, Cin, Cout, Ho, Wo, taps, ups, down, nchw_out;
    long long M;         // B * Ho * Wo
};

// A ksize x ksize convolution of [B, Hi, Wi, Cin] and the output size that follows from `resample`:
// 0 same size, > 0 the 2x nearest upsample folded in front, < 0 Downsample (pad right/bottom, stride 2)
inline ConvArgs conv_args(const float* in, const float* w, const float* bias, const float* resid, float* out, int B, int Hi,
                          int Wi, int Cin, int Cout, int ksize, int resample, int nchw_out = 0) {
    ConvArgs g{};
    g.in = in; g.w = w; g.bias = bias; g.resid = resid; g.out = out;
    g.B = B; g.Hi = Hi; g.Wi = Wi; g.Cin = Cin; g.Cout = Cout;
    g.ups = resample > 0; g.down = resample < 0;
    g.Ho = g.down ? (Hi - 2) / 2 + 1 : Hi << g.ups;
    g.Wo = g.down ? (Wi - 2) / 2 + 1 : Wi << g.ups;
    g.taps = ksize * ksize; g.nchw_out = nchw_out;
    g.M = (long long)B * g.Ho * g.Wo;
    return g;
}

inline size_t group_norm_scratch_bytes(int B) { return (size_t)B * GN_GROUPS * GN_MAX_CHUNKS * 2 * sizeof(double); }

// vq_kernels.hip.  Every launcher returns 0, or 1 after mm_fail.
int launch_conv(const ConvArgs& g, hipStream_t s);
int launch_group_norm(const float* x, const float* gamma, const float* beta, float* out, double* partial, int B, int HW,
                      int C, int swish, hipStream_t s);
int launch_vq_softmax_rows(float* S, int rows, int n, float scale, hipStream_t s);             // in place, after scaling
int launch_vq_transpose(const float* in, float* out, int R, int Cc, hipStream_t s);            // out[c][r] = in[r][c]
// codes <-> latent rows (NHWC): the learned codebook cb [n_embed, D] or the lookup-free code of nbits sign bits
int launch_vq_gather(const int64_t* idx, const float* cb, float* out, long long n, int D, int n_embed, hipStream_t s);
int launch_vq_nearest_code(const float* z, const float* cb, int64_t* idx, long long n, int D, int n_embed, hipStream_t s);
int launch_vq_lfq_entry(const int64_t* idx, float* out, long long n, int nbits, hipStream_t s);
int launch_vq_lfq_index(const float* z, int64_t* idx, long long n, int nbits, hipStream_t s);
int launch_vq_nchw_to_nhwc(const float* in, float* out, int B, int C, long long HW, hipStream_t s);
// [co][ci][kk] (nn.Conv2d) -> [co][kk][ci]
int launch_vq_repack_conv(const float* src, float* dst, int co, int ci, int kk, hipStream_t s);
