// rowstat_fold.h — the one fold of a row's column-tile records (EPI_ROWSTAT, kernels.h) into {max, sum exp(x - max), first
// arg-max}, shared by the one-rank join (gemm.hip: rowstat_combine_kernel) and the tensor-parallel join (tp_heads.hip:
// tp_score_join_kernel), so that the two cannot drift apart: the order below IS the result's definition.
#pragma once
#include "common.h"

// Joins the column-tile records of a row in a FIXED order (so that neither the tile order of the GEMM nor its configuration
// nor the rank that produced a tile shows in the result): 16 rows x 16 tile groups per workgroup; group j folds tiles j, j + 16,
// ... in ascending order (online soft-max: rescale by exp(m_tile - m_row)), then thread (row, 0) folds the 16 groups in ascending
// order.
constexpr int RS_ROWS = 16, RS_GROUPS = 16;

// Called by every thread of a workgroup of RS_ROWS * RS_GROUPS threads (thread = (row rl, group j), row = blockIdx.x * RS_ROWS + rl).
// fetch(t, row) -> float4 record of tile t.  Returns true on the one thread per row (< R) that holds the row's result.
template <class Fetch>
MM_DEVICE bool rowstat_fold(Fetch fetch, int row, int R, int ntn, float& m, float& sum, int& arg) {
    __shared__ float sm[RS_GROUPS][RS_ROWS], ss[RS_GROUPS][RS_ROWS];
    __shared__ int sa[RS_GROUPS][RS_ROWS];
    const int rl = threadIdx.x % RS_ROWS, j = threadIdx.x / RS_ROWS;
    m = -__builtin_inff(); sum = 0.f;
    arg = 0x7fffffff;
    if (row < R)
        for (int t = j; t < ntn; t += RS_GROUPS) {
            const float4 p = fetch(t, row);
            const int a = __float_as_int(p.z);
            if (p.x > m) {   // tiles ascend inside a group: an equal maximum further right does not replace
                sum = sum * expf(m - p.x) + p.y;
                m = p.x;
                arg = a;
            } else
                sum += p.y * expf(p.x - m);
        }
    sm[j][rl] = m; ss[j][rl] = sum; sa[j][rl] = arg;
    __syncthreads();
    if (j != 0 || row >= R) return false;
    for (int q = 1; q < RS_GROUPS; ++q) {
        const float mq = sm[q][rl], sq = ss[q][rl];
        const int aq = sa[q][rl];
        if (mq > m) {
            sum = sum * expf(m - mq) + sq;
            m = mq;
            arg = aq;
        } else if (mq > -__builtin_inff()) {
            sum += sq * expf(mq - m);
            if (mq == m && aq < arg) arg = aq;   // groups interleave the tiles: the leftmost column wins
        }
    }
    return true;
}

// The row's outputs from its fold and its target logit tx (-inf: the target is no column of the range)
MM_DEVICE void rowstat_finish(int row, float m, float sum, int arg, long long target, float tx, float* logprob, float* lse_out,
                              int32_t* argmax_out, float* max_out) {
    const float lse = m + logf(sum);
    logprob[row] = target < 0 ? 0.f : tx - lse;
    if (lse_out) lse_out[row] = lse;
    if (argmax_out) argmax_out[row] = arg;
    if (max_out) max_out[row] = m;
}
