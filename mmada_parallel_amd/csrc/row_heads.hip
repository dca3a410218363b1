// row_heads.hip — the host side of the LM head's row heads on one rank (the contract: row_heads.h): the GEMM
// D = A · lm_head[col0 : col0 + N]^T runs with one of the row-head epilogues (row_head_epilogue.h), which leaves records per row
// and 256-column tile in the record buffer, and a small kernel joins a row's records (row_head_join.h).  Under tensor parallelism
// the three heads' rounds are tp_heads.hip's, on the same GEMM launch, the same records and the same joins.
#include "row_head_join.h"

size_t head_rowstat_bytes(int R, int N) { return row_head_layout(R, N, EPI_ROWSTAT).bytes; }
size_t head_rowtopk_bytes(int R, int N) { return row_head_layout(R, N, EPI_ROWTOPK).bytes; }
size_t head_rowsample_bytes(int R, int N) { return row_head_layout(R, N, EPI_ROWSAMPLE).bytes; }

int launch_row_head_gemm(int head, const bf16_t* A, const bf16_t* W, int M, int N, int K, const RowHeadArgs& a, bool publish, hipStream_t s) {
    GemmArgs g = gemm_bt_args(A, W, nullptr, M, N, K, 8);
    set_row_head_args(g, a);
    g.publish = publish;
    return launch_gemm(head, g, s);
}

// The one-rank GEMM of head `head` on A [ceil8(R), K] (rows >= R: anything): carves `buf` by row_head_layout and launches.
// In a: target, counter, seed, temperature as the head has them.  Out: where the join finds the records, and the tile count.
static int launch_local_gemm(int head, const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, void* buf, RowHeadArgs a,
                             LocalRecords& src, int& ntn, hipStream_t s) {
    const RowHeadLayout lay = row_head_layout(R, N, head);
    a.part = (float4*)((char*)buf + lay.part);
    a.tx = (float*)((char*)buf + lay.tx);
    a.extra = head == EPI_ROWSTAT ? nullptr : (char*)buf + lay.extra;
    a.rows = R; a.ld = lay.rp; a.col0 = col0;
    // a target outside the column range leaves -inf behind (no lane holds it)
    if (a.target) MM_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)a.tx, 0xff800000u, lay.rp, s));
    src = LocalRecords{a.part, a.tx, a.extra, lay.rp};
    ntn = lay.ntn;
    return launch_row_head_gemm(head, A, W, lay.rp, N, K, a, false, s);
}

// ---- the three joins over the local records (the bodies: row_head_join.h)
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void rowstat_combine_kernel(LocalRecords src, int R, int ntn, ScoreOut out) {
    rowstat_join(src, R, ntn, out);
}
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void rowtopk_combine_kernel(LocalRecords src, int R, int ntn, TopkOut out) {
    rowtopk_join(src, R, ntn, out);
}
// (the last kernel of the call: every workgroup of the GEMM has read *counter)
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void rowsample_combine_kernel(LocalRecords src, int R, int ntn, SampleOut out) {
    rowsample_join(src, R, ntn, out);
}

int launch_head_rowstat(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, const int64_t* targets, void* part,
                        float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s) {
    if (R <= 0 || N <= 0) return 0;
    RowHeadArgs a{};
    LocalRecords src;
    int ntn;
    a.target = targets;
    if (launch_local_gemm(EPI_ROWSTAT, A, W, R, N, K, col0, part, a, src, ntn, s)) return 1;
    hipLaunchKernelGGL(rowstat_combine_kernel, join_grid(R), dim3(RS_ROWS * RS_GROUPS), 0, s, src, R, ntn,
                       ScoreOut{targets, logprob, lse, argmax, vmax});
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_head_rowtopk(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, int k, void* part, int32_t* ids,
                        float* logits, float* lse, hipStream_t s) {
    if (R <= 0 || N <= 0) return 0;
    if (k < 1 || k > TOPK_MAX || k > N) return mm_fail("head top-k: k=%d outside [1, min(%d, N=%d)]", k, TOPK_MAX, N);
    LocalRecords src;
    int ntn;
    if (launch_local_gemm(EPI_ROWTOPK, A, W, R, N, K, col0, part, RowHeadArgs{}, src, ntn, s)) return 1;
    // (no row has a target: the target logits' place takes the join's unused log-probabilities)
    hipLaunchKernelGGL(rowtopk_combine_kernel, join_grid(R), dim3(RS_ROWS * RS_GROUPS), 0, s, src, R, ntn,
                       TopkOut{col0, k, ids, logits, lse, src.tx});
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_head_rowsample(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, float temperature, uint64_t seed,
                          uint64_t* counter, void* part, int32_t* ids, float* logprob, float* lse, int32_t* argmax, float* vmax,
                          hipStream_t s) {
    if (R <= 0 || N <= 0) return 0;
    if (!(temperature >= 0.f) || __builtin_isinf(temperature))
        return mm_fail("head sample: temperature %g is not a finite value >= 0", (double)temperature);
    RowHeadArgs a{};
    LocalRecords src;
    int ntn;
    a.counter = counter; a.seed = seed; a.temperature = temperature;
    if (launch_local_gemm(EPI_ROWSAMPLE, A, W, R, N, K, col0, part, a, src, ntn, s)) return 1;
    hipLaunchKernelGGL(rowsample_combine_kernel, join_grid(R), dim3(RS_ROWS * RS_GROUPS), 0, s, src, R, ntn,
                       SampleOut{ids, logprob, lse, argmax, vmax, counter});
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}
