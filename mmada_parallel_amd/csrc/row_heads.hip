// row_heads.hip — the host side of the LM head's row heads on one rank (the contract: row_heads.h): the GEMM
// D = A · lm_head[col0 : col0 + N]^T runs with one of the row-head epilogues (row_head_epilogue.h), which leaves records per row
// and 256-column tile in the record buffer, and a small kernel joins a row's records.  One launch helper, three joining kernels.
// (Under tensor parallelism the scoring head's GEMMs and join are tp_heads.hip's, on the same records and the same fold.)
#include "row_heads.h"

size_t head_rowstat_bytes(int R, int N) { return row_head_layout(R, N, EPI_ROWSTAT).bytes; }
size_t head_rowtopk_bytes(int R, int N) { return row_head_layout(R, N, EPI_ROWTOPK).bytes; }
size_t head_rowsample_bytes(int R, int N) { return row_head_layout(R, N, EPI_ROWSAMPLE).bytes; }

// The GEMM of head `head` on A [ceil8(R), K] (rows >= R: anything) and W = lm_head rows [col0, col0 + N): pads the rows, carves
// `buf` by row_head_layout and launches.  In a: target, counter, seed, temperature as the head has them; out: the whole block.
static int launch_row_head_gemm(int head, const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, void* buf, RowHeadArgs& a,
                                RowHeadLayout& lay, hipStream_t s) {
    lay = row_head_layout(R, N, head);
    a.part = (float4*)((char*)buf + lay.part);
    a.tx = (float*)((char*)buf + lay.tx);
    a.extra = head == EPI_ROWSTAT ? nullptr : (char*)buf + lay.extra;
    a.rows = R; a.ld = lay.rp; a.col0 = col0;
    GemmArgs g = gemm_bt_args(A, W, nullptr, lay.rp, N, K, 8);
    set_row_head_args(g, a);
    // a target outside the column range leaves -inf behind (no lane holds it)
    if (a.target) MM_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)a.tx, 0xff800000u, lay.rp, s));
    return launch_gemm(head, g, s);
}
static dim3 join_grid(int R) { return dim3((R + RS_ROWS - 1) / RS_ROWS); }

// ---- the scoring head ------------------------------------------------------------------------------------------------------
// Joins the column-tile records of a row in the fixed order of rowstat_fold (row_heads.h; shared with the tensor-parallel join of
// tp_heads.hip): neither the tile order of the GEMM nor its configuration shows in the result.
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void rowstat_combine_kernel(const float4* part, const float* tx, const int64_t* targets,
                                                                               int R, int ld, int ntn, float* logprob, float* lse_out,
                                                                               int32_t* argmax_out, float* max_out) {
    const int row = blockIdx.x * RS_ROWS + threadIdx.x % RS_ROWS;
    float m, sum;
    int arg;
    if (!rowstat_fold([&](int t, int r) { return part[(size_t)t * ld + r]; }, row, R, ntn, m, sum, arg)) return;
    rowstat_finish(row, m, sum, arg, targets[row], tx[row], logprob, lse_out, argmax_out, max_out);
}

int launch_head_rowstat(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, const int64_t* targets, void* part,
                        float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s) {
    if (R <= 0 || N <= 0) return 0;
    RowHeadArgs a{};
    RowHeadLayout lay;
    a.target = targets;
    if (launch_row_head_gemm(EPI_ROWSTAT, A, W, R, N, K, col0, part, a, lay, s)) return 1;
    hipLaunchKernelGGL(rowstat_combine_kernel, join_grid(R), dim3(RS_ROWS * RS_GROUPS), 0, s, a.part, a.tx, targets, R, lay.rp, lay.ntn,
                       logprob, lse, argmax, vmax);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the top-k head: the GEMM also leaves every tile's eight best keys --------------------------------------------------------
// (topk_cand / topk_insert, the candidates' order: row_heads.h, shared with the tensor-parallel join)
// Thread (row, group j) walks the key records of tiles j, j + 16, ... and keeps the best eight candidates sorted in registers (a
// record is sorted: its entries are taken until one does not beat the thread's eighth — most tiles end at their first); thread
// (row, 0) merges the 16 lists of the row through LDS the same way and writes the first k.  The candidates are totally ordered, so
// the walk's order does not show in the result.  lse: the fold and the expression of rowstat_combine_kernel on the same records.
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void rowtopk_combine_kernel(const float4* part, const uint32_t* topk, int R, int ld, int ntn,
                                                                               int col0, int k, int32_t* ids, float* logits, float* lse_out,
                                                                               float* spare /* [ld] */) {
    __shared__ unsigned long long sk[RS_GROUPS][TOPK_MAX][RS_ROWS];
    const int rl = threadIdx.x % RS_ROWS, j = threadIdx.x / RS_ROWS;
    const int row = blockIdx.x * RS_ROWS + rl;
    unsigned long long best[TOPK_MAX];
#pragma unroll
    for (int e = 0; e < TOPK_MAX; ++e) best[e] = 0ull;
    if (row < R)
        for (int t = j; t < ntn; t += RS_GROUPS) {
            const u32x4* rec = (const u32x4*)(topk + ((size_t)t * ld + row) * TOPK_MAX);
            const u32x4 lo = rec[0], hi = rec[1];
            const uint32_t key[TOPK_MAX] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
            for (int e = 0; e < TOPK_MAX; ++e) {
                const unsigned long long c = topk_cand(key[e], t);
                if (c <= best[TOPK_MAX - 1]) break;
                topk_insert(best, c);
            }
        }
#pragma unroll
    for (int e = 0; e < TOPK_MAX; ++e) sk[j][e][rl] = best[e];
    float m, sum;
    int arg;
    // (its barrier also orders the candidate lists above)
    if (!rowstat_fold([&](int t, int r) { return part[(size_t)t * ld + r]; }, row, R, ntn, m, sum, arg)) return;
    for (int q = 1; q < RS_GROUPS; ++q)
#pragma unroll
        for (int e = 0; e < TOPK_MAX; ++e) {
            const unsigned long long c = sk[q][e][rl];
            if (c <= best[TOPK_MAX - 1]) break;
            topk_insert(best, c);
        }
#pragma unroll
    for (int e = 0; e < TOPK_MAX; ++e)
        if (e < k) {
            ids[(size_t)row * k + e] = col0 + (int)~(uint32_t)best[e];
            logits[(size_t)row * k + e] = topk_key_logit((uint32_t)(best[e] >> 32) << 16);
        }
    rowstat_finish(row, m, sum, arg, -1, 0.f, spare, lse_out, nullptr, nullptr);
}

int launch_head_rowtopk(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, int k, void* part, int32_t* ids,
                        float* logits, float* lse, hipStream_t s) {
    if (R <= 0 || N <= 0) return 0;
    if (k < 1 || k > TOPK_MAX || k > N) return mm_fail("head top-k: k=%d outside [1, min(%d, N=%d)]", k, TOPK_MAX, N);
    RowHeadArgs a{};
    RowHeadLayout lay;
    if (launch_row_head_gemm(EPI_ROWTOPK, A, W, R, N, K, col0, part, a, lay, s)) return 1;
    // (no row has a target: the target logits' place takes the join's unused log-probabilities)
    hipLaunchKernelGGL(rowtopk_combine_kernel, join_grid(R), dim3(RS_ROWS * RS_GROUPS), 0, s, a.part, (const uint32_t*)a.extra, R, lay.rp,
                       lay.ntn, col0, k, ids, logits, lse, a.tx);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the sampling head: the GEMM also leaves every tile's best key ------------------------------------------------------------
// Thread (row, group j) walks the key records of tiles j, j + 16, ... in ascending order (a later equal key lies further right and
// does not replace); thread (row, 0) folds the 16 groups through LDS, where the groups interleave the tiles and the lowest column
// wins on equal keys.  The order of keys is total (key, then column), so neither the GEMM's tile order nor its configuration shows.
// lse / argmax / max: the fold and the expression of rowstat_combine_kernel on the same records, with the drawn column's logit as
// the target logit: logprob = x_drawn - lse.  The kernel is the last of the call: every workgroup of the GEMM has read *counter.
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void rowsample_combine_kernel(const float4* part, const float4* samp, int R, int ld, int ntn,
                                                                                 int32_t* ids, float* logprob, float* lse_out, int32_t* argmax_out,
                                                                                 float* max_out, uint64_t* counter) {
    __shared__ float sk[RS_GROUPS][RS_ROWS], sx[RS_GROUPS][RS_ROWS];
    __shared__ int sc[RS_GROUPS][RS_ROWS];
    const int rl = threadIdx.x % RS_ROWS, j = threadIdx.x / RS_ROWS;
    const int row = blockIdx.x * RS_ROWS + rl;
    float bk = -__builtin_inff(), bx = -__builtin_inff();
    int bc = 0x7fffffff;
    if (row < R)
        for (int t = j; t < ntn; t += RS_GROUPS) {
            const float4 p = samp[(size_t)t * ld + row];
            rowsample_take(bk, bc, bx, p.x, __float_as_int(p.y), p.z);
        }
    sk[j][rl] = bk; sc[j][rl] = bc; sx[j][rl] = bx;
    float m, sum;
    int arg;
    // (its barrier also orders the key triples above)
    const bool mine = rowstat_fold([&](int t, int r) { return part[(size_t)t * ld + r]; }, row, R, ntn, m, sum, arg);
    if (mine) {
        for (int q = 1; q < RS_GROUPS; ++q) rowsample_take(bk, bc, bx, sk[q][rl], sc[q][rl], sx[q][rl]);
        ids[row] = bc;
        rowstat_finish(row, m, sum, arg, bc, bx, logprob, lse_out, argmax_out, max_out);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *counter += 1;
}

int launch_head_rowsample(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, float temperature, uint64_t seed,
                          uint64_t* counter, void* part, int32_t* ids, float* logprob, float* lse, int32_t* argmax, float* vmax,
                          hipStream_t s) {
    if (R <= 0 || N <= 0) return 0;
    if (!(temperature >= 0.f) || __builtin_isinf(temperature))
        return mm_fail("head sample: temperature %g is not a finite value >= 0", (double)temperature);
    RowHeadArgs a{};
    RowHeadLayout lay;
    a.counter = counter; a.seed = seed; a.temperature = temperature;
    if (launch_row_head_gemm(EPI_ROWSAMPLE, A, W, R, N, K, col0, part, a, lay, s)) return 1;
    hipLaunchKernelGGL(rowsample_combine_kernel, join_grid(R), dim3(RS_ROWS * RS_GROUPS), 0, s, a.part, (const float4*)a.extra, R, lay.rp,
                       lay.ntn, ids, logprob, lse, argmax, vmax, counter);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}
