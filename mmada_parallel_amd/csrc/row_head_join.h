// row_head_join.h — the joins of the LM head's row heads (device; the records: row_heads.h), ONCE each: a join is a body template
// over a record source, which says where tile t's records of a row lie.  The one-rank kernels (row_heads.hip) run the bodies over
// LocalRecords below, the tensor-parallel kernels (tp_heads.hip) over a source that takes tile t from the rank that owns it — so
// every rank, and a one-rank handle, ends with the same bits, and the two cannot drift apart.  A source has
//     float4 record(t, r)               tile t's 16-byte record of row r
//     void topk_keys(t, r, key)         EPI_ROWTOPK: the tile's eight keys
//     float4 sample_triple(t, r)        EPI_ROWSAMPLE: {key, column (int bits), logit, 0}
//     float target_logit(row, target)   EPI_ROWSTAT: the logit at the target's column, -inf if it is no column of the range (the
//                                       value is passed on for a non-negative target only)
//     void acquire()                    only where other agents wrote the records: the first statement of such a kernel
// Included by row_heads.hip and tp_heads.hip only.
#pragma once
#include "row_heads.h"

// A join's workgroup: 16 rows x 16 tile groups, thread = (row rl, group j), row = blockIdx.x * RS_ROWS + rl
constexpr int RS_ROWS = 16, RS_GROUPS = 16;
static inline dim3 join_grid(int R) { return dim3((R + RS_ROWS - 1) / RS_ROWS); }

// The records of a one-rank launch, as row_head_layout carves them (ld: its rp)
struct LocalRecords {
    const float4* part;
    float* tx;           // (a head without targets lends it to its join: TopkOut::spare)
    const void* extra;
    int ld;
    MM_DEVICE float4 record(int t, int r) const { return part[(size_t)t * ld + r]; }
    MM_DEVICE void topk_keys(int t, int r, uint32_t (&key)[TOPK_MAX]) const {
        const u32x4* rec = (const u32x4*)((const uint32_t*)extra + ((size_t)t * ld + r) * TOPK_MAX);
        const u32x4 lo = rec[0], hi = rec[1];
        key[0] = lo[0]; key[1] = lo[1]; key[2] = lo[2]; key[3] = lo[3];
        key[4] = hi[0]; key[5] = hi[1]; key[6] = hi[2]; key[7] = hi[3];
    }
    MM_DEVICE float4 sample_triple(int t, int r) const { return ((const float4*)extra)[(size_t)t * ld + r]; }
    MM_DEVICE float target_logit(int row, long long) const { return tx[row]; }   // (the launcher preset -inf)
};

// What a join writes.  Rows are the launch's: the tensor-parallel launchers pass pointers to a round's first row.
struct ScoreOut {
    const int64_t* targets;    // [R] column in the whole vocabulary, or negative: none
    float *logprob, *lse;      // lse / argmax / vmax: or null
    int32_t* argmax;
    float* vmax;
};
struct TopkOut {
    int col0, k;               // first column of the launch, places to write
    int32_t* ids;              // [R, k]
    float *logits, *lse;       // [R, k]; [R] or null
    float* spare;              // [ld] private floats: the fold's unused log-probabilities
};
struct SampleOut {
    int32_t* ids;              // [R]
    float *logprob, *lse;      // lse / argmax / vmax: or null
    int32_t* argmax;
    float* vmax;
    uint64_t* counter;         // + 1 by the call's last join, behind every GEMM that reads it; null: not this launch
};

// ---- the one fold of a row's column-tile records into {max, sum exp(x - max), first arg-max}: the order below IS the result's
// definition.  The records are joined in a FIXED order (so that neither the tile order of the GEMM nor its configuration nor the
// rank that produced a tile shows in the result): group j folds tiles j, j + 16, ... in ascending order (online soft-max: rescale
// by exp(m_tile - m_row)), then thread (row, 0) folds the 16 groups in ascending order.
// Called by every thread of a workgroup of RS_ROWS * RS_GROUPS threads.  Returns true on the one thread per row (< R) that holds
// the row's result.  HEAD: the join's head — an instantiation per join, and `static`, so that each kernel has LDS arrays of
// its own, private to the unit, and the compiler drops what a join never reads (top-k: the arg-max, its array and the load of a
// record's third word).
template <int HEAD, class Src>
static MM_DEVICE bool rowstat_fold(const Src& src, int row, int R, int ntn, float& m, float& sum, int& arg) {
    __shared__ float sm[RS_GROUPS][RS_ROWS], ss[RS_GROUPS][RS_ROWS];
    __shared__ int sa[RS_GROUPS][RS_ROWS];
    const int rl = threadIdx.x % RS_ROWS, j = threadIdx.x / RS_ROWS;
    m = -__builtin_inff(); sum = 0.f;
    arg = 0x7fffffff;
    if (row < R)
        for (int t = j; t < ntn; t += RS_GROUPS) {
            const float4 p = src.record(t, row);
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

// ---- the scoring head
template <class Src>
MM_DEVICE void rowstat_join(const Src& src, int R, int ntn, const ScoreOut& o) {
    const int row = blockIdx.x * RS_ROWS + threadIdx.x % RS_ROWS;
    float m, sum;
    int arg;
    if (!rowstat_fold<EPI_ROWSTAT>(src, row, R, ntn, m, sum, arg)) return;
    const long long t = o.targets[row];
    rowstat_finish(row, m, sum, arg, t, src.target_logit(row, t), o.logprob, o.lse, o.argmax, o.vmax);
}

// ---- the top-k head: the GEMM also leaves every tile's eight best keys
// A candidate: {order value of the logit, ~column inside the launch} as one 64-bit number — logit descending, then tile ascending,
// then column ascending is ONE unsigned compare, and candidates of a row are distinct.  0: no candidate.
MM_DEVICE unsigned long long topk_cand(uint32_t key, int tile) {
    if (key == 0u) return 0ull;
    const uint32_t col = (uint32_t)tile * (uint32_t)ROW_HEAD_BN + (255u - (key & 255u));
    return ((unsigned long long)(key >> 16) << 32) | (unsigned long long)(~col);
}
// best[] stays sorted in descending order; c replaces the last entry and moves up to its place
MM_DEVICE void topk_insert(unsigned long long (&best)[TOPK_MAX], unsigned long long c) {
    best[TOPK_MAX - 1] = c;
#pragma unroll
    for (int i = TOPK_MAX - 1; i > 0; --i) {
        const unsigned long long lo = best[i], hi = best[i - 1];
        best[i - 1] = lo > hi ? lo : hi;
        best[i] = lo > hi ? hi : lo;
    }
}
// Thread (row, group j) walks the key records of tiles j, j + 16, ... and keeps the best eight candidates sorted in registers (a
// record is sorted: its entries are taken until one does not beat the thread's eighth — most tiles end at their first); thread
// (row, 0) merges the 16 lists of the row through LDS the same way and writes the first k.  The candidates are totally ordered, so
// neither the walk's order nor the rank a tile came from shows in the result.  lse: the fold and the expression of the scoring
// head on the same records.
template <class Src>
MM_DEVICE void rowtopk_join(const Src& src, int R, int ntn, const TopkOut& o) {
    __shared__ unsigned long long sk[RS_GROUPS][TOPK_MAX][RS_ROWS];
    const int rl = threadIdx.x % RS_ROWS, j = threadIdx.x / RS_ROWS;
    const int row = blockIdx.x * RS_ROWS + rl;
    unsigned long long best[TOPK_MAX];
#pragma unroll
    for (int e = 0; e < TOPK_MAX; ++e) best[e] = 0ull;
    if (row < R)
        for (int t = j; t < ntn; t += RS_GROUPS) {
            uint32_t key[TOPK_MAX];
            src.topk_keys(t, row, key);
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
    if (!rowstat_fold<EPI_ROWTOPK>(src, row, R, ntn, m, sum, arg)) return;
    for (int q = 1; q < RS_GROUPS; ++q)
#pragma unroll
        for (int e = 0; e < TOPK_MAX; ++e) {
            const unsigned long long c = sk[q][e][rl];
            if (c <= best[TOPK_MAX - 1]) break;
            topk_insert(best, c);
        }
#pragma unroll
    for (int e = 0; e < TOPK_MAX; ++e)
        if (e < o.k) {
            o.ids[(size_t)row * o.k + e] = o.col0 + (int)~(uint32_t)best[e];
            o.logits[(size_t)row * o.k + e] = topk_key_logit((uint32_t)(best[e] >> 32) << 16);
        }
    rowstat_finish(row, m, sum, arg, -1, 0.f, o.spare, o.lse, nullptr, nullptr);
}

// ---- the sampling head: the GEMM also leaves every tile's best key
// Thread (row, group j) walks the triples of tiles j, j + 16, ... in ascending order (a later equal key lies further right and
// does not replace); thread (row, 0) folds the 16 groups through LDS, where the groups interleave the tiles and the lowest column
// wins on equal keys.  rowsample_take is a total order (key, then column), so neither the GEMM's tile order nor its configuration
// nor the rank a tile came from shows.  lse / argmax / max: the fold and the expression of the scoring head on the same records,
// with the drawn column's logit as the target logit: logprob = x_drawn - lse.
template <class Src>
MM_DEVICE void rowsample_join(const Src& src, int R, int ntn, const SampleOut& o) {
    __shared__ float sk[RS_GROUPS][RS_ROWS], sx[RS_GROUPS][RS_ROWS];
    __shared__ int sc[RS_GROUPS][RS_ROWS];
    const int rl = threadIdx.x % RS_ROWS, j = threadIdx.x / RS_ROWS;
    const int row = blockIdx.x * RS_ROWS + rl;
    float bk = -__builtin_inff(), bx = -__builtin_inff();
    int bc = 0x7fffffff;
    if (row < R)
        for (int t = j; t < ntn; t += RS_GROUPS) {
            const float4 p = src.sample_triple(t, row);
            rowsample_take(bk, bc, bx, p.x, __float_as_int(p.y), p.z);
        }
    sk[j][rl] = bk; sc[j][rl] = bc; sx[j][rl] = bx;
    float m, sum;
    int arg;
    // (its barrier also orders the key triples above)
    const bool mine = rowstat_fold<EPI_ROWSAMPLE>(src, row, R, ntn, m, sum, arg);
    if (mine) {
        for (int q = 1; q < RS_GROUPS; ++q) rowsample_take(bk, bc, bx, sk[q][rl], sc[q][rl], sx[q][rl]);
        o.ids[row] = bc;
        rowstat_finish(row, m, sum, arg, bc, bx, o.logprob, o.lse, o.argmax, o.vmax);
    }
    if (o.counter && blockIdx.x == 0 && threadIdx.x == 0) *o.counter += 1;
}
