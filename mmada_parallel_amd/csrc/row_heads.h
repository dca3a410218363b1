// row_heads.h — the contract of the LM head's row heads (host and device): what the launchers (row_heads.hip, tp_heads.hip), the
// GEMM epilogue (row_head_epilogue.h) and the joins (row_head_join.h) must agree on.  Nothing of D = A · lm_head[col0 : col0 + N]^T is
// stored: per row m < rows and 256-column tile nt the GEMM leaves records over the bf16-rounded logits x of that tile.
//   EPI_ROWSTAT   (scoring, mmada_head_logprobs)  part[nt * ld + m] = {max, sum exp(x - max), first column of the max in the whole
//                 vocabulary (int bits), 0}, and the logit at column target[m] - col0 (if that is a column of the launch) to tx[m].
//   EPI_ROWTOPK   (top-k, mmada_head_topk)        the same record with the same bits (and the target logit where `target` is not
//                 null — null: no row has one), plus extra[(nt * ld + m) * 8 .. + 8): the tile's eight best logits as 32-bit keys
//                 (topk_key below) in descending order = logit descending, then column ascending.  Places beyond the tile's columns
//                 (N - 256 * nt < 8) hold 0, below every real key.
//   EPI_ROWSAMPLE (Gumbel-max draw, mmada_head_sample)  the same record with the same bits (no row has a target), plus
//                 extra[nt * ld + m] = {max key, its column in the whole vocabulary (int bits), the bf16 logit at that column as
//                 fp32, 0} — key = x + T * g(seed, *counter, row row0 + m, column in the whole vocabulary) (sample_noise.h); highest key,
//                 then lowest column.  Columns beyond N carry the key -inf.
// M may be `rows` rounded up to 8 (pad rows of A hold anything; their results are dropped).
#pragma once
#include "kernels.h"

constexpr bool is_row_head(int epi) { return epi == EPI_ROWSTAT || epi == EPI_ROWTOPK || epi == EPI_ROWSAMPLE; }

constexpr int ROW_HEAD_BN = 256;   // columns per record: one column tile of either GEMM kernel
constexpr int TOPK_MAX = 8;        // = MMADA_TOPK_MAX (include/mmada_mi355x.h); entries of a tile's key record

// ---- the argument block.  It travels in GemmArgs fields the row-head epilogue has no other use for, so that the argument block
// every GEMM kernel takes keeps its layout and no other kernel's compiled code changes.  THE aliasing, the only statement of it:
//     part -> C        tx -> resid      target -> pos_map      rows -> rwin      ld -> rlp      col0 -> rbeg
//     extra -> q       counter -> k     seed -> Hq (low half), Hkv (high half)   temperature -> Lq (its bits)
//     row0 -> m_base
// (ldc = ldr = 8: the 8-phase kernel's shape contract looks at them.)  A head that has no use for a field leaves it zero.
struct RowHeadArgs {
    float4* part;              // [ceil(N / 256)][ld] records
    float* tx;                 // [ld] target logits; -inf where no lane holds the target (preset by the launcher)
    const int64_t* target;     // [rows] column in the whole vocabulary, or negative: none.  Null (top-k, sample): no row has one
    int rows, ld, col0;
    void* extra;               // EPI_ROWTOPK: uint32_t [ceil(N / 256)][ld][8] keys; EPI_ROWSAMPLE: float4 [ceil(N / 256)][ld]
    const uint64_t* counter;   // EPI_ROWSAMPLE: device [1], one scalar load per wave
    uint64_t seed;             // EPI_ROWSAMPLE
    float temperature;         // EPI_ROWSAMPLE: finite, T >= 0
    int row0;                  // EPI_ROWSAMPLE: index in the CALL of the GEMM's row 0, for the noise only (a round of the tensor-parallel
                               // head: tp_heads.hip); zero everywhere else
};
static inline __host__ __device__ RowHeadArgs row_head_args(const GemmArgs& g) {
    float t;
    __builtin_memcpy(&t, &g.Lq, 4);
    return RowHeadArgs{(float4*)g.C, (float*)g.resid, (const int64_t*)g.pos_map, g.rwin, g.rlp, g.rbeg, (void*)g.q, (const uint64_t*)g.k,
                       (uint64_t)(uint32_t)g.Hq | ((uint64_t)(uint32_t)g.Hkv << 32), t, g.m_base};
}
static inline void set_row_head_args(GemmArgs& g, const RowHeadArgs& a) {
    g.C = (bf16_t*)a.part; g.resid = (const bf16_t*)a.tx; g.pos_map = (const int32_t*)a.target;
    g.ldc = 8; g.ldr = 8;
    g.rwin = a.rows; g.rlp = a.ld; g.rbeg = a.col0;
    g.q = (bf16_t*)a.extra;
    g.k = (bf16_t*)a.counter;
    g.Hq = (int)(uint32_t)a.seed; g.Hkv = (int)(uint32_t)(a.seed >> 32);
    __builtin_memcpy(&g.Lq, &a.temperature, 4);
    g.m_base = a.row0;
}
// What launch_gemm refuses: the message, or null when the block is complete for `head` (M: rows of the GEMM)
static inline const char* row_head_args_fault(int head, const RowHeadArgs& a, int M) {
    const bool sample = head == EPI_ROWSAMPLE;
    const bool missing = !a.part || !a.tx || (head == EPI_ROWSTAT ? !a.target : !a.extra) || (sample && !a.counter);
    const bool bad_t = sample && (!(a.temperature >= 0.f) || __builtin_isinf(a.temperature));
    if (!missing && a.rows > 0 && a.rows <= M && a.ld >= a.rows && !bad_t) return nullptr;
    return head == EPI_ROWSTAT   ? "gemm/rowstat: record buffers missing"
           : head == EPI_ROWTOPK ? "gemm/rowtopk: record buffers missing"
                                 : "gemm/rowsample: record buffers or counter missing, or a temperature that is not finite and >= 0";
}

// The GEMM of head `head`: A [M, K] (M: `a.rows` rounded up to 8) times W = lm_head rows [a.col0, a.col0 + N), with the records
// going where the caller has carved a.part / a.tx / a.extra.  publish: the records are read by other ranks (GemmArgs::publish).
// (row_heads.hip; the one launch of both the one-rank heads and a round of the tensor-parallel ones.)
int launch_row_head_gemm(int head, const bf16_t* A, const bf16_t* W, int M, int N, int K, const RowHeadArgs& a, bool publish, hipStream_t s);

// Bytes of a head's extra record per (row, tile): none (scoring), the tile's keys (top-k), one triple (sample)
constexpr uint32_t row_head_extra_bytes(int head) {
    return head == EPI_ROWTOPK ? TOPK_MAX * (uint32_t)sizeof(uint32_t) : head == EPI_ROWSAMPLE ? (uint32_t)sizeof(float4) : 0u;
}

// ---- the record buffer of a one-rank launch: records | target logits | extra records.  Per row 1/32 (scoring), 3/32 (top-k) or
// 1/16 (sample) of the bytes of the bf16 logits it stands for, plus 4 bytes.  (The tensor-parallel heads publish their records in
// a layout of their own: tp_comm.h, ScoreLayout.)
struct RowHeadLayout {
    int rp, ntn;                   // rows rounded up to 8 (the records' leading dimension), 256-column tiles
    size_t part, tx, extra, bytes; // byte offsets of the three sub-buffers, total size
};
static inline RowHeadLayout row_head_layout(int R, int N, int head) {
    RowHeadLayout l;
    l.rp = (R + 7) / 8 * 8;
    l.ntn = (N + ROW_HEAD_BN - 1) / ROW_HEAD_BN;
    const size_t recs = (size_t)l.rp * l.ntn;
    l.part = 0;
    l.tx = recs * sizeof(float4);
    l.extra = l.tx + (size_t)l.rp * sizeof(float);
    l.bytes = l.extra + recs * row_head_extra_bytes(head);
    return l;
}

// ---- the key of the top-k head: high half = the bf16 bits of the logit mapped to an unsigned value of the same order, low byte =
// 255 - column inside the tile; an unsigned compare is the whole order and the keys of a tile are distinct.
// Order value of a bf16-rounded logit x (an fp32 whose low 16 bits are zero), in the HIGH half of the result: negatives with all
// bits flipped, the rest with the sign bit flipped, so that an unsigned compare orders as the floats do.  -0.0 is taken as +0.0
// first (x + 0.0f): torch's sort compares floats, for which the two are equal and the lower column wins.  NaN: outside the contract.
static inline __host__ __device__ uint32_t topk_order(float x) {
    const float c = x + 0.0f;
    uint32_t u;
    __builtin_memcpy(&u, &c, 4);
    return u ^ ((uint32_t)((int32_t)u >> 31) & 0x7fff0000u) ^ 0x80000000u;
}
static inline __host__ __device__ uint32_t topk_key(float x, int col_in_tile) { return (topk_order(x) & 0xffff0000u) | (uint32_t)(255 - col_in_tile); }
static inline __host__ __device__ float topk_key_logit(uint32_t key) {   // inverse of topk_order on the key's high half
    const uint32_t o = key & 0xffff0000u, u = (o & 0x80000000u) ? o ^ 0x80000000u : o ^ 0xffff0000u;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// ---- the order of the sampling head's triples {key, column, logit}: highest key, then lowest column (the epilogue's and the join's)
MM_DEVICE void rowsample_take(float& k, int& c, float& x, float ok, int oc, float ox) {
    if (ok > k || (ok == k && oc < c)) { k = ok; c = oc; x = ox; }
}
