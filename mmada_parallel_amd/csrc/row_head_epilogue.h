// row_head_epilogue.h — the GEMM epilogue of the LM head's row heads (EPI_ROWSTAT, EPI_ROWTOPK, EPI_ROWSAMPLE; the contract:
// row_heads.h), for both accumulator layouts.  Included by gemm_epilogue.h only.
//
// Nothing of D is stored: a workgroup reduces its BM x 256 logits to one record per row, {max, sum exp(x - max), first column of
// the max}, and hands the one logit at the row's target column out.  x is the accumulator ROUNDED TO BF16 first — the logits
// nn.Linear would have written (the rounding point every other epilogue keeps).  ONE skeleton (rowstat_epilogue) of three steps and
// two workgroup barriers, through the LDS the main loop has finished with:
//   1. every wave: max / first arg-max over its 64 columns of each of its rows — in registers over the lane's values, then
//      across the lanes that share the row (RowLanes::reduce);
//   2. with the TILE's max of the row (the 4 waves' maxima from LDS): sum of exp2((x - max) * log2 e), one v_exp_f32 per logit;
//   3. thread r of the workgroup joins the 4 waves' records of tile row r and writes the record (one 16-byte store, 256 B per 16
//      lanes).
// The top-k and the sampling head add their own work at steps 1 and 3 (rowtopk_rounds / rowtopk_merge, rowsample_wave_best /
// rowsample_merge below), each behind the scoring head's LDS arrays.
// The sum is evaluated in ONE fixed tree whatever kernel, tile height or operand order ran: groups of 4 consecutive columns
// (e0 + e1) + (e2 + e3); the 4 fragments of a wave's 64 columns in order; the 4 column groups of a fragment (g0 + g1) + (g2 + g3);
// the 4 waves (w0 + w1) + (w2 + w3).  fp32 addition commutes, so both layouts produce the same bits; max, arg-max and the target
// logit are functions of the bf16 logits alone.
#pragma once
#include "row_heads.h"
#include "sample_noise.h"

namespace gemm_detail {

// LDS addresses are plain integers here (gemm8.hip)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"
template <class T>
MM_DEVICE T lds_ld(int byte_off) { return *(__attribute__((address_space(3))) T*)(uint32_t)byte_off; }
template <class T>
MM_DEVICE void lds_st(int byte_off, T v) { *(__attribute__((address_space(3))) T*)(uint32_t)byte_off = v; }
#pragma clang diagnostic pop

// The scoring head's arrays, [wave column][tile row] each: 15 KiB
struct RowStatLds {
    static constexpr int ROWS = 320, WAVES = 4;   // tallest row tile, wave columns of a 256-column tile of 64-column waves
    static constexpr int MAX = 0, ARG = ROWS * WAVES * 4, SUM = 2 * ROWS * WAVES * 4, BYTES = 3 * ROWS * WAVES * 4;
    static MM_DEVICE int at(int wn, int rt) { return (wn * ROWS + rt) * 4; }   // byte offset inside one array
};
// EPI_ROWTOPK: behind them every wave column's eight keys of a row (32 B), 40 KiB
struct RowTopkLds {
    static constexpr int KEYS = RowStatLds::BYTES, BYTES = KEYS + RowStatLds::ROWS * RowStatLds::WAVES * TOPK_MAX * 4;
    static MM_DEVICE int at(int wn, int rt) { return KEYS + (wn * RowStatLds::ROWS + rt) * (TOPK_MAX * 4); }
};
// EPI_ROWSAMPLE: behind them every wave column's best {key, column, logit} of a row, three arrays
struct RowSampleLds {
    static constexpr int N1 = RowStatLds::ROWS * RowStatLds::WAVES * 4;
    static constexpr int KEY = RowStatLds::BYTES, COL = KEY + N1, X = COL + N1, BYTES = X + N1;
};
static_assert(RowSampleLds::BYTES <= RowTopkLds::BYTES, "the sampling head fits the LDS the top-k head reserves");

// ---- the two accumulator layouts (TR: transposed, gemm_epilogue_t; else gemm_epilogue), lane = (lq = lane >> 4, l15 = lane & 15).
// A SLOT is a row a lane takes part in; per slot the lane holds NR consecutive columns of each of the wave's FN fragments:
//     TR:    FM slots,     row sl*16 + l15,                       columns ni*16 + lq*4 + r, r < 4
//     else:  FM * 4 slots, row (sl >> 2)*16 + lq*4 + (sl & 3),    column  ni*16 + l15
template <bool TR>
struct RowLanes {
    static constexpr int NR = TR ? 4 : 1;
    static constexpr int slots(int fm) { return TR ? fm : fm * 4; }
    // row of slot sl and column of its value (ni, r), from the wave's first row / column.  (Sums in this order: the compiled
    // 16-wave kernels are sensitive to it.)
    static MM_DEVICE int row(int row0, int sl, int l15, int lq) { return TR ? row0 + sl * 16 + l15 : row0 + (sl >> 2) * 16 + lq * 4 + (sl & 3); }
    static MM_DEVICE int col(int col0, int ni, int r, int l15, int lq) { return col0 + ni * 16 + (TR ? lq * 4 + r : l15); }
    static MM_DEVICE bool writer(int l15, int lq) { return TR ? lq == 0 : l15 == 0; }   // the one lane of a row that stores the wave's result
    template <int FM, int FN>
    static MM_DEVICE float acc_at(const f32x4 (&acc)[FM][FN], int sl, int ni, int r) {
        if constexpr (TR) return acc[sl][ni][r];
        else return acc[sl >> 2][ni][sl & 3];
    }
    // step(o) combines a lane's value with lane ^ o's; over the lanes that share a row (TR: ^16, ^32; else ^1 ... ^8), or with
    // FROM = 4 over the row's four groups of 4 consecutive columns only (the same lanes when TR: a lane holds a whole group)
    template <int FROM = 1, class Step>
    static MM_DEVICE void reduce(Step step) {
#pragma unroll
        for (int o = TR ? 16 : FROM; o < (TR ? 64 : 16); o <<= 1) step(o);
    }
};

MM_DEVICE uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
MM_DEVICE void rowstat_take(float& m, int& a, float om, int oa) {   // torch's arg-max tie rule: the first index wins
    if (om > m || (om == m && oa < a)) { m = om; a = oa; }
}
MM_DEVICE float rowstat_exp(float x, float m) {
#pragma clang fp contract(off)
    return __builtin_amdgcn_exp2f((x - m) * 1.44269504088896340736f);
}
// column (inside the launch of N columns) of row m's target, or -1: none in this launch
MM_DEVICE int rowstat_target(const RowHeadArgs& a, int N, int m) {
    const long long t = a.target[m] - (long long)a.col0;
    return t >= 0 && t < (long long)N ? (int)t : -1;
}

// ---- EPI_ROWTOPK, step 1: the wave column's eight best keys of a row, from the lane's NV keys of it (topk_key; the skeleton fills
// them).  Eight rounds of { the lane's best remaining key ; the best of the lanes that share the row ; the lane that holds the
// winner retires it — keys are distinct, an equality compare finds it }.  The writer lane stores the eight (two 16-byte LDS stores)
// at `at`.  A retired key is 0, below every real key (the order value of -inf is 0x007f).
template <bool TR, int NV>
MM_DEVICE void rowtopk_rounds(uint32_t (&key)[NV], bool writer, int at) {
    uint32_t win[TOPK_MAX];
#pragma unroll
    for (int e = 0; e < TOPK_MAX; ++e) {
        uint32_t b = key[0];
#pragma unroll
        for (int i = 1; i < NV; ++i) b = umax32(b, key[i]);
        RowLanes<TR>::reduce([&](int o) { b = umax32(b, __shfl_xor(b, o, 64)); });
        win[e] = b;
#pragma unroll
        for (int i = 0; i < NV; ++i) key[i] = key[i] == b ? 0u : key[i];
    }
    if (writer) {
        lds_st(at, u32x4{win[0], win[1], win[2], win[3]});
        lds_st(at + 16, u32x4{win[4], win[5], win[6], win[7]});
    }
}
// ---- EPI_ROWTOPK, step 3: the thread that joins tile row rt merges the four wave columns' sorted lists (eight rounds over the four
// list heads) and writes the 32-byte record as two 16-byte stores
template <int WN>
MM_DEVICE void rowtopk_merge(int lds, int rt, u32x4* dst) {
    int at4[WN];
    uint32_t head[WN], best[TOPK_MAX];
#pragma unroll
    for (int w = 0; w < WN; ++w) {
        at4[w] = lds + RowTopkLds::at(w, rt);
        head[w] = lds_ld<uint32_t>(at4[w]);
    }
#pragma unroll
    for (int e = 0; e < TOPK_MAX; ++e) {
        const uint32_t b = umax32(umax32(head[0], head[1]), umax32(head[2], head[3]));
        best[e] = b;
        if (e + 1 < TOPK_MAX) {   // the list that held the winner moves on (b = 0: every list is exhausted, zeros follow)
#pragma unroll
            for (int w = 0; w < WN; ++w) {
                at4[w] += head[w] == b ? 4 : 0;
                head[w] = lds_ld<uint32_t>(at4[w]);
            }
        }
    }
    dst[0] = u32x4{best[0], best[1], best[2], best[3]};
    dst[1] = u32x4{best[4], best[5], best[6], best[7]};
}

// ---- EPI_ROWSAMPLE, step 1: the wave column's best {key, column, logit} of noise row m: key = x + T * g of the lane's values, the lane's
// best (the first column on equal keys), then the best of the lanes that share the row.  When a lane holds four consecutive columns
// they cost one Philox evaluation (two when the launch's first column is no multiple of 4), otherwise every value costs one.  The
// writer lane stores the triple at `at`.  val(ni, r): the lane's logits of this row; c0: the lane's first column inside the launch
// of N columns (columns beyond N carry the key -inf).
template <bool TR, int FN, class Val>
MM_DEVICE void rowsample_wave_best(Val val, const RowHeadArgs& a, uint64_t ctr, int m, int c0, int N, bool writer, int at) {
    using L = RowLanes<TR>;
    const float NEG = -__builtin_inff();
    const uint32_t gc0 = (uint32_t)(a.col0 + c0);     // column in the whole vocabulary of the lane's first value
    const uint32_t sh = (uint32_t)a.col0 & 3u;        // wave-uniform: c0 is a multiple of 4 in the transposed layout
    float bk = NEG, bx = NEG;
    int bc = c0;
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) {
        const uint32_t gc = gc0 + ni * 16;
        uint32_t w0, w1 = 0u, w2 = 0u, w3 = 0u;
        if constexpr (TR) {
            sample_words4(a.seed, ctr, (uint32_t)m, gc >> 2, w0, w1, w2, w3);
            if (sh) {   // the lane's four columns straddle two blocks
                uint32_t q0, q1, q2, q3;
                sample_words4(a.seed, ctr, (uint32_t)m, (gc >> 2) + 1u, q0, q1, q2, q3);
                const uint32_t a1 = w1, a2 = w2, a3 = w3;    // the columns are words sh .. sh + 3 of the pair
                w0 = sh == 1u ? a1 : sh == 2u ? a2 : a3;
                w1 = sh == 1u ? a2 : sh == 2u ? a3 : q0;
                w2 = sh == 1u ? a3 : sh == 2u ? q0 : q1;
                w3 = sh == 1u ? q0 : sh == 2u ? q1 : q2;
            }
        } else
            w0 = sample_word(a.seed, ctr, (uint32_t)m, gc);
#pragma unroll
        for (int r = 0; r < L::NR; ++r) {
            const float x = val(ni, r);
            const int n = c0 + ni * 16 + r;
            const uint32_t w = r == 0 ? w0 : r == 1 ? w1 : r == 2 ? w2 : w3;
            const float key = n < N ? sample_key(x, a.temperature, sample_gumbel(w)) : NEG;
            if (key > bk) { bk = key; bc = c0 + ni * 16 + r; bx = x; }
        }
    }
    L::reduce([&](int o) { rowsample_take(bk, bc, bx, __shfl_xor(bk, o, 64), __shfl_xor(bc, o, 64), __shfl_xor(bx, o, 64)); });
    if (writer) {
        lds_st(RowSampleLds::KEY + at, bk);
        lds_st(RowSampleLds::COL + at, bc);
        lds_st(RowSampleLds::X + at, bx);
    }
}
// ---- EPI_ROWSAMPLE, step 3: the thread that joins tile row rt takes the best of the four wave columns (they ascend: a later equal
// key does not replace) and writes the second 16-byte record
template <int WN>
MM_DEVICE void rowsample_merge(int lds, int rt, int col0, float4* dst) {
    float bk = lds_ld<float>(lds + RowSampleLds::KEY + rt * 4), bx = lds_ld<float>(lds + RowSampleLds::X + rt * 4);
    int bc = lds_ld<int>(lds + RowSampleLds::COL + rt * 4);
#pragma unroll
    for (int w = 1; w < WN; ++w) {
        const int at = lds + RowStatLds::at(w, rt);
        const float ok = lds_ld<float>(RowSampleLds::KEY + at);
        if (ok > bk) { bk = ok; bc = lds_ld<int>(RowSampleLds::COL + at); bx = lds_ld<float>(RowSampleLds::X + at); }
    }
    *dst = float4{bk, __int_as_float(bc + col0), bx, 0.f};
}

// ---- the skeleton.  EPI: the head; TR: the accumulator layout; lds: byte address of RowStatLds::BYTES free bytes (EPI_ROWTOPK:
// RowTopkLds::BYTES, EPI_ROWSAMPLE: RowSampleLds::BYTES)
template <int EPI, bool TR, int TM, int TN, int WN>
MM_DEVICE void rowstat_epilogue(const GemmArgs& g, int m0, int n0, f32x4 (&acc)[TM / 16][TN / 16], int wave, int lane, int m_lim, int lds,
                                 int bm /* rows of the workgroup's tile, <= RowStatLds::ROWS */) {
#pragma clang fp contract(off)
    using L = RowLanes<TR>;
    constexpr int FM = TM / 16, FN = TN / 16, NS = L::slots(FM);
    constexpr bool TOPK = EPI == EPI_ROWTOPK, SAMPLE = EPI == EPI_ROWSAMPLE;
    static_assert(is_row_head(EPI) && TN == 64 && WN == RowStatLds::WAVES && TN * WN == ROW_HEAD_BN, "row heads: 256-column tiles of four 64-column waves");
    const int wm = wave / WN, wn = wave % WN;
    const int l15 = lane & 15, lq = lane >> 4;
    const int wcol0 = n0 + wn * TN;
    const RowHeadArgs a = row_head_args(g);
    const int rows = min(m_lim, a.rows);
    const float NEG = -__builtin_inff();
    const bool writer = L::writer(l15, lq);
    uint64_t ctr = 0;
    if constexpr (SAMPLE) ctr = *a.counter;   // the same address in every lane: one scalar load per wave
    // SAMPLE in the untransposed layout (the 16-wave kernel: 128 VGPRs per lane): the logits are needed as bf16 values only, so
    // they are rounded once and kept two to a register — 40 registers instead of 80 at 320 rows — which is what lets the draw's
    // Philox state and logarithms fit beside them without scratch.  Unpacking a value is one shift or mask, exact.
    constexpr bool PACKED = SAMPLE && !TR;
    uint32_t pk[PACKED ? FM : 1][PACKED ? FN : 1][2];
    if constexpr (PACKED) {
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) {
                pk[mi][ni][0] = pack_bf2(acc[mi][ni][0], acc[mi][ni][1]);
                pk[mi][ni][1] = pack_bf2(acc[mi][ni][2], acc[mi][ni][3]);
            }
    }
    // between two steps: the unpacked values of one step are not kept in registers for the next (the compiler would otherwise
    // reuse them — all 80 again); every step unpacks what it needs, when it needs it
    auto repack = [&]() {
        if constexpr (PACKED) {
#pragma unroll
            for (int mi = 0; mi < FM; ++mi)
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) asm volatile("" : "+v"(pk[mi][ni][0]), "+v"(pk[mi][ni][1]));
        }
    };
    repack();   // ... and the packing itself happens HERE, not where a value is first used (the fp32 accumulators die now)
    auto slot_row = [&](int sl) { return L::row(wm * TM, sl, l15, lq); };   // row inside the workgroup's tile
    auto val = [&](int sl, int ni, int r) {   // bf16-rounded logit; columns beyond N never win and add nothing
        const int n = L::col(wcol0, ni, r, l15, lq);
        if constexpr (PACKED) {
            const uint32_t p = pk[sl >> 2][ni][(sl & 3) >> 1];
            return n < g.N ? __uint_as_float((sl & 1) ? p & 0xffff0000u : p << 16) : NEG;
        } else
            return n < g.N ? bfround(L::acc_at(acc, sl, ni, r)) : NEG;
    };
    // ---- 1: wave maxima; the target logit; the head's own keys ----
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
        const int rt = slot_row(sl), m = m0 + rt;
        // (the scoring head always has targets, the top-k head may, the sampling head never)
        const int tc = !SAMPLE && m < rows && (!TOPK || a.target) ? rowstat_target(a, g.N, m) : -1;
        const int c0 = L::col(wcol0, 0, 0, l15, lq);   // the lane's first column inside the launch: value (ni, r) is column c0 + ni*16 + r
        float bm = NEG;
        int ba = c0;
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
#pragma unroll
            for (int r = 0; r < L::NR; ++r) {
                const float x = val(sl, ni, r);
                if (x > bm) { bm = x; ba = c0 + ni * 16 + r; }
            }
        const int d = tc - c0;   // this lane holds the target column if d = ni*16 + r
        if (tc >= 0 && d >= 0 && d < TN && (d & 15) < L::NR) {
            float x = NEG;
#pragma unroll
            for (int ni = 0; ni < FN; ++ni)
#pragma unroll
                for (int r = 0; r < L::NR; ++r)
                    if (d == ni * 16 + r) x = val(sl, ni, r);
            a.tx[m] = x;
        }
        L::reduce([&](int o) { rowstat_take(bm, ba, __shfl_xor(bm, o, 64), __shfl_xor(ba, o, 64)); });
        if (writer) {
            lds_st(lds + RowStatLds::MAX + RowStatLds::at(wn, rt), bm);
            lds_st(lds + RowStatLds::ARG + RowStatLds::at(wn, rt), ba);
        }
        if constexpr (TOPK) {
            // the lane's keys; columns beyond N carry key 0.  They read the accumulators HERE, in the skeleton, and not through val()
            // or inside a helper: either costs 3 registers on every 16-wave kernel and more scratch on the 320-row one
            uint32_t key[FN * L::NR];
#pragma unroll
            for (int ni = 0; ni < FN; ++ni)
#pragma unroll
                for (int r = 0; r < L::NR; ++r) {
                    const int ct = L::col(wn * TN, ni, r, l15, lq);   // column inside the 256-column tile
                    key[ni * L::NR + r] = n0 + ct < g.N ? topk_key(bfround(L::acc_at(acc, sl, ni, r)), ct) : 0u;
                }
            rowtopk_rounds<TR>(key, writer, lds + RowTopkLds::at(wn, rt));
        }
        if constexpr (SAMPLE)
            // (the noise row: the row's index in the CALL — a.row0 is wave-uniform and zero outside a tensor-parallel round)
            rowsample_wave_best<TR, FN>([&](int ni, int r) { return val(sl, ni, r); }, a, ctr, m + a.row0, c0, g.N, writer, lds + RowStatLds::at(wn, rt));
    }
    repack();
    __syncthreads();
    // ---- 2: sums of exponentials against the tile's row max ----
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
        const int rt = slot_row(sl);
        float mt = lds_ld<float>(lds + RowStatLds::MAX + rt * 4);
#pragma unroll
        for (int w = 1; w < WN; ++w) mt = fmaxf(mt, lds_ld<float>(lds + RowStatLds::MAX + RowStatLds::at(w, rt)));
        float s = 0.f;
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
            float gsum;   // a group of 4 consecutive columns: in the lane, or over 4 lanes
            if constexpr (TR) {
                gsum = (rowstat_exp(val(sl, ni, 0), mt) + rowstat_exp(val(sl, ni, 1), mt)) +
                       (rowstat_exp(val(sl, ni, 2), mt) + rowstat_exp(val(sl, ni, 3), mt));
            } else {
                gsum = rowstat_exp(val(sl, ni, 0), mt);
                gsum += __shfl_xor(gsum, 1, 64);
                gsum += __shfl_xor(gsum, 2, 64);
            }
            s = ni == 0 ? gsum : s + gsum;
        }
        L::template reduce<4>([&](int o) { s += __shfl_xor(s, o, 64); });
        if (writer) lds_st(lds + RowStatLds::SUM + RowStatLds::at(wn, rt), s);
    }
    __syncthreads();
    // ---- 3: one record per tile row ----
    const int rt = wave * 64 + lane, m = m0 + rt;
    if (rt < bm && m < rows) {
        float mw[WN], sw[WN];
        int aw[WN];
#pragma unroll
        for (int w = 0; w < WN; ++w) {
            mw[w] = lds_ld<float>(lds + RowStatLds::MAX + RowStatLds::at(w, rt));
            aw[w] = lds_ld<int>(lds + RowStatLds::ARG + RowStatLds::at(w, rt));
            sw[w] = lds_ld<float>(lds + RowStatLds::SUM + RowStatLds::at(w, rt));
        }
        float mt = mw[0];
        int at = aw[0];
#pragma unroll
        for (int w = 1; w < WN; ++w)
            if (mw[w] > mt) { mt = mw[w]; at = aw[w]; }   // wave columns ascend: a later equal maximum does not replace
        const float st = (sw[0] + sw[1]) + (sw[2] + sw[3]);
        const size_t rec = (size_t)(n0 / ROW_HEAD_BN) * a.ld + m;
        a.part[rec] = float4{mt, st, __int_as_float(at + a.col0), 0.f};
        if constexpr (TOPK) rowtopk_merge<WN>(lds, rt, (u32x4*)((uint32_t*)a.extra + rec * TOPK_MAX));
        if constexpr (SAMPLE) rowsample_merge<WN>(lds, rt, a.col0, (float4*)a.extra + rec);
    }
}

}  // namespace gemm_detail
