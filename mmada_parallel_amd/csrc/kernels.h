// kernels.h — host-side launcher declarations shared between the .hip translation units and api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

enum GemmEpilogue { EPI_STORE = 0, EPI_RESID = 1, EPI_SWIGLU = 2, EPI_QKV = 3, EPI_ROWSTAT = 4, EPI_ROWTOPK = 5, EPI_ROWSAMPLE = 6 };

struct GemmArgs {
    const bf16_t* A;   // [M, lda]   activations, K-contiguous
    const bf16_t* W;   // [N, ldw]   nn.Linear weight layout (out, in), K-contiguous
    bf16_t* C;         // [M, ldc]   (EPI_STORE / EPI_RESID / EPI_SWIGLU: ldc = N/2)
    int M, N, K;
    int lda, ldw, ldc;
    // EPI_RESID: C = bf16(resid + bf16(acc)) on the rows this rank owns the residual of, else bf16(acc).
    // Row m's residual is added by rank (m >> 4) % resid_mod, so that under tensor parallelism every rank reads
    // 1/tp of the residual stream instead of rank 0 reading all of it (resid_mod = 1: always add).
    const bf16_t* resid;
    int ldr;
    int resid_mod, resid_rank;
    // Row map of the residual read (0 = identity): C/A rows are compact [b*rwin + i], the residual is read from the
    // full-layout row b*rlp + rbeg + i (last block of a forward whose consumer only reads a row window).
    int rwin, rlp, rbeg;
    // >= K zeros: source of the A rows of the last row tile that lie beyond M (set by launch_gemm; null = re-read row M-1)
    const bf16_t* zero_row;
    // EPI_QKV: rows are (b, l) with m = b*Lp + l; columns are [q heads | k heads | v heads] x 128
    bf16_t* q;         // [B, Hq , Lkv, 128]
    bf16_t* k;         // [B, Hkv, Lkv, 128]
    bf16_t* vT;        // [B, Hkv, 128, Lkv]
    const float* rope_cos;  // [max_seq, 64]
    const float* rope_sin;  // [max_seq, 64]
    int Lp, Lkv, Hq, Hkv;
    int publish;       // != 0: C is read by OTHER agents / other XCDs' kernels polling a counter (tensor-parallel partials):
                       // every workgroup ends with a system-scope release so its stores have left this XCD's L2
    int m_base;        // EPI_QKV on a row chunk: A/M describe rows [m_base, m_base+M) of the [B*Lp] stream (b, l from m_base+m)
    // EPI_QKV with a position map (compute-mask forward of the dLLM cache, model/modeling_llada.py:929-937): stream row
    // m = b*Lp + i is the token at sequence position pos_map[m] (< 0: pad row).  q goes to the COMPACT row i of
    // q [B, Hq, Lq, 128]; k / v are scattered to row pos of the cache-resident k / vT (stride Lkv); nothing of a pad row is
    // kept.  Rotary position: k always pos; q pos, or i + q_pos_shift when q_pos_shift >= 0 (the reference's rotary
    // q_mask quirk with caching() off, :714-716,416-428).
    const int32_t* pos_map;
    int Lq, q_pos_shift;
    // EPI_SWIGLU in the 8-phase kernel: SiLU of a bf16 value as a table (gemm_epilogue.h: SiluLut) in device memory, or null =
    // evaluate it (set by launch_gemm)
    const uint16_t* silu_lut;
    int row_drop;      // set by gemm8's launcher only: row tiles of pitch BM - 16 (gemm8.hip, "short row tiles")
    int tile_gm, tile_gn;  // set by gemm8's launcher only: tile-order groups of tile_gm row tiles (0: all) x tile_gn column tiles
};

// A plain C[M, ldc] = A[M, K] · W[N, K]^T on K-contiguous operands (lda = ldw = K), epilogue fields left zero.
static inline GemmArgs gemm_bt_args(const bf16_t* A, const bf16_t* W, bf16_t* C, int M, int N, int K, int ldc) {
    GemmArgs g{};
    g.A = A; g.W = W; g.C = C;
    g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldw = K; g.ldc = ldc;
    return g;
}

// The measurement / test switches of mmada_set_option (include/mmada_mi355x.h: what each value means), resolved at one point in
// time: a switch never set takes the environment's default (MMADA_GEMM_CFG, MMADA_GEMM_SILU_LUT, MMADA_GEMM_SHORT_TILES,
// MMADA_GEMM_TILE_ORDER, MMADA_ATTN_FORM, MMADA_TP_EMULATE_MBPS: parsed once per process).  A launch takes one snapshot and decides
// everything from it.
struct Switches {
    int gemm_config, gemm_silu_lut, gemm_short_tiles, gemm_tile_order, attention_form, probe_variant, tp_allow_single_rank;
    int tp_emulate_mbps;   // >= 1: MB/s per link and direction of the emulated link (mmada_comm_set_mode 5)
};
Switches switches();

// gemm.hip: the launcher of every epilogue (it picks the kernel and the tile), the planner and the per-device constants.
// EPI_ROWSTAT, EPI_ROWTOPK, EPI_ROWSAMPLE are the row heads of the LM head: nothing of C is stored, and their arguments travel in
// GemmArgs fields these epilogues have no other use for (row_heads.h: RowHeadArgs, the records, the record buffer's layout).
// gemm8.hip: the 8-phase kernel, cfg = one of the GEMM8_* configurations; returns nonzero on a launch error.
// ran (or null): receives the configuration launch_gemm launched — 0..3 = GEMM8_*, 1000 + BM = the 16-wave kernel; left alone when
// nothing is launched
int launch_gemm(int epi, const GemmArgs& g, hipStream_t s, int* ran = nullptr);
enum Gemm8Cfg { GEMM8_320x256 = 0, GEMM8_256x256 = 1, GEMM8_160x256 = 2, GEMM8_320x128 = 3, GEMM8_NCFG = 4 };
bool gemm8_supports(const GemmArgs& g);  // shape contract of the 8-phase kernel (K % 128 == 0, K >= 256, M, N % 8 == 0, ...)
int launch_gemm8(int epi, int cfg, const GemmArgs& g, const Switches& sw, hipStream_t s);  // sw: short row tiles, tile order
int gemm_plan_code(int M, int N, int K);  // the planner's pick for a plain product: 0..3 or 1000 + BM; -1: unsupported shape
// allocate + fill the per-device constants of the GEMM launchers now (zero rows, SiLU table) instead of at the first launch
int gemm_prepare_device();

// row_heads.hip: the scoring head.  A [ceil8(R), K] (rows >= R: anything), W = lm_head rows [col0, col0 + N).  `part` holds
// head_rowstat_bytes(R, N) bytes (row_heads.h: row_head_layout).  Outputs [R] (lse / argmax / max may be null): logprob =
// x_target - lse (0 for a negative target, -inf for a target outside [col0, col0 + N)), argmax = column index in the WHOLE
// vocabulary (first maximum).
size_t head_rowstat_bytes(int R, int N);
int launch_head_rowstat(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, const int64_t* targets, void* part,
                        float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s);

// row_heads.hip: the top-k head.  Same operands; `part` holds head_rowtopk_bytes(R, N) bytes.  ids [R, k] (column in the whole
// vocabulary) and logits [R, k] in the order logit descending, column ascending; lse [R] or null: the bits launch_head_rowstat
// returns.  1 <= k <= TOPK_MAX, k <= N.
size_t head_rowtopk_bytes(int R, int N);
int launch_head_rowtopk(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, int k, void* part, int32_t* ids,
                        float* logits, float* lse, hipStream_t s);

// row_heads.hip: the sampling head.  Same operands; `part` holds head_rowsample_bytes(R, N) bytes.  ids [R]: arg-max of the key,
// column in the whole vocabulary; logprob [R] = x_drawn - lse; lse / argmax / vmax [R] or null: the bits launch_head_rowstat
// returns.  *counter is read by the GEMM's workgroups and incremented by the joining kernel, the last of the call.
size_t head_rowsample_bytes(int R, int N);
int launch_head_rowsample(const bf16_t* A, const bf16_t* W, int R, int N, int K, int col0, float temperature, uint64_t seed,
                          uint64_t* counter, void* part, int32_t* ids, float* logprob, float* lse, int32_t* argmax, float* vmax,
                          hipStream_t s);

// elementwise.hip
// norm_w != null: also xn = RMSNorm(x) * norm_w (the first norm of the forward, fused: SURVEY §2.3 K1)
int launch_embed(const int64_t* ids, const bf16_t* wte, bf16_t* x, int B, int L, int Lp, int d, int vocab, hipStream_t s,
                 const bf16_t* norm_w = nullptr, bf16_t* xn = nullptr, float eps = 0.f);
int launch_rmsnorm(const bf16_t* x, const bf16_t* w, bf16_t* out, int rows, int d, float eps, hipStream_t s);
// gathered rmsnorm: out[r] = rmsnorm(x[map(rows[r])]) where rows[r] = b*L + l and x rows are b*Lp + l
// x row of the flat index b*L + l is b*row_stride + l - row_off (row_stride = Lp, row_off = 0 for the full layout)
int launch_rmsnorm_gather(const bf16_t* x, const bf16_t* w, bf16_t* out, const int32_t* rows, int R, int L, int row_stride,
                          int d, float eps, hipStream_t s, int row_off = 0, int nflat = 0);
int launch_rope_table(float* cos_t, float* sin_t, const float* inv_freq_dev, int max_seq, hipStream_t s);
int launch_unpad_rows(const bf16_t* x, bf16_t* out, int B, int L, int Lp, int d, hipStream_t s);
int launch_iota_rows(int32_t* rows, int n, hipStream_t s);
// dLLM cache helpers: posmap[b*Lp + i] = pos[b*Tc + i] (i < Tc) or -1; dst[b*Lp_dst + pos] = src[b*Lp + i] for mapped rows
int launch_expand_pos(const int32_t* pos, int32_t* posmap, int B, int Tc, int Lp, int L, hipStream_t s);
int launch_scatter_rows(const bf16_t* src, bf16_t* dst, const int32_t* posmap, int M, int Lp, int Lp_dst, int d, hipStream_t s);
// weight repack
int launch_pack_qkv(const bf16_t* wq, const bf16_t* wk, const bf16_t* wv, bf16_t* out, int d, int Hq, int Hkv, int tp_rank,
                    int tp_size, hipStream_t s);
int launch_pack_gate_up(const bf16_t* gate, const bf16_t* up, bf16_t* out, int d, int F, int tp_rank, int tp_size,
                        hipStream_t s);
int launch_pack_cols(const bf16_t* w, bf16_t* out, int rows, int cols, int tp_rank, int tp_size, hipStream_t s);
// [B,H,L,128] -> padded q/k layout or K-major V copy (for the standalone mmada_sdpa entry point)
int launch_pad_heads(const bf16_t* in, bf16_t* out, int BH, int L, int Lkv, hipStream_t s);
int launch_transpose_v(const bf16_t* v, bf16_t* vT, int BH, int L, int Lkv, hipStream_t s);
int launch_lfq_gather(const int64_t* idx, void* out, int B, int N, int nbits, int f32, hipStream_t s);

// attention.hip:  q [B,Hq,Lkv,128], k [B,Hkv,Lkv,128], vT [B,Hkv,128,Lkv] -> out rows (b*Lp_out + l) x (Hq*128)
// Lq_alloc > 0: q is [B,Hq,Lq_alloc,128] (compact queries against longer cached keys); 0: q shares the keys' Lkv
int launch_attention(const bf16_t* q, const bf16_t* k, const bf16_t* vT, bf16_t* out, int B, int Hq, int Hkv, int L,
                     int Lq_rows, int Lkv, int out_row_stride_per_batch, int ld_out, hipStream_t s, int q_begin = 0,
                     int Lq_alloc = 0);

int attention_chunks(int pairs, int groups, int keys);  // workgroups per (batch, head) pair (the launch plan; host arithmetic)

// sampler.hip: three row kernels, one launcher and one argument record each.  A field a variant has no use for stays zero.
struct TextStat { float lmax; int32_t arg; double sum; };  // one rank's record of a text row (vocabulary-parallel head)

// Text step part 1: per masked (b, t) row x0 = arg-max, conf = softmax_f64(logits)[x0].
enum TextMode {
    TEXT_PLAIN,    // the logits as they are
    TEXT_CFG,      // logits = cond + text_cfg * (unc - cond), bf16 per op (the M variant)
    TEXT_PARTIAL,  // this rank's columns [col_off, col_off + V) only: a TextStat per row instead of conf / x0
};
struct TextStatsArgs {
    TextMode mode;
    const bf16_t* logits;    // [B*T, ld]; TEXT_CFG: the conditional branch
    const bf16_t* noisy;     // [B*T, ld] or null: the arg-max is taken over these instead (not TEXT_PARTIAL)
    const bf16_t* unc;       // TEXT_CFG: the unconditional branch
    float text_cfg;          // TEXT_CFG
    const int32_t* x0_in;    // [B*T] or null: an externally sampled x0 (not TEXT_PARTIAL)
    int B, T, V, ld;         // ld % 8 == 0
    int64_t* ids;            // [B, L]: read here; launch_text_select's commit writes it
    int L, text_start, mask_id;
    double* conf_out;        // [B*T]  (launch_text_select points both into its scratch)
    int32_t* x0_out;         // [B*T]
    int col_off;             // TEXT_PARTIAL
    TextStat* stat_out;      // TEXT_PARTIAL: [B*T], published to the other ranks
};
int launch_text_stats(const TextStatsArgs& a, hipStream_t s);
// scratch: conf [B*T] fp64 | x0 [B*T] int32
int launch_text_commit(const void* scratch, int B, int T, int64_t* ids, int L, int text_start, const int32_t* k, hipStream_t s);
// the scratch layout of launch_text_commit from a draw: x0 [B*T] int32 is already in place (scratch + B*T*8); conf[i] =
// (double)logprob[i] where ids holds the mask token, else -inf
int launch_text_sampled_conf(const float* logprob, int B, int T, const int64_t* ids, int L, int text_start, int mask_id, void* scratch,
                             hipStream_t s);
// the whole text step: launch_text_stats (TEXT_PLAIN / TEXT_CFG) into scratch, conf replaced by rand_conf [B*T] on masked rows
// when it is not null (remasking == 'random'), launch_text_commit
int launch_text_select(TextStatsArgs a, const int32_t* k, void* scratch, const float* rand_conf, hipStream_t s);

// Image step part 1: per (b, n) row the combined logits' bf16 soft-max statistics and, with a draw, the token.
enum ImageCombine {
    IMAGE_COMBINE_A,  // cond + cfg_scale * (cond - ut) + cfg_img * (cond - ui); a null branch or a zero scale drops its term
    IMAGE_COMBINE_M,  // cfg_img * cond - cfg_scale * ut with ut = the uncond branch, cfg_scale = image_cfg, cfg_img = 1 + image_cfg
};
enum ImageDraw {
    IMAGE_DRAW_NONE,         // statistics only: probs_out (may be null), argmax_out, pmax_out
    IMAGE_DRAW_UNIT,         // Gumbel-max draw at (seed, *counter) with the key at T = 1 (sample_noise.h)
    IMAGE_DRAW_TEMPERATURE,  // IMAGE_COMBINE_M only: the key at `temperature` (finite, >= 0; 0 = the arg-max of the logits); the
                             // statistics stay those of the unscaled logits
};
struct ImageRowArgs {
    ImageCombine combine;
    ImageDraw draw;
    const bf16_t *cond, *ut, *ui;  // [B*N, CB]
    int B, N, CB;
    float cfg_scale, cfg_img;
    int col0;                      // draw: the column of codebook entry 0 in the whole vocabulary
    uint64_t seed;                 // draw
    const uint64_t* counter;       // draw: device [1], read only
    float temperature;             // IMAGE_DRAW_TEMPERATURE: by value, a constant of the whole run
    bf16_t* probs_out;             // IMAGE_DRAW_NONE: [B*N, CB] or null
    int32_t* sampled_out;          // draw: [B*N]
    bf16_t* p_sel_out;             // draw: [B*N], the bits probs_out would hold at the drawn entry
    int32_t* argmax_out;           // [B*N]; a draw may leave it and pmax_out null
    bf16_t* pmax_out;              // [B*N]
};
int launch_image_row(const ImageRowArgs& a, hipStream_t s);

// Image step part 2: per batch row confidence, re-mask, write-back.
enum CommitRule {
    COMMIT_RULE_A,       // ids clamped to the codebook, log(p + 1e-10), the mask_len lowest in stable order, floor of 1
    COMMIT_RULE_M,       // no clamp, log(clamp(p, 1e-20)), cut-off compare, floor of 1
    COMMIT_RULE_M_KEEP,  // COMMIT_RULE_M with generate_image's keep rule: keep_n.clamp(0, unknown - 1), no floor of 1
};
enum CommitNoise {
    COMMIT_NOISE_TENSOR,  // `noise`, temperature temp_value
    COMMIT_NOISE_DEVICE,  // the normal (A) or Gumbel (M) value of (seed, *counter) (sample_noise.h), temperature *temp_dev —
                          // with COMMIT_RULE_M_KEEP, and only there, temp_dev is null and the temperature is temp_value.  The
                          // last launch adds 1 to *counter.
};
struct ImageCommitArgs {
    CommitRule rule;
    CommitNoise noise_from;
    int64_t* ids;                   // [B, L]
    int B, L;
    const int32_t* pos_map;         // [N]
    int N;                          // <= 8192
    const int32_t* sampled_in;      // [B, N]
    const bf16_t* p_in;             // [B, N]
    const int32_t* mask_len_sched;  // device [1]
    int mask_id, text_vocab, codebook;
    const bf16_t* noise;            // COMMIT_NOISE_TENSOR: [B, N]; null with COMMIT_RULE_A = no noise term, required otherwise
    float temp_value;
    const float* temp_dev;          // COMMIT_NOISE_DEVICE: device [1]
    uint64_t seed;                  // COMMIT_NOISE_DEVICE
    uint64_t* counter;              // COMMIT_NOISE_DEVICE: device [1]
    int32_t* sampled_out;           // COMMIT_NOISE_DEVICE with an M rule: [B, N] or null, the ids the commit writes back from
};
int launch_image_commit(const ImageCommitArgs& a, hipStream_t s);

// the M text draw: x0_out[b*T + t] = arg-max of the CFG-combined logits' keys at (seed, *counter); its last launch adds 1 to *counter
int launch_text_draw_cfg(const bf16_t* cond, const bf16_t* unc, float text_cfg, int B, int T, int V, int ld, float temperature,
                         uint64_t seed, uint64_t* counter, int32_t* x0_out, hipStream_t s);

// probe.hip: MFMA-only diagnostic (attainable roof at the sustained clock on random data)
int launch_f2bf_probe(const float* in, bf16_t* out, long long n, hipStream_t s);
int launch_gumbel_probe(uint64_t seed, uint64_t counter, int row0, int R, int col0, int N, uint32_t* words, float* g, hipStream_t s);
int launch_normal_probe(uint64_t seed, uint64_t counter, int row0, int R, uint32_t* words01, float* z, bf16_t* z_bf16, hipStream_t s);
int launch_mfma_probe(const bf16_t* data, float* sink, int iters, int launches, hipStream_t s, double* tflops_out, double* ms_out);
