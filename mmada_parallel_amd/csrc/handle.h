// handle.h — the library's private state behind the opaque mmada_handle (shared by api.hip, forward.hip, cache.hip, heads.hip
// and the tensor-parallel units).
#pragma once
#include <utility>
#include <vector>

#include "../../include/mmada_mi355x.h"
#include "kernels.h"

struct TpComm;  // tp_comm.h (private to tp_comm.hip / tp_heads.hip)

struct LayerWeights {
    bf16_t* wqkv = nullptr;   // [(Hq_l + 2 Hkv_l) * 128, d]   fused, rotary-partner permuted
    bf16_t* wo = nullptr;     // [d, Hq_l * 128]
    bf16_t* wgu = nullptr;    // [2 F_l, d]                    16-row interleaved ff_proj / up_proj
    bf16_t* wdown = nullptr;  // [d, F_l]
    bf16_t* attn_norm = nullptr;  // [d]
    bf16_t* ff_norm = nullptr;    // [d]
    bool bound = false;
};

// One dLLM-cache slot (the reference's `cat` key: model/modeling_llada.py:593-597,929-940,1406-1413): caller-owned device
// memory holding, for B sequences of length L, every block's keys (rotated, attention layout) and K-major values plus
// the residual stream after the last block; see mmada_cache_bind.
struct CacheSlot {
    char* mem = nullptr;
    size_t bytes = 0, layer_stride = 0, kv_bytes = 0;
    int B = 0, L = 0, Lp = 0, Lkv = 0;
    bool normalized = false;   // the final rows are ALREADY ln_f-normalised (written by a tensor-parallel forward, whose last
                               // exchange applies ln_f on the owners' rows): mmada_cache_head_rows gathers them without a norm
    bf16_t* K(int layer) const { return (bf16_t*)(mem + (size_t)layer * layer_stride); }
    bf16_t* vT(int layer) const { return (bf16_t*)(mem + (size_t)layer * layer_stride + kv_bytes); }
    bf16_t* xfin(int n_layers) const { return (bf16_t*)(mem + (size_t)n_layers * layer_stride); }
};
constexpr int MMADA_CACHE_SLOTS = 16;

// Which forward is resident in the workspace (mmada_handle::res).  One rule, for every entry point:
//   - a call that fails BEFORE it has written to the workspace leaves the resident forward as it was;
//   - a call that fails AFTER that leaves none resident.
// (A cache step and mmada_sdpa leave none resident when they succeed, too: what they wrote is not a plain forward.)
struct Resident {
    int B = 0, L = 0, Lp = 0, Lkv = 0;
    int M = 0;   // stream rows B * Lp; 0: nothing is resident — read through resident(h), cleared through invalidate(h)
    // consumed-row window (mmada_set_consumed_rows): while a forward whose last block ran windowed is resident, the stream is
    // compact: cur_W rows per sequence starting at row cur_beg, Mcur rows in all (no window: cur_W = 0, Mcur = M)
    int cur_W = 0, cur_beg = 0, Mcur = 0;
    // xn already holds ln_f(x) for every row (the last reduce-scatter of a tensor-parallel forward applies ln_f on the owned rows)
    bool xn_is_final = false;
    bool xn_is_layer0 = false;  // mmada_embed already wrote xn = RMSNorm(x) * blocks[0].attn_norm (fused, K1)
    // dLLM cache: the slot a forward in flight writes its keys / values into (non-null only inside a CacheStep); cc_pos: position
    // map of a compute-mask step (null: every row is computed); cc_qshift >= 0: queries are rotated by row index + shift
    const CacheSlot* cc = nullptr;
    const int32_t* cc_pos = nullptr;
    int cc_qshift = -1;
};

struct mmada_handle {
    mmada_cfg cfg;
    int hq_l, hkv_l, f_l;  // per-rank heads / mlp columns
    float* rope_cos = nullptr;
    float* rope_sin = nullptr;
    const bf16_t* wte = nullptr;
    const bf16_t* ln_f = nullptr;
    const bf16_t* lm_head = nullptr;
    std::vector<LayerWeights> layers;
    bool owns_weights = true;  // false for mmada_clone_shared handles
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    // current carve, and the forward it holds
    Resident res;
    bf16_t *x = nullptr, *y = nullptr, *xn = nullptr, *att = nullptr, *hbuf = nullptr, *q = nullptr, *k = nullptr,
           *vT = nullptr, *xg = nullptr;
    int32_t* rows_all = nullptr;
    int32_t* posmap = nullptr;  // [B*Lp] sequence position of every compact stream row (compute-mask forward)
    CacheSlot slots[MMADA_CACHE_SLOTS];
    int win_beg = 0, win_end = 0;  // mmada_set_consumed_rows: requested [win_beg, win_end) per sequence
    // live timing (mmada_profile_begin/end)
    int prof_layer = -1;
    struct ProfRec { int kind; hipEvent_t a, b; double flops; };
    std::vector<ProfRec> prof;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
    TpComm* tp = nullptr;  // tensor-parallel collective engine (tp_comm.hip; mmada_comm_*)
    // record buffer of mmada_head_logprobs / mmada_head_topk / mmada_head_sample (row_heads.h: row_head_layout; head_rowstat_bytes, head_rowtopk_bytes,
    // head_rowsample_bytes), grown at first use, freed with the handle
    void* score_buf = nullptr;
    size_t score_bytes = 0;
};

inline bool resident(const mmada_handle* h) { return h->res.M != 0; }
inline void invalidate(mmada_handle* h) { h->res.M = 0; }

// forward.hip: the start of every forward — weights bound, workspace carved for (B, L) (a failure up to here leaves the resident
// forward alone), then a fresh Resident: no window, xn = the first norm of the embedding kernel
int begin_forward(mmada_handle* h, int B, int L, hipStream_t s);
// forward.hip: the cache step of mmada_forward_cached.  While it lives, the block builders below read and write the slot's keys /
// values; when it goes, on every exit, they no longer do and no forward is resident (the step ran on the compact stream of
// the computed tokens, and its result lives in the slot)
struct CacheStep {
    mmada_handle* h;
    CacheStep(mmada_handle* h, const CacheSlot* slot, const int32_t* pos, int qshift);
    ~CacheStep();
    CacheStep(const CacheStep&) = delete;
    CacheStep& operator=(const CacheStep&) = delete;
};

// forward.hip: one block's launches (the one-rank forward: m0 = 0, every row; the tensor-parallel forward: one row chunk each).  The
// GemmArgs of block `layer`'s projections on stream rows [m0, m0 + rows): xn -> q / k / vT + RoPE (a dLLM-cache step writes keys /
// values into the slot), xn -> hbuf (SiLU·mul), att -> y and hbuf -> y (the caller adds its residual or its own target)
GemmArgs qkv_args(const mmada_handle* h, int layer, int m0, int rows);
GemmArgs gate_up_args(const mmada_handle* h, int layer, int m0, int rows);
GemmArgs attn_out_args(const mmada_handle* h, int layer, int m0, int rows);
GemmArgs down_args(const mmada_handle* h, int layer, int m0, int rows);
// the block's attention over this rank's heads, timed as kernel class 1: a cache step's queries against the slot, the row window
// [wbeg, wbeg + W) of each sequence (W > 0: the one-rank forward's last block), or every row.  [b0, b1) (b1 < 0: the whole batch):
// only these sequences, for the tensor-parallel forward's sequence chains — pointer offsets into q / k / vT / att and a launch
// over b1 - b0 sequences; a plain forward only (no cache slot, no window)
int block_attention(mmada_handle* h, int layer, hipStream_t s, int wbeg = 0, int W = 0, int b0 = 0, int b1 = -1);
// every block of a one-rank forward, after the embedding
int run_blocks(mmada_handle* h, void* stream);
// heads.hip: the (R, limit, col_begin, col_end) checks of a head entry point named `who` (R <= 0 is the caller's early return)
int check_head_range(const mmada_handle* h, const char* who, int R, int limit, int col_begin, int col_end);

// tp_comm.hip
int tp_forward_body(mmada_handle* h, hipStream_t s);              // all blocks of a tensor-parallel forward, after mmada_embed
int tp_gather_stream(mmada_handle* h, bf16_t* full_out, hipStream_t s);  // residual stream rows of every owner -> [M, d]
void tp_comm_free(mmada_handle* h);
bool tp_comm_connected(const mmada_handle* h);   // a transport (or the no-exchange diagnostic / the emulated link) is active on this handle
// nonzero (mm_fail) when a tensor-parallel forward over B sequences of Lp stream rows each (cached: through a dLLM-cache slot) must
// not start: the emulated link would wait beyond its cap
int tp_forward_refused(const mmada_handle* h, int B, int Lp, bool cached);
// this handle's forward is the tensor-parallel one (a connected one-rank group: the tp_allow_single_rank test switch)
inline bool runs_tensor_parallel(const mmada_handle* h) { return h->cfg.tp_size != 1 || tp_comm_connected(h); }
// tp_heads.hip
int tp_head_gather(mmada_handle* h, const int32_t* rows, int R, hipStream_t s);  // xg[r] = xn[row r] (xn already = ln_f(x))
// mmada_head_logprobs on a connected handle: the 256-column tiles split over the ranks, records exchanged, every rank joins
int tp_head_logprobs(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, const int64_t* targets,
                     float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s);
// mmada_head_topk / mmada_head_sample on a connected group of two or more ranks (pull or copy transport): the same exchange with
// the tiles' key records behind the 16-byte records; every rank ends with the bits of a one-rank handle on the same rows
int tp_head_topk(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, int k, int32_t* ids, float* logits,
                 float* lse, hipStream_t s);
int tp_head_sample(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, float temperature, uint64_t seed,
                   uint64_t* counter, int32_t* ids, float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s);
// out[r] = src[b * Lp + l] for rows[r] = b * L + l: the plain row gather behind tp_head_gather, on any [B * Lp, d] buffer
int tp_gather_rows(const bf16_t* src, const int32_t* rows, int R, int L, int Lp, int d, int nflat, bf16_t* out, hipStream_t s);

// (forward.hip and tp_comm.hip both time their launches, so the bodies stay here)
struct ProfScope {
    mmada_handle* h; hipStream_t s; bool on; hipEvent_t a{}, b{}; int kind; double flops;
    ProfScope(mmada_handle* h_, int layer, int kind_, double flops_, hipStream_t s_)
        : h(h_), s(s_), on(h_->prof_layer == layer), kind(kind_), flops(flops_) {
        // a stream under hipGraph capture records nothing: event timing only exists for eager launches
        if (on && stream_capturing(s)) on = false;
        if (!on) return;
        if (h->prof_pool.empty()) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
        } else {
            a = h->prof_pool.back().first; b = h->prof_pool.back().second;
            h->prof_pool.pop_back();
        }
        (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(b, s);
        h->prof.push_back({kind, a, b, flops});
    }
};

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int ceil_to(int v, int a) { return (v + a - 1) / a * a; }

struct Carve {
    size_t x, y, xn, att, h, q, k, vT, xg, rows, posmap, total;
    int Lp, Lkv, M;
};
Carve carve_for(const mmada_handle* h, int B, int L);  // forward.hip: the workspace layout of a (B, L) forward
