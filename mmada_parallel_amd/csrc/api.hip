// api.hip — the front door of the C-ABI of include/mmada_mi355x.h: error string, the handle's life cycle and weight repack, the
// workspace, the option switches and the stateless pass-throughs (GEMM, norm, probes, sampler).  The forward is forward.hip, the
// dLLM cache cache.hip, the LM head heads.hip.  Host code only; every kernel lives in gemm.hip / attention.hip / elementwise.hip /
// sampler.hip.
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/mmada_mi355x.h"
#include "handle.h"

static thread_local char g_err[1024] = "";

int mm_fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

// ---- the measurement / test switches of mmada_set_option: set from any thread, read by a launch once, through switches() ----
static struct {
    std::atomic<int> gemm_config{-2};        // -2: the environment's (MMADA_GEMM_CFG, else -1)
    std::atomic<int> gemm_silu_lut{-1};      // -1: the environment's (MMADA_GEMM_SILU_LUT=0: off, else on)
    std::atomic<int> gemm_short_tiles{-1};   // -1: the environment's (MMADA_GEMM_SHORT_TILES=0: off, else on)
    std::atomic<int> gemm_tile_order{-1};    // < 0: the environment's (MMADA_GEMM_TILE_ORDER, else 0)
    std::atomic<int> attention_form{-1};     // < 0: the environment's (MMADA_ATTN_FORM, else 1)
    std::atomic<int> probe_variant{0};
    std::atomic<int> tp_allow_single_rank{0};
    std::atomic<int> tp_emulate_mbps{0};     // 0: the environment's (MMADA_TP_EMULATE_MBPS >= 1, else 76000)
} g_switches;

static int env_int(const char* name, int fallback) {
    const char* e = getenv(name);
    return e ? atoi(e) : fallback;
}
static int env_flag(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0' ? 0 : 1;
}

Switches switches() {
    static const Switches env = {env_int("MMADA_GEMM_CFG", -1), env_flag("MMADA_GEMM_SILU_LUT"), env_flag("MMADA_GEMM_SHORT_TILES"),
                                 env_int("MMADA_GEMM_TILE_ORDER", 0), env_int("MMADA_ATTN_FORM", 1), 0, 0,
                                 env_int("MMADA_TP_EMULATE_MBPS", 0) >= 1 ? env_int("MMADA_TP_EMULATE_MBPS", 0) : 76000};
    const int cfg = g_switches.gemm_config, lut = g_switches.gemm_silu_lut, shrt = g_switches.gemm_short_tiles,
              order = g_switches.gemm_tile_order, form = g_switches.attention_form, mbps = g_switches.tp_emulate_mbps;
    return {cfg == -2 ? env.gemm_config : cfg, lut < 0 ? env.gemm_silu_lut : lut, shrt < 0 ? env.gemm_short_tiles : shrt,
            order < 0 ? env.gemm_tile_order : order, form < 0 ? env.attention_form : form, g_switches.probe_variant,
            g_switches.tp_allow_single_rank, mbps < 1 ? env.tp_emulate_mbps : mbps};
}

// the [text_start, text_start + T) span of the three mmada_text_select* calls lies inside the sequence
static int check_text_span(const char* who, int text_start, int T, int L) {
    if (text_start < 0 || text_start + T > L) return mm_fail("%s: text span outside the sequence", who);
    return 0;
}

extern "C" {

int mmada_abi_version(void) { return 1; }
const char* mmada_last_error(void) { return g_err; }

int mmada_create(const mmada_cfg* cfg, const float* inv_freq_host, mmada_handle** out) {
    if (!cfg || !out) return mm_fail("mmada_create: null argument");
    if (cfg->head_dim != 128) return mm_fail("mmada_create: head_dim must be 128 (got %d)", cfg->head_dim);
    if (cfg->d_model != cfg->n_heads * cfg->head_dim) return mm_fail("mmada_create: d_model != n_heads*head_dim");
    if (cfg->n_kv_heads <= 0 || cfg->n_heads % cfg->n_kv_heads) return mm_fail("mmada_create: bad n_kv_heads");
    if (cfg->tp_size < 1 || cfg->tp_rank < 0 || cfg->tp_rank >= cfg->tp_size) return mm_fail("mmada_create: bad tp rank/size");
    if (cfg->n_kv_heads % cfg->tp_size || cfg->n_heads % cfg->tp_size) return mm_fail("mmada_create: heads not divisible by tp_size");
    if (cfg->mlp_hidden % (64 * cfg->tp_size)) return mm_fail("mmada_create: mlp_hidden must be a multiple of 64*tp_size");
    if (cfg->d_model % 64) return mm_fail("mmada_create: d_model must be a multiple of 64");
    if (cfg->max_seq <= 0 || cfg->n_layers <= 0 || cfg->vocab <= 0) return mm_fail("mmada_create: bad sizes");
    if (gemm_prepare_device()) return 1;   // no launch of this handle ever allocates or synchronises (gemm.hip)
    mmada_handle* h = new mmada_handle();   // owned from here on: every failing exit goes through mmada_destroy
    h->cfg = *cfg;
    h->hq_l = cfg->n_heads / cfg->tp_size;
    h->hkv_l = cfg->n_kv_heads / cfg->tp_size;
    h->f_l = cfg->mlp_hidden / cfg->tp_size;
    h->layers.resize(cfg->n_layers);
    // RoPE tables (model/modeling_llada.py:391-397)
    float inv[64];
    for (int i = 0; i < 64; ++i)
        inv[i] = inv_freq_host ? inv_freq_host[i] : (float)(1.0 / pow((double)cfg->rope_theta, (double)(2 * i) / 128.0));
    float* inv_dev = nullptr;
    auto fill_tables = [&]() -> int {
        MM_CHECK_HIP(hipMalloc(&inv_dev, sizeof(inv)));
        MM_CHECK_HIP(hipMemcpy(inv_dev, inv, sizeof(inv), hipMemcpyHostToDevice));
        MM_CHECK_HIP(hipMalloc(&h->rope_cos, (size_t)cfg->max_seq * 64 * 4));
        MM_CHECK_HIP(hipMalloc(&h->rope_sin, (size_t)cfg->max_seq * 64 * 4));
        if (launch_rope_table(h->rope_cos, h->rope_sin, inv_dev, cfg->max_seq, 0)) return 1;
        MM_CHECK_HIP(hipDeviceSynchronize());
        return 0;
    };
    const int rc = fill_tables();
    (void)hipFree(inv_dev);
    if (rc) {
        mmada_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

int mmada_clone_shared(mmada_handle* h, mmada_handle** out) {
    if (!h || !out) return mm_fail("mmada_clone_shared: null argument");
    mmada_handle* c = new mmada_handle();
    c->cfg = h->cfg;
    c->hq_l = h->hq_l; c->hkv_l = h->hkv_l; c->f_l = h->f_l;
    c->rope_cos = h->rope_cos; c->rope_sin = h->rope_sin;
    c->wte = h->wte; c->ln_f = h->ln_f; c->lm_head = h->lm_head;
    c->layers = h->layers;  // pointer copies
    c->owns_weights = false;
    *out = c;
    return 0;
}

int mmada_destroy(mmada_handle* h) {
    if (!h) return 0;
    for (auto& r : h->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto& e : h->prof_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    tp_comm_free(h);
    (void)hipFree(h->score_buf);   // a clone grows its own record buffer (mmada_head_logprobs)
    if (!h->owns_weights) { delete h; return 0; }
    for (auto& lw : h->layers) {
        (void)hipFree(lw.wqkv); (void)hipFree(lw.wo); (void)hipFree(lw.wgu);
        (void)hipFree(lw.wdown); (void)hipFree(lw.attn_norm); (void)hipFree(lw.ff_norm);
    }
    (void)hipFree(h->rope_cos);
    (void)hipFree(h->rope_sin);
    delete h;
    return 0;
}

int mmada_bind_globals(mmada_handle* h, const void* wte, const void* ln_f, const void* lm_head) {
    if (!h || !wte || !ln_f || !lm_head) return mm_fail("mmada_bind_globals: null argument");
    h->wte = (const bf16_t*)wte;
    h->ln_f = (const bf16_t*)ln_f;
    h->lm_head = (const bf16_t*)lm_head;
    return 0;
}

int mmada_bind_layer(mmada_handle* h, int layer, const void* attn_norm, const void* ff_norm, const void* q_proj,
                     const void* k_proj, const void* v_proj, const void* attn_out, const void* ff_proj,
                     const void* up_proj, const void* ff_out, void* stream) {
    if (!h) return mm_fail("mmada_bind_layer: null handle");
    if (!h->owns_weights) return mm_fail("mmada_bind_layer: handle is a shared clone");
    if (layer < 0 || layer >= h->cfg.n_layers) return mm_fail("mmada_bind_layer: layer %d out of range", layer);
    if (!attn_norm || !ff_norm || !q_proj || !k_proj || !v_proj || !attn_out || !ff_proj || !up_proj || !ff_out)
        return mm_fail("mmada_bind_layer: null weight pointer");
    hipStream_t s = (hipStream_t)stream;
    const mmada_cfg& c = h->cfg;
    const int d = c.d_model;
    LayerWeights& lw = h->layers[layer];
    const size_t nqkv = (size_t)(h->hq_l + 2 * h->hkv_l) * 128;
    if (!lw.wqkv) {
        MM_CHECK_HIP(hipMalloc(&lw.wqkv, nqkv * d * 2));
        MM_CHECK_HIP(hipMalloc(&lw.wo, (size_t)d * h->hq_l * 128 * 2));
        MM_CHECK_HIP(hipMalloc(&lw.wgu, (size_t)2 * h->f_l * d * 2));
        MM_CHECK_HIP(hipMalloc(&lw.wdown, (size_t)d * h->f_l * 2));
        MM_CHECK_HIP(hipMalloc(&lw.attn_norm, (size_t)d * 2));
        MM_CHECK_HIP(hipMalloc(&lw.ff_norm, (size_t)d * 2));
    }
    if (launch_pack_qkv((const bf16_t*)q_proj, (const bf16_t*)k_proj, (const bf16_t*)v_proj, lw.wqkv, d, c.n_heads,
                        c.n_kv_heads, c.tp_rank, c.tp_size, s)) return 1;
    if (launch_pack_cols((const bf16_t*)attn_out, lw.wo, d, c.n_heads * 128, c.tp_rank, c.tp_size, s)) return 1;
    if (launch_pack_gate_up((const bf16_t*)ff_proj, (const bf16_t*)up_proj, lw.wgu, d, c.mlp_hidden, c.tp_rank,
                            c.tp_size, s)) return 1;
    if (launch_pack_cols((const bf16_t*)ff_out, lw.wdown, d, c.mlp_hidden, c.tp_rank, c.tp_size, s)) return 1;
    MM_CHECK_HIP(hipMemcpyAsync(lw.attn_norm, attn_norm, (size_t)d * 2, hipMemcpyDeviceToDevice, s));
    MM_CHECK_HIP(hipMemcpyAsync(lw.ff_norm, ff_norm, (size_t)d * 2, hipMemcpyDeviceToDevice, s));
    lw.bound = true;
    return 0;
}

size_t mmada_workspace_bytes(const mmada_handle* h, int B, int L) {
    if (!h || B <= 0 || L <= 0) return 0;
    return carve_for(h, B, L).total;
}

int mmada_set_workspace(mmada_handle* h, void* ws, size_t bytes) {
    if (!h || !ws) return mm_fail("mmada_set_workspace: null argument");
    if (((uintptr_t)ws) & 255) return mm_fail("mmada_set_workspace: workspace must be 256-byte aligned");
    h->ws = (char*)ws;
    h->ws_bytes = bytes;
    h->res.B = h->res.L = 0;
    return 0;
}

int mmada_set_option(const char* name, int value) {
    if (!name) return mm_fail("mmada_set_option: null name");
    static const struct { const char* name; std::atomic<int>* field; bool flag; int least; } table[] = {   // least: smallest value taken
        {"gemm_config", &g_switches.gemm_config, false, INT_MIN},
        {"gemm_silu_lut", &g_switches.gemm_silu_lut, true, INT_MIN},
        {"gemm_short_tiles", &g_switches.gemm_short_tiles, true, INT_MIN},
        {"gemm_tile_order", &g_switches.gemm_tile_order, false, INT_MIN},
        {"attention_form", &g_switches.attention_form, false, INT_MIN},
        {"probe_variant", &g_switches.probe_variant, false, INT_MIN},
        {"tp_allow_single_rank", &g_switches.tp_allow_single_rank, true, INT_MIN},
        {"tp_emulate_mbps", &g_switches.tp_emulate_mbps, false, 1},
    };
    for (const auto& o : table)
        if (!strcmp(name, o.name)) {
            if (value < o.least) return mm_fail("mmada_set_option: '%s' must be an integer >= %d (got %d)", name, o.least, value);
            o.field->store(o.flag ? value != 0 : value);   // flag: nonzero -> 1
            return 0;
        }
    return mm_fail("mmada_set_option: unknown option '%s'", name);
}

int mmada_gemm_swiglu_bt(const void* A, const void* W, void* C, int M, int N, int K, void* stream) {
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0 || N % 64) return mm_fail("mmada_gemm_swiglu_bt: bad argument");
    return launch_gemm(EPI_SWIGLU, gemm_bt_args((const bf16_t*)A, (const bf16_t*)W, (bf16_t*)C, M, N, K, N / 2), (hipStream_t)stream);
}

// The launcher itself on caller data (tests): the three epilogues of the block's plain projections with what forward.hip sets for them.
int mmada_probe_gemm(mmada_gemm_probe* p, void* stream) {
    if (!p) return mm_fail("mmada_probe_gemm: null argument");
    p->ran = -1;
    if (!p->A || !p->W || !p->C) return mm_fail("mmada_probe_gemm: null operand");
    if (p->epi < EPI_STORE || p->epi > EPI_SWIGLU) return mm_fail("mmada_probe_gemm: epi=%d is not 0 (store), 1 (resid) or 2 (swiglu)", p->epi);
    if (p->epi == EPI_RESID && !p->resid) return mm_fail("mmada_probe_gemm: the residual epilogue needs resid");
    if (p->resid_mod < 1 || p->resid_rank < 0 || p->resid_rank >= p->resid_mod)
        return mm_fail("mmada_probe_gemm: resid_mod=%d must be >= 1 and resid_rank=%d inside [0, resid_mod)", p->resid_mod, p->resid_rank);
    if (p->rwin < 0) return mm_fail("mmada_probe_gemm: rwin=%d is negative", p->rwin);
    if (p->rwin > 0 && p->M % p->rwin != 0) return mm_fail("mmada_probe_gemm: M=%d is not a multiple of rwin=%d", p->M, p->rwin);
    if (p->rwin > 0 && (p->rbeg < 0 || p->rbeg + p->rwin > p->rlp))
        return mm_fail("mmada_probe_gemm: rows [%d, %d) lie outside a sequence of rlp=%d rows", p->rbeg, p->rbeg + p->rwin, p->rlp);
    if (p->epi == EPI_SWIGLU && p->N % 64 != 0) return mm_fail("mmada_probe_gemm: SwiGLU needs N=%d to be a multiple of 64", p->N);
    const int ncol = p->epi == EPI_SWIGLU ? p->N / 2 : p->N;
    if (p->ldc < ncol || (p->epi == EPI_RESID && p->ldr < ncol))
        return mm_fail("mmada_probe_gemm: ldc=%d (ldr=%d) is shorter than a row of %d columns", p->ldc, p->ldr, ncol);
    GemmArgs g = gemm_bt_args((const bf16_t*)p->A, (const bf16_t*)p->W, (bf16_t*)p->C, p->M, p->N, p->K, p->ldc);
    if (p->epi == EPI_RESID) {   // (forward.hip: add_residual and the consumed-row window)
        g.resid = (const bf16_t*)p->resid; g.ldr = p->ldr; g.resid_mod = p->resid_mod; g.resid_rank = p->resid_rank;
        g.rwin = p->rwin; g.rlp = p->rlp; g.rbeg = p->rbeg;
    }
    g.publish = p->publish;
    int ran = -1;
    const int rc = launch_gemm(p->epi, g, (hipStream_t)stream, &ran);
    p->ran = ran;
    return rc;
}

int mmada_gemm_plan(int M, int N, int K) { return gemm_plan_code(M, N, K); }
int mmada_attention_plan(int pairs, int groups, int keys) {
    if (pairs <= 0 || groups <= 0 || keys <= 0) return mm_fail("mmada_attention_plan: bad argument"), -1;
    return attention_chunks(pairs, groups, keys);
}

int mmada_probe_f2bf(const float* in, uint16_t* out, int64_t n, void* stream) {
    if (!in || !out || n < 0) return mm_fail("mmada_probe_f2bf: bad argument");
    return launch_f2bf_probe(in, out, (long long)n, (hipStream_t)stream);
}

size_t mmada_mfma_probe_bytes(void) { return (size_t)64 * 8 * 16 * 64 * 16; }

int mmada_mfma_probe(const void* data, void* sink, int iters, int launches, void* stream, double* tflops_out, double* ms_out) {
    if (!data || !sink || iters <= 0 || launches <= 0) return mm_fail("mmada_mfma_probe: bad argument");
    return launch_mfma_probe((const bf16_t*)data, (float*)sink, iters, launches, (hipStream_t)stream, tflops_out, ms_out);
}

// The records of sampler.hip's launchers (kernels.h: what each field means) from what every entry point of a kernel passes; the
// entry points set the fields of their variant by name.
static TextStatsArgs text_stats_args(TextMode mode, const mmada_handle* h, const void* logits, int B, int T, int V, int ld, int64_t* ids,
                                     int L, int text_start) {
    TextStatsArgs a{};
    a.mode = mode;
    a.logits = (const bf16_t*)logits;
    a.B = B; a.T = T; a.V = V; a.ld = ld;
    a.ids = ids; a.L = L; a.text_start = text_start; a.mask_id = h->cfg.mask_token_id;
    return a;
}
static ImageRowArgs image_row_args(ImageCombine combine, const void* cond, const void* ut, const void* ui, int B, int N, int CB,
                                   float cfg_scale, float cfg_img, int32_t* argmax_out, void* pmax_out) {
    ImageRowArgs a{};
    a.combine = combine;
    a.cond = (const bf16_t*)cond; a.ut = (const bf16_t*)ut; a.ui = (const bf16_t*)ui;
    a.B = B; a.N = N; a.CB = CB;
    a.cfg_scale = cfg_scale; a.cfg_img = cfg_img;
    a.argmax_out = argmax_out; a.pmax_out = (bf16_t*)pmax_out;
    return a;
}
static void image_row_draw(ImageRowArgs& a, ImageDraw draw, int col0, uint64_t seed, const uint64_t* counter, int32_t* sampled_out,
                           void* p_sel_out) {
    a.draw = draw;
    a.col0 = col0; a.seed = seed; a.counter = counter;
    a.sampled_out = sampled_out; a.p_sel_out = (bf16_t*)p_sel_out;
}
static ImageCommitArgs image_commit_args(CommitRule rule, const mmada_handle* h, int64_t* ids, int B, int L, const int32_t* pos_map, int N,
                                         const int32_t* sampled_in, const void* p_in, const int32_t* mask_len_sched, int text_vocab,
                                         int codebook) {
    ImageCommitArgs a{};
    a.rule = rule;
    a.ids = ids; a.B = B; a.L = L; a.pos_map = pos_map; a.N = N;
    a.sampled_in = sampled_in; a.p_in = (const bf16_t*)p_in;
    a.mask_len_sched = mask_len_sched; a.mask_id = h->cfg.mask_token_id; a.text_vocab = text_vocab; a.codebook = codebook;
    return a;
}
static void image_commit_device_noise(ImageCommitArgs& a, uint64_t seed, uint64_t* counter) {
    a.noise_from = COMMIT_NOISE_DEVICE;
    a.seed = seed; a.counter = counter;
}

int mmada_text_select(mmada_handle* h, const void* logits, const void* noisy, int B, int T, int V, int ld_logits,
                      int64_t* ids, int L, int text_start, const int32_t* k, void* scratch, void* stream) {
    if (!h || !logits || !ids || !k || !scratch) return mm_fail("mmada_text_select: null argument");
    if (check_text_span("mmada_text_select", text_start, T, L)) return 1;
    TextStatsArgs a = text_stats_args(TEXT_PLAIN, h, logits, B, T, V, ld_logits, ids, L, text_start);
    a.noisy = (const bf16_t*)noisy;
    return launch_text_select(a, k, scratch, nullptr, (hipStream_t)stream);
}

int mmada_text_select_random(mmada_handle* h, const void* logits, const void* noisy, const float* uniform, int B, int T,
                             int V, int ld_logits, int64_t* ids, int L, int text_start, const int32_t* k, void* scratch,
                             void* stream) {
    if (!h || !logits || !uniform || !ids || !k || !scratch) return mm_fail("mmada_text_select_random: null argument");
    if (check_text_span("mmada_text_select_random", text_start, T, L)) return 1;
    TextStatsArgs a = text_stats_args(TEXT_PLAIN, h, logits, B, T, V, ld_logits, ids, L, text_start);
    a.noisy = (const bf16_t*)noisy;
    return launch_text_select(a, k, scratch, uniform, (hipStream_t)stream);
}

int mmada_text_select_cfg(mmada_handle* h, const void* cond, const void* uncond, float text_cfg, const int32_t* x0_in,
                          int B, int T, int V, int ld_logits, int64_t* ids, int L, int text_start, const int32_t* k,
                          void* scratch, void* stream) {
    if (!h || !cond || !uncond || !ids || !k || !scratch) return mm_fail("mmada_text_select_cfg: null argument");
    if (check_text_span("mmada_text_select_cfg", text_start, T, L)) return 1;
    TextStatsArgs a = text_stats_args(TEXT_CFG, h, cond, B, T, V, ld_logits, ids, L, text_start);
    a.unc = (const bf16_t*)uncond; a.text_cfg = text_cfg; a.x0_in = x0_in;
    return launch_text_select(a, k, scratch, nullptr, (hipStream_t)stream);
}

int mmada_image_probs_m(mmada_handle* h, const void* cond, const void* uncond, int B, int N, int CB, float image_cfg,
                        void* probs_out, int32_t* argmax_out, void* pmax_out, void* stream) {
    if (!h || !cond || !uncond || !argmax_out || !pmax_out) return mm_fail("mmada_image_probs_m: null argument");
    const float one_plus = (float)(1.0 + (double)image_cfg);
    ImageRowArgs a = image_row_args(IMAGE_COMBINE_M, cond, uncond, nullptr, B, N, CB, image_cfg, one_plus, argmax_out, pmax_out);
    a.probs_out = (bf16_t*)probs_out;
    return launch_image_row(a, (hipStream_t)stream);
}

int mmada_image_commit_m(mmada_handle* h, int64_t* ids, int B, int L, const int32_t* pos_map, int N,
                         const int32_t* sampled_in, const void* p_in, const void* gumbel, float remask_temp,
                         const int32_t* mask_len_sched, int text_vocab_size, void* stream) {
    if (!h || !ids || !pos_map || !sampled_in || !p_in || !gumbel || !mask_len_sched)
        return mm_fail("mmada_image_commit_m: null argument");
    ImageCommitArgs a = image_commit_args(COMMIT_RULE_M, h, ids, B, L, pos_map, N, sampled_in, p_in, mask_len_sched, text_vocab_size, 0);
    a.noise = (const bf16_t*)gumbel; a.temp_value = remask_temp;
    return launch_image_commit(a, (hipStream_t)stream);
}

int mmada_image_commit_g(mmada_handle* h, int64_t* ids, int B, int L, const int32_t* pos_map, int N,
                         const int32_t* sampled_in, const void* p_in, const void* gumbel, float remask_temp,
                         const int32_t* keep_n, int text_vocab_size, void* stream) {
    if (!h || !ids || !pos_map || !sampled_in || !p_in || !gumbel || !keep_n)
        return mm_fail("mmada_image_commit_g: null argument");
    ImageCommitArgs a = image_commit_args(COMMIT_RULE_M_KEEP, h, ids, B, L, pos_map, N, sampled_in, p_in, keep_n, text_vocab_size, 0);
    a.noise = (const bf16_t*)gumbel; a.temp_value = remask_temp;
    return launch_image_commit(a, (hipStream_t)stream);
}

int mmada_image_probs(mmada_handle* h, const void* cond, const void* unc_text, const void* unc_img, int B, int N, int CB,
                      float cfg_scale, float cfg_img, void* probs_out, int32_t* argmax_out, void* pmax_out,
                      void* stream) {
    if (!h || !cond || !argmax_out || !pmax_out) return mm_fail("mmada_image_probs: null argument");
    ImageRowArgs a = image_row_args(IMAGE_COMBINE_A, cond, unc_text, unc_img, B, N, CB, cfg_scale, cfg_img, argmax_out, pmax_out);
    a.probs_out = (bf16_t*)probs_out;
    return launch_image_row(a, (hipStream_t)stream);
}

int mmada_image_commit(mmada_handle* h, int64_t* ids, int B, int L, const int32_t* pos_map, int N,
                       const int32_t* sampled_in, const void* p_in, const void* noise, float remask_temp,
                       const int32_t* mask_len_sched, int text_vocab_size, int codebook_size, void* stream) {
    if (!h || !ids || !pos_map || !sampled_in || !p_in || !mask_len_sched) return mm_fail("mmada_image_commit: null argument");
    ImageCommitArgs a = image_commit_args(COMMIT_RULE_A, h, ids, B, L, pos_map, N, sampled_in, p_in, mask_len_sched, text_vocab_size,
                                          codebook_size);
    a.noise = (const bf16_t*)noise; a.temp_value = remask_temp;
    return launch_image_commit(a, (hipStream_t)stream);
}

int mmada_image_sample(mmada_handle* h, const void* cond, const void* unc_text, const void* unc_img, int B, int N, int CB,
                       float cfg_scale, float cfg_img, int col0, uint64_t seed, const uint64_t* counter, int32_t* sampled_out,
                       void* p_sel_out, int32_t* argmax_out, void* pmax_out, void* stream) {
    if (!h || !cond || !counter || !sampled_out || !p_sel_out) return mm_fail("mmada_image_sample: null argument");
    ImageRowArgs a = image_row_args(IMAGE_COMBINE_A, cond, unc_text, unc_img, B, N, CB, cfg_scale, cfg_img, argmax_out, pmax_out);
    image_row_draw(a, IMAGE_DRAW_UNIT, col0, seed, counter, sampled_out, p_sel_out);
    return launch_image_row(a, (hipStream_t)stream);
}

int mmada_image_sample_m(mmada_handle* h, const void* cond, const void* uncond, int B, int N, int CB, float image_cfg, int col0,
                         uint64_t seed, const uint64_t* counter, int32_t* sampled_out, void* p_sel_out, int32_t* argmax_out,
                         void* pmax_out, void* stream) {
    if (!h || !cond || !uncond || !counter || !sampled_out || !p_sel_out) return mm_fail("mmada_image_sample_m: null argument");
    const float one_plus = (float)(1.0 + (double)image_cfg);  // as mmada_image_probs_m
    ImageRowArgs a = image_row_args(IMAGE_COMBINE_M, cond, uncond, nullptr, B, N, CB, image_cfg, one_plus, argmax_out, pmax_out);
    image_row_draw(a, IMAGE_DRAW_UNIT, col0, seed, counter, sampled_out, p_sel_out);
    return launch_image_row(a, (hipStream_t)stream);
}

int mmada_image_commit_m_sampled(mmada_handle* h, int64_t* ids, int B, int L, const int32_t* pos_map, int N,
                                 const int32_t* sampled_in, const void* p_in, const float* remask_temp, uint64_t seed,
                                 uint64_t* counter, const int32_t* mask_len_sched, int text_vocab_size, int32_t* sampled_out,
                                 void* stream) {
    if (!h || !ids || !pos_map || !sampled_in || !p_in || !remask_temp || !counter || !mask_len_sched)
        return mm_fail("mmada_image_commit_m_sampled: null argument");
    ImageCommitArgs a = image_commit_args(COMMIT_RULE_M, h, ids, B, L, pos_map, N, sampled_in, p_in, mask_len_sched, text_vocab_size, 0);
    image_commit_device_noise(a, seed, counter);
    a.temp_dev = remask_temp; a.sampled_out = sampled_out;
    return launch_image_commit(a, (hipStream_t)stream);
}

int mmada_image_sample_g(mmada_handle* h, const void* cond, const void* uncond, int B, int N, int CB, float cfg_scale,
                         float temperature, int col0, uint64_t seed, const uint64_t* counter, int32_t* sampled_out, void* p_sel_out,
                         int32_t* argmax_out, void* pmax_out, void* stream) {
    if (!h || !cond || !uncond || !counter || !sampled_out || !p_sel_out) return mm_fail("mmada_image_sample_g: null argument");
    if (!(temperature >= 0.f) || __builtin_isinf(temperature))
        return mm_fail("mmada_image_sample_g: temperature %g is not a finite value >= 0", (double)temperature);
    const float one_plus = (float)(1.0 + (double)cfg_scale);  // as mmada_image_probs_m
    ImageRowArgs a = image_row_args(IMAGE_COMBINE_M, cond, uncond, nullptr, B, N, CB, cfg_scale, one_plus, argmax_out, pmax_out);
    image_row_draw(a, IMAGE_DRAW_TEMPERATURE, col0, seed, counter, sampled_out, p_sel_out);
    a.temperature = temperature;
    return launch_image_row(a, (hipStream_t)stream);
}

int mmada_image_commit_g_sampled(mmada_handle* h, int64_t* ids, int B, int L, const int32_t* pos_map, int N,
                                 const int32_t* sampled_in, const void* p_in, float remask_temp, uint64_t seed, uint64_t* counter,
                                 const int32_t* keep_n, int text_vocab_size, void* stream) {
    if (!h || !ids || !pos_map || !sampled_in || !p_in || !counter || !keep_n)
        return mm_fail("mmada_image_commit_g_sampled: null argument");
    ImageCommitArgs a = image_commit_args(COMMIT_RULE_M_KEEP, h, ids, B, L, pos_map, N, sampled_in, p_in, keep_n, text_vocab_size, 0);
    image_commit_device_noise(a, seed, counter);
    a.temp_value = remask_temp;  // a constant of the run: by value
    return launch_image_commit(a, (hipStream_t)stream);
}

int mmada_text_draw_cfg(mmada_handle* h, const void* cond, const void* uncond, float text_cfg, int B, int T, int V, int ld_logits,
                        float temperature, uint64_t seed, uint64_t* counter, int32_t* x0_out, void* stream) {
    if (!h || !cond || !uncond || !counter || !x0_out) return mm_fail("mmada_text_draw_cfg: null argument");
    if (!(temperature >= 0.f) || __builtin_isinf(temperature))
        return mm_fail("mmada_text_draw_cfg: temperature %g is not a finite value >= 0", (double)temperature);
    return launch_text_draw_cfg((const bf16_t*)cond, (const bf16_t*)uncond, text_cfg, B, T, V, ld_logits, temperature, seed, counter,
                                x0_out, (hipStream_t)stream);
}

int mmada_image_commit_sampled(mmada_handle* h, int64_t* ids, int B, int L, const int32_t* pos_map, int N,
                               const int32_t* sampled_in, const void* p_in, const float* remask_temp, uint64_t seed,
                               uint64_t* counter, const int32_t* mask_len_sched, int text_vocab_size, int codebook_size,
                               void* stream) {
    if (!h || !ids || !pos_map || !sampled_in || !p_in || !remask_temp || !counter || !mask_len_sched)
        return mm_fail("mmada_image_commit_sampled: null argument");
    ImageCommitArgs a = image_commit_args(COMMIT_RULE_A, h, ids, B, L, pos_map, N, sampled_in, p_in, mask_len_sched, text_vocab_size,
                                          codebook_size);
    image_commit_device_noise(a, seed, counter);
    a.temp_dev = remask_temp;
    return launch_image_commit(a, (hipStream_t)stream);
}

int mmada_lfq_gather(mmada_handle* h, const int64_t* idx, int B, int N, int nbits, int dtype_f32, void* out,
                     void* stream) {
    (void)h;
    if (!idx || !out) return mm_fail("mmada_lfq_gather: null argument");
    if (nbits <= 0 || nbits > 62) return mm_fail("mmada_lfq_gather: bad nbits");
    return launch_lfq_gather(idx, out, B, N, nbits, dtype_f32, (hipStream_t)stream);
}

int mmada_gemm_bt(const void* A, const void* W, void* C, int M, int N, int K, void* stream) {
    if (!A || !W || !C) return mm_fail("mmada_gemm_bt: null argument");
    return launch_gemm(EPI_STORE, gemm_bt_args((const bf16_t*)A, (const bf16_t*)W, (bf16_t*)C, M, N, K, N), (hipStream_t)stream);
}

int mmada_rmsnorm(const void* x, const void* w, void* out, int rows, int d, float eps, void* stream) {
    if (!x || !w || !out) return mm_fail("mmada_rmsnorm: null argument");
    return launch_rmsnorm((const bf16_t*)x, (const bf16_t*)w, (bf16_t*)out, rows, d, eps, (hipStream_t)stream);
}

}  // extern "C"
