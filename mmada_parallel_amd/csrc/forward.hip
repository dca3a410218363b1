// forward.hip — workspace carving, the resident-forward record and the launch sequence of one denoiser forward (embedding →
// n_layers × [RMSNorm → QKV+RoPE GEMM → flash attention → attn_out GEMM + residual → RMSNorm → gate/up GEMM + SiLU·mul → down
// GEMM + residual]), its parity taps and live timing.  The LM-head rows are heads.hip, the dLLM cache is cache.hip.
// Host code only; every kernel lives in gemm.hip / attention.hip / elementwise.hip / sampler.hip.
#include <algorithm>
#include <utility>

#include "../../include/mmada_mi355x.h"
#include "handle.h"

Carve carve_for(const mmada_handle* h, int B, int L) {
    Carve c;
    const int d = h->cfg.d_model;
    c.Lp = ceil_to(L, 8);
    c.Lkv = ceil_to(L, 64);
    c.M = B * c.Lp;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    // tensor parallel: a row chunk is split into tp equal owner slices of a multiple of 8 rows; the last chunk's slices
    // may reach past M (equal counts for the RCCL reduce-scatter / all-gather), so the stream buffers carry pad rows
    const size_t mrows = (size_t)c.M + (h->cfg.tp_size > 1 ? 8 * h->cfg.tp_size : 0);
    c.x = take(mrows * d * 2);
    c.y = take(mrows * d * 2);
    c.xn = take(mrows * d * 2);
    c.att = take((size_t)c.M * h->hq_l * 128 * 2);
    c.h = take((size_t)c.M * h->f_l * 2);
    c.q = take((size_t)B * h->hq_l * c.Lkv * 128 * 2);
    c.k = take((size_t)B * h->hkv_l * c.Lkv * 128 * 2);
    c.vT = take((size_t)B * h->hkv_l * 128 * c.Lkv * 2);
    c.xg = take(((size_t)B * L + 8) * d * 2);   // + 8: the scoring head multiplies ceil8(R) rows (pad rows: any content)
    c.rows = take((size_t)B * L * 4);
    c.posmap = take((size_t)c.M * 4);
    c.total = off;
    return c;
}

static int apply_carve(mmada_handle* h, int B, int L, hipStream_t s) {
    if (B <= 0 || L <= 0) return mm_fail("forward: bad shape B=%d L=%d", B, L);
    if (L > h->cfg.max_seq) return mm_fail("forward: L=%d exceeds max_seq=%d", L, h->cfg.max_seq);
    const Carve c = carve_for(h, B, L);
    if (!h->ws || c.total > h->ws_bytes)
        return mm_fail("forward: workspace too small (%zu needed, %zu set)", c.total, h->ws_bytes);
    Resident& r = h->res;
    r.B = B; r.L = L; r.Lp = c.Lp; r.Lkv = c.Lkv; r.M = c.M;
    h->x = (bf16_t*)(h->ws + c.x); h->y = (bf16_t*)(h->ws + c.y); h->xn = (bf16_t*)(h->ws + c.xn);
    h->att = (bf16_t*)(h->ws + c.att); h->hbuf = (bf16_t*)(h->ws + c.h); h->q = (bf16_t*)(h->ws + c.q);
    h->k = (bf16_t*)(h->ws + c.k); h->vT = (bf16_t*)(h->ws + c.vT); h->xg = (bf16_t*)(h->ws + c.xg);
    h->rows_all = (int32_t*)(h->ws + c.rows);
    h->posmap = (int32_t*)(h->ws + c.posmap);
    // vT columns never written by the QKV epilogue (keys >= Lp; the key order inside a 32-key block is permuted, so
    // start at the last block boundary) are multiplied by P == 0: keep them finite
    const int z0 = c.Lp & ~31;
    if (c.Lkv > z0)
        MM_CHECK_HIP(hipMemset2DAsync(h->vT + z0, (size_t)c.Lkv * 2, 0, (size_t)(c.Lkv - z0) * 2,
                                      (size_t)B * h->hkv_l * 128, s));
    return 0;
}

static int check_bound(const mmada_handle* h) {
    if (!h->wte) return mm_fail("forward: mmada_bind_globals was not called");
    for (int i = 0; i < h->cfg.n_layers; ++i)
        if (!h->layers[i].bound) return mm_fail("forward: layer %d not bound", i);
    return 0;
}

int begin_forward(mmada_handle* h, int B, int L, hipStream_t s) {
    if (check_bound(h) || apply_carve(h, B, L, s)) return 1;
    Resident& r = h->res;
    r.cur_W = 0; r.cur_beg = 0; r.Mcur = r.M;
    r.xn_is_final = false;
    r.xn_is_layer0 = true;
    return 0;
}

CacheStep::CacheStep(mmada_handle* h_, const CacheSlot* slot, const int32_t* pos, int qshift) : h(h_) {
    h->res.cc = slot; h->res.cc_pos = pos; h->res.cc_qshift = qshift;
}
CacheStep::~CacheStep() {
    h->res.cc = nullptr; h->res.cc_pos = nullptr; h->res.cc_qshift = -1;
    invalidate(h);  // mmada_head_rows / mmada_read_stream must not read the compact stream
}

// ---- one block's launches, shared by this file's forward (m0 = 0, every row) and the tensor-parallel forward (tp_comm.hip, one
// call per row chunk); each caller adds its own output side (residual and row window here, the partial-sum target there) ----
GemmArgs qkv_args(const mmada_handle* h, int layer, int m0, int rows) {
    const int d = h->cfg.d_model;
    const Resident& r = h->res;
    GemmArgs g = gemm_bt_args(h->xn + (size_t)m0 * d, h->layers[layer].wqkv, nullptr, rows, (h->hq_l + 2 * h->hkv_l) * 128, d, 0);
    g.m_base = m0;
    g.q = h->q; g.k = h->k; g.vT = h->vT; g.rope_cos = h->rope_cos; g.rope_sin = h->rope_sin;
    g.Lp = r.Lp; g.Lkv = r.Lkv; g.Hq = h->hq_l; g.Hkv = h->hkv_l;
    if (const CacheSlot* cc = r.cc) {  // dLLM cache step: this block's keys / values live in (and are written to) the slot
        g.k = cc->K(layer); g.vT = cc->vT(layer); g.Lkv = cc->Lkv;
        g.pos_map = r.cc_pos; g.Lq = r.Lkv; g.q_pos_shift = r.cc_qshift;
    }
    return g;
}

GemmArgs gate_up_args(const mmada_handle* h, int layer, int m0, int rows) {
    const int d = h->cfg.d_model;
    return gemm_bt_args(h->xn + (size_t)m0 * d, h->layers[layer].wgu, h->hbuf + (size_t)m0 * h->f_l, rows, 2 * h->f_l, d, h->f_l);
}

GemmArgs attn_out_args(const mmada_handle* h, int layer, int m0, int rows) {
    const int d = h->cfg.d_model, K = h->hq_l * 128;
    return gemm_bt_args(h->att + (size_t)m0 * K, h->layers[layer].wo, h->y + (size_t)m0 * d, rows, d, K, d);
}

GemmArgs down_args(const mmada_handle* h, int layer, int m0, int rows) {
    const int d = h->cfg.d_model;
    return gemm_bt_args(h->hbuf + (size_t)m0 * h->f_l, h->layers[layer].wdown, h->y + (size_t)m0 * d, rows, d, h->f_l, d);
}

int block_attention(mmada_handle* h, int layer, hipStream_t s, int wbeg, int W, int b0, int b1) {
    const Resident& r = h->res;
    const CacheSlot* cc = r.cc;
    if (b1 < 0) b1 = r.B;
    if (b0 < 0 || b0 >= b1 || b1 > r.B) return mm_fail("forward: attention over sequences [%d,%d) of a batch of %d", b0, b1, r.B);
    const int nb = b1 - b0;
    if (nb != r.B && (cc || W)) return mm_fail("forward: a sequence range of the attention needs a plain forward (no cache slot, no row window)");
    const double rows = W ? (double)nb * W : (double)nb * r.L;
    ProfScope p(h, layer, 1, 4.0 * h->hq_l * rows * (cc ? cc->L : r.L) * 128.0, s);
    if (cc)  // compact (or all) queries of this call against the slot's keys / values of the whole sequence
        return launch_attention(h->q, cc->K(layer), cc->vT(layer), h->att, r.B, h->hq_l, h->hkv_l, cc->L, r.Lp, cc->Lkv, r.Lp,
                                h->hq_l * 128, s, 0, r.Lkv);
    if (W)
        return launch_attention(h->q, h->k, h->vT, h->att, r.B, h->hq_l, h->hkv_l, r.L, wbeg + W, r.Lkv, W, h->hq_l * 128, s,
                                wbeg);
    // sequences [b0, b1): the same launch on a batch of nb whose first sequence is b0 (q / k / vT are [B, heads, ...], att is [B * Lp, ...])
    const size_t per_q = (size_t)h->hq_l * r.Lkv * 128, per_kv = (size_t)h->hkv_l * r.Lkv * 128;
    return launch_attention(h->q + b0 * per_q, h->k + b0 * per_kv, h->vT + b0 * per_kv, h->att + (size_t)b0 * r.Lp * h->hq_l * 128, nb,
                            h->hq_l, h->hkv_l, r.L, r.Lp, r.Lkv, r.Lp, h->hq_l * 128, s);
}

// the one-rank output side of a row-parallel GEMM: + the residual stream, on the rows this rank owns (GemmArgs::resid_mod)
static void add_residual(GemmArgs& o, const mmada_handle* h) {
    o.resid = h->x; o.ldr = h->cfg.d_model; o.resid_mod = h->cfg.tp_size; o.resid_rank = h->cfg.tp_rank;
}

int run_blocks(mmada_handle* h, void* stream) {
    for (int i = 0; i < h->cfg.n_layers; ++i)
        if (mmada_attn_partial(h, i, stream) || mmada_mlp_partial(h, i, stream)) return 1;
    return 0;
}

extern "C" {

int mmada_embed(mmada_handle* h, const int64_t* ids, int B, int L, void* stream) {
    if (!h || !ids) return mm_fail("mmada_embed: null argument");
    hipStream_t s = (hipStream_t)stream;
    if (begin_forward(h, B, L, s)) return 1;
    return launch_embed(ids, h->wte, h->x, B, L, h->res.Lp, h->cfg.d_model, h->cfg.vocab, s, h->layers[0].attn_norm, h->xn,
                        h->cfg.rms_eps);
}

int mmada_attn_partial(mmada_handle* h, int layer, void* stream) {
    if (!h || !resident(h)) return mm_fail("mmada_attn_partial: call mmada_embed first");
    if (layer < 0 || layer >= h->cfg.n_layers) return mm_fail("mmada_attn_partial: bad layer");
    hipStream_t s = (hipStream_t)stream;
    Resident& r = h->res;
    const int d = h->cfg.d_model;
    if (layer == 0 && r.xn_is_layer0) {
        r.xn_is_layer0 = false;  // the embedding kernel normalised its rows already
    } else if (launch_rmsnorm(h->x, h->layers[layer].attn_norm, h->xn, r.M, d, h->cfg.rms_eps, s)) return 1;
    const GemmArgs g = qkv_args(h, layer, 0, r.M);
    const double rows = (double)r.B * r.L;
    {
        ProfScope p(h, layer, 0, 2.0 * rows * g.N * g.K, s);
        if (launch_gemm(EPI_QKV, g, s)) return 1;
    }
    // last block + consumed-row window: only the rows the caller will read are attended / projected (bit-identical on
    // them: the window start is rounded down to the 32-query wave granule, so every wave sees the queries it saw before)
    // The window END is rounded up to a multiple of 8 rows (inside the Lp-padded stream): the compact panel then meets the
    // shape contract of the 8-phase GEMM (whole 8-row LDS-DMA pieces); the up to 7 extra rows are computed like any other.
    int wbeg = 0, wend = 0, W = 0;
    if (!r.cc && layer == h->cfg.n_layers - 1 && h->win_end > h->win_beg) {
        if (h->win_end > r.L) return mm_fail("forward: consumed rows [%d,%d) exceed L=%d", h->win_beg, h->win_end, r.L);
        wbeg = h->win_beg & ~31;
        wend = std::min((h->win_end + 7) & ~7, r.Lp);
        W = wend - wbeg;
        if (W >= r.Lp) { wbeg = 0; W = 0; }  // nothing to skip
    }
    if (block_attention(h, layer, s, wbeg, W)) return 1;
    const int Mo = W ? r.B * W : r.M;
    const double orows = W ? (double)r.B * W : rows;
    GemmArgs o = attn_out_args(h, layer, 0, Mo);
    add_residual(o, h);
    if (W) { o.rwin = W; o.rlp = r.Lp; o.rbeg = wbeg; }
    {
        ProfScope p(h, layer, 2, 2.0 * orows * o.N * o.K, s);
        if (launch_gemm(EPI_RESID, o, s)) return 1;
    }
    std::swap(h->x, h->y);
    if (W) { r.cur_W = W; r.cur_beg = wbeg; r.Mcur = Mo; }
    return 0;
}

int mmada_mlp_partial(mmada_handle* h, int layer, void* stream) {
    if (!h || !resident(h)) return mm_fail("mmada_mlp_partial: call mmada_embed first");
    if (layer < 0 || layer >= h->cfg.n_layers) return mm_fail("mmada_mlp_partial: bad layer");
    hipStream_t s = (hipStream_t)stream;
    const Resident& r = h->res;
    const int d = h->cfg.d_model;
    if (launch_rmsnorm(h->x, h->layers[layer].ff_norm, h->xn, r.Mcur, d, h->cfg.rms_eps, s)) return 1;
    const GemmArgs g = gate_up_args(h, layer, 0, r.Mcur);
    const double rows = r.cur_W ? (double)r.Mcur : (double)r.B * r.L;
    {
        ProfScope p(h, layer, 3, 2.0 * rows * g.N * g.K, s);
        if (launch_gemm(EPI_SWIGLU, g, s)) return 1;
    }
    GemmArgs o = down_args(h, layer, 0, r.Mcur);
    add_residual(o, h);
    {
        ProfScope p(h, layer, 4, 2.0 * rows * o.N * o.K, s);
        if (launch_gemm(EPI_RESID, o, s)) return 1;
    }
    std::swap(h->x, h->y);
    return 0;
}

int mmada_forward_body(mmada_handle* h, const int64_t* ids, int B, int L, void* stream) {
    if (!h) return mm_fail("mmada_forward_body: null handle");
    if (runs_tensor_parallel(h)) {
        // tensor parallel: the exchange step lives in the library (tp_comm.hip); the residual stream stays sharded by rows
        if (!h->tp)
            return mm_fail("mmada_forward_body: tp_size=%d needs a connected collective (mmada_comm_create + "
                           "mmada_comm_connect_*) or the host-issued all-reduce of the segment API", h->cfg.tp_size);
        if (B > 0 && L > 0 && tp_forward_refused(h, B, (L + 7) / 8 * 8, false)) return 1;  // before anything is enqueued
        if (mmada_embed(h, ids, B, L, stream)) return 1;
        return tp_forward_body(h, (hipStream_t)stream);
    }
    if (mmada_embed(h, ids, B, L, stream)) return 1;
    return run_blocks(h, stream);
}

int mmada_set_consumed_rows(mmada_handle* h, int row_begin, int row_end) {
    if (!h) return mm_fail("mmada_set_consumed_rows: null handle");
    if (row_begin < 0 || row_end < row_begin) return mm_fail("mmada_set_consumed_rows: bad range [%d,%d)", row_begin, row_end);
    h->win_beg = row_begin;
    h->win_end = row_end;  // row_begin == row_end: no window (every row is computed)
    return 0;
}

int mmada_forward(mmada_handle* h, const int64_t* ids, int B, int L, void* logits_out, void* stream) {
    if (h && h->win_end > h->win_beg) return mm_fail("mmada_forward: returns every row; clear mmada_set_consumed_rows first");
    if (mmada_forward_body(h, ids, B, L, stream)) return 1;
    if (launch_iota_rows(h->rows_all, B * L, (hipStream_t)stream)) return 1;
    return mmada_head_rows(h, h->rows_all, B * L, 0, h->cfg.vocab, logits_out, stream);
}

void* mmada_stream_ptr(mmada_handle* h) { return h ? (void*)h->x : nullptr; }
size_t mmada_stream_bytes(const mmada_handle* h) { return h ? (size_t)h->res.Mcur * h->cfg.d_model * 2 : 0; }

int mmada_read_stream(mmada_handle* h, void* out, void* stream) {
    if (!h || !resident(h) || !out) return mm_fail("mmada_read_stream: no forward resident");
    const Resident& r = h->res;
    if (r.cur_W) return mm_fail("mmada_read_stream: the resident stream only holds rows [%d,%d) of each sequence", r.cur_beg, r.cur_beg + r.cur_W);
    if (r.xn_is_final) {  // rows of the residual stream live on their owners: collect them (parity tap only)
        if (tp_gather_stream(h, h->y, (hipStream_t)stream)) return 1;
        return launch_unpad_rows(h->y, (bf16_t*)out, r.B, r.L, r.Lp, h->cfg.d_model, (hipStream_t)stream);
    }
    return launch_unpad_rows(h->x, (bf16_t*)out, r.B, r.L, r.Lp, h->cfg.d_model, (hipStream_t)stream);
}

int mmada_debug_buffer(mmada_handle* h, int which, void** ptr_out, int32_t* lp_out, int32_t* lkv_out) {
    if (!h || !resident(h) || !ptr_out) return mm_fail("mmada_debug_buffer: no forward resident");
    bf16_t* tab[6] = {h->xn, h->q, h->k, h->vT, h->att, h->hbuf};
    if (which < 0 || which > 5) return mm_fail("mmada_debug_buffer: which=%d", which);
    *ptr_out = tab[which];
    if (lp_out) *lp_out = h->res.Lp;
    if (lkv_out) *lkv_out = h->res.Lkv;
    return 0;
}

int mmada_profile_begin(mmada_handle* h, int layer) {
    if (!h) return mm_fail("mmada_profile_begin: null handle");
    for (auto& r : h->prof) h->prof_pool.push_back({r.a, r.b});
    h->prof.clear();
    h->prof_layer = layer;
    return 0;
}

int mmada_profile_end(mmada_handle* h, int32_t* count_out, double* ms_out, double* flops_out) {
    if (!h || !count_out || !ms_out || !flops_out) return mm_fail("mmada_profile_end: null argument");
    for (int i = 0; i < 5; ++i) { count_out[i] = 0; ms_out[i] = 0.0; flops_out[i] = 0.0; }
    for (auto& r : h->prof) {
        MM_CHECK_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        MM_CHECK_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        count_out[r.kind] += 1; ms_out[r.kind] += ms; flops_out[r.kind] += r.flops;
        h->prof_pool.push_back({r.a, r.b});
    }
    h->prof.clear();
    h->prof_layer = -1;
    return 0;
}

int mmada_sdpa(mmada_handle* h, const void* q, const void* k, const void* v, void* out, int B, int H, int Hkv, int L,
               void* stream) {
    if (!h || !q || !k || !v || !out) return mm_fail("mmada_sdpa: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int Lkv = ceil_to(L, 64);
    const size_t qb = align_up((size_t)B * H * Lkv * 128 * 2, 256), kb = align_up((size_t)B * Hkv * Lkv * 128 * 2, 256);
    if (!h->ws || qb + 2 * kb > h->ws_bytes) return mm_fail("mmada_sdpa: workspace too small (%zu needed)", qb + 2 * kb);
    bf16_t* qp = (bf16_t*)h->ws;
    bf16_t* kp = (bf16_t*)(h->ws + qb);
    bf16_t* vt = (bf16_t*)(h->ws + qb + kb);
    invalidate(h);  // the resident forward (if any) is clobbered
    if (launch_pad_heads((const bf16_t*)q, qp, B * H, L, Lkv, s)) return 1;
    if (launch_pad_heads((const bf16_t*)k, kp, B * Hkv, L, Lkv, s)) return 1;
    if (launch_transpose_v((const bf16_t*)v, vt, B * Hkv, L, Lkv, s)) return 1;
    return launch_attention(qp, kp, vt, (bf16_t*)out, B, H, Hkv, L, L, Lkv, L, H * 128, s);
}

}  // extern "C"
