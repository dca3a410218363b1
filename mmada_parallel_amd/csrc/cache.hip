// cache.hip — the dLLM cache (model/modeling_llada.py:593-600,929-940,1244-1245,1406-1426): slot layout and binding, and the
// forward that runs through a slot.  Reading a slot's logits is mmada_cache_head_rows (heads.hip).  Host code only.
#include "../../include/mmada_mi355x.h"
#include "handle.h"

static void slot_layout(const mmada_handle* h, int B, int L, CacheSlot& c) {
    c.B = B; c.L = L; c.Lp = ceil_to(L, 8); c.Lkv = ceil_to(L, 64);
    c.kv_bytes = align_up((size_t)B * h->hkv_l * c.Lkv * 128 * 2, 256);
    c.layer_stride = 2 * c.kv_bytes;
    c.bytes = (size_t)h->cfg.n_layers * c.layer_stride + align_up((size_t)B * c.Lp * h->cfg.d_model * 2, 256);
}

extern "C" {

size_t mmada_cache_bytes(const mmada_handle* h, int B, int L) {
    if (!h || B <= 0 || L <= 0) return 0;
    CacheSlot c;
    slot_layout(h, B, L, c);
    return c.bytes;
}

int mmada_cache_bind(mmada_handle* h, int slot, void* mem, size_t bytes, int B, int L, void* stream) {
    if (!h) return mm_fail("mmada_cache_bind: null handle");
    if (slot < 0 || slot >= MMADA_CACHE_SLOTS) return mm_fail("mmada_cache_bind: slot %d outside [0,%d)", slot, MMADA_CACHE_SLOTS);
    if (!mem) {  // release
        h->slots[slot] = CacheSlot{};
        return 0;
    }
    if (runs_tensor_parallel(h) && !tp_comm_connected(h))
        return mm_fail("mmada_cache_bind: tp_size=%d needs the library's exchange connected (mmada_comm_create + mmada_comm_connect_*)", h->cfg.tp_size);
    if (B <= 0 || L <= 0 || L > h->cfg.max_seq) return mm_fail("mmada_cache_bind: bad shape B=%d L=%d", B, L);
    if (((uintptr_t)mem) & 255) return mm_fail("mmada_cache_bind: memory must be 256-byte aligned");
    CacheSlot c;
    slot_layout(h, B, L, c);
    if (bytes < c.bytes) return mm_fail("mmada_cache_bind: %zu bytes given, %zu needed", bytes, c.bytes);
    c.mem = (char*)mem;
    // the reference starts a cache at zeros (torch.zeros_like, :930-932,1407-1408): a never-computed position has zero
    // keys / values (a zero score, a zero value row) and zero logits (ln_f(0) = 0)
    MM_CHECK_HIP(hipMemsetAsync(mem, 0, c.bytes, (hipStream_t)stream));
    h->slots[slot] = c;
    return 0;
}

int mmada_forward_cached(mmada_handle* h, int slot, const int64_t* ids, const int32_t* pos, int B, int L, int Tc,
                         int q_pos_from_map, void* stream) {
    if (!h || !ids) return mm_fail("mmada_forward_cached: null argument");
    if (slot < 0 || slot >= MMADA_CACHE_SLOTS || !h->slots[slot].mem) return mm_fail("mmada_forward_cached: slot %d is not bound", slot);
    const CacheSlot& c = h->slots[slot];
    if (c.B != B || c.L != L) return mm_fail("mmada_forward_cached: slot holds B=%d L=%d, call has B=%d L=%d", c.B, c.L, B, L);
    const bool tp = runs_tensor_parallel(h);
    if (tp && !tp_comm_connected(h)) return mm_fail("mmada_forward_cached: tp_size=%d needs the library's exchange connected", h->cfg.tp_size);
    if (!pos) Tc = L;
    if (Tc <= 0 || Tc > L) return mm_fail("mmada_forward_cached: Tc=%d outside (0,%d]", Tc, L);
    hipStream_t s = (hipStream_t)stream;
    // buffers are carved for the whole (B, L) shape — mmada_cache_head_rows may ask for any row — and the blocks then run on
    // the compact [B, ceil8(Tc)] stream of the computed tokens
    if (begin_forward(h, B, L, s)) return 1;
    // from here on every exit, failing or not, leaves no plain forward resident (handle.h: Resident)
    CacheStep step(h, &c, pos ? h->posmap : nullptr, (pos && !q_pos_from_map) ? L - Tc : -1);
    Resident& r = h->res;
    if (pos) {
        r.L = Tc; r.Lp = ceil_to(Tc, 8); r.Lkv = ceil_to(Tc, 64); r.M = r.Mcur = B * r.Lp;
        if (launch_expand_pos(pos, h->posmap, B, Tc, r.Lp, L, s)) return 1;
    }
    const int d = h->cfg.d_model;
    if (launch_embed(ids, h->wte, h->x, B, r.L, r.Lp, d, h->cfg.vocab, s, h->layers[0].attn_norm, h->xn, h->cfg.rms_eps)) return 1;
    // tensor parallel: the blocks, their exchanges and the cache hooks of this rank's heads run in tp_forward_body; its last
    // exchange leaves xn = ln_f(x) on EVERY row of every rank, which is what the slot keeps (CacheSlot::normalized)
    if (tp ? tp_forward_body(h, s) : run_blocks(h, stream)) return 1;
    // the rows just computed replace theirs in the slot's final residual stream (the reference scatters the logits,
    // :1409-1411; a logit row is a function of its residual row alone, so the head runs on demand: mmada_cache_head_rows)
    bf16_t* xfin = c.xfin(h->cfg.n_layers);
    const bf16_t* fin = tp ? h->xn : h->x;
    h->slots[slot].normalized = tp;
    if (pos) {
        if (launch_scatter_rows(fin, xfin, h->posmap, r.M, r.Lp, c.Lp, d, s)) return 1;
    } else {
        MM_CHECK_HIP(hipMemcpyAsync(xfin, fin, (size_t)r.M * d * 2, hipMemcpyDeviceToDevice, s));
    }
    r.xn_is_final = false;
    return 0;
}

}  // extern "C"
