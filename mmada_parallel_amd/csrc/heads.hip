// heads.hip — the LM head on demand: logit rows of the resident forward (mmada_head_rows) or of a dLLM-cache slot
// (mmada_cache_head_rows), the fused scoring head (mmada_head_logprobs), its top-k form (mmada_head_topk) and its sampling form
// (mmada_head_sample, mmada_text_select_sampled; the noise: sample_noise.h).  Host code only.
#include "../../include/mmada_mi355x.h"
#include "handle.h"
#include "row_heads.h"
#include "sample_noise.h"

int check_head_range(const mmada_handle* h, const char* who, int R, int limit, int col_begin, int col_end) {
    if (R > limit) return mm_fail("%s: R=%d exceeds B*L=%d", who, R, limit);
    if (col_begin < 0 || col_end > h->cfg.vocab || col_begin >= col_end) return mm_fail("%s: bad column range", who);
    return 0;
}

// xg[i] = ln_f(x[rows[i]]) of the resident one-rank forward.  A windowed forward left the stream compact: row (b, l) sits at
// b*cur_W + l - cur_beg; rows outside the window the caller declared with mmada_set_consumed_rows were never computed and must
// not be requested
static int gather_resident_rows(mmada_handle* h, const int32_t* rows, int R, hipStream_t s) {
    const Resident& r = h->res;
    return launch_rmsnorm_gather(h->x, h->ln_f, h->xg, rows, R, r.L, r.cur_W ? r.cur_W : r.Lp, h->cfg.d_model, h->cfg.rms_eps, s,
                                 r.cur_beg, r.B * r.L);
}

// out [R, col_end - col_begin] = xg rows × lm_head[col_begin:col_end]
static int store_logits(const mmada_handle* h, const bf16_t* xg, int R, int col_begin, int col_end, void* out, hipStream_t s) {
    const int d = h->cfg.d_model, N = col_end - col_begin;
    return launch_gemm(EPI_STORE, gemm_bt_args(xg, h->lm_head + (size_t)col_begin * d, (bf16_t*)out, R, N, d, N), s);
}

// the record buffer of mmada_head_logprobs / mmada_head_topk / mmada_head_sample (`who`) holds at least `need` bytes
static int grow_score_buffer(mmada_handle* h, const char* who, size_t need, hipStream_t s) {
    if (need <= h->score_bytes) return 0;
    if (stream_capturing(s))
        return mm_fail("%s: the record buffer must grow (%zu bytes): run the call once outside the capture", who, need);
    MM_CHECK_HIP(hipStreamSynchronize(s));   // an earlier call on this stream may still read the old buffer
    (void)hipFree(h->score_buf);
    h->score_buf = nullptr; h->score_bytes = 0;
    MM_CHECK_HIP(hipMalloc(&h->score_buf, need));
    h->score_bytes = need;
    return 0;
}

// What the three fused heads share.  First: a forward is resident and no required pointer is null ...
static int fused_head_entry(const mmada_handle* h, const char* who, bool null_argument) {
    if (!h || !resident(h)) return mm_fail("%s: no forward resident", who);
    if (null_argument) return mm_fail("%s: null argument", who);
    return 0;
}
// ... then, behind the entry point's own checks: one rank only (`refusal`: the entry point's words for a handle that is not), the
// range, the record buffer (`bytes`: the head's size function, kernels.h), the same gather as mmada_head_rows (compact stream of a
// windowed forward; rows outside the window are an error there), and launch(A rows, W rows, N, K), the head's launcher.
template <class Launch>
static int fused_head_on_one_rank(mmada_handle* h, const char* who, bool one_rank, const char* refusal, const int32_t* rows, int R,
                                  int col_begin, int col_end, size_t (*bytes)(int, int), hipStream_t s, Launch launch) {
    if (!one_rank) return mm_fail("%s", refusal);
    if (R <= 0) return 0;
    if (check_head_range(h, who, R, h->res.B * h->res.L, col_begin, col_end)) return 1;
    const int d = h->cfg.d_model, N = col_end - col_begin;
    if (grow_score_buffer(h, who, bytes(R, N), s)) return 1;
    if (gather_resident_rows(h, rows, R, s)) return 1;
    return launch(h->xg, h->lm_head + (size_t)col_begin * d, N, d);
}

// mmada_head_topk / mmada_head_sample take the vocabulary-parallel form (tp_heads.hip) on a group of two or more ranks whose
// exchange runs in the library; that form refuses what it cannot serve (the RCCL transport, the diagnostic modes).  A handle
// with tp_size >= 2 but no exchange in the library, and the connected ONE-rank group of the test switch, keep the refusals below.
static bool vocabulary_parallel_group(const mmada_handle* h) { return h->cfg.tp_size >= 2 && tp_comm_connected(h); }

extern "C" {

int mmada_cache_head_rows(mmada_handle* h, int slot, const int32_t* rows, int R, int col_begin, int col_end,
                          void* logits_out, void* stream) {
    if (!h || !rows || !logits_out) return mm_fail("mmada_cache_head_rows: null argument");
    if (slot < 0 || slot >= MMADA_CACHE_SLOTS || !h->slots[slot].mem) return mm_fail("mmada_cache_head_rows: slot %d is not bound", slot);
    const CacheSlot& c = h->slots[slot];
    if (R <= 0) return 0;
    if (check_head_range(h, "mmada_cache_head_rows", R, c.B * c.L, col_begin, col_end)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const int d = h->cfg.d_model;
    // staging rows for ln_f: the gather buffer of the workspace.  While a plain forward is resident its carve is live, so
    // its own gather buffer (B*L rows of that forward) is the only region that may be written; otherwise the carve of the
    // slot's shape applies
    bf16_t* xg;
    if (resident(h)) {
        if ((size_t)R > (size_t)h->res.B * h->res.L)
            return mm_fail("mmada_cache_head_rows: %d rows do not fit the resident forward's gather buffer (%d x %d rows); "
                           "ask for fewer rows per call", R, h->res.B, h->res.L);
        xg = h->xg;
    } else {
        const Carve cv = carve_for(h, c.B, c.L);
        if (!h->ws || cv.total > h->ws_bytes) return mm_fail("mmada_cache_head_rows: workspace too small (%zu needed)", cv.total);
        xg = (bf16_t*)(h->ws + cv.xg);
    }
    if (c.normalized) {   // rows written by a tensor-parallel forward: ln_f already applied by the owners
        if (tp_gather_rows(c.xfin(h->cfg.n_layers), rows, R, c.L, c.Lp, d, c.B * c.L, xg, s)) return 1;
    } else if (launch_rmsnorm_gather(c.xfin(h->cfg.n_layers), h->ln_f, xg, rows, R, c.L, c.Lp, d, h->cfg.rms_eps, s, 0, c.B * c.L))
        return 1;
    return store_logits(h, xg, R, col_begin, col_end, logits_out, s);
}

int mmada_head_rows(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, void* logits_out,
                    void* stream) {
    if (!h || !resident(h)) return mm_fail("mmada_head_rows: no forward resident");
    if (!rows || !logits_out) return mm_fail("mmada_head_rows: null argument");
    if (R <= 0) return 0;
    if (check_head_range(h, "mmada_head_rows", R, h->res.B * h->res.L, col_begin, col_end)) return 1;
    hipStream_t s = (hipStream_t)stream;
    // tensor-parallel forward: the last exchange already applied ln_f on the owners' rows
    if (h->res.xn_is_final ? tp_head_gather(h, rows, R, s) : gather_resident_rows(h, rows, R, s)) return 1;
    return store_logits(h, h->xg, R, col_begin, col_end, logits_out, s);
}

int mmada_head_logprobs(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, const int64_t* targets,
                        float* logprob_out, float* lse_out, int32_t* argmax_out, float* max_out, void* stream) {
    if (fused_head_entry(h, "mmada_head_logprobs", !rows || !targets || !logprob_out)) return 1;
    hipStream_t s = (hipStream_t)stream;
    // a connected handle (also a one-rank group): the vocabulary-parallel head, same records, same fold (tp_heads.hip)
    if (tp_comm_connected(h)) return tp_head_logprobs(h, rows, R, col_begin, col_end, targets, logprob_out, lse_out, argmax_out, max_out, s);
    return fused_head_on_one_rank(
        h, "mmada_head_logprobs", !h->res.xn_is_final && h->cfg.tp_size == 1,
        "mmada_head_logprobs: a tensor-parallel handle scores through the library's exchange only (mmada_comm_create + "
        "mmada_comm_connect_*): a vocabulary-parallel score exchanges the same records as mmada_text_select_tp",
        rows, R, col_begin, col_end, head_rowstat_bytes, s, [&](const bf16_t* A, const bf16_t* W, int N, int K) {
            return launch_head_rowstat(A, W, R, N, K, col_begin, targets, h->score_buf, logprob_out, lse_out, argmax_out, max_out, s);
        });
}

int mmada_head_topk(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, int k, int32_t* ids_out,
                    float* logit_out, float* lse_out, void* stream) {
    if (k < 1 || k > MMADA_TOPK_MAX) return mm_fail("mmada_head_topk: k=%d outside [1, MMADA_TOPK_MAX=%d]", k, MMADA_TOPK_MAX);
    if ((long long)k > (long long)col_end - col_begin)
        return mm_fail("mmada_head_topk: k=%d exceeds the column range [%d, %d)", k, col_begin, col_end);
    if (fused_head_entry(h, "mmada_head_topk", !rows || !ids_out || !logit_out)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (vocabulary_parallel_group(h)) return tp_head_topk(h, rows, R, col_begin, col_end, k, ids_out, logit_out, lse_out, s);
    return fused_head_on_one_rank(
        h, "mmada_head_topk", !runs_tensor_parallel(h) && !h->res.xn_is_final,
        "mmada_head_topk: top-k runs on one rank (a handle without a tensor-parallel exchange): the vocabulary-parallel "
        "top-k, whose key records would ride the score exchange of mmada_head_logprobs, is a follow-up",
        rows, R, col_begin, col_end, head_rowtopk_bytes, s, [&](const bf16_t* A, const bf16_t* W, int N, int K) {
            return launch_head_rowtopk(A, W, R, N, K, col_begin, k, h->score_buf, ids_out, logit_out, lse_out, s);
        });
}

unsigned mmada_topk_order_key(unsigned bf16_bits) { return topk_order(__builtin_bit_cast(float, (uint32_t)(bf16_bits & 0xffffu) << 16)) >> 16; }

int mmada_head_sample(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, float temperature, uint64_t seed,
                      uint64_t* counter, int32_t* ids_out, float* logprob_out, float* lse_out, int32_t* argmax_out, float* max_out,
                      void* stream) {
    if (fused_head_entry(h, "mmada_head_sample", !rows || !counter || !ids_out || !logprob_out)) return 1;
    if (!(temperature >= 0.f) || __builtin_isinf(temperature))
        return mm_fail("mmada_head_sample: temperature %g is not a finite value >= 0", (double)temperature);
    hipStream_t s = (hipStream_t)stream;
    if (vocabulary_parallel_group(h))
        return tp_head_sample(h, rows, R, col_begin, col_end, temperature, seed, counter, ids_out, logprob_out, lse_out, argmax_out, max_out, s);
    return fused_head_on_one_rank(
        h, "mmada_head_sample", !runs_tensor_parallel(h) && !h->res.xn_is_final,
        "mmada_head_sample: the draw runs on one rank (a handle without a tensor-parallel exchange): the "
        "vocabulary-parallel draw, whose key records would ride the score exchange of mmada_head_logprobs, is a follow-up",
        rows, R, col_begin, col_end, head_rowsample_bytes, s, [&](const bf16_t* A, const bf16_t* W, int N, int K) {
            return launch_head_rowsample(A, W, R, N, K, col_begin, temperature, seed, counter, h->score_buf, ids_out, logprob_out, lse_out,
                                         argmax_out, max_out, s);
        });
}

// The text step with the draw above (generators/parallel_generator.py:181-217, low-confidence re-masking).  scratch is the layout
// of launch_text_commit, conf [B*T] fp64 | x0 [B*T] int32, and its last B*T*4 bytes hold the draws' log-probabilities meanwhile:
// the head writes x0 and the log-probabilities in place, one small kernel turns the latter into the confidences.
int mmada_text_select_sampled(mmada_handle* h, const int32_t* rows, int B, int T, float temperature, uint64_t seed, uint64_t* counter,
                              int64_t* ids, int L, int text_start, const int32_t* k, void* scratch, void* stream) {
    if (!h || !resident(h)) return mm_fail("mmada_text_select_sampled: no forward resident");
    if (!rows || !counter || !ids || !k || !scratch) return mm_fail("mmada_text_select_sampled: null argument");
    if (B <= 0 || T <= 0) return 0;
    if (text_start < 0 || text_start + T > L) return mm_fail("mmada_text_select_sampled: text span outside the sequence");
    if (T > 8192) return mm_fail("mmada_text_select_sampled: T=%d too large", T);
    if ((long long)B * T > (long long)h->res.B * h->res.L) return mm_fail("mmada_text_select_sampled: B*T=%lld exceeds the resident forward", (long long)B * T);
    const size_t n = (size_t)B * T;
    int32_t* x0 = (int32_t*)((char*)scratch + n * 8);
    float* logprob = (float*)((char*)scratch + n * 12);
    if (mmada_head_sample(h, rows, B * T, 0, h->cfg.vocab, temperature, seed, counter, x0, logprob, nullptr, nullptr, nullptr, stream)) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (launch_text_sampled_conf(logprob, B, T, ids, L, text_start, h->cfg.mask_token_id, scratch, s)) return 1;
    return launch_text_commit(scratch, B, T, ids, L, text_start, k, s);
}

uint32_t mmada_sample_word(uint64_t seed, uint64_t counter, uint32_t row, uint32_t col) { return sample_word(seed, counter, row, col); }
float mmada_sample_uniform(uint32_t word) { return sample_uniform(word); }

int mmada_probe_gumbel(uint64_t seed, uint64_t counter, int row0, int R, int col0, int N, uint32_t* words_out, float* g_out, void* stream) {
    if (R <= 0 || N <= 0 || col0 < 0 || row0 < -1 || (!words_out && !g_out)) return mm_fail("mmada_probe_gumbel: bad argument");
    return launch_gumbel_probe(seed, counter, row0, R, col0, N, words_out, g_out, (hipStream_t)stream);
}

float mmada_sample_normal(uint64_t seed, uint64_t counter, uint32_t r) { return sample_normal(seed, counter, r); }
float mmada_sample_remask_gumbel(uint64_t seed, uint64_t counter, uint32_t r) { return sample_remask_gumbel(seed, counter, r); }

int mmada_probe_normal(uint64_t seed, uint64_t counter, int row0, int R, uint32_t* words01_out, float* z_out, uint16_t* z_bf16_out,
                       void* stream) {
    if (R <= 0 || row0 < 0 || (!words01_out && !z_out && !z_bf16_out)) return mm_fail("mmada_probe_normal: bad argument");
    return launch_normal_probe(seed, counter, row0, R, words01_out, z_out, z_bf16_out, (hipStream_t)stream);
}

size_t mmada_score_buffer_bytes(const mmada_handle* h) { return h ? h->score_bytes : 0; }

}  // extern "C"
