// tp_heads.hip — the LM head under tensor parallelism, on the transports of tp_comm.hip: the row gather in front of every head,
// the vocabulary-parallel text head (mmada_text_select_tp) and the vocabulary-parallel scoring head (tp_head_logprobs).
#include "row_heads.h"
#include "tp_comm.h"

static_assert(SCORE_BN == ROW_HEAD_BN, "the published score records are the one-rank launch's, tile for tile");

namespace {

// out[r] = src[b*Lp + l] for rows[r] = b*L + l (LM-head rows of an already normalised stream)
__global__ __launch_bounds__(256) void gather_rows_kernel(const bf16_t* src, const int32_t* rows, int R, int L, int Lp, int d,
                                                          int nflat, bf16_t* out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int flat = min(max(rows[r], 0), nflat - 1);
    const int b = flat / L, l = flat - b * L;
    const u32x4* s = (const u32x4*)(src + ((size_t)b * Lp + l) * d);
    for (int c = threadIdx.x & 63; c < (d >> 3); c += 64) ((u32x4*)(out + (size_t)r * d))[c] = s[c];
}

// Vocabulary-parallel text head: combine the tp per-rank records of every row into the conf (fp64 soft-max probability of
// the arg-max, generators/parallel_generator.py:185-205) and x0 the one-rank kernel writes.  One thread per row.
__global__ void tp_text_combine_kernel(TpPeers p, int size, int rank, const TextStat* own, const TextStat* gathered,
                                       int stat_stride, int R, double* conf_out, int32_t* x0_out) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= R) return;
    if (!gathered) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    TextStat st[TP_MAX];
    for (int j = 0; j < size; ++j) {
        if (gathered) st[j] = gathered[(size_t)j * stat_stride + row];
        else if (j == rank) st[j] = own[row];
        else {
            const u32x4 v = load_sys16(p.stats[j], (uint32_t)row * 16u);  // one 16-byte record
            st[j].lmax = __uint_as_float(v[0]);
            st[j].arg = (int32_t)v[1];
            st[j].sum = __longlong_as_double((long long)(((uint64_t)v[3] << 32) | v[2]));
        }
    }
    float mx = -INFINITY;
    int arg = 0;
    for (int j = 0; j < size; ++j)
        if (st[j].lmax > mx) { mx = st[j].lmax; arg = st[j].arg; }  // strict >: the lowest rank (lowest column) wins a tie
    if (!(mx > -INFINITY)) {  // not a masked position (or an all -inf row)
        conf_out[row] = -INFINITY;
        x0_out[row] = 0;
        return;
    }
    double tot = 0.0;
    for (int j = 0; j < size; ++j)
        if (st[j].lmax > -INFINITY) tot += st[j].sum * exp((double)st[j].lmax - (double)mx);
    conf_out[row] = 1.0 / tot;  // exp(l[x0] - max) / sum with x0 the arg-max
    x0_out[row] = arg;
}

// ---- vocabulary-parallel scoring head ---------------------------------------------------------------------------------------
// tx[0, n) = -inf in a PUBLISHED buffer (a target outside a rank's columns leaves it behind): ends like every publishing kernel
__global__ __launch_bounds__(256) void tp_score_reset_kernel(float* tx, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) tx[i] = -__builtin_inff();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

struct ScoreJoinArgs {
    const char* src[TP_MAX];  // rank j's record buffer of this round where THIS rank reads it: its own memory, a peer's mapped
                              // buffer (pull) or the gathered / staged copy (RCCL, copy)
    int sys;                  // pull: src[j != rank] is remote, read with system-scope loads
    int size, rank;
    int q;                    // tiles per rank: tile t is record (t - owner * q) of rank owner = t / q
    uint32_t rec_off;         // byte offset of the records behind the target logits
    int ld, ntn, R, col_begin, col_end;
    const int64_t* targets;
    float *logprob, *lse;
    int32_t* argmax;
    float* vmax;
};

// The join of rowstat_combine_kernel (row_heads.hip) with tile t's record taken from the rank that owns t: the same fold
// (row_heads.h: rowstat_fold), so every rank — and a one-rank handle — ends with the same bits.  Every rank joins every row.
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void tp_score_join_kernel(ScoreJoinArgs a) {
    if (a.sys) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // see tp_reduce_norm_kernel
    const int row = blockIdx.x * RS_ROWS + threadIdx.x % RS_ROWS;
    auto fetch = [&](int t, int r) -> float4 {
        const int owner = t / a.q;
        const uint32_t off = a.rec_off + ((uint32_t)(t - owner * a.q) * (uint32_t)a.ld + (uint32_t)r) * 16u;
        u32x4 v = {0u, 0u, 0u, 0u};
        // the lanes of a wave hold neighbouring tiles, which may belong to two owners: one pass per rank (unrolled: src[o] is a
        // kernel argument in SGPRs) keeps the base pointer wave-uniform, as load_sys16's descriptor needs it
#pragma unroll
        for (int o = 0; o < TP_MAX; ++o) {
            if (o != owner) continue;
            if (a.sys && o != a.rank) v = load_sys16(a.src[o], off);
            else v = *(const u32x4*)(a.src[o] + off);
        }
        return float4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
    };
    float m, sum;
    int arg;
    if (!rowstat_fold(fetch, row, a.R, a.ntn, m, sum, arg)) return;
    const long long t = a.targets[row];
    float tx = -__builtin_inff();
    if (t >= a.col_begin && t < a.col_end) {  // the target logit lives with the rank that owns the target's tile
        const int owner = (int)((t - a.col_begin) / SCORE_BN) / a.q;
#pragma unroll
        for (int o = 0; o < TP_MAX; ++o) {
            if (o != owner) continue;
            const float* p = (const float*)a.src[o] + row;
            tx = (a.sys && o != a.rank) ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : *p;
        }
    }
    rowstat_finish(row, m, sum, arg, t, tx, a.logprob, a.lse, a.argmax, a.vmax);
}

}  // namespace

int tp_gather_rows(const bf16_t* src, const int32_t* rows, int R, int L, int Lp, int d, int nflat, bf16_t* out, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, s, src, rows, R, L, Lp, d, nflat, out);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

int tp_head_gather(mmada_handle* h, const int32_t* rows, int R, hipStream_t s) {
    return tp_gather_rows(h->xn, rows, R, h->res.L, h->res.Lp, h->cfg.d_model, h->res.B * h->res.L, h->xg, s);
}

/* Vocabulary-parallel text step (generators/parallel_generator.py:185-217 at text_temperature == 0) after a
 * tensor-parallel forward: this rank multiplies the ln_f rows by ITS slice of ff_out.weight (vocab / tp_size columns; the
 * [B*T, vocab] logits exist nowhere), reduces each row to {max, first arg-max, fp64 sum-exp}, the tp records are exchanged
 * (16 bytes per row and rank) and combined, and the k[b] most confident masked positions are committed on every rank.
 * rows: device int32 [B*T] = b*L + text_start + t.  scratch: device, >= B*T*16 bytes (receives conf f64 / x0 i32). */
extern "C" int mmada_text_select_tp(mmada_handle* h, const int32_t* rows, int B, int T, int64_t* ids, int L, int text_start,
                                    const int32_t* k, void* scratch, void* stream) {
    if (!h || !transport_connected(h->tp)) return mm_fail("mmada_text_select_tp: no tensor-parallel transport connected");
    if (!h->res.xn_is_final || !resident(h)) return mm_fail("mmada_text_select_tp: no tensor-parallel forward resident");
    if (!rows || !ids || !k || !scratch) return mm_fail("mmada_text_select_tp: null argument");
    TpComm* c = h->tp;
    const int R = B * T;
    if (R <= 0) return 0;
    if (R > STAT_ROWS || R > h->res.B * h->res.L) return mm_fail("mmada_text_select_tp: %d rows exceed the limit", R);
    if (text_start < 0 || text_start + T > L) return mm_fail("mmada_text_select_tp: text span outside the sequence");
    hipStream_t s = (hipStream_t)stream;
    const int d = h->cfg.d_model, V = h->cfg.vocab;
    const int w = ((V + c->size - 1) / c->size + 7) / 8 * 8;
    const int v0 = min(V, c->rank * w), v1 = min(V, v0 + w);
    const size_t need = (size_t)R * w * 2;
    if (need > c->head_bytes) {  // first use (or a larger batch): not capturable, like every first call
        (void)hipFree(c->head_buf);
        c->head_buf = nullptr; c->head_bytes = 0;
        MM_CHECK_HIP(hipMalloc(&c->head_buf, need));
        c->head_bytes = need;
    }
    if (tp_head_gather(h, rows, R, s)) return 1;
    if (v1 > v0) {
        if (launch_gemm(EPI_STORE, gemm_bt_args(h->xg, h->lm_head + (size_t)v0 * d, c->head_buf, R, v1 - v0, d, w), s)) return 1;
    }
    TextStatsArgs ta{};
    ta.mode = TEXT_PARTIAL;
    ta.logits = c->head_buf;
    ta.B = B; ta.T = T; ta.V = v1 - v0; ta.ld = w; ta.col_off = v0;
    ta.ids = ids; ta.L = L; ta.text_start = text_start; ta.mask_id = h->cfg.mask_token_id;
    ta.stat_out = c->stats_pub;
    if (launch_text_stats(ta, s)) return 1;
    double* conf = (double*)scratch;
    int32_t* x0 = (int32_t*)((char*)scratch + (size_t)R * 8);
    const TextStat* gathered = nullptr;
    if (peers_mapped(c)) {
        if (signal_wait(c, s)) return 1;
    } else {
        ncclResult_t r = c->nccl.AllGather(c->stats_pub, c->stats_all, (size_t)R * sizeof(TextStat), ncclUint8, c->comm, s);
        if (r != ncclSuccess) return nccl_fail(c, "ncclAllGather", r);
        gathered = c->stats_all;
    }
    hipLaunchKernelGGL(tp_text_combine_kernel, dim3((R + 255) / 256), dim3(256), 0, s, c->peers, c->size, c->rank, c->stats_pub,
                       gathered, gathered ? R : 0, R, conf, x0);
    MM_CHECK_HIP(hipGetLastError());
    return launch_text_commit(scratch, B, T, ids, L, text_start, k, s);
}

// Vocabulary-parallel scoring head (mmada_head_logprobs on a connected handle).  The launch's 256-column tiles are split over
// the ranks in contiguous blocks (tp.py: score_tile_slice); each rank runs the one-rank EPI_ROWSTAT launch on its own tiles —
// the same columns, col0-based arg-max indices and partial last tile, hence the same records — into a published buffer, the
// ranks hand off, and every rank joins every row with the fold of the one-rank head.  Rows go in rounds of c->score.round.
//
// Buffer reuse (write after read).  A rank writes round i's records while a slower peer may still be joining an earlier
// round, in this call or in the previous one (two calls with no forward between them are legal).  The two published buffers
// alternate from round to round, ACROSS calls (c->score_flip; every rank makes the same calls, so the ranks agree on it).
// Round i + 2 is the next writer of round i's buffer.  This rank enqueues those writes behind its wait of hand-off i + 1;
// that wait returns only after every peer has signalled hand-off i + 1; a peer enqueues that signal behind its own join of
// round i (same stream), and a kernel starts only after its predecessor in the stream has retired.  So every peer's reads of
// round i are over before the first write of round i + 2 — whatever hand-off "i + 1" is: the next round's, the next call's,
// or one of a forward in between.  A graph replay breaks the alternation (the buffer choice is frozen into the graph, and
// eager calls and replays interleave freely), so a captured call brackets itself with a hand-off of its own at both ends:
// behind the first every earlier join has retired, and nothing later writes before the last.  The RCCL transport needs neither
// argument: an all-gather completes on a rank only when its send buffer may be reused.
int tp_head_logprobs(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, const int64_t* targets,
                     float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s) {
    TpComm* c = h->tp;
    if (!transport_connected(c)) return mm_fail("mmada_head_logprobs: no tensor-parallel transport connected");
    if (!h->res.xn_is_final || !resident(h)) return mm_fail("mmada_head_logprobs: no tensor-parallel forward resident");
    if (R <= 0) return 0;
    if (R > c->max_rows)
        return mm_fail("mmada_head_logprobs: %d rows exceed the %d rows this handle's comm was created for (mmada_comm_create max_rows)",
                       R, c->max_rows);
    if (check_head_range(h, "mmada_head_logprobs", R, h->res.B * h->res.L, col_begin, col_end)) return 1;
    const int d = h->cfg.d_model, tp = c->size;
    const ScoreLayout& lay = c->score;
    const int ntn = (col_end - col_begin + SCORE_BN - 1) / SCORE_BN, q = (ntn + tp - 1) / tp;
    if (q > lay.tiles) return mm_fail("mmada_head_logprobs: %d tiles per rank exceed the record buffers (%d)", q, lay.tiles);
    auto tiles_of = [&](int j) { return min(ntn, (j + 1) * q) - min(ntn, j * q); };
    const int t0 = min(ntn, c->rank * q), nt_own = tiles_of(c->rank);
    const int c0 = col_begin + t0 * SCORE_BN, n_own = nt_own > 0 ? min(col_end, c0 + nt_own * SCORE_BN) - c0 : 0;
    const bool mapped = peers_mapped(c);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    const bool bracket = mapped && cs != hipStreamCaptureStatusNone;
    if (tp_head_gather(h, rows, R, s)) return 1;
    if (bracket && signal_wait(c, s)) return 1;
    for (int r0 = 0; r0 < R; r0 += lay.round) {
        const int rr = min(lay.round, R - r0), rp = (rr + 7) / 8 * 8;
        char* buf = c->score_pub[c->score_flip];
        float* tx = (float*)buf;
        hipLaunchKernelGGL(tp_score_reset_kernel, dim3((rp + 255) / 256), dim3(256), 0, s, tx, rp);
        MM_CHECK_HIP(hipGetLastError());
        if (n_own > 0) {
            GemmArgs g = gemm_bt_args(h->xg + (size_t)r0 * d, h->lm_head + (size_t)c0 * d, nullptr, rp, n_own, d, 8);
            RowHeadArgs ra{};
            ra.part = (float4*)(buf + lay.rec_off); ra.tx = tx; ra.target = targets + r0;
            ra.rows = rr; ra.ld = rp; ra.col0 = c0;
            set_row_head_args(g, ra);
            g.publish = mapped;
            if (launch_gemm(EPI_ROWSTAT, g, s)) return 1;
        }
        ScoreJoinArgs a{};
        a.sys = c->mode == TP_PULL; a.size = tp; a.rank = c->rank; a.q = q; a.rec_off = lay.rec_off; a.ld = rp; a.ntn = ntn; a.R = rr;
        a.col_begin = col_begin; a.col_end = col_end; a.targets = targets + r0;
        a.logprob = logprob + r0; a.lse = lse ? lse + r0 : nullptr; a.argmax = argmax ? argmax + r0 : nullptr;
        a.vmax = vmax ? vmax + r0 : nullptr;
        if (mapped) {
            if (signal_wait(c, s)) return 1;  // every rank's records of this round are complete
            for (int j = 0; j < tp; ++j) {
                const char* peer = (const char*)c->peers.stats[j] + lay.text_bytes + (size_t)c->score_flip * lay.buf_bytes;
                if (j == c->rank) a.src[j] = buf;
                else if (c->mode == TP_PULL) a.src[j] = peer;
                else {  // copy engines: the peer's target logits and records of ITS tiles -> local staging
                    char* dst = c->score_all + (size_t)j * lay.buf_bytes;
                    if (tiles_of(j) > 0)
                        MM_CHECK_HIP(hipMemcpyAsync(dst, peer, (size_t)lay.rec_off + (size_t)tiles_of(j) * rp * 16, hipMemcpyDefault, s));
                    a.src[j] = dst;
                }
            }
        } else {
            const size_t cnt = (size_t)lay.rec_off + (size_t)q * rp * 16;  // equal counts: a rank with fewer tiles sends stale bytes nobody reads
            ncclResult_t r = c->nccl.AllGather(buf, c->score_all, cnt, ncclUint8, c->comm, s);
            if (r != ncclSuccess) return nccl_fail(c, "ncclAllGather", r);
            for (int j = 0; j < tp; ++j) a.src[j] = j == c->rank ? buf : c->score_all + (size_t)j * cnt;
        }
        hipLaunchKernelGGL(tp_score_join_kernel, dim3((rr + RS_ROWS - 1) / RS_ROWS), dim3(RS_ROWS * RS_GROUPS), 0, s, a);
        MM_CHECK_HIP(hipGetLastError());
        c->score_flip ^= 1;
    }
    if (bracket && signal_wait(c, s)) return 1;
    return 0;
}
