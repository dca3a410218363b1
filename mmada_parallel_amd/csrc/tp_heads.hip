// tp_heads.hip — the LM head under tensor parallelism, on the transports of tp_comm.hip: the row gather in front of every head,
// the vocabulary-parallel text head (mmada_text_select_tp) and the vocabulary-parallel row heads: scoring, top-k and the
// Gumbel-max draw (tp_head_logprobs, tp_head_topk, tp_head_sample — one round loop, three joins).
#include "row_head_join.h"
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

// Where a join finds the records of a round — the record source (row_head_join.h) of the three joins below: tile t's records
// come from the rank that owns t.  What the round loop (tp_head_rounds) hands every head's join.
struct JoinSrc {
    const char* src[TP_MAX];  // rank j's record buffer of this round where THIS rank reads it: its own memory, a peer's mapped
                              // buffer (pull) or the gathered / staged copy (RCCL, copy)
    int sys;                  // pull: src[j != rank] is remote, read with system-scope loads
    int size, rank;
    int q;                    // tiles per rank: tile t is record (t - owner * q) of rank owner = t / q
    uint32_t rec_off;         // byte offset of the records behind the target logits
    int ld, ntn, R;
    int col_begin, col_end;   // the call's column range (the owner of a target's tile)

    // 16 bytes at byte offset `off` of the buffer of rank `owner` (per lane; src[o] is a kernel argument in SGPRs).  The lanes of
    // a wave hold neighbouring tiles, which may belong to two owners: one pass per rank (unrolled) keeps the base pointer
    // wave-uniform, as load_sys16's descriptor needs it
    MM_DEVICE u32x4 load16(int owner, uint32_t off) const {
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int o = 0; o < TP_MAX; ++o) {
            if (o != owner) continue;
            if (sys && o != rank) v = load_sys16(src[o], off);
            else v = *(const u32x4*)(src[o] + off);
        }
        return v;
    }
    // byte offset of tile t's extra record of `bytes` bytes for row r (behind the owner's records)
    MM_DEVICE uint32_t extra_off(int t, int r, uint32_t bytes) const {
        const int owner = t / q, nt = min(ntn, (owner + 1) * q) - owner * q;   // tiles the owner has in this call (t is one)
        return rec_off + (uint32_t)nt * (uint32_t)ld * 16u + ((uint32_t)(t - owner * q) * (uint32_t)ld + (uint32_t)r) * bytes;
    }
    static MM_DEVICE float4 as_float4(u32x4 v) {
        return float4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
    }

    MM_DEVICE float4 record(int t, int r) const {
        const int owner = t / q;
        return as_float4(load16(owner, rec_off + ((uint32_t)(t - owner * q) * (uint32_t)ld + (uint32_t)r) * 16u));
    }
    MM_DEVICE void topk_keys(int t, int r, uint32_t (&key)[TOPK_MAX]) const {
        const uint32_t off = extra_off(t, r, row_head_extra_bytes(EPI_ROWTOPK));
        const u32x4 lo = load16(t / q, off), hi = load16(t / q, off + 16u);
        key[0] = lo[0]; key[1] = lo[1]; key[2] = lo[2]; key[3] = lo[3];
        key[4] = hi[0]; key[5] = hi[1]; key[6] = hi[2]; key[7] = hi[3];
    }
    MM_DEVICE float4 sample_triple(int t, int r) const {
        return as_float4(load16(t / q, extra_off(t, r, row_head_extra_bytes(EPI_ROWSAMPLE))));
    }
    MM_DEVICE float target_logit(int row, long long t) const {
        float tx = -__builtin_inff();
        if (t >= col_begin && t < col_end) {  // the target logit lives with the rank that owns the target's tile
            const int owner = (int)((t - col_begin) / SCORE_BN) / q;
#pragma unroll
            for (int o = 0; o < TP_MAX; ++o) {
                if (o != owner) continue;
                const float* p = (const float*)src[o] + row;
                tx = (sys && o != rank) ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : *p;
            }
        }
        return tx;
    }
    MM_DEVICE void acquire() const {
        if (sys) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // see tp_reduce_norm_kernel
    }
};

// The joins of row_heads.hip's kernels (the bodies: row_head_join.h) over the ranks' records.  Every rank joins every row.
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void tp_score_join_kernel(JoinSrc src, ScoreOut out) {
    src.acquire();
    rowstat_join(src, src.R, src.ntn, out);
}
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void tp_topk_join_kernel(JoinSrc src, TopkOut out) {
    src.acquire();
    rowtopk_join(src, src.R, src.ntn, out);
}
// (with out.counter — the last round of a call — the call's last kernel: every GEMM of this rank has read *counter)
__global__ __launch_bounds__(RS_ROWS * RS_GROUPS) void tp_sample_join_kernel(JoinSrc src, SampleOut out) {
    src.acquire();
    rowsample_join(src, src.R, src.ntn, out);
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

// Vocabulary-parallel row heads (mmada_head_logprobs on a connected handle; mmada_head_topk and mmada_head_sample on a group of
// two or more ranks over a mapped transport): ONE round loop, tp_head_rounds, parameterised by the head.  The launch's
// 256-column tiles are split over the ranks in contiguous blocks (tp.py: score_tile_slice); each rank runs the one-rank launch
// of the head's epilogue on its own tiles — the same columns, col0-based indices and partial last tile, hence the same records
// — into a published buffer, the ranks hand off, and every rank joins every row with the fold of the one-rank head (and, for
// top-k and the draw, the totally ordered candidates of the one-rank join).  Rows go in rounds of c->score.round; the draw's
// noise row is the row's index in the CALL (RowHeadArgs::row0 = the round's first row).  The three heads share the two
// published buffers and the flip, so their calls may follow each other in any order.
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
//
// head: the epilogue; who: the entry point's name in messages.  fill(ra, r0): the head's own fields of a round's RowHeadArgs
// (target / counter / seed / temperature / row0) for the round that starts at row r0 — part, tx, extra, rows, ld, col0 are set
// here.  join(src, r0, rr, last): launches the head's join of the round's rr rows (last: the call's last round).
template <class Fill, class Join>
static int tp_head_rounds(mmada_handle* h, const char* who, int head, const int32_t* rows, int R, int col_begin, int col_end,
                          hipStream_t s, Fill fill, Join join) {
    TpComm* c = h->tp;
    if (!transport_connected(c)) return mm_fail("%s: no tensor-parallel transport connected", who);
    if (!h->res.xn_is_final || !resident(h)) return mm_fail("%s: no tensor-parallel forward resident", who);
    const uint32_t xrec = row_head_extra_bytes(head);
    static_assert(row_head_extra_bytes(EPI_ROWTOPK) <= SCORE_EXTRA_MAX && row_head_extra_bytes(EPI_ROWSAMPLE) <= SCORE_EXTRA_MAX,
                  "the published buffers hold the larger extra record");
    const bool mapped = peers_mapped(c);
    if (xrec && !mapped)
        return mm_fail("%s: over the RCCL transport the vocabulary-parallel head is not built (nothing on one device can exercise "
                       "it: RCCL refuses two ranks per device); connect the pull or the copy transport", who);
    if (R <= 0) return 0;
    if (R > c->max_rows)
        return mm_fail("%s: %d rows exceed the %d rows this handle's comm was created for (mmada_comm_create max_rows)", who, R, c->max_rows);
    if (check_head_range(h, who, R, h->res.B * h->res.L, col_begin, col_end)) return 1;
    const int d = h->cfg.d_model, tp = c->size;
    const ScoreLayout& lay = c->score;
    const int ntn = (col_end - col_begin + SCORE_BN - 1) / SCORE_BN, q = (ntn + tp - 1) / tp;
    if (q > lay.tiles) return mm_fail("%s: %d tiles per rank exceed the record buffers (%d)", who, q, lay.tiles);
    auto tiles_of = [&](int j) { return min(ntn, (j + 1) * q) - min(ntn, j * q); };
    const int t0 = min(ntn, c->rank * q), nt_own = tiles_of(c->rank);
    const int c0 = col_begin + t0 * SCORE_BN, n_own = nt_own > 0 ? min(col_end, c0 + nt_own * SCORE_BN) - c0 : 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    const bool bracket = mapped && cs != hipStreamCaptureStatusNone;
    if (tp_head_gather(h, rows, R, s)) return 1;
    if (bracket && signal_wait(c, s)) return 1;
    for (int r0 = 0; r0 < R; r0 += lay.round) {
        const int rr = min(lay.round, R - r0), rp = (rr + 7) / 8 * 8;
        char* buf = c->score_pub[c->score_flip];
        float* tx = (float*)buf;
        if (head == EPI_ROWSTAT) {   // (the other heads have no targets: nothing reads tx)
            hipLaunchKernelGGL(tp_score_reset_kernel, dim3((rp + 255) / 256), dim3(256), 0, s, tx, rp);
            MM_CHECK_HIP(hipGetLastError());
        }
        if (n_own > 0) {
            RowHeadArgs ra{};
            fill(ra, r0);
            ra.part = (float4*)(buf + lay.rec_off); ra.tx = tx;
            ra.extra = xrec ? buf + score_extra_off(lay.rec_off, nt_own, rp) : nullptr;
            ra.rows = rr; ra.ld = rp; ra.col0 = c0;
            if (launch_row_head_gemm(head, h->xg + (size_t)r0 * d, h->lm_head + (size_t)c0 * d, rp, n_own, d, ra, mapped, s)) return 1;
        }
        JoinSrc a{};
        a.sys = c->mode == TP_PULL; a.size = tp; a.rank = c->rank; a.q = q; a.rec_off = lay.rec_off; a.ld = rp; a.ntn = ntn; a.R = rr;
        a.col_begin = col_begin; a.col_end = col_end;
        if (mapped) {
            if (signal_wait(c, s)) return 1;  // every rank's records of this round are complete
            for (int j = 0; j < tp; ++j) {
                const char* peer = (const char*)c->peers.stats[j] + lay.text_bytes + (size_t)c->score_flip * lay.buf_bytes;
                if (j == c->rank) a.src[j] = buf;
                else if (c->mode == TP_PULL) a.src[j] = peer;
                else {  // copy engines: the peer's target logits, records and extra records of ITS tiles -> local staging
                    char* dst = c->score_all + (size_t)j * lay.buf_bytes;
                    if (tiles_of(j) > 0)
                        MM_CHECK_HIP(hipMemcpyAsync(dst, peer, (size_t)lay.rec_off + (size_t)tiles_of(j) * rp * (16 + xrec), hipMemcpyDefault, s));
                    a.src[j] = dst;
                }
            }
        } else {
            const size_t cnt = (size_t)lay.rec_off + (size_t)q * rp * 16;  // equal counts: a rank with fewer tiles sends stale bytes nobody reads
            ncclResult_t r = c->nccl.AllGather(buf, c->score_all, cnt, ncclUint8, c->comm, s);
            if (r != ncclSuccess) return nccl_fail(c, "ncclAllGather", r);
            for (int j = 0; j < tp; ++j) a.src[j] = j == c->rank ? buf : c->score_all + (size_t)j * cnt;
        }
        join(a, r0, rr, r0 + lay.round >= R);
        MM_CHECK_HIP(hipGetLastError());
        c->score_flip ^= 1;
    }
    if (bracket && signal_wait(c, s)) return 1;
    return 0;
}

int tp_head_logprobs(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, const int64_t* targets,
                     float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s) {
    return tp_head_rounds(
        h, "mmada_head_logprobs", EPI_ROWSTAT, rows, R, col_begin, col_end, s, [&](RowHeadArgs& ra, int r0) { ra.target = targets + r0; },
        [&](const JoinSrc& src, int r0, int rr, bool) {
            const ScoreOut out{targets + r0, logprob + r0, lse ? lse + r0 : nullptr, argmax ? argmax + r0 : nullptr, vmax ? vmax + r0 : nullptr};
            hipLaunchKernelGGL(tp_score_join_kernel, join_grid(rr), dim3(RS_ROWS * RS_GROUPS), 0, s, src, out);
        });
}

int tp_head_topk(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, int k, int32_t* ids, float* logits,
                 float* lse, hipStream_t s) {
    return tp_head_rounds(
        h, "mmada_head_topk", EPI_ROWTOPK, rows, R, col_begin, col_end, s, [&](RowHeadArgs&, int) {},
        [&](const JoinSrc& src, int r0, int rr, bool) {
            // the join's unused log-probabilities go to this rank's own slot of the private staging, which no transport uses
            float* spare = (float*)(h->tp->score_all + (size_t)h->tp->rank * h->tp->score.buf_bytes);
            const TopkOut out{col_begin, k, ids + (size_t)r0 * k, logits + (size_t)r0 * k, lse ? lse + r0 : nullptr, spare};
            hipLaunchKernelGGL(tp_topk_join_kernel, join_grid(rr), dim3(RS_ROWS * RS_GROUPS), 0, s, src, out);
        });
}

int tp_head_sample(mmada_handle* h, const int32_t* rows, int R, int col_begin, int col_end, float temperature, uint64_t seed,
                   uint64_t* counter, int32_t* ids, float* logprob, float* lse, int32_t* argmax, float* vmax, hipStream_t s) {
    return tp_head_rounds(
        h, "mmada_head_sample", EPI_ROWSAMPLE, rows, R, col_begin, col_end, s,
        [&](RowHeadArgs& ra, int r0) { ra.counter = counter; ra.seed = seed; ra.temperature = temperature; ra.row0 = r0; },
        [&](const JoinSrc& src, int r0, int rr, bool last) {
            const SampleOut out{ids + r0, logprob + r0, lse ? lse + r0 : nullptr, argmax ? argmax + r0 : nullptr, vmax ? vmax + r0 : nullptr,
                                last ? counter : nullptr};   // once per call, behind every GEMM of this rank that reads it
            hipLaunchKernelGGL(tp_sample_join_kernel, join_grid(rr), dim3(RS_ROWS * RS_GROUPS), 0, s, src, out);
        });
}
