// tp_comm.hip — the tensor-parallel exchange step of the denoiser forward, inside the library (SURVEY.md §8b
// mmada_allreduce_init, §8e).  The reference has no tensor parallelism (inference.py:83-85 loads one replica); this is
// the one place the 8B block needs a collective: after each of the two row-parallel GEMMs (attn_out, ff_out;
// model/modeling_llada.py:741-744, 968-970) every rank holds a partial [M, d] sum.
//
// Instead of an all-reduce of the replicated residual stream followed by a replicated RMSNorm, one exchange is
//     reduce-scatter  ->  residual add + RMSNorm on the 1/tp rows this rank OWNS  ->  all-gather of the normalised rows
// so the residual stream itself is never communicated (each rank keeps only its own rows of it), the RMSNorm work is
// divided by tp, and the all-gathered tensor is exactly the A operand of the next column-parallel GEMM (or, after the
// last block, ln_f(x) for the LM head).  Bytes on the fabric are those of one all-reduce.
//
// Two transports behind the same step:
//   pull (mode 1)  every rank maps its peers' published buffers (hipIpc handles between processes, plain pointers for
//                  peers in one process) and only ever READS remote memory: the reduce kernel pulls the tp partial
//                  slices of its own rows with system-scope loads and sums them in rank order (deterministic); the
//                  gather kernel pulls the other owners' normalised rows.  Everything a GEMM reads was therefore written
//                  by a kernel of its own device.  Hand-offs are monotonic sequence counters in fine-grained memory,
//                  published by a 1-thread kernel after the producing kernel has retired and awaited by a 1-wave kernel
//                  (bounded spin: a lost peer raises an error flag, it never hangs the device).  The counters live in
//                  device memory, so the whole exchange is hipGraph-replayable.  xGMI is a full mesh of point-to-point
//                  links: the tp-1 pulls of a rank run over tp-1 different links at once (SURVEY.md §5.8 two-shot).
//   RCCL (mode 2)  ncclReduceScatter / ncclAllGather issued from here (librccl is dlopen'ed: no link-time dependency, the
//                  host may hand in the library torch already loaded), same owner-side kernel in between.
//   copy (mode 4)  round 5: the same mapped peer buffers and hand-off counters as pull, but the bytes are moved by the COPY
//                  ENGINES (hipMemcpyAsync on the mapped peer pointers: SDMA between devices): the tp-1 peer slices of this
//                  rank's rows into local staging, then the owner kernel reads LOCAL memory only; the all-gather half is
//                  tp-1 copies and no kernel.  No compute unit waits on a remote load, so nothing of the exchange competes
//                  with the GEMMs for CUs except the owner kernel (1/tp of the rows, local operands).
// Two diagnostics (values void, timing only) share one data path, the owner kernel on this rank's own partial with no hand-off:
//   no exchange (mode 3)    nothing stands for the transfers: a rank's compute alone.
//   emulated link (mode 5)  one tp_link_wait_kernel in front of the owner kernel (the reduce-scatter half) and one behind it (the
//                  all-gather half), on the exchange's stream: each sleeps for the bytes one link would carry over the
//                  "tp_emulate_mbps" switch.  Forward time in mode 5 minus mode 3 is the exchange time the schedule leaves
//                  exposed against a fixed-rate link without contention — measurable on one GPU.
// CU partition (round 5, mmada_comm_set_partition): the 8-phase GEMM's 320x256 tile holds 2 waves x 256 VGPRs per SIMD and
// 144+ KiB of LDS — while one runs on a CU no exchange wave can be resident there, so "the exchange runs under the next GEMM" was
// time-slicing at workgroup granularity driven by stream priority.  With a partition the exchange stream is created with a CU
// mask of `n` CUs (bit i of the mask is CU i / 8 of XCD i % 8: the low n bits spread over all eight XCDs) and the forward's
// compute kernels run on a library stream masked to the OTHER CUs, joined to the caller's stream by events at both ends:
// the exchange kernels own their CUs by construction, the GEMMs lose n / 256 of the chip, deterministically.
// Overlap: the M rows are cut into two chunks; the exchange of chunk i runs on a second (high-priority) stream under the
// row-parallel GEMM of chunk i+1 / the next column-parallel GEMM of chunk i-1 — also at batch 1, the only join point is
// the attention (needs every key).  MMADA_TP_CHUNKS = 4 or 8 (opt-in) on a batch of two or more sequences replaces the row chunks by
// SEQUENCE CHAINS (tp_plan.h: chunk_plan_of): up to 8 groups of whole sequences, each an independent chain through the block —
// a sequence's attention needs that sequence's keys only — so a chain's exchange hides under every other chain's compute
// (tp_forward_body_on).
// The LM heads on top of these transports (text select, scoring) are tp_heads.hip; the state both units share is tp_comm.h.
#include <dlfcn.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "tp_comm.h"

namespace {

constexpr int MAXCH = 8;  // 16-B chunks per lane: d <= 4096

// ---- hand-off ------------------------------------------------------------------------------------------------------
// `seq` (private) and `ctr` (published) live in one fine-grained block and are only ever touched with system-scope atomics:
// the 1-thread kernels below land on a different XCD every time, and a plain load could be served from that XCD's L2
// (a line left there by an earlier owner of the address) instead of memory.
__global__ void tp_signal_kernel(uint32_t* seq, uint32_t* ctr) {
    const uint32_t v = __hip_atomic_load(seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) + 1u;
    __hip_atomic_store(seq, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // the producing kernel retired before this one started (stream order) and each of its workgroups ended with a
    // system-scope release; this fence + drain orders the counter behind everything this wave has seen
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(ctr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void tp_wait_kernel(const uint32_t* seq, TpPeers p, int size, int rank, int* err, long long timeout_ticks) {
    const int j = threadIdx.x;
    if (j < size && j != rank && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        const uint32_t v = __hip_atomic_load(seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const long long t0 = wall_clock64();
        while ((int)(__hip_atomic_load(p.ctr[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - v) < 0) {
            __builtin_amdgcn_s_sleep(20);
            if (wall_clock64() - t0 > timeout_ticks) {  // never hang the device: flag it, results are void
                __hip_atomic_store(err, 1 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
}

struct ReduceArgs {
    TpPeers p;
    int size, rank;
    int nsrc;              // pull: = size (source j = rank j's partial, the own one read locally); RCCL: 1 (pre-summed rows)
    const bf16_t* presum;  // RCCL: [r1 - r0, d] rows already summed over ranks (row 0 = global row r0)
    int src_row0[TP_MAX];  // row of source j's buffer that holds stream row 0 of this launch: 0 for a peer's whole partial buffer
                           // (pull), r0 for a staged slice whose first row is this rank's first owned row (copy transport)
    const bf16_t* part;    // this rank's own partial [*, d]
    bf16_t* x;             // residual stream [*, d]: rows [r0, r1) are this rank's, updated in place
    const bf16_t* w;       // RMSNorm weight [d]
    bf16_t* hn_pub;        // published normalised rows (global row index)
    bf16_t* xn;            // this rank's full normalised buffer: own rows are written here directly
    int r0, r1, d;
    float eps;
};

// One wave per owned row:  s = sum_j partial_j[m]  (fp32, rank order) ; out = bf16(s) ; x[m] = bf16(x[m] + out)
// (the reference: x + attn_out(att) / x + ff_out(h), model/modeling_llada.py:953, 968-970 — every nn.Linear output is
// rounded to bf16 before the residual add) ; hn = RMSLayerNorm(x[m]) (:315-329, cast-then-scale, same summation order as
// rmsnorm_row in elementwise.hip, so a row normalises to the same bits on any rank count).
// TP = compile-time rank count (0: run-time a.size): with it the peer loop unrolls and the tp-1 remote loads of a chunk are
// all in flight together — one fabric round trip per 16-byte chunk instead of one per (chunk, peer).
template <int TP>
__global__ __launch_bounds__(256) void tp_reduce_norm_kernel(ReduceArgs a) {
    const int m = a.r0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.r1) return;
    // consumer side of the hand-off (guide G16): the wait kernel saw every peer's counter, but THIS wave's caches may still
    // hold lines of the peers' buffers from the previous exchange
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    const int lane = threadIdx.x & 63;
    const int nchunk = a.d >> 3;
    u32x4 xv[MAXCH];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = lane + 64 * i;
        if (c >= nchunk) break;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        if (a.presum) {
            const u32x4 v = ((const u32x4*)(a.presum + (size_t)(m - a.r0) * a.d))[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] = __uint_as_float(v[e] << 16);
                acc[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
            }
        } else {
            if constexpr (TP > 0) {
                u32x4 pv[TP];
#pragma unroll
                for (int j = 0; j < TP; ++j)  // p.part[rank] is this rank's own buffer: one uniform load form, no branch
                    pv[j] = load_sys16(a.p.part[j], ((uint32_t)(m - a.src_row0[j]) * (uint32_t)a.d + c * 8) * 2u);
#pragma unroll
                for (int j = 0; j < TP; ++j)  // rank order: the sum is the same on whichever rank owns the row
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[2 * e] += __uint_as_float(pv[j][e] << 16);
                        acc[2 * e + 1] += __uint_as_float(pv[j][e] & 0xffff0000u);
                    }
            } else {
                for (int j = 0; j < a.size; ++j) {
                    const u32x4 v = (j == a.rank) ? ((const u32x4*)(a.part + (size_t)m * a.d))[c]
                                                  : load_sys16(a.p.part[j], ((uint32_t)(m - a.src_row0[j]) * (uint32_t)a.d + c * 8) * 2u);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[2 * e] += __uint_as_float(v[e] << 16);
                        acc[2 * e + 1] += __uint_as_float(v[e] & 0xffff0000u);
                    }
                }
            }
        }
        const u32x4 r = ((const u32x4*)(a.x + (size_t)m * a.d))[c];
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = bfround(__uint_as_float(r[e] << 16) + bfround(acc[2 * e]));
            const float hi = bfround(__uint_as_float(r[e] & 0xffff0000u) + bfround(acc[2 * e + 1]));
            ss += lo * lo;
            ss += hi * hi;
            o[e] = (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
        }
        xv[i] = o;
        ((u32x4*)(a.x + (size_t)m * a.d))[c] = o;
    }
    ss = wave_sum(ss);
    const float var = ss / (float)a.d;
    const float rs = 1.0f / sqrtf(var + a.eps);
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = lane + 64 * i;
        if (c >= nchunk) break;
        const u32x4 wv = ((const u32x4*)a.w)[c];
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(xv[i][e] << 16), hi = __uint_as_float(xv[i][e] & 0xffff0000u);
            const float wl = __uint_as_float(wv[e] << 16), wh = __uint_as_float(wv[e] & 0xffff0000u);
            o[e] = pack_bf2(wl * bfround(lo * rs), wh * bfround(hi * rs));
        }
        ((u32x4*)(a.hn_pub + (size_t)m * a.d))[c] = o;
        ((u32x4*)(a.xn + (size_t)m * a.d))[c] = o;
    }
    // producer side: the published row must have left this XCD's L2 before the counter that follows this kernel moves
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// rows [m0, m1) owned by other ranks: pull them from their owner's published buffer into dst (one wave per row)
__global__ __launch_bounds__(256) void tp_gather_kernel(TpPeers p, int rank, int m0, int m1, int slice, int d,
                                                        bf16_t* dst, int use_part) {
    const int m = m0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= m1) return;
    const int owner = (m - m0) / slice;
    if (owner == rank) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // see tp_reduce_norm_kernel
    // one row per wave: the owner IS wave-uniform, but it derives from threadIdx and the compiler cannot prove it — say so,
    // so that the buffer descriptor is built once in SGPRs (no per-lane waterfall loop around every load, guide T20)
    const int owner_u = __builtin_amdgcn_readfirstlane(owner);
    const bf16_t* src = use_part ? p.part[owner_u] : p.hn[owner_u];
    const int nchunk = d >> 3;
#pragma unroll 8
    for (int c = threadIdx.x & 63; c < nchunk; c += 64)
        ((u32x4*)(dst + (size_t)m * d))[c] = load_sys16(src, ((uint32_t)m * (uint32_t)d + c * 8) * 2u);
}

__global__ __launch_bounds__(256) void copy_rows_kernel(const bf16_t* src, bf16_t* dst, int r0, int r1, int d) {
    const int m = r0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= r1) return;
    for (int c = threadIdx.x & 63; c < (d >> 3); c += 64) ((u32x4*)(dst + (size_t)m * d))[c] = ((const u32x4*)(src + (size_t)m * d))[c];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // dst may be a published buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One wave on (at least) every XCD writes that XCD's L2 back: for partials that were NOT produced by a publishing kernel
// of this library (mmada_comm_exchange: the caller filled the buffer with its own kernels).  Workgroup b runs on XCD b % 8.
__global__ void tp_flush_kernel() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The emulated link (mode 5): one wave that does nothing for `ticks` of the device's constant-rate wall clock, counted from its
// own first read.  It stands where a transfer would sit — same stream, same dependencies — and occupies no CU while it sleeps
// beyond the one wave slot.  Bounded by construction: the loop ends on elapsed time, never on another agent, and the host caps
// `ticks` (link_wait_ticks).  No memory is touched, so it is capturable and leaves no state.
__global__ void tp_link_wait_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);  // 8 x 64 clocks: well under a microsecond per turn
}

// kHz of wall_clock64() on the current device (hipDeviceAttributeWallClockRate), asked once per device
int wall_clock_khz(int* out) {
    static std::atomic<int> khz[16];
    int dev = 0;
    MM_CHECK_HIP(hipGetDevice(&dev));
    int v = dev >= 0 && dev < 16 ? khz[dev].load(std::memory_order_relaxed) : 0;
    if (v <= 0) {
        MM_CHECK_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, dev));
        if (v <= 0) return mm_fail("emulated link: the device reports no wall clock rate");
        if (dev >= 0 && dev < 16) khz[dev].store(v, std::memory_order_relaxed);
    }
    *out = v;
    return 0;
}

// Ticks of one emulated phase over `rows` stream rows at `mbps`; refuses a wait beyond the cap (nothing is launched by this)
int link_wait_ticks(const TpComm* c, int rows, int mbps, long long* ticks) {
    const long long ns = link_wait_ns(rows, c->d, c->size, mbps);
    if (ns > LINK_WAIT_CAP_NS)
        return mm_fail("emulated link: one wait of %lld ns (%d rows x %d over %d ranks at tp_emulate_mbps=%d) exceeds the cap of %lld ns "
                       "(20 ms) per wait", ns, rows, c->d, c->size, mbps, LINK_WAIT_CAP_NS);
    int khz = 0;
    if (wall_clock_khz(&khz)) return 1;
    *ticks = (ns * khz + 999999) / 1000000;
    return 0;
}

int launch_link_wait(long long ticks, hipStream_t s) {
    hipLaunchKernelGGL(tp_link_wait_kernel, dim3(1), dim3(64), 0, s, ticks);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

long long default_timeout_ticks() {
    const char* e = getenv("MMADA_TP_TIMEOUT_S");
    const double sec = e ? atof(e) : 20.0;
    return (long long)(sec * 100e6);  // wall_clock64 runs at 100 MHz on gfx9
}

}  // namespace

int signal_wait(TpComm* c, hipStream_t s) {
    hipLaunchKernelGGL(tp_signal_kernel, dim3(1), dim3(1), 0, s, c->seq, c->ctr);
    hipLaunchKernelGGL(tp_wait_kernel, dim3(1), dim3(64), 0, s, c->seq, c->peers, c->size, c->rank, c->err, c->timeout);
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

namespace {

// The owner kernel over `own` rows; tp = the compile-time rank count to use (0, or a count without an instantiation: run-time a.size)
int launch_reduce_norm(const ReduceArgs& a, int own, int tp, hipStream_t s) {
    const dim3 grid((own + 3) / 4), blk(256);
    switch (tp) {
        case 2: hipLaunchKernelGGL(tp_reduce_norm_kernel<2>, grid, blk, 0, s, a); break;
        case 4: hipLaunchKernelGGL(tp_reduce_norm_kernel<4>, grid, blk, 0, s, a); break;
        case 8: hipLaunchKernelGGL(tp_reduce_norm_kernel<8>, grid, blk, 0, s, a); break;
        default: hipLaunchKernelGGL(tp_reduce_norm_kernel<0>, grid, blk, 0, s, a);
    }
    MM_CHECK_HIP(hipGetLastError());
    return 0;
}

// One exchange over rows [m0, m1): partial sums in c->part  ->  x (own rows), xn (all rows) ; on stream s
// emulate_mbps: the caller's snapshot of the "tp_emulate_mbps" switch (read in mode 5 only)
int exchange(mmada_handle* h, const Slice& sl, const bf16_t* norm_w, int emulate_mbps, hipStream_t s) {
    TpComm* c = h->tp;
    if (c->mode == TP_NONE) return mm_fail("tensor-parallel forward: no transport connected (mmada_comm_connect_ipc / _local / _rccl)");
    const int d = h->cfg.d_model, tp = c->size, own = sl.r1 - sl.r0;
    // emulated link: each half of the exchange is one timed wait where its transfer would sit (callers have checked the cap for
    // every slice before their first launch: emulated_waits_ok)
    long long wait_ticks = 0;
    if (c->mode == TP_EMULATE && link_wait_ticks(c, sl.m1 - sl.m0, emulate_mbps, &wait_ticks)) return 1;
    const bool mapped = peers_mapped(c);
    // RCCL: every rank contributes its `slice` rows (rows past M are pad rows of the buffers: never read by a GEMM)
    const size_t cnt = (size_t)sl.slice * d;
    ReduceArgs a{};
    a.p = c->peers; a.size = tp; a.rank = c->rank; a.nsrc = mapped ? tp : 1;
    a.part = c->part; a.x = h->x; a.w = norm_w; a.hn_pub = c->hn_pub; a.xn = h->xn;
    a.r0 = sl.r0; a.r1 = sl.r1; a.d = d; a.eps = h->cfg.rms_eps;
    // ---- reduce-scatter half: the sources of the owner kernel (pull: the peers' buffers as they are mapped) ----
    if (mapped && signal_wait(c, s)) return 1;  // every rank's partial of this chunk is complete
    if (c->mode == TP_COPY) {
        // the tp - 1 peer slices of MY rows -> local staging, by the copy engines; the kernel then sums local operands
        // (src_row0[j] = r0: staging row 0 of peer j is stream row r0)
        for (int j = 0; j < tp && own > 0; ++j) {
            if (j == c->rank) { a.p.part[j] = c->part; continue; }
            bf16_t* dst = c->stage + (size_t)j * c->stage_stride;
            MM_CHECK_HIP(hipMemcpyAsync(dst, c->peers.part[j] + (size_t)sl.r0 * d, (size_t)own * d * 2, hipMemcpyDefault, s));
            a.p.part[j] = dst;
            a.src_row0[j] = sl.r0;
        }
    } else if (c->mode == TP_RCCL) {
        ncclResult_t r = c->nccl.ReduceScatter(c->part + (size_t)sl.m0 * d, c->rs_tmp, cnt, ncclBfloat16, ncclSum, c->comm, s);
        if (r != ncclSuccess) return nccl_fail(c, "ncclReduceScatter", r);
        a.presum = c->rs_tmp;
    } else if (exchange_void(c)) {  // diagnostic: the forward without its exchange (bench.py: exposed exchange time = real - this)
        a.presum = c->part + (size_t)sl.r0 * d;
        if (c->mode == TP_EMULATE && launch_link_wait(wait_ticks, s)) return 1;  // where the pulls / copies / reduce-scatter sit
    }
    if (own > 0 && launch_reduce_norm(a, own, mapped ? tp : 0, s)) return 1;
    // ---- all-gather half ----
    if (mapped && signal_wait(c, s)) return 1;  // every owner's normalised rows are published
    if (c->mode == TP_PULL) {
        hipLaunchKernelGGL(tp_gather_kernel, dim3((sl.m1 - sl.m0 + 3) / 4), dim3(256), 0, s, c->peers, c->rank, sl.m0, sl.m1,
                           sl.slice, d, h->xn, 0);
        MM_CHECK_HIP(hipGetLastError());
    } else if (c->mode == TP_COPY) {  // tp - 1 copies, no kernel
        for (int j = 0; j < tp; ++j) {
            if (j == c->rank) continue;
            const int j0 = min(sl.m1, sl.m0 + j * sl.slice), j1 = min(sl.m1, j0 + sl.slice);
            if (j1 > j0)
                MM_CHECK_HIP(hipMemcpyAsync(h->xn + (size_t)j0 * d, c->peers.hn[j] + (size_t)j0 * d, (size_t)(j1 - j0) * d * 2,
                                            hipMemcpyDefault, s));
        }
    } else if (c->mode == TP_RCCL) {
        ncclResult_t r = c->nccl.AllGather(c->hn_pub + (size_t)(sl.m0 + c->rank * sl.slice) * d, h->xn + (size_t)sl.m0 * d, cnt,
                                           ncclBfloat16, c->comm, s);
        if (r != ncclSuccess) return nccl_fail(c, "ncclAllGather", r);
    } else if (c->mode == TP_EMULATE) {  // where the gather kernel / the copies / the all-gather sit
        if (launch_link_wait(wait_ticks, s)) return 1;
    }
    return 0;
}

// Mode 5, before the first launch of a forward / an exchange over M rows: every wait its slices ask for is within the cap
int emulated_waits_ok(const TpComm* c, const ChunkPlan& plan, int mbps) {
    long long ticks = 0;
    for (int k = 0; k < plan.n; ++k)
        if (link_wait_ticks(c, plan.sl[k].m1 - plan.sl[k].m0, mbps, &ticks)) return 1;
    return 0;
}

int load_rccl(RcclApi* api, const char* path) {
    if (api->dl) return 0;
    const char* cand[3] = {path && path[0] ? path : nullptr, "librccl.so", "librccl.so.1"};
    for (const char* p : cand) {
        if (!p) continue;
        api->dl = dlopen(p, RTLD_NOW | RTLD_GLOBAL);
        if (api->dl) break;
    }
    if (!api->dl) return mm_fail("RCCL: cannot dlopen librccl (%s)", dlerror());
#define LOAD(field, sym)                                                            \
    api->field = (decltype(api->field))dlsym(api->dl, sym);                        \
    if (!api->field) return mm_fail("RCCL: symbol %s missing", sym)
    LOAD(GetUniqueId, "ncclGetUniqueId");
    LOAD(CommInitRank, "ncclCommInitRank");
    LOAD(CommDestroy, "ncclCommDestroy");
    LOAD(ReduceScatter, "ncclReduceScatter");
    LOAD(AllGather, "ncclAllGather");
    LOAD(GetErrorString, "ncclGetErrorString");
#undef LOAD
    api->CommCount = (decltype(api->CommCount))dlsym(api->dl, "ncclCommCount");
    return 0;
}

// what a rank hands its peers (mmada_comm_create -> mmada_comm_connect_ipc): 4 x 64 B
struct CommExport { hipIpcMemHandle_t buf[PUB_COUNT]; };

// this rank's own published buffers, in export order
void own_pubs(const TpComm* c, void* buf[PUB_COUNT]) {
    buf[PUB_PART] = c->part; buf[PUB_HN] = c->hn_pub; buf[PUB_CTR] = c->ctr; buf[PUB_STATS] = c->stats_pub;
}

// mmada_comm_create behind its argument checks: fills the (empty) comm the handle already owns; on a failing exit the caller
// frees it with whatever was allocated up to there
int comm_init(mmada_handle* h, int max_rows, void* export_out) {
    TpComm* c = h->tp;
    c->rank = h->cfg.tp_rank; c->size = h->cfg.tp_size; c->d = h->cfg.d_model;
    c->max_rows = max_rows;
    const size_t rows = (size_t)max_rows + 8 * c->size;
    if (rows * (size_t)h->cfg.d_model * 2 >= (1ull << 32))
        return mm_fail("mmada_comm_create: %zu rows x %d exceed the 4 GiB the pull kernels address with 32-bit offsets", rows, h->cfg.d_model);
    const size_t bytes = rows * c->d * 2;
    // The hand-off counters and the 16-byte text records are read by other agents while their owner keeps writing them:
    // fine-grained (coherent) device memory when the runtime grants it.  The two bandwidth-critical buffers (partials,
    // normalised rows) stay ordinary allocations — a GEMM epilogue's 2-byte stores must combine in L2 — and are handed
    // over by the release / acquire fences of their producers and consumers; MMADA_TP_FINE_DATA=1 makes them fine-grained too.
    const char* fd_env = getenv("MMADA_TP_FINE_DATA");
    const bool fine_data_wanted = fd_env && fd_env[0] == '1';
    auto alloc_pub = [&](void** p, size_t n, bool want_fine, bool* fine) -> hipError_t {
        if (want_fine && hipExtMallocWithFlags(p, n, hipDeviceMallocFinegrained) == hipSuccess) {
            if (fine) *fine = true;
            return hipSuccess;
        }
        (void)hipGetLastError();
        if (fine) *fine = false;
        return hipMalloc(p, n);
    };
    bool fine_data = false;
    MM_CHECK_HIP(alloc_pub((void**)&c->part, bytes, fine_data_wanted, &fine_data));
    MM_CHECK_HIP(alloc_pub((void**)&c->hn_pub, bytes, fine_data_wanted, nullptr));
    MM_CHECK_HIP(hipMemset(c->part, 0, bytes));
    MM_CHECK_HIP(hipMemset(c->hn_pub, 0, bytes));
    // counters: [0] published sequence number, [64] private sequence number, [128] error flag — 4 KiB of their own
    MM_CHECK_HIP(alloc_pub((void**)&c->ctr, 4096, true, &c->ctr_fine));
    MM_CHECK_HIP(hipMemset(c->ctr, 0, 4096));
    c->seq = c->ctr + 64;
    c->err = (int*)(c->ctr + 128);
    c->data_fine = fine_data;
    MM_CHECK_HIP(hipMalloc(&c->rs_tmp, ((size_t)(max_rows + c->size - 1) / c->size + 16) * c->d * 2));
    c->stage_stride = ((size_t)(max_rows + c->size - 1) / c->size + 16) * c->d;   // one owner slice of the largest chunk
    c->stage = nullptr;  // the copy transport's landing zone: allocated by the first mmada_comm_set_mode(4)
    MM_CHECK_HIP(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    MM_CHECK_HIP(hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
    // the scoring head's record buffers are sized here, once: a call never allocates (and so never synchronises the host)
    c->score = score_layout(max_rows, h->cfg.vocab, c->size);
    if (c->score.total >= (1ull << 32)) return mm_fail("mmada_comm_create: %zu bytes of published records exceed 4 GiB", c->score.total);
    MM_CHECK_HIP(alloc_pub((void**)&c->stats_pub, c->score.total, true, nullptr));
    MM_CHECK_HIP(hipMemset(c->stats_pub, 0, c->score.total));
    for (int b = 0; b < 2; ++b) c->score_pub[b] = (char*)c->stats_pub + c->score.text_bytes + (size_t)b * c->score.buf_bytes;
    MM_CHECK_HIP(hipMalloc(&c->score_all, (size_t)c->size * c->score.buf_bytes));
    MM_CHECK_HIP(hipMalloc(&c->stats_all, (size_t)c->size * STAT_ROWS * sizeof(TextStat)));
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // the exchange must not queue behind a whole round of GEMM workgroups
    MM_CHECK_HIP(hipStreamCreateWithPriority(&c->sc, hipStreamNonBlocking, hi));
    for (int k = 0; k < TP_CHUNKS_MAX; ++k) {
        MM_CHECK_HIP(hipEventCreateWithFlags(&c->ev_g[k], hipEventDisableTiming));
        MM_CHECK_HIP(hipEventCreateWithFlags(&c->ev_c[k], hipEventDisableTiming));
    }
    const char* e = getenv("MMADA_TP_CHUNKS");
    c->chunks = normalise_chunks(e ? atoi(e) : 2);
    c->timeout = default_timeout_ticks();
    MM_CHECK_HIP(hipDeviceSynchronize());
    if (export_out) {
        CommExport ex;
        memset(&ex, 0, sizeof(ex));
        void* own[PUB_COUNT];
        own_pubs(c, own);
        for (int b = 0; b < PUB_COUNT; ++b) {
            const hipError_t e = hipIpcGetMemHandle(&ex.buf[b], own[b]);
            if (e == hipSuccess) continue;
            (void)hipGetLastError();
            memset(export_out, 0, sizeof(ex));
            return mm_fail("mmada_comm_create: hipIpcGetMemHandle failed (%s): peers in other processes cannot map this rank; "
                           "use mmada_comm_connect_rccl", hipGetErrorString(e));
        }
        memcpy(export_out, &ex, sizeof(ex));
    }
    return 0;
}

}  // namespace

// ---- forward ---------------------------------------------------------------------------------------------------------
// All blocks of a tensor-parallel forward.  h->x holds the embeddings (replicated), every rank keeps its own rows of the
// residual stream from here on.  Compute on `s`, exchanges on the library's second stream.
static int tp_forward_body_on(mmada_handle* h, hipStream_t s);

int tp_forward_body(mmada_handle* h, hipStream_t s_user) {
    TpComm* c = h->tp;
    if (!c || c->mode == TP_NONE) return mm_fail("tensor-parallel forward: no transport connected (mmada_comm_create + connect)");
    if (tp_forward_refused(h, h->res.B, h->res.Lp, h->res.cc != nullptr)) return 1;
    if (!c->s_cmp) return tp_forward_body_on(h, s_user);
    // CU partition: the blocks run on the library's masked compute stream, forked from and joined to the caller's stream
    MM_CHECK_HIP(hipEventRecord(c->ev_in, s_user));
    MM_CHECK_HIP(hipStreamWaitEvent(c->s_cmp, c->ev_in, 0));
    const int rc = tp_forward_body_on(h, c->s_cmp);
    MM_CHECK_HIP(hipEventRecord(c->ev_out, c->s_cmp));
    MM_CHECK_HIP(hipStreamWaitEvent(s_user, c->ev_out, 0));
    return rc;
}

static int tp_forward_body_on(mmada_handle* h, hipStream_t s) {
    TpComm* c = h->tp;
    if (h->res.M > c->max_rows) return mm_fail("tensor-parallel forward: %d rows exceed the comm buffers (%d)", h->res.M, c->max_rows);
    const int d = h->cfg.d_model, M = h->res.M, nl = h->cfg.n_layers;
    if ((d >> 3) > 64 * MAXCH) return mm_fail("tensor-parallel forward: d_model > %d is not supported", 64 * MAXCH * 8);
    const ChunkPlan plan = chunk_plan(c, h->res);
    c->fwd_chains = plan.chains;
    const int emulate_mbps = switches().tp_emulate_mbps;  // one snapshot for every exchange of this forward
    const double rows_real = (double)h->res.B * h->res.L / M;  // fraction of stream rows that are not padding (FLOP accounting)
    // first RMSNorm of the forward: the embeddings are replicated, no exchange needed
    if (h->res.xn_is_layer0) h->res.xn_is_layer0 = false;  // fused into the embedding kernel
    else if (launch_rmsnorm(h->x, h->layers[0].attn_norm, h->xn, M, d, h->cfg.rms_eps, s)) return 1;
    bool pending[TP_CHUNKS_MAX] = {};  // chunk k's xn rows are being produced on the exchange stream
    using ArgsOf = GemmArgs (*)(const mmada_handle*, int, int, int);  // handle.h: qkv_args, gate_up_args, attn_out_args, down_args
    // chunk k of a column-parallel GEMM (ProfScope kind `kind`): wait for the chunk's xn rows, multiply
    auto column_chunk = [&](int layer, int kind, int epi, ArgsOf args_of, int k) -> int {
        if (pending[k]) {
            MM_CHECK_HIP(hipStreamWaitEvent(s, c->ev_c[k], 0));
            pending[k] = false;
        }
        const GemmArgs g = args_of(h, layer, plan.sl[k].m0, plan.sl[k].m1 - plan.sl[k].m0);
        ProfScope p(h, layer, kind, 2.0 * g.M * rows_real * g.N * g.K, s);
        return launch_gemm(epi, g, s);
    };
    // chunk k of a row-parallel GEMM into c->part, then the chunk's exchange (RMSNorm weight w) on the exchange stream: it runs
    // under whatever the compute stream is given next
    auto row_chunk = [&](int layer, int kind, ArgsOf args_of, const bf16_t* w, int k) -> int {
        GemmArgs o = args_of(h, layer, plan.sl[k].m0, plan.sl[k].m1 - plan.sl[k].m0);
        o.C = c->part + (size_t)plan.sl[k].m0 * d; o.publish = peers_mapped(c);
        {
            ProfScope p(h, layer, kind, 2.0 * o.M * rows_real * o.N * o.K, s);
            if (launch_gemm(EPI_STORE, o, s)) return 1;
        }
        MM_CHECK_HIP(hipEventRecord(c->ev_g[k], s));
        MM_CHECK_HIP(hipStreamWaitEvent(c->sc, c->ev_g[k], 0));
        if (exchange(h, plan.sl[k], w, emulate_mbps, c->sc)) return 1;
        MM_CHECK_HIP(hipEventRecord(c->ev_c[k], c->sc));
        pending[k] = true;
        return 0;
    };
    auto column_parallel = [&](int layer, int kind, int epi, ArgsOf args_of) -> int {
        for (int k = 0; k < plan.n; ++k)
            if (column_chunk(layer, kind, epi, args_of, k)) return 1;
        return 0;
    };
    auto row_parallel = [&](int layer, int kind, ArgsOf args_of, const bf16_t* w) -> int {
        for (int k = 0; k < plan.n; ++k)
            if (row_chunk(layer, kind, args_of, w, k)) return 1;
        return 0;
    };
    // Write-after-read on the published buffers, for any number n of chunks or chains.  Three facts: (1) a rank's ev_c[k] completes
    // only behind the SECOND hand-off of that exchange on its exchange stream; (2) a peer signals a hand-off behind everything
    // earlier on ITS exchange stream — its reads included: the owner kernel (or the staging copies) reads part[] before the second
    // hand-off's signal, the gather (kernel or copies) reads hn_pub[] before the first signal of the peer's next exchange;
    // (3) every rank takes the same plan from the same inputs and issues its exchanges in one total order: per block c_0 .. c_n-1
    // after attn_out, then c_0 .. c_n-1 after down — the hand-off counters are a plain sequence number, so the i-th hand-off of one
    // rank only ever meets the i-th of another.
    //   part[c_k] is rewritten by the NEXT row-parallel GEMM of chunk k (down after attn_out, the next block's attn_out after
    //   down).  That GEMM follows, on the compute stream, the column-parallel GEMM of chunk k, which waited for ev_c[k]: by (1) this
    //   rank's second hand-off of the exchange has passed, i.e. every peer has signalled its second hand-off, by (2) behind its
    //   owner kernel's reads of part[c_k].  No peer reads part[c_k] again before its next first hand-off, which needs this rank's
    //   signal behind the rewriting GEMM (ev_g[k]).
    //   hn_pub[c_k] is rewritten by the owner kernel of chunk k's NEXT exchange on this rank's exchange stream, behind that
    //   exchange's first hand-off: every peer has signalled it, by (2) behind everything of its previous exchanges — the gather of
    //   chunk k's previous exchange among them, however many other chunks' exchanges lie between the two by (3).
    // Nothing in this depends on n or on where the chunk boundaries lie; the chains only change what the compute stream runs
    // between a chunk's two GEMMs.  The buffers of a rank's own device (xn, x, att, hbuf, q / k / vT) are ordered by ev_g / ev_c and
    // stream order; chain k's attention reads the keys and values of chain k's sequences only, written by its own QKV launch.
    for (int layer = 0; layer < nl; ++layer) {
        const bf16_t* next_norm = layer + 1 < nl ? h->layers[layer + 1].attn_norm : h->ln_f;
        if (plan.chains) {
            // sequence chains: chain k runs QKV -> attention of its sequences -> attn_out without a join; its exchange hides under
            // the chains that follow, and its gate/up waits for it only after every other chain's attention half was issued
            for (int k = 0; k < plan.n; ++k) {
                if (column_chunk(layer, 0, EPI_QKV, qkv_args, k)) return 1;
                if (block_attention(h, layer, s, 0, 0, plan.b0[k], plan.b1[k])) return 1;
                if (row_chunk(layer, 2, attn_out_args, h->layers[layer].ff_norm, k)) return 1;
            }
            for (int k = 0; k < plan.n; ++k) {
                if (column_chunk(layer, 3, EPI_SWIGLU, gate_up_args, k)) return 1;
                if (row_chunk(layer, 4, down_args, next_norm, k)) return 1;
            }
            continue;
        }
        // q/k/v (column-parallel: this rank's heads), RoPE in the epilogue; a dLLM cache step writes this rank's heads of the
        // block's keys / values into the slot
        if (column_parallel(layer, 0, EPI_QKV, qkv_args)) return 1;
        // attention over this rank's heads: the one join point (every key of a sequence)
        if (block_attention(h, layer, s)) return 1;
        if (row_parallel(layer, 2, attn_out_args, h->layers[layer].ff_norm)) return 1;
        // gate/up (column-parallel) + SiLU*mul, then down (row-parallel)
        if (column_parallel(layer, 3, EPI_SWIGLU, gate_up_args)) return 1;
        if (row_parallel(layer, 4, down_args, next_norm)) return 1;
    }
    for (int k = 0; k < plan.n; ++k)
        if (pending[k]) MM_CHECK_HIP(hipStreamWaitEvent(s, c->ev_c[k], 0));
    h->res.xn_is_final = true;  // xn = ln_f(x) on every row
    return 0;
}

// Residual stream of every owner -> full [M, d] (parity taps; the forward itself never moves the residual stream)
int tp_gather_stream(mmada_handle* h, bf16_t* full_out, hipStream_t s) {
    TpComm* c = h->tp;
    if (!transport_connected(c)) return mm_fail("tp_gather_stream: no transport connected (or the no-exchange diagnostic is on)");
    const int d = h->cfg.d_model;
    const ChunkPlan plan = chunk_plan(c, h->res);  // the owners of the forward that is resident
    if (plan.chains != c->fwd_chains)  // the plan depends on the transport: RCCL never runs sequence chains
        return mm_fail("tp_gather_stream: the transport was switched to or from RCCL since the resident forward ran; its rows have other owners");
    for (int k = 0; k < plan.n; ++k) {
        const Slice& sl = plan.sl[k];
        const int own = sl.r1 - sl.r0;
        if (own > 0) {
            hipLaunchKernelGGL(copy_rows_kernel, dim3((own + 3) / 4), dim3(256), 0, s, h->x, c->hn_pub, sl.r0, sl.r1, d);
            hipLaunchKernelGGL(copy_rows_kernel, dim3((own + 3) / 4), dim3(256), 0, s, h->x, full_out, sl.r0, sl.r1, d);
        }
        if (peers_mapped(c)) {
            if (signal_wait(c, s)) return 1;
            hipLaunchKernelGGL(tp_gather_kernel, dim3((sl.m1 - sl.m0 + 3) / 4), dim3(256), 0, s, c->peers, c->rank, sl.m0,
                               sl.m1, sl.slice, d, full_out, 0);
            if (signal_wait(c, s)) return 1;  // hn_pub may be overwritten only after every peer has pulled
        } else {
            ncclResult_t r = c->nccl.AllGather(c->hn_pub + (size_t)(sl.m0 + c->rank * sl.slice) * d,
                                               full_out + (size_t)sl.m0 * d, (size_t)sl.slice * d, ncclBfloat16, c->comm, s);
            if (r != ncclSuccess) return nccl_fail(c, "ncclAllGather", r);
        }
        MM_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

bool tp_comm_connected(const mmada_handle* h) { return h->tp && h->tp->mode != TP_NONE; }

int tp_forward_refused(const mmada_handle* h, int B, int Lp, bool cached) {
    const TpComm* c = h->tp;
    if (!c || c->mode != TP_EMULATE) return 0;
    return emulated_waits_ok(c, chunk_plan(c, B * Lp, B, Lp, cached), switches().tp_emulate_mbps);
}

void tp_comm_free(mmada_handle* h) {
    TpComm* c = h->tp;
    if (!c) return;
    for (int j = 0; j < TP_MAX; ++j)
        for (int b = 0; b < PUB_COUNT; ++b)
            if (c->opened[j][b]) (void)hipIpcCloseMemHandle(c->opened[j][b]);
    if (c->comm && c->nccl.CommDestroy) (void)c->nccl.CommDestroy(c->comm);
    for (int k = 0; k < TP_CHUNKS_MAX; ++k) {
        if (c->ev_g[k]) (void)hipEventDestroy(c->ev_g[k]);
        if (c->ev_c[k]) (void)hipEventDestroy(c->ev_c[k]);
    }
    if (c->sc) (void)hipStreamDestroy(c->sc);
    if (c->s_cmp) (void)hipStreamDestroy(c->s_cmp);
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    if (c->ev_out) (void)hipEventDestroy(c->ev_out);
    (void)hipFree(c->stage);
    (void)hipFree(c->part); (void)hipFree(c->hn_pub); (void)hipFree(c->ctr);
    (void)hipFree(c->rs_tmp); (void)hipFree(c->stats_pub); (void)hipFree(c->stats_all); (void)hipFree(c->head_buf);
    (void)hipFree(c->score_all);
    delete c;
    h->tp = nullptr;
}

extern "C" {

int mmada_comm_export_bytes(void) { return (int)sizeof(CommExport); }

int mmada_comm_create(mmada_handle* h, int max_rows, void* export_out) {
    if (!h || max_rows <= 0) return mm_fail("mmada_comm_create: bad argument");
    // tp_size == 1 behind mmada_set_option("tp_allow_single_rank", 1): a one-rank group runs EVERY line of the exchange (RCCL
    // reduce-scatter / all-gather of one rank are copies, the pull transport has no peer to wait for) and must reproduce the
    // plain forward bit for bit — the test that executes the RCCL transport without a second GPU (tests/test_gpu_tp.py)
    if ((h->cfg.tp_size < 2 && !(h->cfg.tp_size == 1 && switches().tp_allow_single_rank)) || h->cfg.tp_size > TP_MAX)
        return mm_fail("mmada_comm_create: tp_size must be 2..%d", TP_MAX);
    if (h->tp) tp_comm_free(h);
    h->tp = new TpComm();  // the handle owns it from here: a failing exit releases everything allocated so far (the error message stays)
    if (comm_init(h, max_rows, export_out)) {
        tp_comm_free(h);
        return 1;
    }
    return 0;
}

int mmada_comm_connect_ipc(mmada_handle* h, const void* exports) {
    if (!h || !h->tp || !exports) return mm_fail("mmada_comm_connect_ipc: call mmada_comm_create first");
    TpComm* c = h->tp;
    const CommExport* ex = (const CommExport*)exports;
    void* own[PUB_COUNT];
    own_pubs(c, own);
    for (int j = 0; j < c->size; ++j) {
        if (j == c->rank) { set_peer(c->peers, j, own); continue; }
        for (int b = 0; b < PUB_COUNT; ++b) {
            void* p = nullptr;
            hipError_t e = hipIpcOpenMemHandle(&p, ex[j].buf[b], hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return mm_fail("mmada_comm_connect_ipc: hipIpcOpenMemHandle(rank %d, buffer %d): %s", j, b, hipGetErrorString(e));
            }
            c->opened[j][b] = p;
        }
        set_peer(c->peers, j, c->opened[j]);
    }
    c->mode = TP_PULL;
    return 0;
}

int mmada_comm_connect_local(mmada_handle* h, mmada_handle* const* ranks) {
    if (!h || !h->tp || !ranks) return mm_fail("mmada_comm_connect_local: call mmada_comm_create first");
    TpComm* c = h->tp;
    for (int j = 0; j < c->size; ++j) {
        if (!ranks[j] || !ranks[j]->tp) return mm_fail("mmada_comm_connect_local: rank %d has no comm", j);
        if (ranks[j]->cfg.tp_rank != j) return mm_fail("mmada_comm_connect_local: handle %d is tp_rank %d", j, ranks[j]->cfg.tp_rank);
        void* theirs[PUB_COUNT];
        own_pubs(ranks[j]->tp, theirs);
        set_peer(c->peers, j, theirs);
    }
    c->mode = TP_PULL;
    return 0;
}

int mmada_comm_unique_id(void* out128, const char* librccl_path) {
    if (!out128) return mm_fail("mmada_comm_unique_id: null argument");
    static RcclApi api;
    if (load_rccl(&api, librccl_path)) return 1;
    ncclUniqueId id;
    ncclResult_t r = api.GetUniqueId(&id);
    if (r != ncclSuccess) return mm_fail("ncclGetUniqueId: %s", api.GetErrorString(r));
    memcpy(out128, &id, sizeof(id));
    return 0;
}

int mmada_comm_connect_rccl(mmada_handle* h, const void* unique_id128, const char* librccl_path) {
    if (!h || !h->tp || !unique_id128) return mm_fail("mmada_comm_connect_rccl: call mmada_comm_create first");
    TpComm* c = h->tp;
    if (load_rccl(&c->nccl, librccl_path)) return 1;
    ncclUniqueId id;
    memcpy(&id, unique_id128, sizeof(id));
    ncclResult_t r = c->nccl.CommInitRank(&c->comm, c->size, id, c->rank);
    if (r != ncclSuccess) return nccl_fail(c, "ncclCommInitRank", r);
    c->mode = TP_RCCL;
    MM_CHECK_HIP(hipMemset(c->err, 0, sizeof(int)));  // a failed attempt with the pull transport must not stick to this one
    return 0;
}

/* Hand-off timeout of the pull transport in seconds (<= 0: back to MMADA_TP_TIMEOUT_S / 20 s); also clears a sticky error.
 * A start-up self-test uses a short one so that a transport that cannot work is abandoned quickly. */
int mmada_comm_set_timeout(mmada_handle* h, double seconds) {
    if (!h || !h->tp) return mm_fail("mmada_comm_set_timeout: no comm");
    h->tp->timeout = seconds > 0 ? (long long)(seconds * 100e6) : default_timeout_ticks();
    MM_CHECK_HIP(hipDeviceSynchronize());
    MM_CHECK_HIP(hipMemset(h->tp->err, 0, sizeof(int)));
    return 0;
}

/* mode: 0 none, 1 pull (IPC / same-process peers), 2 RCCL, 4 copy engines, 3 the "no exchange" DIAGNOSTIC and 5 the emulated link on
 * top of it (the forward's values are void: callers that report results must treat 3 and 5 as an error — check_tp_exchange
 * does).  err: != 0 after a hand-off timed out (synchronises `stream`). */
int mmada_comm_status(mmada_handle* h, int* mode_out, int* err_out, int* finegrained_out, void* stream) {
    if (!h) return mm_fail("mmada_comm_status: null handle");
    if (mode_out) *mode_out = h->tp ? h->tp->mode : 0;
    if (finegrained_out) *finegrained_out = h->tp ? ((int)h->tp->ctr_fine | ((int)h->tp->data_fine << 1)) : 0;
    if (err_out) {
        *err_out = 0;
        if (h->tp) {
            MM_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
            MM_CHECK_HIP(hipStreamSynchronize(h->tp->sc));
            MM_CHECK_HIP(hipMemcpy(err_out, h->tp->err, sizeof(int), hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

int mmada_comm_set_mode(mmada_handle* h, int mode) {
    if (!h || !h->tp) return mm_fail("mmada_comm_set_mode: no comm");
    TpComm* c = h->tp;
    if (mode < TP_PULL || mode > TP_EMULATE)
        return mm_fail("mmada_comm_set_mode: mode must be 1 (pull), 2 (RCCL), 3 (diagnostic: no exchange), 4 (copy engines) or 5 (diagnostic: emulated link)");
    const int other = c->size == 1 ? 0 : (c->rank == 0 ? 1 : 0);
    if (mode == TP_PULL && !c->peers.ctr[other]) return mm_fail("mmada_comm_set_mode: the pull transport was never connected");
    if (mode == TP_RCCL && !c->comm) return mm_fail("mmada_comm_set_mode: the RCCL transport was never connected");
    if (mode == TP_NO_EXCHANGE && c->mode == TP_NONE) return mm_fail("mmada_comm_set_mode: connect a transport before the no-exchange diagnostic");
    if (mode == TP_EMULATE && c->mode == TP_NONE) return mm_fail("mmada_comm_set_mode: connect a transport before the emulated link");
    if (mode == TP_COPY && !c->peers.ctr[other]) return mm_fail("mmada_comm_set_mode: the copy transport needs the mapped peer buffers (connect_ipc / connect_local)");
    if (mode == TP_COPY && !c->stage) MM_CHECK_HIP(hipMalloc(&c->stage, c->stage_stride * c->size * 2));  // pull / RCCL users never pay for it
    c->mode = (TpMode)mode;
    return 0;
}

/* Ranks of the RCCL communicator this handle created (ncclCommCount), 0 when none was created. */
int mmada_comm_rccl_nranks(mmada_handle* h) {
    if (!h || !h->tp || !h->tp->comm) return 0;
    int n = 0;
    if (h->tp->nccl.CommCount && h->tp->nccl.CommCount(h->tp->comm, &n) == ncclSuccess) return n;
    return h->tp->size;  // a librccl without ncclCommCount: the size the communicator was initialised with
}

/* CU partition of the exchange (see the header comment): exchange_cus = 0 removes it; else the exchange stream is re-created on
 * `exchange_cus` CUs (a multiple of 8: the same number on every XCD) and the forward's compute kernels run on a library stream
 * masked to the remaining CUs.  Call between forwards (synchronises the device). */
int mmada_comm_set_partition(mmada_handle* h, int exchange_cus) {
    if (!h || !h->tp) return mm_fail("mmada_comm_set_partition: no comm");
    TpComm* c = h->tp;
    int dev = 0, ncu = 0;
    MM_CHECK_HIP(hipGetDevice(&dev));
    MM_CHECK_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    if (exchange_cus < 0 || exchange_cus % 8 || exchange_cus >= ncu)
        return mm_fail("mmada_comm_set_partition: exchange_cus=%d must be a multiple of 8 below the device's %d CUs", exchange_cus, ncu);
    MM_CHECK_HIP(hipDeviceSynchronize());
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (c->s_cmp) { (void)hipStreamDestroy(c->s_cmp); c->s_cmp = nullptr; }
    if (c->sc) { (void)hipStreamDestroy(c->sc); c->sc = nullptr; }
    c->part_cus = 0;
    // whatever happens below, the exchange keeps a usable stream: the un-partitioned one (high priority, non-blocking)
    MM_CHECK_HIP(hipStreamCreateWithPriority(&c->sc, hipStreamNonBlocking, hi));
    if (exchange_cus == 0) return 0;
    const int words = (ncu + 31) / 32;
    uint32_t mx[16] = {}, mc[16] = {};
    if (words > 16) return mm_fail("mmada_comm_set_partition: %d CUs exceed the mask buffer", ncu);
    for (int i = 0; i < ncu; ++i) (i < exchange_cus ? mx : mc)[i / 32] |= 1u << (i % 32);
    // hipExtStreamCreateWithCUMask takes no flags: both masked streams are BLOCKING, default-priority streams, i.e. implicitly
    // ordered against the legacy null stream.  A caller that drives the forward on the null stream (torch's default stream on
    // ROCm) therefore serialises with them and sees no overlap; pass a non-default stream while a partition is active
    // (bench.py and the probes do).  The partition is reported (mmada_comm_partition) only once BOTH streams exist.
    hipStream_t sx = nullptr, scmp = nullptr;
    hipError_t e = hipExtStreamCreateWithCUMask(&sx, words, mx);
    if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&scmp, words, mc);
    if (e != hipSuccess) {
        if (sx) (void)hipStreamDestroy(sx);
        return mm_fail("mmada_comm_set_partition: hipExtStreamCreateWithCUMask: %s (no partition in effect)", hipGetErrorString(e));
    }
    (void)hipStreamDestroy(c->sc);
    c->sc = sx;
    c->s_cmp = scmp;
    c->part_cus = exchange_cus;
    return 0;
}
int mmada_comm_partition(mmada_handle* h) { return h && h->tp ? h->tp->part_cus : 0; }
/* The library's exchange stream and (with a partition) masked compute stream, for probes that time kernels on them. */
int mmada_comm_streams(mmada_handle* h, void** exchange_out, void** compute_out) {
    if (!h || !h->tp) return mm_fail("mmada_comm_streams: no comm");
    if (exchange_out) *exchange_out = (void*)h->tp->sc;
    if (compute_out) *compute_out = (void*)h->tp->s_cmp;
    return 0;
}

void* mmada_comm_part_ptr(mmada_handle* h) { return h && h->tp ? (void*)h->tp->part : nullptr; }

/* One exchange over every row of the resident (B, L) carve, for probes and self-tests: the caller filled the partial
 * buffer (mmada_comm_part_ptr, [B*Lp, d]) and the residual stream; afterwards x holds own rows + sum and xn (debug buffer
 * 0) the RMSNorm of every row with norm_w (device bf16 [d]).  Runs on `stream` (no second stream, no chunking). */
int mmada_comm_exchange(mmada_handle* h, const void* norm_w, void* stream) {
    if (!h || !h->tp || !resident(h) || !norm_w) return mm_fail("mmada_comm_exchange: need a comm and a resident carve (mmada_embed)");
    const Slice sl = chunk_slice(h->res.M, h->tp->size, h->tp->rank, 1, 0);
    const int emulate_mbps = switches().tp_emulate_mbps;
    if (h->tp->mode == TP_EMULATE) {  // refuse a wait beyond the cap before anything is launched
        ChunkPlan one{};
        one.n = 1; one.sl[0] = sl;
        if (emulated_waits_ok(h->tp, one, emulate_mbps)) return 1;
    }
    h->res.xn_is_layer0 = false;  // xn is about to be overwritten
    if (peers_mapped(h->tp)) hipLaunchKernelGGL(tp_flush_kernel, dim3(256), dim3(64), 0, (hipStream_t)stream);
    return exchange(h, sl, (const bf16_t*)norm_w, emulate_mbps, (hipStream_t)stream);
}

int mmada_comm_destroy(mmada_handle* h) {
    if (h) tp_comm_free(h);
    return 0;
}

}  // extern "C"
