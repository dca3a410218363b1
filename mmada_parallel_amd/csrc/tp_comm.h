// tp_comm.h — state and small helpers shared by the two tensor-parallel units: tp_comm.hip (transports, the exchange, the
// forward) and tp_heads.hip (the vocabulary-parallel text head and row heads: scoring, top-k, the draw).  Private to them: every other unit sees the
// opaque `struct TpComm;` and the function declarations of handle.h only.
#pragma once
#include <rccl/rccl.h>

#include "handle.h"
#include "tp_plan.h"

constexpr int TP_MAX = 8;
constexpr int STAT_ROWS = 16384;   // text rows (B*T) a vocabulary-parallel select can take
constexpr int SCORE_ROUND = 1280;  // rows per round of the vocabulary-parallel scoring head: whole 320 / 256 / 160 / 128-row GEMM tiles
constexpr int SCORE_BN = 256;      // columns per record of EPI_ROWSTAT (row_heads.h: ROW_HEAD_BN)

// The values of the public header (mmada_comm_status / mmada_comm_set_mode) and of tp_link.py.
enum TpMode {
    TP_NONE = 0,         // buffers allocated, not connected
    TP_PULL = 1,         // pull over mapped peer buffers
    TP_RCCL = 2,
    TP_NO_EXCHANGE = 3,  // DIAGNOSTIC: owner-side kernel on this rank's own partial only (wrong values, timing only)
    TP_COPY = 4,         // copy engines over the mapped peer buffers (connected like pull)
    TP_EMULATE = 5,      // DIAGNOSTIC: mode 3's data path with a timed wait of bytes / link rate where each transfer would sit
};

// The four allocations a rank publishes to its peers, in the order of the export record (mmada_comm_create -> connect_ipc)
enum PubBuf { PUB_PART = 0, PUB_HN, PUB_CTR, PUB_STATS, PUB_COUNT };

struct TpPeers {  // passed to kernels by value
    const bf16_t* part[TP_MAX];
    const bf16_t* hn[TP_MAX];
    const uint32_t* ctr[TP_MAX];
    const TextStat* stats[TP_MAX];
};

struct RcclApi {
    void* dl = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;  // optional (reporting only)
};

// The published record allocation (stats_pub; one hipIpc handle covers it all): [STAT_ROWS] text records, then at text_bytes
// the scoring head's two record buffers of buf_bytes each, used alternately.  One buffer = `round` target logits (fp32),
// then at rec_off [tiles][ld] 16-byte tile records of this rank's tiles (ld = the round's rows, rounded up to 8), and right
// behind the records of the nt tiles the rank owns in THIS call — at score_extra_off(rec_off, nt, ld) — the head's extra
// records, [nt][ld] again: 32 bytes (top-k: the tile's eight keys) or 16 bytes (sampling: the tile's best triple), none for
// scoring.  What a peer needs of a round is therefore one contiguous range from the buffer's start.
constexpr uint32_t SCORE_EXTRA_MAX = 32;  // the larger extra record (row_heads.h: TOPK_MAX keys of 4 bytes)
struct ScoreLayout {
    int round;  // rows per round: min(SCORE_ROUND, ceil8(max_rows))
    int tiles;  // 256-column tiles a rank can own: ceil(ceil(vocab / 256) / size)
    size_t text_bytes, buf_bytes, total;
    uint32_t rec_off;
};
inline uint32_t score_extra_off(uint32_t rec_off, int nt, int ld) { return rec_off + (uint32_t)nt * (uint32_t)ld * 16u; }
inline ScoreLayout score_layout(int max_rows, int vocab, int size) {
    ScoreLayout l;
    l.round = min(SCORE_ROUND, (max_rows + 7) / 8 * 8);
    l.tiles = ((vocab + SCORE_BN - 1) / SCORE_BN + size - 1) / size;
    l.rec_off = (uint32_t)l.round * 4u;
    l.buf_bytes = align_up((size_t)l.rec_off + (size_t)l.tiles * l.round * (16 + SCORE_EXTRA_MAX), 256);
    l.text_bytes = (size_t)STAT_ROWS * sizeof(TextStat);
    l.total = l.text_bytes + 2 * l.buf_bytes;
    return l;
}

struct TpComm {
    TpMode mode = TP_NONE;
    int rank = 0, size = 1, max_rows = 0, d = 0;
    bf16_t* part = nullptr;    // [max_rows + 8*size, d]  published: this rank's partial of the row-parallel GEMM
    bf16_t* hn_pub = nullptr;  // [max_rows + 8*size, d]  published: normalised rows this rank owns (at their global row)
    uint32_t* ctr = nullptr;   // [16] published sequence counter (fine-grained memory when the runtime grants it)
    TextStat* stats_pub = nullptr;  // published: this rank's per-row record of the vocabulary-parallel text head + the score buffers
    TextStat* stats_all = nullptr;  // [size][STAT_ROWS] RCCL transport: all-gathered records
    // vocabulary-parallel scoring head (tp_head_logprobs)
    ScoreLayout score{};
    char* score_pub[2] = {nullptr, nullptr};  // the two published record buffers inside stats_pub's allocation
    char* score_all = nullptr;      // [size][score.buf_bytes] private: the peers' buffers as gathered (RCCL) / staged (copy)
    int score_flip = 0;             // the buffer the next round writes
    bf16_t* head_buf = nullptr;     // [head_rows, ceil(V/size)] this rank's logit slice (allocated at first use)
    size_t head_bytes = 0;
    uint32_t* seq = nullptr;   // [1]  private: number of hand-offs this rank has published
    int* err = nullptr;        // [1]  private: != 0 after a wait timed out (1 + the peer that never arrived)
    bool ctr_fine = false, data_fine = false;
    TpPeers peers{};
    void* opened[TP_MAX][PUB_COUNT] = {};  // hipIpc mappings of the peers' published buffers (closed by tp_comm_free)
    hipStream_t sc = nullptr;  // exchange stream
    hipStream_t s_cmp = nullptr;  // CU partition: compute stream masked to the CUs the exchange stream does not own (else null)
    int part_cus = 0;             // CUs of the exchange stream's mask (0: no partition)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    bf16_t* stage = nullptr;   // copy transport: [size][ceil(max_rows / size) + 16, d] peer slices of this rank's rows
    size_t stage_stride = 0;   // elements per peer
    hipEvent_t ev_g[TP_CHUNKS_MAX] = {}, ev_c[TP_CHUNKS_MAX] = {};  // per chunk: its row-parallel GEMM is done / its exchange is done
    int chunks = 2;            // 1, 2, 4 or 8: normalise_chunks(MMADA_TP_CHUNKS) at mmada_comm_create
    bool fwd_chains = false;   // the last forward ran a sequence-chain plan (tp_gather_stream must find the same owners)
    long long timeout = 0;     // hand-off timeout in wall_clock64 ticks (100 MHz)
    // RCCL
    RcclApi nccl;
    ncclComm_t comm = nullptr;
    bf16_t* rs_tmp = nullptr;  // [ceil(max_rows/size)+8, d]
};

// the peers' published buffers are mapped: hand-offs by counters, remote reads or copies
inline bool peers_mapped(const TpComm* c) { return c->mode == TP_PULL || c->mode == TP_COPY; }
// a transport that really exchanges is connected (not none, not the no-exchange diagnostic, not the emulated link)
inline bool transport_connected(const TpComm* c) {
    return c && c->mode != TP_NONE && c->mode != TP_NO_EXCHANGE && c->mode != TP_EMULATE;
}
// the timing-only modes: the owner kernel runs on this rank's own partial, nothing is handed off and no peer is touched
inline bool exchange_void(const TpComm* c) { return c->mode == TP_NO_EXCHANGE || c->mode == TP_EMULATE; }

// The emulated link (TP_EMULATE).  One phase of an exchange over `rows` stream rows — the reduce-scatter half or the all-gather
// half — moves ceil(rows / tp) * d bf16 values over each link (a full mesh, every peer's share on a link of its
// own), so it lasts that many bytes over `mbps` MB/s (10^6 bytes per second, per link and direction), rounded up to a whole
// nanosecond.  tp.link_wait_ns is the same arithmetic.  No single wait may exceed the cap: 20 MB at 76 GB/s is 0.26 ms.
constexpr long long LINK_WAIT_CAP_NS = 20 * 1000 * 1000;
inline long long link_wait_ns(int rows, int d, int tp, int mbps) {
    const long long bytes = (long long)((rows + tp - 1) / tp) * d * 2;
    return (bytes * 1000 + mbps - 1) / mbps;
}

// rank j's published buffers as this rank addresses them -> the table the kernels take
inline void set_peer(TpPeers& p, int j, void* const buf[PUB_COUNT]) {
    p.part[j] = (const bf16_t*)buf[PUB_PART]; p.hn[j] = (const bf16_t*)buf[PUB_HN];
    p.ctr[j] = (const uint32_t*)buf[PUB_CTR]; p.stats[j] = (const TextStat*)buf[PUB_STATS];
}

// 16 bytes of a peer's buffer at system scope (sc0 sc1: never served from this agent's caches) as ONE 16-byte request.
// A relaxed system-scope __hip_atomic_load lowers to an sc0 sc1 load only up to 8 bytes, and two of those per 16 bytes use
// half of every 64-byte fabric request each and ask for every line twice (round-2 review: 2x read amplification on xGMI).
// The buffer form carries the cache-policy bits in its aux operand (1 = sc0, 16 = sc1) and is counted by hipcc's own
// s_waitcnt bookkeeping, unlike an inline-asm load.  `base` must be wave-uniform (a kernel argument): the descriptor is
// built in SGPRs; the per-lane part is a 32-bit byte offset (mmada_comm_create refuses buffers of 4 GiB or more).
MM_DEVICE u32x4 load_sys16(const void* base, uint32_t byte_off) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0xffffffffu, 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 17);
}

// One hand-off on stream s: publish this rank's next sequence number, then wait (bounded) for every peer's (tp_comm.hip)
int signal_wait(TpComm* c, hipStream_t s);

inline int nccl_fail(TpComm* c, const char* what, ncclResult_t r) {
    return mm_fail("%s: %s", what, c->nccl.GetErrorString ? c->nccl.GetErrorString(r) : "RCCL error");
}

static_assert(TP_RCCL == PLAN_MODE_RCCL, "tp_plan.h names the RCCL mode by its value");
// the plan of a forward over M stream rows, B sequences of Lp rows each, on comm c in its current mode
inline ChunkPlan chunk_plan(const TpComm* c, int M, int B, int Lp, bool cached) {
    return chunk_plan_of(M, B, Lp, c->size, c->rank, c->chunks, c->mode, cached);
}
inline ChunkPlan chunk_plan(const TpComm* c, const Resident& r) { return chunk_plan(c, r.M, r.B, r.Lp, r.cc != nullptr); }
