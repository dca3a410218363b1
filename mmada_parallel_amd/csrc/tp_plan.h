// tp_plan.h — the chunk plan of the tensor-parallel forward as plain host arithmetic: which stream rows form a chunk, which of them a
// rank owns, which sequences' attention runs with the chunk.  No device code and no dependency beyond the language, so that a
// host-only program can include it (tests/test_tp_chains_host.py does, to hold tp.py's mirror to it).  Included by tp_comm.h.
// The reference has no tensor parallelism: nothing here stands for a line of it.
#pragma once

constexpr int TP_CHUNKS_MAX = 8;     // row chunks / sequence chains of a forward in flight (MMADA_TP_CHUNKS)
constexpr int PLAN_MODE_RCCL = 2;    // mmada_comm_status: the one transport that never runs sequence chains (tp_comm.h: TP_RCCL)

inline int plan_min(int a, int b) { return a < b ? a : b; }
inline int plan_max(int a, int b) { return a > b ? a : b; }

struct Slice { int m0, m1, slice, r0, r1; };

// the owner split of rows [m0, m1): tp slices of a multiple of 8 rows, clipped to the chunk (a trailing rank may own nothing)
inline Slice owner_split(int m0, int m1, int tp, int rank) {
    Slice s;
    s.m0 = m0; s.m1 = m1;
    const int rows = m1 - m0;
    s.slice = plan_max(8, ((rows + tp - 1) / tp + 7) / 8 * 8);
    s.r0 = plan_min(s.m1, s.m0 + rank * s.slice);
    s.r1 = plan_min(s.m1, s.r0 + s.slice);
    return s;
}

// chunk k of `nch` (1 or 2) over M rows; every chunk but the last is a multiple of 8*tp rows, so only the last one is padded
inline Slice chunk_slice(int M, int tp, int rank, int nch, int k) {
    const int unit = 8 * tp;
    const int first = nch == 2 ? (M / 2 + unit - 1) / unit * unit : M;
    return owner_split(k == 0 ? 0 : plan_min(first, M), (k == nch - 1) ? M : plan_min(first, M), tp, rank);
}

// What MMADA_TP_CHUNKS asks for -> the chunk count a comm keeps: 1, 2, 4 or 8 (tp.normalise_chunks is the same table)
inline int normalise_chunks(int v) { return v <= 1 ? 1 : v < 4 ? 2 : v < 8 ? 4 : 8; }

// The row chunks of a forward.  Two kinds of plan:
//   row chunks (chains == false)  today's: one chunk, or two once M >= 4 * 8 * tp rows, cut on a multiple of 8 * tp rows whatever
//       sequence the boundary falls into; the attention joins the whole batch, [b0, b1) = [0, B) for every chunk.
//   sequence chains (chains == true)  a count of 4 or 8 on a plain forward (no dLLM-cache slot, M == B * Lp) of B >= 2 sequences over
//       any transport but RCCL (whose collectives pad every chunk to slice * tp rows: with chunks that are no multiple of 8 * tp
//       rows its all-gather would write into the next chunk's rows): n = min(count, B) chains, chain k = the whole sequences
//       [k * B / n, (k + 1) * B / n), i.e. rows [b0 * Lp, b1 * Lp); chain sizes differ by at most one sequence.  A sequence's
//       attention needs that sequence's keys only, so a chain runs through a whole block without a join with the others.
// Every consumer (the forward, its refusal check, tp_gather_stream) calls this with the same inputs; tp.chunk_plan is its mirror,
// held to it over a grid of shapes by tests/test_tp_chains_host.py, which compiles this header into a small host program.
struct ChunkPlan { int n; bool chains; Slice sl[TP_CHUNKS_MAX]; int b0[TP_CHUNKS_MAX], b1[TP_CHUNKS_MAX]; };
inline ChunkPlan chunk_plan_of(int M, int B, int Lp, int tp, int rank, int chunks, int mode, bool cached) {
    ChunkPlan p{};
    chunks = normalise_chunks(chunks);
    p.chains = chunks >= 4 && !cached && B >= 2 && M == B * Lp && mode != PLAN_MODE_RCCL;
    if (p.chains) {
        p.n = plan_min(chunks, B);
        for (int k = 0; k < p.n; ++k) {
            p.b0[k] = (int)((long long)k * B / p.n);
            p.b1[k] = (int)((long long)(k + 1) * B / p.n);
            p.sl[k] = owner_split(p.b0[k] * Lp, p.b1[k] * Lp, tp, rank);
        }
        return p;
    }
    p.n = (chunks >= 2 && M >= 4 * 8 * tp) ? 2 : 1;
    for (int k = 0; k < p.n; ++k) {
        p.sl[k] = chunk_slice(M, tp, rank, p.n, k);
        p.b0[k] = 0; p.b1[k] = B;
    }
    return p;
}
