"""Tensor-parallel shard plan of one LLaDA block (the slicing the bind-time repack kernels implement,
csrc/elementwise.hip pack_qkv/pack_gate_up/pack_cols) as plain index arithmetic, so it can be checked on CPU.

Megatron-style: q/k/v and ff_proj/up_proj are column-parallel (output-feature slices: whole heads / MLP columns),
attn_out and ff_out are row-parallel (input-feature slices).  Each rank produces a partial sum of the two
row-parallel outputs, rounded to bf16; the residual of row m is added by exactly one rank — its owner
`residual_owner(m, size)` = (m >> 4) % size, i.e. ownership rotates over the ranks in 16-row groups so every rank reads
1/size of the residual stream (csrc/gemm.hip EPI_RESID, GemmArgs::resid_mod/resid_rank) — so the sum over ranks of the
per-rank buffers IS the new residual stream (reference block: model/modeling_llada.py:906-972).
Because every rank rounds its partial to bf16 before the sum, TP=k results differ from TP=1 by bf16 rounding of the
partials (not bit-identical; the tolerance is stated in INTEGRATION.md and asserted in tests/test_gpu_model.py).
"""
from __future__ import annotations

from typing import Dict, Tuple


def residual_owner(row: int, size: int) -> int:
    """Rank whose row-parallel GEMM epilogue adds the residual of stream row `row` (16-row groups, round robin)."""
    return (row >> 4) % size


def head_range(n_heads: int, rank: int, size: int) -> Tuple[int, int]:
    if n_heads % size:
        raise ValueError(f"{n_heads} heads not divisible by tp_size {size}")
    per = n_heads // size
    return rank * per, (rank + 1) * per


def layer_shards(cfg: dict, rank: int, size: int) -> Dict[str, Tuple[int, slice]]:
    """name -> (dim, slice) of the checkpoint tensor `blocks.{i}.<name>.weight` kept by `rank`."""
    hd = cfg["d_model"] // cfg["n_heads"]
    n_kv = cfg.get("n_kv_heads") or cfg["n_heads"]
    F = cfg["mlp_hidden_size"]
    if F % size:
        raise ValueError("mlp_hidden_size not divisible by tp_size")
    q0, q1 = head_range(cfg["n_heads"], rank, size)
    k0, k1 = head_range(n_kv, rank, size)
    f0, f1 = rank * (F // size), (rank + 1) * (F // size)
    return {
        "q_proj": (0, slice(q0 * hd, q1 * hd)), "k_proj": (0, slice(k0 * hd, k1 * hd)),
        "v_proj": (0, slice(k0 * hd, k1 * hd)), "attn_out": (1, slice(q0 * hd, q1 * hd)),
        "ff_proj": (0, slice(f0, f1)), "up_proj": (0, slice(f0, f1)), "ff_out": (1, slice(f0, f1)),
    }


def shard_layer_weights(weights: dict, cfg: dict, rank: int, size: int) -> dict:
    """Apply layer_shards to a dict of full block tensors (norm weights are replicated)."""
    plan = layer_shards(cfg, rank, size)
    out = {}
    for name, w in weights.items():
        if name in plan:
            dim, sl = plan[name]
            out[name] = w[sl] if dim == 0 else w[:, sl]
        else:
            out[name] = w
    return out


# ---- the library's exchange step (csrc/tp_comm.hip) as plain index arithmetic --------------------------------------------
TP_CHUNKS_MAX = 8
MODE_RCCL = 2   # mmada_comm_status: the one transport that never runs sequence chains


def normalise_chunks(value: int) -> int:
    """What mmada_comm_create keeps of MMADA_TP_CHUNKS: 1 (<= 1), 2 (2, 3), 4 (4..7) or 8 (>= 8) — normalise_chunks in csrc/tp_plan.h."""
    return 1 if value <= 1 else 2 if value < 4 else 4 if value < 8 else 8


def _owner_split(m0: int, m1: int, size: int):
    return max(8, ((m1 - m0 + size - 1) // size + 7) // 8 * 8)


def runs_chains(n_chunks: int, batch, rccl: bool = False, cached: bool = False) -> bool:
    """True when a forward of batch = (B, Lp) runs SEQUENCE CHAINS: a count of 4 or 8, a plain forward (no dLLM-cache slot) of two
    or more sequences, any transport but RCCL (chunk_plan_of in csrc/tp_plan.h)."""
    return normalise_chunks(n_chunks) >= 4 and batch is not None and batch[0] >= 2 and not rccl and not cached


def chunk_slices(M: int, size: int, n_chunks: int = 2, *, batch=None, rccl: bool = False, cached: bool = False):
    """Row plan of one exchange over M stream rows: [(m0, m1, slice)] per chunk; inside a chunk rank r owns rows
    [min(m1, m0 + r*slice), min(m1, m0 + (r+1)*slice)).  Row chunks (n_chunks 1 or 2, and every case that does not run chains):
    every chunk but the last is a multiple of 8*size rows, so only the last one is padded (chunk_slice in csrc/tp_plan.h).
    batch = (B, Lp) with M == B * Lp and a count of 4 or 8 (runs_chains): min(count, B) chains of whole sequences,
    chain k = sequences [k*B // n, (k+1)*B // n), owners clipped to the chain."""
    if runs_chains(n_chunks, batch, rccl, cached):
        B, Lp = batch
        if M != B * Lp:
            raise ValueError(f"chunk_slices: M={M} is not B*Lp={B}*{Lp}")
        n = min(normalise_chunks(n_chunks), B)
        bounds = [(k * B // n * Lp, (k + 1) * B // n * Lp) for k in range(n)]
    else:
        unit = 8 * size
        if n_chunks >= 2 and M >= 4 * unit:
            first = (M // 2 + unit - 1) // unit * unit
            bounds = [(0, min(first, M)), (min(first, M), M)]
        else:
            bounds = [(0, M)]
    return [(m0, m1, _owner_split(m0, m1, size)) for m0, m1 in bounds]


def owned_rows(M: int, rank: int, size: int, n_chunks: int = 2, *, batch=None, rccl: bool = False, cached: bool = False):
    """Row ranges of the residual stream rank `rank` keeps (and normalises) — one per chunk (a trailing rank's may be empty)."""
    return [(min(m1, m0 + rank * sl), min(m1, m0 + (rank + 1) * sl))
            for m0, m1, sl in chunk_slices(M, size, n_chunks, batch=batch, rccl=rccl, cached=cached)]


def chunk_plan(B: int, Lp: int, tp: int, rank: int, chunks: int, transport_mode: int = 1, cached: bool = False):
    """chunk_plan_of (csrc/tp_plan.h) as Python, held to it by tests/test_tp_chains_host.py: [(m0, m1, slice, r0, r1, b0, b1)] per chunk of a forward over B sequences of Lp stream rows
    on rank `rank` of `tp`; [b0, b1) are the sequences whose attention runs with the chunk (a chain's own, else the whole batch)."""
    M, rccl = B * Lp, transport_mode == MODE_RCCL
    chains = runs_chains(chunks, (B, Lp), rccl, cached)
    out = []
    for m0, m1, sl in chunk_slices(M, tp, normalise_chunks(chunks), batch=(B, Lp), rccl=rccl, cached=cached):
        r0 = min(m1, m0 + rank * sl)
        out.append((m0, m1, sl, r0, min(m1, r0 + sl)) + ((m0 // Lp, m1 // Lp) if chains else (0, B)))
    return out


# ---- the emulated link (mmada_comm_set_mode 5, csrc/tp_comm.h link_wait_ns) ----------------------------------------------
LINK_WAIT_CAP_NS = 20_000_000   # the library refuses a single wait beyond 20 ms
DEFAULT_EMULATE_MBPS = 76000    # "tp_emulate_mbps" when neither mmada_set_option nor MMADA_TP_EMULATE_MBPS sets it


def link_wait_ns(rows: int, d: int, tp: int, mbps: int) -> int:
    """Nanoseconds one phase (the reduce-scatter half or the all-gather half) of an exchange over `rows` stream rows waits on the
    emulated link: ceil(rows / tp) * d bf16 values over one link at `mbps` MB/s (10^6 bytes per second), rounded up."""
    if rows < 0 or d < 1 or tp < 1 or mbps < 1:
        raise ValueError(f"link_wait_ns({rows}, {d}, {tp}, {mbps})")
    nbytes = (rows + tp - 1) // tp * d * 2
    return (nbytes * 1000 + mbps - 1) // mbps


def forward_link_waits_ns(M: int, d: int, tp: int, n_layers: int, mbps: int, n_chunks: int = 2, *, batch=None, rccl: bool = False,
                          cached: bool = False):
    """Every wait a forward over M stream rows asks of the emulated link, in launch order: per block two exchanges (after attn_out
    and after ff_out), per exchange and row chunk (chunk_slices; batch = (B, Lp) for the sequence chains of a count of 4 or 8) two
    phases.  sum() of it is the requested wait per forward."""
    per_exchange = [link_wait_ns(m1 - m0, d, tp, mbps)
                    for m0, m1, _ in chunk_slices(M, tp, n_chunks, batch=batch, rccl=rccl, cached=cached) for _phase in (0, 1)]
    return per_exchange * (2 * n_layers)


def vocab_slice(V: int, rank: int, size: int) -> Tuple[int, int]:
    """Columns of ff_out.weight rank `rank` multiplies in the vocabulary-parallel text head (mmada_text_select_tp)."""
    w = ((V + size - 1) // size + 7) // 8 * 8
    v0 = min(V, rank * w)
    return v0, min(V, v0 + w)


def score_tile_slice(n_cols: int, rank: int, size: int) -> Tuple[int, int]:
    """256-column tiles [t0, t1) of a scoring launch over `n_cols` columns that rank `rank` multiplies in the vocabulary-parallel
    scoring head (mmada_head_logprobs on a connected handle, tp_head_logprobs in csrc/tp_comm.hip): contiguous blocks of
    q = ceil(tiles / size) tiles, so a rank produces exactly the records the one-rank launch produces for its tiles.  The range
    of a trailing rank may be empty.  Tile t covers columns [col_begin + 256 t, min(col_end, col_begin + 256 (t + 1)))."""
    ntn = (n_cols + 255) // 256
    q = (ntn + size - 1) // size
    return min(ntn, rank * q), min(ntn, (rank + 1) * q)
