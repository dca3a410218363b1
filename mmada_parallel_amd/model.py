"""Host-side mirror of the reference model contract, backed by libmmada_mi355x.so.

`LLaDAForMultiModalGeneration` keeps the surface `generate_ti2ti` / `inference.py` use:
    model = LLaDAForMultiModalGeneration.from_pretrained(path, torch_dtype=torch.bfloat16, device_map="auto")
    model(ids, infer=True, use_cache=False).logits        # [B, L, V] bf16
    model.config.text_vocab_size / codebook_size ; model.device
(reference: model/modeling_xllmx_dimoo.py:24-72, model/modeling_llada.py:1462-1511, inference.py:83-89).

Extra fast-path methods (`forward_body`, `head_rows`) let the accelerated sampler avoid materialising [L, V] logits.
PyTorch is used for device memory, streams and (TP) torch.distributed only.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import abi
from .tp_link import TpLink, TpLinkMixin

_SUPPORTED = dict(block_type="llama", activation_type="silu", layer_norm_type="rms")
# what the reference's ModelConfig assumes for a key that is absent from config.json (model/configuration_llada.py:147-317):
# a trimmed config must be read the way the reference would read it, not silently as the llama/silu/untied layout
_REFERENCE_DEFAULTS = dict(block_type="sequential", activation_type="swiglu", layer_norm_type="default", rope=False,
                           rope_full_precision=True, weight_tying=True, include_bias=False, alibi=False,
                           attention_layer_norm=False, scale_logits=False, input_emb_norm=False, include_qkv_bias=None,
                           rms_norm_eps=1e-5, rope_theta=10000.0, max_sequence_length=1024, mlp_ratio=4,
                           multi_query_attention=None, n_kv_heads=None)


class CausalLMOutputLite(SimpleNamespace):
    """Minimal stand-in for transformers' CausalLMOutputWithPast: only `.logits` is consumed on this path."""


class LLaDAConfigLite(SimpleNamespace):
    def get(self, k, default=None):
        return getattr(self, k, default)

    def ref(self, k):
        """Value of a ModelConfig field, falling back to the REFERENCE's default when the key is absent."""
        return getattr(self, k, _REFERENCE_DEFAULTS[k])


def effective_n_kv_heads(cfg: LLaDAConfigLite) -> int:
    """ModelConfig.effective_n_kv_heads (model/configuration_llada.py:366-384)."""
    n_kv, mqa = cfg.ref("n_kv_heads"), cfg.ref("multi_query_attention")
    if n_kv is None:
        return 1 if mqa is True else cfg.n_heads
    if mqa is None:
        return n_kv
    should = 1 if mqa else cfg.n_heads
    if n_kv != should:
        raise ValueError("You can't set `multi_query_attention` and `n_kv_heads` at the same time.")
    return should


def _validate(cfg: LLaDAConfigLite) -> None:
    def _name(v):
        return getattr(v, "value", v)

    for k, want in _SUPPORTED.items():
        got = _name(cfg.ref(k))
        if str(got) != want:
            how = "" if hasattr(cfg, k) else " (the reference's default for a key missing from the config)"
            raise NotImplementedError(f"config.{k}={got!r}{how}: only {want!r} is on the MI355X hot path")
    for flag in ("alibi", "attention_layer_norm", "scale_logits", "input_emb_norm", "include_bias", "include_qkv_bias"):
        if cfg.ref(flag):
            raise NotImplementedError(f"config.{flag}=True is not supported on the MI355X hot path")
    if not cfg.ref("rope") or not cfg.ref("rope_full_precision"):
        raise NotImplementedError("rope=True and rope_full_precision=True are required (reference default when the key "
                                  "is missing: rope=False)")
    if cfg.d_model // cfg.n_heads != 128:
        raise NotImplementedError("head_dim must be 128")


# special ids of the reference class (model/modeling_xllmx_dimoo.py:28-34)
IMAGE_START_TOKEN, IMAGE_END_TOKEN = 126349, 126350
ANSWER_START_TOKEN, ANSWER_END_TOKEN = 126354, 126355
BREAKLINE_TOKEN = 126084
IGNORE_INDEX = -100
TOPK_MAX = 8   # MMADA_TOPK_MAX (include/mmada_mi355x.h): entries the top-k head keeps per row


def pad_id_lists(input_ids, labels=None):
    """The reference's ragged-batch handling (model/modeling_xllmx_dimoo.py:56-59,80-81): id lists are padded with token 0,
    label lists with -100, to the longest.  Tensors pass through (every length = L).  Returns (ids [B, L] int64 CPU tensor or
    the given tensor, labels likewise or None, lengths list)."""
    if torch.is_tensor(input_ids):
        ids = input_ids.to(torch.long)
        lengths = [ids.shape[1]] * ids.shape[0]
    else:
        lengths = [len(e) for e in input_ids]
        L = max(lengths)
        ids = torch.tensor([list(e) + [0] * (L - len(e)) for e in input_ids], dtype=torch.long)
    if labels is None:
        return ids, None, lengths
    if torch.is_tensor(labels):
        lab = labels.to(torch.long)
    else:
        L = ids.shape[1]
        lab = torch.tensor([list(e) + [IGNORE_INDEX] * (L - len(e)) for e in labels], dtype=torch.long)
    if lab.shape != ids.shape:
        raise ValueError(f"labels {tuple(lab.shape)} do not match input_ids {tuple(ids.shape)}")
    return ids, lab, lengths


def loss_regions(unscaled_loss: torch.Tensor, input_ids: torch.Tensor, labels: torch.Tensor, lengths, t=None):
    """interleave / text / image loss of the reference from per-token losses (model/modeling_xllmx_dimoo.py:93-173), as tensor
    operations on whatever device the arguments live on.

    unscaled_loss [B, L] (0 where labels == -100; the reference's dtype is the logits': bf16), input_ids / labels [B, L] int64,
    lengths: the sequences' lengths before padding.  Regions, per sequence with an answer-start token (others contribute to
    the interleave loss only): the answer span runs from the first answer-start token to the first answer-end token behind it
    (else to the sequence's length).  With an image-start token inside the span and an image-end token anywhere behind it:
    image loss = every position strictly between the two that is not a break-line token (labelled or not), text loss = the
    labelled positions behind the image end inside the span; an image start without an end contributes nothing.  Without an
    image: text loss = the labelled positions of the span behind the answer-start token.  Each loss is the mean over its
    positions in (sequence, position) order — the order of the reference's lists — or 0.0 (fp32) when there are none;
    t: text_loss / t.mean().clamp(min=0.01) when any text position exists.
    Returns (interleave_loss, text_loss, image_loss), 0-dim tensors."""
    dev = unscaled_loss.device
    ids, lab = input_ids.to(dev), labels.to(dev)
    B, L = ids.shape
    pos = torch.arange(L, device=dev)[None, :]
    lens = torch.as_tensor(lengths, device=dev, dtype=torch.long)

    def first(cond):   # (any, index of the first True or L)
        return cond.any(1), torch.where(cond, pos, L).amin(1)

    valid = lab != IGNORE_INDEX
    has_as, a_start = first(ids == ANSWER_START_TOKEN)
    has_ae, a_end = first((ids == ANSWER_END_TOKEN) & (pos >= a_start[:, None]))
    a_end = torch.where(has_ae, a_end, lens)
    in_answer = (pos >= a_start[:, None]) & (pos < a_end[:, None])
    has_img, i_start = first((ids == IMAGE_START_TOKEN) & in_answer)
    has_ie, i_end = first((ids == IMAGE_END_TOKEN) & (pos >= i_start[:, None]))
    img_ok = has_as & has_img & has_ie
    image_mask = img_ok[:, None] & (pos > i_start[:, None]) & (pos < i_end[:, None]) & (ids != BREAKLINE_TOKEN)
    behind = torch.where(has_img[:, None], has_ie[:, None] & (pos > i_end[:, None]), pos > a_start[:, None])
    text_mask = has_as[:, None] & valid & behind & (pos < a_end[:, None])

    def mean_of(mask):
        sel = unscaled_loss[mask]
        return sel.mean() if sel.numel() else torch.tensor(0.0, device=dev)

    interleave_loss = mean_of(valid)
    text_loss, image_loss = mean_of(text_mask), mean_of(image_mask)
    if t is not None and bool(text_mask.any()):
        text_loss = text_loss / torch.as_tensor(t, device=dev).mean().clamp(min=0.01)
    return interleave_loss, text_loss, image_loss


@dataclass
class _Lane:
    """An activation context of the library with its workspace: lane 0 is the model's handle, lane 1 a clone over the same weights."""
    handle: C.c_void_p
    ws: Optional[torch.Tensor] = None
    ws_bytes: int = 0   # bytes registered with the library (the tensor is padded for alignment)


@dataclass
class _Resident:
    """What forward_body left in the lanes: None after a cached forward."""
    shape: Optional[tuple] = None      # (B, L)
    split: Optional[int] = None        # B0: lane 0 holds sequences [0, B0), lane 1 the rest; None = everything in lane 0
    consumed: Optional[tuple] = None   # the row window forward_body(consumed=...) declared


def equal_cut(n_rows: int, B: int, B0: int) -> int:
    """head_rows' way to find where lane 1's rows begin: the same number of rows per batch element — host arithmetic only."""
    if n_rows % B:
        raise ValueError("head_rows on a micro-batched forward needs an equal row count per batch element")
    return B0 * (n_rows // B)


def counted_cut(rows: torch.Tensor, base: int) -> int:
    """token_logprobs' way: count the rows below `base` = B0 * L (any count per batch element; synchronises the host)."""
    cut = int((rows < base).sum())
    if cut and cut < rows.numel() and not bool((rows[:cut] < base).all()):
        raise ValueError("token_logprobs on a micro-batched forward needs batch-major rows")
    return cut


def lane_calls(handles, n: int, cut: Optional[int], rows: Optional[torch.Tensor] = None, base: int = 0):
    """The per-lane calls of a read over `n` batch-major items: [(handle, lo, hi, rows of that lane)], [lo, hi) being the lane's
    share of the items and of the output.  cut None: lane 0 holds everything and `rows` passes through untouched.  Otherwise items
    [cut, n) live in lane 1, whose rows are re-based by `base` = B0 * L: the second micro-batch indexes its own batch from 0."""
    if cut is None:
        return [(handles[0], 0, n, rows)]
    if rows is None:
        return [(handles[0], 0, cut, None), (handles[1], cut, n, None)]
    return [(handles[0], 0, cut, rows[:cut]), (handles[1], cut, n, (rows[cut:] - base).contiguous())]


class LLaDAForMultiModalGeneration(TpLinkMixin):
    """MI355X-native drop-in for the reference class of the same name (inference and scoring; no backward pass).  The
    tensor-parallel link (init_tp_comm, comm_status, the probes, ...) is tp_link.TpLinkMixin."""

    MASK_TOKEN = 126336

    def __init__(self, config, state_dict: Dict[str, torch.Tensor], device: Optional[torch.device] = None,
                 tp_rank: int = 0, tp_size: int = 1, max_batch: int = 3, max_seq: Optional[int] = None):
        if isinstance(config, dict):
            config = LLaDAConfigLite(**config)
        _validate(config)
        if not torch.cuda.is_available():
            raise abi.MmadaError("LLaDAForMultiModalGeneration needs an MI355X (torch.cuda unavailable); "
                                 "there is no CPU fallback")
        self.config = config
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.dtype = torch.bfloat16
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self._lib = abi.lib()
        self._handle = C.c_void_p()
        self._lanes = [_Lane(self._handle)]  # lane 1 joins on first use (_lane)
        self._resident = _Resident()
        self._ws_epoch = 0       # bumped whenever a workspace is (re)allocated: captured step graphs hold its addresses
        self.graph_replays, self.graph_nodes = 0, {}  # hipGraph step replays issued / nodes per captured step kind
        self._link = TpLink()
        self._cache, self.use_cache = {}, False   # dLLM cache slots by `cat` / the blocks' use_cache flag (caching())
        self.n_kv_heads = effective_n_kv_heads(config)
        self.vocab = config.get("embedding_size") or config.vocab_size
        self.mlp_hidden = config.get("mlp_hidden_size") or config.ref("mlp_ratio") * config.d_model
        self.max_seq = max_seq or max(int(config.ref("max_sequence_length")), 4096)
        self.max_batch = max_batch

        c = abi.MmadaCfg(
            d_model=config.d_model, n_layers=config.n_layers, n_heads=config.n_heads, n_kv_heads=self.n_kv_heads,
            head_dim=128, mlp_hidden=self.mlp_hidden, vocab=self.vocab, max_seq=self.max_seq,
            rms_eps=float(config.ref("rms_norm_eps")), rope_theta=float(config.ref("rope_theta")),
            tp_rank=tp_rank, tp_size=tp_size, mask_token_id=int(config.get("mask_token_id", self.MASK_TOKEN)),
            text_vocab_size=int(config.get("text_vocab_size", 126356)),
            codebook_size=int(config.get("codebook_size", 8192)), reserved=0)
        # inv_freq exactly as RotaryEmbedding.get_rotary_embedding computes it (model/modeling_llada.py:391-393)
        inv_freq = 1.0 / (c.rope_theta ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))
        inv = (C.c_float * 64)(*inv_freq.tolist())
        with torch.cuda.device(self.device):
            abi.check(self._lib.mmada_create(C.byref(c), inv, C.byref(self._handle)), "mmada_create")
            self._bind(state_dict)

    # ---- loading ------------------------------------------------------------------------------------------------
    def _bind(self, sd: Dict[str, torch.Tensor]) -> None:
        p = "model.transformer."
        dev, dt = self.device, torch.bfloat16

        def get(name):
            if name not in sd:
                raise KeyError(f"checkpoint is missing {name}")
            return sd[name].to(device=dev, dtype=dt).contiguous()

        self._wte = get(p + "wte.weight")
        self._ln_f = get(p + "ln_f.weight")
        self._head = self._wte if self.config.ref("weight_tying") else get(p + "ff_out.weight")
        abi.check(self._lib.mmada_bind_globals(self._handle, self._wte.data_ptr(), self._ln_f.data_ptr(),
                                               self._head.data_ptr()), "mmada_bind_globals")
        st = abi.stream_ptr()
        for i in range(self.config.n_layers):
            b = f"{p}blocks.{i}."
            names = ["attn_norm", "ff_norm", "q_proj", "k_proj", "v_proj", "attn_out", "ff_proj", "up_proj", "ff_out"]
            ts = [get(b + n + ".weight") for n in names]
            abi.check(self._lib.mmada_bind_layer(self._handle, i, *[t.data_ptr() for t in ts], st), "mmada_bind_layer")
            torch.cuda.current_stream().synchronize()  # originals may be freed once the repack has drained
            del ts

    @classmethod
    def from_state_dict(cls, config, state_dict, **kw):
        return cls(config, state_dict, **kw)

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype=torch.bfloat16, device_map="auto", **kw):
        """Loads config.json + *.safetensors with the reference's state-dict keys (checkpoints drop in unchanged)."""
        from safetensors import safe_open

        if torch_dtype not in (None, torch.bfloat16):
            raise NotImplementedError("the MI355X hot path computes in bf16")
        with open(os.path.join(path, "config.json")) as f:
            config = LLaDAConfigLite(**json.load(f))
        files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {path}")

        class _Lazy(dict):
            def __init__(self):
                super().__init__()
                self._where = {}
                for fn in files:
                    with safe_open(os.path.join(path, fn), "pt") as sf:
                        for k in sf.keys():
                            self._where[k] = fn

            def __contains__(self, k):
                return k in self._where

            def __getitem__(self, k):
                with safe_open(os.path.join(path, self._where[k]), "pt") as sf:
                    return sf.get_tensor(k)

        return cls(config, _Lazy(), **kw)

    # ---- workspace ------------------------------------------------------------------------------------------------
    def _lane(self, lane: int) -> _Lane:
        if lane == len(self._lanes):   # the second activation context over the same weights
            h = C.c_void_p()
            abi.check(self._lib.mmada_clone_shared(self._handle, C.byref(h)), "mmada_clone_shared")
            self._lanes.append(_Lane(h))
        return self._lanes[lane]

    def _lane_handle(self, lane: int):
        return self._lane(lane).handle

    def _ensure_ws(self, B: int, L: int, lane: int = 0) -> None:
        ln = self._lane(lane)
        need = self._lib.mmada_workspace_bytes(ln.handle, B, L)
        if need > ln.ws_bytes:  # compare with what the LIBRARY was given, not with the padded tensor
            grow = max(need, self._lib.mmada_workspace_bytes(ln.handle, max(B, self.max_batch), L))
            ws = torch.empty(grow + 256, dtype=torch.uint8, device=self.device)
            base = (ws.data_ptr() + 255) // 256 * 256
            abi.check(self._lib.mmada_set_workspace(ln.handle, base, grow), "mmada_set_workspace")
            ln.ws, ln.ws_bytes = ws, grow
            self._ws_epoch += 1

    # the resident forward, as the tests and tools spell it.  Assigning _shape declares a plain forward of that shape resident
    # in lane 0 (what a caller that drives mmada_embed itself has to say before it reads the stream).
    _ws_bytes = property(lambda self: [ln.ws_bytes for ln in self._lanes])
    _shape = property(lambda self: self._resident.shape, lambda self, shape: setattr(self, "_resident", _Resident(shape)))
    _split = property(lambda self: self._resident.split, lambda self, split: setattr(self._resident, "split", split))

    def _lane_calls(self, n: int, cut: Optional[int], rows: Optional[torch.Tensor] = None):
        res = self._resident
        return lane_calls([ln.handle for ln in self._lanes], n, cut, rows, 0 if cut is None else res.split * res.shape[1])

    # ---- forward ---------------------------------------------------------------------------------------------------
    def forward_body(self, input_ids: torch.Tensor, consumed: Optional[tuple] = None) -> None:
        """Embedding + all blocks; the final residual stream stays resident for head_rows().

        consumed = (row_begin, row_end): the caller promises to read only rows [row_begin, row_end) of each sequence
        through head_rows(); the last block then skips the other rows (mmada_set_consumed_rows; bit-identical on the
        consumed rows).  None = every row.

        Tensor parallel (tp_size > 1): after each of the two row-parallel GEMMs of a block the partial residual
        stream is all-reduced over RCCL.  With B >= 2 the batch is split into two micro-batches living in two
        activation contexts over the same weights, and the all-reduce of one micro-batch is issued asynchronously
        so that it overlaps the other micro-batch's GEMMs / attention."""
        ids = input_ids.to(device=self.device, dtype=torch.long).contiguous()
        B, L = ids.shape
        st = abi.stream_ptr()
        in_lib = self.tp_size > 1 and self._comm_in_library
        microbatch = B >= 2 and not in_lib and (self.tp_size > 1 or os.environ.get("MMADA_MICROBATCH") == "1")
        lo, hi = (int(consumed[0]), int(consumed[1])) if consumed is not None else (0, 0)
        if consumed is not None and not 0 <= lo < hi <= L:
            raise ValueError(f"consumed rows {consumed} outside [0, {L})")
        self._resident = _Resident((B, L), (B + 1) // 2 if microbatch else None, (lo, hi) if consumed is not None else None)
        for lane in ((0, 1) if microbatch else (0,)):
            abi.check(self._lib.mmada_set_consumed_rows(self._lane_handle(lane), lo, hi), "mmada_set_consumed_rows")
        if not microbatch:
            self._ensure_ws(B, L)
            if self.tp_size == 1 or in_lib:
                # tp_size > 1: the reduce-scatter / RMSNorm / all-gather exchanges are issued by the library (tp_comm.hip)
                if in_lib and B * ((L + 7) // 8 * 8) > self._comm_rows:
                    raise abi.MmadaError(f"forward of {B}x{L} exceeds the {self._comm_rows} rows init_tp_comm() was sized for")
                abi.check(self._lib.mmada_forward_body(self._handle, ids.data_ptr(), B, L, st), "mmada_forward_body")
            else:
                import torch.distributed as dist

                abi.check(self._lib.mmada_embed(self._handle, ids.data_ptr(), B, L, st), "mmada_embed")
                for i in range(self.config.n_layers):
                    for seg in (self._lib.mmada_attn_partial, self._lib.mmada_mlp_partial):
                        abi.check(seg(self._handle, i, st), "mmada_*_partial")
                        dist.all_reduce(self._stream_view())
        else:
            import torch.distributed as dist

            reduce = dist.is_available() and dist.is_initialized()
            B0 = self._resident.split
            parts = [ids[:B0].contiguous(), ids[B0:].contiguous()]
            handles = [self._lane_handle(0), self._lane_handle(1)]
            for j in (0, 1):
                self._ensure_ws(parts[j].shape[0], L, lane=j)
                abi.check(self._lib.mmada_embed(handles[j], parts[j].data_ptr(), parts[j].shape[0], L, st), "mmada_embed")
            pending = [None, None]
            for i in range(self.config.n_layers):
                for seg in (self._lib.mmada_attn_partial, self._lib.mmada_mlp_partial):
                    for j in (0, 1):
                        if pending[j] is not None:
                            pending[j].wait()  # this lane's previous all-reduce (ran under the other lane's kernels)
                            pending[j] = None
                        abi.check(seg(handles[j], i, st), "mmada_*_partial")
                        if reduce:
                            pending[j] = dist.all_reduce(self._stream_view(j), async_op=True)
            for j in (0, 1):
                if pending[j] is not None:
                    pending[j].wait()

    def _stream_view(self, lane: int = 0) -> torch.Tensor:
        """Torch view of the library's current residual-stream buffer (inside our workspace tensor)."""
        ln = self._lane(lane)
        p = self._lib.mmada_stream_ptr(ln.handle)
        n = self._lib.mmada_stream_bytes(ln.handle)
        off = p - ln.ws.data_ptr()
        return ln.ws[off:off + n].view(torch.bfloat16)

    def head_rows(self, rows: torch.Tensor, col_begin: int, col_end: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits[r] = lm_head[col_begin:col_end] · ln_f(x[rows[r]]), rows = b*L + l (int32, device).

        `rows` must be batch-major with the same number of rows per batch element (what generate_ti2ti builds).
        `out` (bf16 [R, col_end - col_begin], contiguous): write there instead of allocating (fixed address: capturable)."""
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        res = self._resident
        if os.environ.get("MMADA_CHECK_ROWS") == "1" and res.consumed is not None and rows.numel():
            l = rows % res.shape[1]  # debug aid (forces a device sync): rows must lie inside the declared window
            assert int(l.min()) >= res.consumed[0] and int(l.max()) < res.consumed[1], "head_rows outside forward_body(consumed=...)"
        if out is None:
            out = torch.empty((rows.numel(), col_end - col_begin), dtype=torch.bfloat16, device=self.device)
        elif out.shape != (rows.numel(), col_end - col_begin) or out.dtype != torch.bfloat16 or not out.is_contiguous():
            raise ValueError("head_rows(out=...): need a contiguous bf16 [rows, col_end - col_begin] tensor")
        st = abi.stream_ptr()
        cut = None if res.split is None else equal_cut(rows.numel(), res.shape[0], res.split)
        for handle, lo, hi, r in self._lane_calls(rows.numel(), cut, rows):
            abi.check(self._lib.mmada_head_rows(handle, r.data_ptr(), hi - lo, col_begin, col_end,
                                                out.data_ptr() if lo == 0 else out[lo:].data_ptr(), st), "mmada_head_rows")
        return out

    _TP_SCORE = ("scoring under tensor parallelism needs the library's exchange (init_tp_comm): a vocabulary-parallel score is the "
                 "same records exchanged as in mmada_text_select_tp, which the host all-reduce fallback does not carry")

    def _refuse_tp_score(self):
        if self.tp_size != 1 and not self._comm_in_library:
            raise NotImplementedError(self._TP_SCORE)

    def token_logprobs(self, rows: torch.Tensor, targets: torch.Tensor, col_begin: int = 0, col_end: Optional[int] = None,
                       return_stats: bool = False):
        """log softmax(logits[rows[r], col_begin:col_end])[targets[r]] as fp32 [R], after forward_body(), without materialising
        the logits (mmada_head_logprobs: the head GEMM reduces its tiles to row statistics in the epilogue).

        rows = b*L + l (batch-major); targets = column in the WHOLE vocabulary, < 0: ignored (0.0), outside the column range:
        -inf.  return_stats: also (lse fp32, argmax int32 — column in the whole vocabulary, first maximum —, max fp32).

        Under tensor parallelism with the library's exchange connected (init_tp_comm) every rank must make the call: each
        multiplies its block of the launch's 256-column tiles (tp.score_tile_slice), the records are exchanged and every rank
        returns the same bits — those of a one-rank handle on the same normalised rows.  The call never synchronises the host."""
        self._refuse_tp_score()
        col_end = self.vocab if col_end is None else col_end
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        targets = targets.to(device=self.device, dtype=torch.long).contiguous()
        R = rows.numel()
        if targets.numel() != R:
            raise ValueError("token_logprobs: one target per row")
        lp = torch.empty(R, dtype=torch.float32, device=self.device)
        stats = (torch.empty(R, dtype=torch.float32, device=self.device), torch.empty(R, dtype=torch.int32, device=self.device),
                 torch.empty(R, dtype=torch.float32, device=self.device)) if return_stats else None
        res = self._resident   # micro-batched forward: any row count per batch element, so the cut is counted
        cut = None if res.split is None else counted_cut(rows, res.split * res.shape[1])
        for handle, lo, hi, row_t in self._lane_calls(R, cut, rows):
            if hi > lo:
                ptrs = [t_[lo:hi].data_ptr() for t_ in (targets, lp) + (stats or ())] + [None] * (0 if stats else 3)
                abi.check(self._lib.mmada_head_logprobs(handle, row_t.data_ptr(), hi - lo, col_begin, col_end, *ptrs,
                                                        abi.stream_ptr()), "mmada_head_logprobs")
        return (lp, *stats) if return_stats else lp

    def vocab_parallel_row_heads(self) -> bool:
        """top_logprobs / sample_tokens (and the generators' device samplers) run their vocabulary-parallel form: a group of two or
        more ranks whose exchange runs in the library over a mapped transport.  Every rank must then make the same calls."""
        return self.tp_size >= 2 and self._comm_in_library and self.tp_collective in ("pull", "copy")

    _TP_TOPK = ("top_logprobs runs on one rank: the library's top-k head (mmada_head_topk) refuses a tensor-parallel handle; the "
                "vocabulary-parallel top-k, whose key records would ride the score exchange, is a follow-up")

    def top_logprobs(self, rows: torch.Tensor, k: int, col_begin: int = 0, col_end: Optional[int] = None):
        """The k likeliest columns of logits[rows[r], col_begin:col_end] after forward_body(), without materialising the logits
        (mmada_head_topk: the scoring head's GEMM also keeps every 256-column tile's eight best).  Returns (ids int32 [R, k] —
        column in the WHOLE vocabulary —, logprobs fp32 [R, k], lse fp32 [R]); 1 <= k <= 8, k <= col_end - col_begin.

        Order of a row: logit descending, then column ascending (a stable descending sort).  logprobs = logit - lse in fp32, the
        expression of token_logprobs: top_logprobs(rows, k)[1][:, j] equals token_logprobs(rows, ids[:, j]) bit for bit, and lse,
        ids[:, 0] are its lse / argmax.  rows as in token_logprobs (batch-major on a micro-batched forward).

        One rank, or a tensor-parallel group of two or more ranks with the library's exchange connected over the pull or the copy
        transport: every rank must make the call, the tiles' key records ride the score exchange of token_logprobs and every rank
        returns the same bits — those of a one-rank handle on the same normalised rows.  The call never synchronises the host."""
        if (self.tp_size != 1 or self._comm_in_library) and not self.vocab_parallel_row_heads():
            raise NotImplementedError(self._TP_TOPK)
        col_end = self.vocab if col_end is None else col_end
        if not 1 <= k <= TOPK_MAX or k > col_end - col_begin:
            raise ValueError(f"top_logprobs: k={k} outside [1, min({TOPK_MAX}, col_end - col_begin)]")
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        R = rows.numel()
        ids = torch.empty((R, k), dtype=torch.int32, device=self.device)
        logit = torch.empty((R, k), dtype=torch.float32, device=self.device)
        lse = torch.empty(R, dtype=torch.float32, device=self.device)
        res = self._resident
        cut = None if res.split is None else counted_cut(rows, res.split * res.shape[1])
        for handle, lo, hi, row_t in self._lane_calls(R, cut, rows):
            if hi > lo:
                abi.check(self._lib.mmada_head_topk(handle, row_t.data_ptr(), hi - lo, col_begin, col_end, k, ids[lo:hi].data_ptr(),
                                                    logit[lo:hi].data_ptr(), lse[lo:hi].data_ptr(), abi.stream_ptr()), "mmada_head_topk")
        return ids, logit - lse[:, None], lse

    _TP_SAMPLE = ("sample_tokens runs on one rank: the library's sampling head (mmada_head_sample) refuses a tensor-parallel handle; "
                  "the vocabulary-parallel draw, whose key records would ride the score exchange, is a follow-up")
    _LANES_SAMPLE = ("sample_tokens on a forward resident in micro-batched lanes: the noise is indexed by the row's index inside "
                     "the library call, which would restart per lane; run the forward without MMADA_MICROBATCH")

    @property
    def sample_counter(self) -> torch.Tensor:
        """The model's own draw counter (int64 [1] on the device, created at 0 on first use): sample_tokens reads it and the
        library adds 1 per call."""
        if getattr(self, "_sample_counter", None) is None:
            self._sample_counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        return self._sample_counter

    def sample_tokens(self, rows: torch.Tensor, temperature: float, col_begin: int = 0, col_end: Optional[int] = None, *,
                      seed: int, counter: Optional[torch.Tensor] = None, return_stats: bool = False):
        """One token per row drawn from softmax(logits[rows[r], col_begin:col_end] / temperature) after forward_body(), without
        materialising the logits or a noise tensor (mmada_head_sample: a Gumbel-max draw in the head GEMM's epilogue).  Returns
        (ids int32 [R] — column in the WHOLE vocabulary —, logprobs fp32 [R], lse fp32 [R]) and, with return_stats, argmax int32 and
        max fp32 as well.

        logprobs is the unperturbed log-probability of the drawn token: token_logprobs(rows, ids) bit for bit; lse / argmax / max
        are its return_stats values.  temperature is finite and >= 0; at 0 the draw is the arg-max.  The noise is a pure function of (seed,
        counter, r, column) — r the row's index in `rows` — so a call is reproducible: `counter` (int64 [1] on the device, default
        the model's own, `sample_counter`) is read by the call and incremented by 1 on the device; reset it to repeat a draw.
        The draws do not reproduce torch's RNG stream.  Not on a micro-batched forward.

        One rank, or a tensor-parallel group as in top_logprobs: every rank must make the same calls with the same seed; each
        rank's counter lives on that rank and advances alike, and every rank draws the same ids."""
        if (self.tp_size != 1 or self._comm_in_library) and not self.vocab_parallel_row_heads():
            raise NotImplementedError(self._TP_SAMPLE)
        if self._resident.split is not None:
            raise NotImplementedError(self._LANES_SAMPLE)
        if not 0 <= temperature < float("inf"):
            raise ValueError(f"sample_tokens: temperature {temperature} is not a finite value >= 0")
        counter = self.sample_counter if counter is None else counter
        if counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != self.device:
            raise ValueError("sample_tokens: counter must be an int64 [1] tensor on the model's device")
        col_end = self.vocab if col_end is None else col_end
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        R = rows.numel()
        ids = torch.empty(R, dtype=torch.int32, device=self.device)
        lp, lse = (torch.empty(R, dtype=torch.float32, device=self.device) for _ in range(2))
        stats = (torch.empty(R, dtype=torch.int32, device=self.device), torch.empty(R, dtype=torch.float32, device=self.device)) if return_stats else ()
        abi.check(self._lib.mmada_head_sample(self._handle, rows.data_ptr(), R, col_begin, col_end, float(temperature),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, counter.data_ptr(), ids.data_ptr(), lp.data_ptr(),
                                              lse.data_ptr(), *[t_.data_ptr() for t_ in stats], *([None] * (2 - len(stats))),
                                              abi.stream_ptr()), "mmada_head_sample")
        return (ids, lp, lse, *stats)

    def score(self, input_ids: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """Per-token negative log-likelihood, fp32 [B, L]: -log softmax(logits[b, l])[labels[b, l]], 0 where labels == -100 —
        F.cross_entropy(logits.view(-1, V), labels.view(-1), ignore_index=-100, reduction='none') of the reference
        (model/modeling_xllmx_dimoo.py:86-91) in fp32.  One forward_body plus one token_logprobs over the labelled rows.

        The labelled-row list (the one host synchronisation) is built BEFORE the forward: between the first launch of the
        forward and the last of the join nothing waits for the device, which a tensor-parallel rank group needs (a rank's
        hand-off spins until its peers' launches arrive)."""
        self._refuse_tp_score()
        ids = input_ids.to(device=self.device, dtype=torch.long)
        lab = labels.to(device=self.device, dtype=torch.long)
        if lab.shape != ids.shape:
            raise ValueError(f"labels {tuple(lab.shape)} do not match input_ids {tuple(ids.shape)}")
        if bool((lab >= self.vocab).any()):
            raise ValueError("labels outside the vocabulary")
        out = torch.zeros(ids.shape, dtype=torch.float32, device=self.device)
        flat = lab.reshape(-1)
        rows = (flat != IGNORE_INDEX).nonzero().flatten()
        self.forward_body(ids)
        if rows.numel():
            out.view(-1)[rows] = -self.token_logprobs(rows.to(torch.int32), flat[rows])
        return out

    def hidden_state(self) -> torch.Tensor:
        """Residual stream after the last block, [B, L, d] (parity tap)."""
        B, L = self._shape
        out = torch.empty((B, L, self.config.d_model), dtype=torch.bfloat16, device=self.device)
        for handle, b0, _, _ in self._lane_calls(B, self._resident.split):   # the items are the batch's sequences
            abi.check(self._lib.mmada_read_stream(handle, out[b0:].data_ptr(), abi.stream_ptr()), "mmada_read_stream")
        return out

    def debug_buffer(self, which: int) -> torch.Tensor:
        """Parity tap (tests only): flat bf16 view of an intermediate of the most recent block, see mmada_debug_buffer."""
        p, lp, lkv = C.c_void_p(), C.c_int32(), C.c_int32()
        abi.check(self._lib.mmada_debug_buffer(self._handle, which, C.byref(p), C.byref(lp), C.byref(lkv)), "debug_buffer")
        B, L = self._shape
        d, F = self.config.d_model, self.mlp_hidden // self.tp_size
        hq, hkv = self.config.n_heads // self.tp_size, self.n_kv_heads // self.tp_size
        shapes = {0: (B * lp.value, d), 1: (B, hq, lkv.value, 128), 2: (B, hkv, lkv.value, 128),
                  3: (B, hkv, 128, lkv.value), 4: (B * lp.value, hq * 128), 5: (B * lp.value, F)}
        shape = shapes[which]
        n = 2
        for v in shape:
            n *= v
        ws = self._lanes[0].ws
        off = p.value - ws.data_ptr()
        t = ws[off:off + n].view(torch.bfloat16).view(*shape)
        if which == 3:  # undo the [0,4,1,5,2,6,3,7] chunk order of every 32-key block (csrc/common.h vt_key_pos)
            t = t.reshape(B, hkv, 128, lkv.value // 32, 8, 4)[..., [0, 2, 4, 6, 1, 3, 5, 7], :].reshape(B, hkv, 128, lkv.value)
        return t

    def _forward_logits(self, input_ids) -> torch.Tensor:
        """forward_body + the head over every row and the whole vocabulary: [B, L, vocab] logits."""
        self.forward_body(input_ids)
        B, L = self._shape
        rows = torch.arange(B * L, dtype=torch.int32, device=self.device)
        return self.head_rows(rows, 0, self.vocab).view(B, L, self.vocab)

    def _forward_loss(self, input_ids, labels, return_dict, compute_separate_losses, t):
        """forward(infer=False): the reference's loss contract (model/modeling_xllmx_dimoo.py:56-194), see forward()."""
        self._refuse_tp_score()
        if labels is None:
            # the reference returns the logits here (:74-78), which forward(infer=True) already does; this combination stays the
            # loud refusal it has always been (tests/test_reference_contract.py pins it)
            raise NotImplementedError("forward(infer=False) needs labels (the loss); forward(infer=True) returns the logits")
        ids, lab, lengths = pad_id_lists(input_ids, labels)
        lab = lab.to(self.device)
        unscaled = self.score(ids, lab).to(torch.bfloat16)   # the reference's per-token loss has the logits' dtype
        logits = self._forward_logits(ids) if return_dict else None
        if not compute_separate_losses:
            valid = lab != IGNORE_INDEX
            loss = unscaled[valid].mean() if bool(valid.any()) else torch.tensor(0.0, device=self.device)
            return {"logits": logits, "loss": loss, "labels": lab} if return_dict else loss
        loss, text_loss, image_loss = loss_regions(unscaled, ids, lab, lengths, t=t)
        if return_dict:
            return {"logits": logits, "loss": loss, "interleave_loss": loss, "text_loss": text_loss, "image_loss": image_loss,
                    "labels": lab}
        return loss, {"text_loss": text_loss, "image_loss": image_loss, "interleave_loss": loss}

    def forward(self, input_ids=None, labels=None, infer=False, use_cache=False, to_compute_mask=None, cat="",
                return_dict=False, compute_separate_losses=True, t=None, **_):
        """LLaDAForMultiModalGeneration.forward(infer=True) (model/modeling_xllmx_dimoo.py:41-72) -> logits [B, L, vocab].

        use_cache / to_compute_mask / cat are LLaDAModelLM.forward's dLLM-cache arguments (model/modeling_llada.py:
        1468-1493,1244-1245,929-940,1406-1413): with use_cache=True the call goes through the cache slot of `cat`
        (forward_cached); to_compute_mask [B, L] bool then selects the tokens that are recomputed — every other position's
        keys, values and logits are reused — and the returned logits are the whole logit cache, as in the reference.

        infer=False (model/modeling_xllmx_dimoo.py:74-194; forward value only, there is no backward pass): input_ids / labels are
        lists of id lists (padded with 0 / -100 to the longest, as the reference does) or [B, L] tensors.  The reference pads a
        ragged batch and then attends to the pad tokens — its attention drops the attention bias the wrapper builds
        (model/modeling_llada.py:671-679) — so a padded batch is simply an equal-length batch whose pad rows are ignored through
        labels = -100; that is reproduced, not repaired.  labels=None (the reference returns the logits, :74-78) stays refused:
        forward(infer=True) is the logits call.  The per-token loss is score() rounded once to bf16 (the logits' dtype in the reference) and the result is the
        reference's: the scalar interleave loss (compute_separate_losses=False), (loss, {'text_loss', 'image_loss',
        'interleave_loss'}), or with return_dict a dict that also holds 'labels' and 'logits' — only that last form materialises
        the [B, L, vocab] logits (through head_rows); every other form runs the fused scoring head.  t: scales text_loss
        (loss_regions).  text_coeff / image_coeff are accepted and unused, as in the reference."""
        if not infer:
            if use_cache or to_compute_mask is not None:
                raise NotImplementedError("forward(infer=False) does not go through the dLLM cache")
            return self._forward_loss(input_ids, labels, return_dict, compute_separate_losses, t)
        if labels is not None:
            raise NotImplementedError("forward(infer=True) returns logits; pass infer=False to score labels")
        if to_compute_mask is not None and not use_cache:
            raise ValueError("to_compute_mask needs use_cache=True (the reference only gathers the tokens then, "
                             "model/modeling_llada.py:1244-1245)")
        if use_cache and (self.tp_size == 1 or self._comm_in_library):
            # also under tensor parallelism when the exchange runs in the library (init_tp_comm): every rank caches its heads
            self.forward_cached(input_ids, to_compute_mask=to_compute_mask, cat=cat)
            B, L = self._cache[cat].shape
            rows = torch.arange(B * L, dtype=torch.int32, device=self.device)
            return CausalLMOutputLite(logits=self.cache_head_rows(cat, rows, 0, self.vocab).view(B, L, self.vocab))
        if to_compute_mask is not None:
            raise NotImplementedError("the dLLM cache under tensor parallelism needs the library's exchange (init_tp_comm); "
                                      "the host all-reduce fallback recomputes every row")
        # host all-reduce fallback + use_cache without a mask: every row is recomputed and nothing is kept (same logits)
        return CausalLMOutputLite(logits=self._forward_logits(input_ids))

    __call__ = forward

    # ---- dLLM cache (model/modeling_llada.py:593-600,929-940,1244-1245,1406-1426) ----------------------------------------
    def caching(self, enable: bool = True):
        """LLaDAModel.caching (model/modeling_llada.py:1417-1421 -> every block's :598-600): sets the blocks' use_cache flag
        — which only decides whether the queries of a compute-mask step are rotated by their own positions (:714-716) — and
        clears every cache."""
        self.use_cache = bool(enable)
        self.empty_cache()

    def empty_cache(self):
        """LLaDAModel.empty_cache (model/modeling_llada.py:1423-1426): drops every slot's keys / values / final rows."""
        for ent in self._cache.values():
            abi.check(self._lib.mmada_cache_bind(self._handle, ent.idx, None, 0, 0, 0, abi.stream_ptr()), "mmada_cache_bind")
        self._cache = {}

    def _cache_slot(self, cat, B: int, L: int, rebind_ok: bool):
        cache = self._cache
        ent = cache.get(cat)
        if ent is not None and ent.shape == (B, L):
            return ent
        if ent is not None and not rebind_ok:
            raise ValueError(f"cache {cat!r} holds sequences of shape {ent.shape}, the masked call has {(B, L)}")
        if ent is None:
            used = {e.idx for e in cache.values()}
            free = [i for i in range(16) if i not in used]
            if not free:
                raise abi.MmadaError("all 16 dLLM cache slots are in use (empty_cache() releases them)")
            idx = free[0]
        else:
            idx = ent.idx
        nbytes = self._lib.mmada_cache_bytes(self._handle, B, L)
        mem = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = (mem.data_ptr() + 255) // 256 * 256
        abi.check(self._lib.mmada_cache_bind(self._handle, idx, base, nbytes, B, L, abi.stream_ptr()), "mmada_cache_bind")
        cache[cat] = SimpleNamespace(idx=idx, mem=mem, shape=(B, L))
        return cache[cat]

    def forward_cached(self, input_ids: torch.Tensor, to_compute_mask: Optional[torch.Tensor] = None, cat="") -> None:
        """One forward through the cache slot `cat` (created at zeros on first use, like the reference's zeros_like).
        Mask None: every token is computed and the slot is (re)filled.  Mask [B, L] bool with the same count in every
        row (the reference's `.view(B, -1)`): only those tokens run through the blocks; read logits with cache_head_rows."""
        if self.tp_size != 1 and not self._comm_in_library:
            raise NotImplementedError("the dLLM cache path under tensor parallelism needs the library's exchange (init_tp_comm)")
        ids = input_ids.to(device=self.device, dtype=torch.long).contiguous()
        B, L = ids.shape
        if self._comm_in_library and B * ((L + 7) // 8 * 8) > self._comm_rows:
            raise abi.MmadaError(f"cached forward of {B}x{L} exceeds the {self._comm_rows} rows init_tp_comm() was sized for")
        self._ensure_ws(B, L)
        ent = self._cache_slot(cat, B, L, rebind_ok=to_compute_mask is None)
        st = abi.stream_ptr()
        if to_compute_mask is None:
            abi.check(self._lib.mmada_forward_cached(self._handle, ent.idx, ids.data_ptr(), None, B, L, L, 1, st),
                      "mmada_forward_cached")
        else:
            m = to_compute_mask.to(device=self.device, dtype=torch.bool)
            if m.shape != (B, L):
                raise ValueError(f"to_compute_mask {tuple(m.shape)} does not match input_ids {(B, L)}")
            cnt = m.sum(1)
            Tc = int(cnt[0])
            if Tc == 0 or not bool((cnt == Tc).all()):
                raise ValueError("to_compute_mask must select the same, non-zero number of tokens in every sequence")
            pos = m.nonzero()[:, 1].view(B, Tc).to(torch.int32).contiguous()
            ids_c = ids[m].view(B, Tc).contiguous()
            abi.check(self._lib.mmada_forward_cached(self._handle, ent.idx, ids_c.data_ptr(), pos.data_ptr(), B, L, Tc,
                                                     int(self.use_cache), st), "mmada_forward_cached")
        self._resident = _Resident()  # no plain forward is resident any more

    def cache_head_rows(self, cat, rows: torch.Tensor, col_begin: int, col_end: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Rows (b*L + l) x columns [col_begin, col_end) of logit_cache[cat] (model/modeling_llada.py:1406-1413)."""
        ent = self._cache.get(cat)
        if ent is None:
            raise KeyError(f"no cache {cat!r}")
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        if out is None:
            out = torch.empty((rows.numel(), col_end - col_begin), dtype=torch.bfloat16, device=self.device)
        elif out.shape != (rows.numel(), col_end - col_begin) or out.dtype != torch.bfloat16 or not out.is_contiguous():
            raise ValueError("cache_head_rows: `out` must be a contiguous bf16 [R, col_end-col_begin] tensor")
        abi.check(self._lib.mmada_cache_head_rows(self._handle, ent.idx, rows.data_ptr(), rows.numel(), col_begin, col_end,
                                                  out.data_ptr(), abi.stream_ptr()), "mmada_cache_head_rows")
        return out

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def __del__(self):
        try:
            for ln in reversed(self._lanes):
                if ln.handle.value:
                    self._lib.mmada_destroy(ln.handle)
                    ln.handle.value = None
        except Exception:
            pass
