"""Tensor-parallel exchange inside the library (csrc/tp_comm.hip): reduce-scatter -> residual add + RMSNorm on the owner's
rows -> all-gather, with the pull transport over mapped peer buffers.

One GPU is enough to exercise the protocol and the kernels: the ranks of a tensor-parallel group are separate handles in
ONE process, each on its own stream, connected with mmada_comm_connect_local (the hand-off counters, the system-scope
pulls, the owner split, the two-chunk overlap schedule on the second stream are the multi-device code path unchanged; only
the peer pointers come from the same process instead of hipIpc).  Nothing may synchronise the host before every rank's
work is enqueued — a rank's wait kernel spins until its peers' launches arrive.  The multi-PROCESS path (hipIpc handles,
one process per rank) is covered by test_bench_multi_rank_tensor_parallel_on_one_gpu.
"""
import os

import pytest
import torch

from helpers import tiny_job, tiny_sd, tp_each, tp_group
from mmada_parallel_amd import abi, synth
from mmada_parallel_amd.tp_link import MODE_NO_EXCHANGE, MODE_OF, connect_local_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
os.environ.setdefault("MMADA_TP_TIMEOUT_S", "8")


_group, _each = tp_group, tp_each


@pytest.mark.parametrize("chunks,transport,cus", [("2", "pull", 0), ("1", "pull", 0), ("2", "copy", 0), ("1", "copy", 0)])
def test_exchange_and_forward_tp2_in_one_process(tiny_tp1, chunks, transport, cus, monkeypatch):
    """transport "copy": the bytes move by hipMemcpyAsync (copy engines) into local staging, the owner kernel reads local memory
    only.  Same protocol, same arithmetic: it must produce the bits of the pull transport.  (The CU partition,
    mmada_comm_set_partition, is exercised on a one-rank group below: two in-process ranks with two CU-masked queues each
    outgrow the hardware queues one process gets, and a rank's spinning wait kernel then blocks its peer's launches.)"""
    monkeypatch.setenv("MMADA_TP_CHUNKS", chunks)
    tp = 2
    job = tiny_job()
    ids = job["input_ids"].repeat(3, 1).to(DEV)
    ids[1, :6] = torch.arange(50, 56, device=DEV)
    ids[2, :4] = torch.arange(7, 11, device=DEV)
    B, L = ids.shape
    Lp = (L + 7) // 8 * 8
    ranks, streams = _group(synth.CFG_TINY, tiny_sd(), tp, B * Lp, transport=transport, exchange_cus=cus)
    d = synth.CFG_TINY["d_model"]
    lib = ranks[0]._lib
    assert ranks[0].comm_status()["mode"] == transport and lib.mmada_comm_partition(ranks[0]._handle) == cus

    # ---- one exchange on known data: every rank's normalised rows must equal the expectation bit for bit ----
    M = B * Lp
    col = torch.arange(d, device=DEV, dtype=torch.float32)[None, :]
    row = torch.arange(M, device=DEV, dtype=torch.float32)[:, None]
    w = (1 + 0.05 * torch.randn(d, device=DEV)).to(torch.bfloat16)
    for it in range(3):  # new data in the same buffers every round
        def pat(r):
            return ((((row * 3 + col * 5 + r * 11 + it * 17) % 13) - 6.0) * (r + 1) * 0.125).to(torch.bfloat16)

        def one(m):
            m._ensure_ws(B, L)
            st = abi.stream_ptr()
            abi.check(lib.mmada_embed(m._handle, ids.data_ptr(), B, L, st), "embed")
            m._shape, m._split = (B, L), None
            m._part_view(M).copy_(pat(m.tp_rank))
            x0 = m._stream_view().view(M, d).clone()
            abi.check(lib.mmada_comm_exchange(m._handle, w.data_ptr(), st), "exchange")
            return x0

        x0s = _each(ranks, streams, one)
        total = sum(pat(r).float() for r in range(tp)).to(torch.bfloat16)
        x_new = (x0s[0].float() + total.float()).to(torch.bfloat16)
        want = torch.empty_like(x_new)
        abi.check(lib.mmada_rmsnorm(x_new.data_ptr(), w.data_ptr(), want.data_ptr(), M, d, 1e-5, abi.stream_ptr()), "rmsnorm")
        for m in ranks:
            assert torch.equal(m.debug_buffer(0).view(-1, d)[:M], want), f"round {it}, rank {m.tp_rank}"
            assert m.comm_status()["error"] == 0

    # ---- whole forward: ranks agree bit for bit with each other and, within the bf16 partial-sum tolerance, with TP=1 ----
    _each(ranks, streams, lambda m: m.forward_body(ids))
    hid = _each(ranks, streams, lambda m: m.hidden_state())
    assert torch.equal(hid[0], hid[1])
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    lg = _each(ranks, streams, lambda m: m.head_rows(rows, synth.TEXT_VOCAB, synth.TEXT_VOCAB + 512))
    assert torch.equal(lg[0], lg[1])
    tiny_tp1.forward_body(ids)
    ref = tiny_tp1.hidden_state().float()
    err = ((hid[0].float() - ref).abs().max() / ref.abs().max()).item()
    mean = ((hid[0].float() - ref).abs().mean() / ref.abs().mean()).item()
    lr = tiny_tp1.head_rows(rows, synth.TEXT_VOCAB, synth.TEXT_VOCAB + 512).float()
    lerr = ((lg[0].float() - lr).abs().max() / lr.abs().max()).item()
    if transport != "pull" or cus:   # against the plain pull transport on the same inputs: bit for bit
        base, bstreams = _group(synth.CFG_TINY, tiny_sd(), tp, B * Lp)
        _each(base, bstreams, lambda m: m.forward_body(ids))
        bh = _each(base, bstreams, lambda m: m.hidden_state())
        assert torch.equal(bh[0], hid[0]), f"{transport}, {cus} exchange CUs: differs from the pull transport"
    print(f"TP=2 (library exchange, chunks={chunks}, {transport}, {cus} exchange CUs) vs TP=1: hidden max rel {err:.3e} mean rel {mean:.3e}; logits max rel {lerr:.3e}")
    # every rank rounds its partial to bf16 before the (fp32, rank-ordered) sum, and partials are larger than their sum:
    # measured on MI355X: max 1.5e-2, mean 3.9e-3 of the stream's magnitude (TP=1 vs the oracle: 1.0e-2 / 6e-4)
    assert err < 2.5e-2 and mean < 6.0e-3 and lerr < 2.5e-2
    for m in ranks:
        assert m.comm_status()["error"] == 0
    tiny_tp1.forward_body(ids[:1])


def test_generate_ti2ti_tp2_in_one_process_ranks_agree(tiny_tp1):
    """Both ranks of a TP=2 group run the sampler (each on its own stream, interleaved step by step on the host): their
    token trajectories must be identical — every rank sees the same all-gathered logits."""
    from mmada_parallel_amd.generators.parallel_generator import _ti2ti_steps

    job = tiny_job()
    ids0 = job["input_ids"].to(DEV)
    L = ids0.shape[1]
    ranks, streams = _group(synth.CFG_TINY, tiny_sd(), 2, 2 * ((L + 7) // 8 * 8))
    gens = []
    for m, s in zip(ranks, streams):
        with torch.cuda.stream(s):
            gens.append(_ti2ti_steps(m, ids0, job["text_start"], job["text_end"], job["image_start"], job["seq_len"],
                                     job["newline_every"], text_steps=8, timesteps=4, temperature=0.0, text_temperature=0.0,
                                     cfg_scale=0.0, cfg_img=4.0, uncon_text=job["uncon_text"], uncon_image=job["uncon_image"]))
    final = [None, None]
    for _ in range(9):
        for i, (g, s) in enumerate(zip(gens, streams)):
            with torch.cuda.stream(s):
                step, ids, info = next(g)  # enqueues one step of rank i (no host sync inside the loop)
                final[i] = ids
    torch.cuda.synchronize()
    assert torch.equal(final[0], final[1])
    assert not bool((final[0][0, job["text_start"]:job["text_end"]] == synth.MASK).any())
    for m in ranks:
        assert m.comm_status()["error"] == 0


def test_vocab_parallel_text_select_matches_replicated_head():
    """mmada_text_select_tp (every rank: its vocab/tp columns of the LM head -> {max, arg-max, fp64 sum-exp} per row ->
    16-byte records exchanged and combined) against the replicated head + mmada_text_select on the SAME tensor-parallel
    forward: identical arg-max tokens, confidences equal to fp64 rounding, identical committed ids."""
    tp = 2
    job = tiny_job()
    ids = job["input_ids"].repeat(2, 1).to(DEV)
    ids[1, :5] = torch.arange(20, 25, device=DEV)
    B, L = ids.shape
    ts, te = job["text_start"], job["text_end"]
    T = te - ts
    ranks, streams = _group(synth.CFG_TINY, tiny_sd(), tp, B * ((L + 7) // 8 * 8))
    lib = ranks[0]._lib
    V = ranks[0].vocab
    rows = (torch.arange(B, device=DEV)[:, None] * L + torch.arange(ts, te, device=DEV)[None, :]).reshape(-1).to(torch.int32)
    k = torch.tensor([5, 3], dtype=torch.int32, device=DEV)
    _each(ranks, streams, lambda m: m.forward_body(ids))

    def both(m):
        st = abi.stream_ptr()
        a, b = ids.clone(), ids.clone()
        sa = torch.zeros(B * T * 16, dtype=torch.uint8, device=DEV)
        sb = torch.zeros(B * T * 16, dtype=torch.uint8, device=DEV)
        logits = m.head_rows(rows, 0, V)
        abi.check(lib.mmada_text_select(m._handle, logits.data_ptr(), None, B, T, V, V, a.data_ptr(), L, ts, k.data_ptr(),
                                        sa.data_ptr(), st), "text_select")
        abi.check(lib.mmada_text_select_tp(m._handle, rows.data_ptr(), B, T, b.data_ptr(), L, ts, k.data_ptr(), sb.data_ptr(),
                                           st), "text_select_tp")
        return a, b, sa, sb

    res = _each(ranks, streams, both)
    for a, b, sa, sb in res:
        ca, cb = sa[: B * T * 8].view(torch.float64), sb[: B * T * 8].view(torch.float64)
        xa, xb = sa[B * T * 8: B * T * 12].view(torch.int32), sb[B * T * 8: B * T * 12].view(torch.int32)
        assert torch.equal(xa, xb)
        fin = torch.isfinite(ca)
        assert torch.equal(fin, torch.isfinite(cb)) and int(fin.sum()) == B * T
        assert ((ca[fin] - cb[fin]).abs() / ca[fin]).max().item() < 1e-12
        assert torch.equal(a, b) and int((a != ids).sum()) == 8
    assert torch.equal(res[0][1], res[1][1])
    for m in ranks:
        assert m.comm_status()["error"] == 0


@pytest.fixture(scope="module")
def tiny_tp1():
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    return LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(synth.CFG_TINY), tiny_sd(), device=DEV)


@pytest.mark.parametrize("transport,cus", [("rccl", 0), ("pull", 0), ("copy", 0), ("pull", 16), ("rccl", 32)])
def test_single_rank_group_runs_the_whole_transport_and_equals_the_plain_forward(tiny_tp1, transport, cus):
    """Round-4 review: the RCCL transport (ncclReduceScatter -> owner kernel -> ncclAllGather, csrc/tp_comm.hip mode 2) had never
    executed a collective — RCCL refuses two ranks on one device and no multi-GPU box is available to the tests.  A ONE-rank
    communicator runs every line of it: the dlopen'ed symbol table, ncclCommInitRank, the datatype / count / offset arithmetic
    of both collectives (one rank: copies), the owner-side kernel on the pre-summed rows, the two-chunk schedule with its
    exchange stream and event joins, the all-gather read-out of the residual stream and the vocabulary-parallel text head
    (one slice = the whole vocabulary).  With one rank there is no second partial to round, so the result must equal the plain
    forward BIT FOR BIT; the exchange self-test compares with the local expectation.  The same for the pull transport with
    no peer (hand-off kernels, the run-time-size reduce kernel), for the copy-engine transport, and with a CU PARTITION (cus > 0:
    the exchange stream owns `cus` CUs, the forward's compute kernels run on the library's stream masked to the others, forked
    from and joined to the caller's stream: mmada_comm_set_partition)."""
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    lib = abi.lib()
    job = tiny_job()
    ids = job["input_ids"].repeat(3, 1).to(DEV)
    ids[1, :6] = torch.arange(50, 56, device=DEV)
    ids[2, :4] = torch.arange(7, 11, device=DEV)
    B, L = ids.shape
    Lp = (L + 7) // 8 * 8
    tiny_tp1.forward_body(ids)
    ref_hidden = tiny_tp1.hidden_state().clone()
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    ref_logits = tiny_tp1.head_rows(rows, synth.TEXT_VOCAB, synth.TEXT_VOCAB + 512).clone()
    tiny_tp1.forward_body(ids[:1])

    m = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(synth.CFG_TINY), tiny_sd(), device=DEV, tp_rank=0, tp_size=1)
    abi.check(lib.mmada_set_option(b"tp_allow_single_rank", 1), "set_option")
    try:
        connect_local_group([m], B * Lp, transport=transport, exchange_cus=cus)
        if transport == "rccl":
            assert lib.mmada_comm_rccl_nranks(m._handle) == 1 and m.rccl_nranks() == 1
        assert lib.mmada_comm_partition(m._handle) == cus
        assert m._comm_in_library and m.tp_collective == transport and m.comm_status()["mode"] == transport
        assert m.comm_selftest(iters=3, L=96), "exchange self-test (known partials vs the local expectation)"
        for chunks_L in (L, 40):   # two row chunks (M >= 32) and one
            x = ids[:, :chunks_L].contiguous()
            tiny_tp1.forward_body(x)
            want_h = tiny_tp1.hidden_state().clone()
            r2 = torch.arange(B * chunks_L, dtype=torch.int32, device=DEV)
            want_l = tiny_tp1.head_rows(r2, synth.TEXT_VOCAB, synth.TEXT_VOCAB + 512).clone()
            m.forward_body(x)      # mmada_forward_body -> tp_forward_body: the connected one-rank group
            got_h = m.hidden_state()
            got_l = m.head_rows(r2, synth.TEXT_VOCAB, synth.TEXT_VOCAB + 512)
            torch.cuda.synchronize()
            assert torch.equal(got_h, want_h), f"{transport}, L={chunks_L}: {int((got_h != want_h).sum())} stream elements differ"
            assert torch.equal(got_l, want_l), f"{transport}, L={chunks_L}: logits differ"
            if chunks_L == L:
                assert torch.equal(want_h, ref_hidden) and torch.equal(want_l, ref_logits), "the plain forward itself is deterministic"
        # the vocabulary-parallel text step over the (one) slice against the replicated head on the same forward
        ts, T = job["text_start"], job["text_end"] - job["text_start"]
        m.forward_body(ids)
        trows = torch.cat([torch.arange(ts, ts + T, dtype=torch.int32, device=DEV) + b * L for b in range(B)])
        k = torch.tensor([3, 2, 4], dtype=torch.int32, device=DEV)
        a, b_ = ids.clone(), ids.clone()
        scratch = torch.empty(B * T * 16, dtype=torch.uint8, device=DEV)
        abi.check(lib.mmada_text_select_tp(m._handle, trows.data_ptr(), B, T, a.data_ptr(), L, ts, k.data_ptr(), scratch.data_ptr(),
                                           abi.stream_ptr()), "text_select_tp")
        tl = m.head_rows(trows, 0, m.vocab)
        abi.check(lib.mmada_text_select(m._handle, tl.data_ptr(), None, B, T, m.vocab, m.vocab, b_.data_ptr(), L, ts, k.data_ptr(),
                                        scratch.data_ptr(), abi.stream_ptr()), "text_select")
        torch.cuda.synchronize()
        assert torch.equal(a, b_) and int((a != ids).sum()) == int(k.sum())
        assert m.comm_status()["error"] == 0
        # the no-exchange diagnostic must be reported, not silently return tokens (round-4 advisor)
        from mmada_parallel_amd.generators.parallel_generator import check_tp_exchange

        abi.check(lib.mmada_comm_set_mode(m._handle, MODE_NO_EXCHANGE), "set_mode")
        with pytest.raises(abi.MmadaError):
            check_tp_exchange(m)
        # ... and its values: with ONE rank "own partial only" is the whole sum, so this branch of the exchange too must
        # reproduce the plain forward bit for bit
        m.forward_body(ids)
        diag_l = m.head_rows(rows, synth.TEXT_VOCAB, synth.TEXT_VOCAB + 512)
        torch.cuda.synchronize()
        assert torch.equal(diag_l, ref_logits), f"{transport}: no-exchange diagnostic of a one-rank group: logits differ"
        abi.check(lib.mmada_comm_set_mode(m._handle, MODE_OF[transport]), "set_mode")
        from helpers import save_parity

        save_parity(f"single_rank_{transport}_transport" + (f"_{cus}_exchange_cus" if cus else ""), {"bit_identical_to_plain_forward": True, "rccl_nranks": int(lib.mmada_comm_rccl_nranks(m._handle)),
                                                          "selftest": True, "vocab_parallel_head_equals_replicated": True})
    finally:
        lib.mmada_set_option(b"tp_allow_single_rank", 0)
        m.disconnect_tp()
        assert not m._comm_in_library


@pytest.mark.parametrize("transport", ["pull", "copy"])
def test_connect_local_group_and_disconnect_tp(transport):
    """The public pair that makes and ends an in-process rank group: connect_local_group (helpers.tp_group is that call on fresh
    models plus the stream pool) leaves every rank connected, self-tested and agreeing bit for bit; disconnect_tp() leaves it
    unconnected; a second connect of the same models gives the bits of the first.  B = 1 with L = 40 is one row chunk, L = 96 two
    (M = 96 >= 4 * 8 * tp, tp.chunk_slices)."""
    from mmada_parallel_amd import tp as tp_plan

    tp, max_rows = 2, 2 * 96   # comm_selftest's carve is 2 x 96 rows; the forwards below need fewer
    assert len(tp_plan.chunk_slices(40, tp)) == 1 and len(tp_plan.chunk_slices(96, tp)) == 2
    ranks, streams = _group(synth.CFG_TINY, tiny_sd(), tp, max_rows, transport=transport)
    ids = {L: ((torch.arange(L, device=DEV) * 7 + 3) % 1000).view(1, L) for L in (40, 96)}
    lo, hi = synth.TEXT_VOCAB, synth.TEXT_VOCAB + 320

    def connected_bits():
        for m in ranks:
            status = m.comm_status()
            assert status["mode"] == transport and status["error"] == 0, status
            assert m._comm_in_library and m.tp_collective == transport and max_rows == m._comm_rows
        verdicts = _each(ranks, streams, lambda m: m.comm_selftest(wait=False))   # nothing synchronises between the ranks
        assert all(bool(v) for v in verdicts) and all(m.comm_status()["error"] == 0 for m in ranks), "comm_selftest"
        bits = []
        for L, x in ids.items():
            rows = torch.arange(L, dtype=torch.int32, device=DEV)
            _each(ranks, streams, lambda m: m.forward_body(x))
            lg = _each(ranks, streams, lambda m: m.head_rows(rows, lo, hi))
            assert torch.equal(lg[0], lg[1]), f"{transport}, L = {L}: the ranks' logits differ"
            bits.append(lg[0].clone())
        assert all(m.comm_status()["error"] == 0 for m in ranks)
        return bits

    first = connected_bits()
    for m in ranks:
        m.disconnect_tp()
        assert not m._comm_in_library and m.tp_collective is None
        assert not m.vocab_parallel_head() and not m.graph_capturable()
    assert connect_local_group(ranks, max_rows, transport=transport) is ranks
    again = connected_bits()
    for a, b in zip(first, again):
        assert torch.equal(a, b), f"{transport}: a second connection of the same models computes other bits"
    for m in ranks:
        m.disconnect_tp()


def test_dllm_cache_under_tensor_parallelism(tiny_tp1):
    """The dLLM cache branch (model/modeling_llada.py:593-600,929-940,1244-1245,1406-1426; mmada_cache_* / mmada_forward_cached)
    with the library's tensor-parallel exchange connected (round 5: every rank caches ITS heads of each block's keys / values;
    the slot's final rows are the all-gathered ln_f rows).  Exact properties on a TP = 2 group: a prime call and a mask over
    every token equal the plain tensor-parallel forward bit for bit; rows outside a compute mask keep their logits bit for bit
    and the computed ones change; the ranks agree bit for bit.  Against TP = 1 on the same script: within the bf16 partial-sum
    tolerance of the tensor-parallel forward."""
    tp = 2
    (_, ids0, _), (_, ids1, m1) = synth.dllm_cache_script()[:2]
    B, L = ids0.shape
    Lp = (L + 7) // 8 * 8
    ranks, streams = _group(synth.CFG_TINY, tiny_sd(), tp, B * Lp)
    ids0, ids1, m1 = ids0.to(DEV), ids1.to(DEV), m1.to(DEV)   # on the device BEFORE any rank enqueues (no host copy between ranks)
    lo, hi = synth.TEXT_VOCAB, synth.TEXT_VOCAB + 512
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    for m in ranks + [tiny_tp1]:
        m.caching(True)

    def plain(m, ids):
        m.forward_body(ids)
        return m.head_rows(rows, lo, hi).clone()

    def cached(m, ids, mask):
        m.forward_cached(ids, mask, cat="c")
        return m.cache_head_rows("c", rows, lo, hi).clone()

    plain0 = _each(ranks, streams, lambda m: plain(m, ids0))
    primed = _each(ranks, streams, lambda m: cached(m, ids0, None))
    assert torch.equal(plain0[0], plain0[1]) and torch.equal(primed[0], primed[1]), "ranks must agree bit for bit"
    assert torch.equal(primed[0], plain0[0]), "a prime call is the plain tensor-parallel forward"
    step = _each(ranks, streams, lambda m: cached(m, ids1, m1))
    assert torch.equal(step[0], step[1])
    keep = (~m1).reshape(-1).to(DEV)
    assert torch.equal(step[0][keep], primed[0][keep]), "rows outside the compute mask keep their logits"
    assert not torch.equal(step[0][~keep], primed[0][~keep])
    plain1 = _each(ranks, streams, lambda m: plain(m, ids1))
    full = _each(ranks, streams, lambda m: cached(m, ids1, torch.ones_like(m1)))
    assert torch.equal(full[0], plain1[0]), "a mask over every token is the plain tensor-parallel forward"
    # the same script on one rank
    ref_primed = cached(tiny_tp1, ids0, None).float()
    ref_step = cached(tiny_tp1, ids1, m1).float()
    for got, ref, what in ((primed[0], ref_primed, "prime"), (step[0], ref_step, "compute-mask step")):
        err = (got.float() - ref).abs()
        scale = ref.abs().max().item()
        print(f"dLLM cache, TP=2 vs TP=1, {what}: max {err.max().item() / scale:.3e} mean {err.mean().item() / scale:.3e}")
        assert err.max().item() < 4e-2 * scale and err.mean().item() < 6e-3 * scale
    # the reference's keyword contract (model/modeling_llada.py:1468-1493) routes to the same branch under TP:
    # model(ids, infer=True, use_cache=True, to_compute_mask=m, cat=c).logits is the whole logit cache
    prime_call = _each(ranks, streams, lambda m: m(ids0, infer=True, use_cache=True, cat="c2").logits.clone())
    step_call = _each(ranks, streams, lambda m: m(ids1, infer=True, use_cache=True, to_compute_mask=m1, cat="c2").logits.clone())
    assert step_call[0].shape == (B, L, ranks[0].vocab) and torch.equal(step_call[0], step_call[1])
    assert torch.equal(prime_call[0].reshape(B * L, -1)[:, lo:hi], primed[0]), "forward(use_cache=True) under TP primes the slot"
    assert torch.equal(step_call[0].reshape(B * L, -1)[:, lo:hi], step[0]), "forward(use_cache=True, to_compute_mask=...) under TP"
    for m in ranks:
        assert m.comm_status()["error"] == 0
        m.empty_cache()
    tiny_tp1.empty_cache()
