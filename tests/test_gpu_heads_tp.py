"""Top-k and the Gumbel-max draw under tensor parallelism: mmada_head_topk / mmada_head_sample (and mmada_text_select_sampled, the
generators' device samplers) on a connected group of two or more ranks (csrc/tp_heads.hip: tp_head_rounds and its joins).  Every
rank multiplies its block of the launch's 256-column tiles, the tiles' key records ride the score exchange behind the 16-byte
records, and every rank joins every row.  Every comparison below is bit equality.

The ranks of a group are handles of ONE process on one device (helpers.tp_group / tp_each, see tests/test_gpu_tp.py): nothing may
synchronise the host before every rank's work is enqueued, so every tensor a rank's calls need exists before tp_each."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch

from helpers import GOLDEN, t2i_job, tiny_job, tiny_sd, tp_each, tp_group
from mmada_parallel_amd import abi, synth
from test_gpu_sample import SEED, keys_of, probe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
os.environ.setdefault("MMADA_TP_TIMEOUT_S", "8")
V = synth.CFG_TINY["vocab_size"]
Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
SCORE_ROUND = 1280   # rows per round of the published record buffers (csrc/tp_comm.h)
BIG_COUNTER = (1 << 62) + 5
# the whole vocabulary; a partial last tile; five tiles; a first column that is no multiple of 4 (the two-block Philox path);
# five columns (top-k places beyond the tile's columns)
RANGES = ((0, V), (0, V - 100), (1000, 2237), (1001, 2238), (1000, 1005))


def counter_at(c):
    return torch.tensor([c], dtype=torch.int64, device=DEV)


def no_target(R):
    return torch.full((R,), -1, dtype=torch.long, device=DEV)


def wide_ids():
    """24 sequences of the fixture's first (they differ in one token): B * L rows, more than one round of the record buffers."""
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)[:1].repeat(24, 1)
    ids[:, 3] = torch.arange(24, device=DEV) + 40
    return ids


@pytest.fixture(scope="module")
def group2():
    """A TP = 2 group (pull) with the forward of wide_ids() resident on both ranks.  Tests leave it on the pull transport."""
    ids = wide_ids()
    B, L = ids.shape
    max_rows = B * ((L + 7) // 8 * 8)
    assert B * L >= SCORE_ROUND + 8 and max_rows >= SCORE_ROUND + 8
    ranks, streams = tp_group(synth.CFG_TINY, tiny_sd(), 2, max_rows)
    tp_each(ranks, streams, lambda m: m.forward_body(ids))
    yield ranks, streams, ids
    torch.cuda.synchronize()
    for m in ranks:
        m.disconnect_tp()


def rows_for(R, n):
    return torch.arange(n, dtype=torch.int32, device=DEV)[:R] if R > 1 else torch.tensor([77], dtype=torch.int32, device=DEV)


def clean(ranks):
    for m in ranks:
        status = m.comm_status()
        assert status["error"] == 0, status


def expect_topk(logits, c0, k):
    """The first k of the stable descending sort (logit descending, then column ascending), as columns of the whole vocabulary."""
    return (torch.sort(logits.float(), dim=1, descending=True, stable=True).indices[:, :k] + c0).int()


def expect_draw(logits, c0, T, g):
    return (keys_of(logits, T, g).argmax(1) + c0).int()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["pull", "copy"])
def test_tp2_against_materialised_logits_of_the_same_rank(group2, transport):
    ranks, streams, ids = group2
    n = ids.numel()
    for m in ranks:
        m.set_transport(transport)
    try:
        for c0, c1 in RANGES:
            ks = tuple(k for k in (1, 3, 8) if k <= c1 - c0) + ((5,) if c1 - c0 == 5 else ())
            for R in (1, 5, 61):
                rows = rows_for(R, n)
                draws = [(T, c) for T in (0.0, 0.7) for c in (0, BIG_COUNTER)]
                ctrs = [[counter_at(c) for _, c in draws] for _ in ranks]

                def one(m):
                    r = ranks.index(m)
                    out = dict(logits=m.head_rows(rows, c0, c1), stats=m.token_logprobs(rows, no_target(R), c0, c1, return_stats=True))
                    for k in ks:
                        ids_k, lp_k, lse_k = m.top_logprobs(rows, k, c0, c1)
                        out["topk", k] = (ids_k, lp_k, lse_k, [m.token_logprobs(rows, ids_k[:, j].long(), c0, c1) for j in range(k)])
                    for i, (T, c) in enumerate(draws):
                        got = m.sample_tokens(rows, T, c0, c1, seed=SEED, counter=ctrs[r][i], return_stats=True)
                        out["draw", T, c] = (got, m.token_logprobs(rows, got[0].long(), c0, c1))
                    return out

                res = tp_each(ranks, streams, one)
                clean(ranks)
                noise = {c: probe(SEED, c, 0, R, c0, c1 - c0, words=False)[1] for c in (0, BIG_COUNTER)}
                for r, out in enumerate(res):
                    what = f"{transport}, rank {r}, cols [{c0},{c1}), R={R}"
                    logits, (_, lse_ref, arg_ref, max_ref) = out["logits"], out["stats"]
                    assert torch.equal(logits, res[0]["logits"])
                    for k in ks:
                        ids_k, lp_k, lse_k, lp_ref = out["topk", k]
                        assert torch.equal(ids_k, expect_topk(logits, c0, k)), f"{what}, k={k}: ids are not the stable sort's first k"
                        assert torch.equal(lse_k, lse_ref), f"{what}, k={k}: lse"
                        for j in range(k):
                            assert torch.equal(lp_k[:, j], lp_ref[j]), f"{what}, k={k}: log-probability of place {j}"
                    for i, (T, c) in enumerate(draws):
                        (ids_d, lp, lse, arg, mx), lp_ref = out["draw", T, c]
                        assert torch.equal(ids_d, expect_draw(logits, c0, T, noise[c])), f"{what}, T={T}, counter {c}: ids"
                        assert torch.equal(lp, lp_ref), f"{what}, T={T}, counter {c}: log-probability of the draw"
                        assert torch.equal(lse, lse_ref) and torch.equal(arg, arg_ref) and torch.equal(mx, max_ref), f"{what}: stats"
                        assert int(ctrs[r][i]) == c + 1, f"{what}: the counter advanced by {int(ctrs[r][i]) - c}"
                        if T == 0:
                            assert torch.equal(ids_d, arg_ref)
    finally:
        for m in ranks:
            m.set_transport("pull")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_result_is_independent_of_rank_count_and_transport():
    """The same normalised rows planted into groups of 2, 4 and 8 ranks (as in test_gpu_score_tp): all ranks of all groups return
    the same bits, on both transports — with the all-zero row (a tie across every tile and rank), two equal head rows in different
    ranks' tiles, and ranks that own no tile (five tiles over 8 ranks: ranks 5-7; over 4 ranks: rank 3)."""
    cfg = synth.CFG_PEAKED
    Vp = cfg["vocab_size"]
    sd = synth.synthetic_state_dict(cfg, seed=5, device=DEV)
    head = sd["model.transformer.ff_out.weight"]
    c_lo, c_hi = 1000, 263 * 256 + 5
    head[c_hi] = head[c_lo]
    g = torch.Generator().manual_seed(17)
    B, L = 2, 61
    ids = torch.randint(0, 126000, (B, L), generator=g).to(DEV)
    Lp = (L + 7) // 8 * 8
    R = B * L
    rows = torch.arange(R, dtype=torch.int32, device=DEV)
    ranges = ((0, Vp), (0, Vp - 100), (1000, 2237))
    results = {}
    xn_ref = None
    for k in (2, 4, 8):
        ranks, streams = tp_group(cfg, sd, k, B * Lp)
        try:
            tp_each(ranks, streams, lambda m: m.forward_body(ids))
            if xn_ref is None:   # the first group's normalised stream, with two planted rows, becomes every rank's
                xn_ref = ranks[0].debug_buffer(0).clone()
                xn_ref[5].zero_()
                xn_ref[9] = (head[c_lo].float() * 40.0).to(torch.bfloat16)
            for transport in ("pull", "copy"):
                for m in ranks:
                    m.set_transport(transport)
                ctrs = [[counter_at(3) for _ in ranges] for _ in ranks]

                def one(m):
                    r = ranks.index(m)
                    m.debug_buffer(0).copy_(xn_ref)
                    return [(m.top_logprobs(rows, 8, c0, c1), m.sample_tokens(rows, 0.7, c0, c1, seed=SEED, counter=ctrs[r][i], return_stats=True))
                            for i, (c0, c1) in enumerate(ranges)]

                out = tp_each(ranks, streams, one)
                for m in ranks:
                    status = m.comm_status()
                    assert status["mode"] == transport and status["error"] == 0, status
                for r, res in enumerate(out):
                    results[(k, transport, r)] = res
                    assert all(int(c) == 4 for c in ctrs[r])
        finally:
            torch.cuda.synchronize()
            for m in ranks:
                m.disconnect_tp()
        del ranks, streams
        torch.cuda.empty_cache()
    ref = results[(2, "pull", 0)]
    for key, res in results.items():
        for rg, (topk, drawn), (topk_ref, drawn_ref) in zip(ranges, res, ref):
            for a, b in zip(topk + drawn, topk_ref + drawn_ref):
                assert a.dtype == b.dtype and torch.equal(a, b), f"tp={key[0]} {key[1]} rank {key[2]}, cols {rg}"
    # the planted rows: the lowest column wins a tie, also when the tie spans tiles and ranks
    for (c0, c1), (topk, drawn) in zip(ranges, ref):
        assert topk[0][5].tolist() == list(range(c0, c0 + 8)), "the all-zero row: ties go to the lowest columns"
        assert bool((topk[1][5] == topk[1][5][0]).all())
    assert ref[0][0][0][9, :2].tolist() == [c_lo, c_hi] and ref[1][0][0][9, :2].tolist() == [c_lo, c_hi]
    assert ref[0][1][3][9].item() == c_lo, "arg-max of the two equal head rows: the lower column"


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_more_than_one_round_keeps_the_rows_own_noise(group2):
    """R = 1288 rows = one round of 1280 and one of 8: rows 1280 and above draw with the noise of THEIR index in the call (the probe
    with row0 = 1280), and the counter moves once."""
    ranks, streams, ids = group2
    R, c, T = SCORE_ROUND + 8, 11, 0.7
    rows = (torch.arange(R, dtype=torch.int32, device=DEV) * 7) % 700      # repeated row indices: rows i and i + 700 read the same logits
    c0, c1 = 1001, 2238
    ctrs = [counter_at(c) for _ in ranks]
    check = torch.cat([torch.arange(0, 8), torch.arange(572, 588), torch.arange(SCORE_ROUND - 8, R)]).to(DEV)

    def one(m):
        drawn = m.sample_tokens(rows, T, c0, c1, seed=SEED, counter=ctrs[ranks.index(m)], return_stats=True)
        return drawn, m.top_logprobs(rows, 8, c0, c1), m.head_rows(rows[check], c0, c1), m.token_logprobs(rows, drawn[0].long(), c0, c1)

    res = tp_each(ranks, streams, one)
    clean(ranks)
    for r, (drawn, topk, logits, lp_ref) in enumerate(res):
        assert int(ctrs[r]) == c + 1, "one call, one step of the counter"
        for a, b in zip(drawn + topk, res[0][0] + res[0][1]):
            assert torch.equal(a, b), f"rank {r} against rank 0"
        g = torch.cat([probe(SEED, c, int(i), 1, c0, c1 - c0, words=False)[1] for i in check.tolist()])
        want = expect_draw(logits, c0, T, g)
        assert torch.equal(drawn[0][check][-8:], want[-8:]), f"rank {r}: rows of the second round do not carry their own noise"
        assert torch.equal(drawn[0][check], want), f"rank {r}: ids"
        assert torch.equal(drawn[1], lp_ref)
        assert torch.equal(topk[0][check], expect_topk(logits, c0, 8))
    same_logits = (torch.arange(R, device=DEV) + 700 < R).nonzero().flatten()     # rows i and i + 700
    a, b = res[0][0][0][same_logits], res[0][0][0][same_logits + 700]
    assert not torch.equal(a, b), "the same logits under another row's noise draw other tokens somewhere"


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_share_the_published_buffers(group2):
    """score, top-k, sample, sample enqueued on every rank with no forward (and no host synchronisation) between them: each result
    equals that of the same call made on its own from the same counter."""
    ranks, streams, ids = group2
    n, c = ids.numel(), 21
    g = torch.Generator().manual_seed(9)
    rows = [torch.randperm(n, generator=g)[:R].to(torch.int32).to(DEV) for R in (700, SCORE_ROUND + 9, 61, 333)]
    targets = torch.randint(0, V, (700,), generator=g).to(DEV)
    calls = [lambda m, ctr: m.token_logprobs(rows[0], targets, 0, V, return_stats=True),
             lambda m, ctr: m.top_logprobs(rows[1], 8, 1000, 2237),
             lambda m, ctr: m.sample_tokens(rows[2], 0.7, 0, V - 100, seed=SEED, counter=ctr, return_stats=True),
             lambda m, ctr: m.sample_tokens(rows[3], 0.7, 1001, 2238, seed=SEED, counter=ctr, return_stats=True)]
    start = (c, c, c, c + 1)          # the counter each call reads when all four run in a row
    alone = []
    for call, c_i in zip(calls, start):
        ctrs = [counter_at(c_i) for _ in ranks]
        alone.append(tp_each(ranks, streams, lambda m: call(m, ctrs[ranks.index(m)])))
    ctrs = [counter_at(c) for _ in ranks]
    together = tp_each(ranks, streams, lambda m: [call(m, ctrs[ranks.index(m)]) for call in calls])
    clean(ranks)
    for r in range(2):
        assert int(ctrs[r]) == c + 2
        for i in range(4):
            for a, b, z in zip(together[r][i], alone[i][r], alone[i][0]):
                assert torch.equal(a, b), f"rank {r}, call {i} back to back against alone"
                assert torch.equal(b, z), f"rank {r} against rank 0, call {i}"
    assert not torch.equal(alone[2][0][0], alone[2][0][3]), "the draws are not all the arg-max"


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_a_captured_draw_replays_on_every_rank(group2):
    ranks, streams, ids = group2
    lib = abi.lib()
    if not all(m.graph_capturable() for m in ranks):
        pytest.fail("a pull group without a CU partition must be capturable")
    R, c, T, c0, c1 = 61, 31, 0.7, 0, V
    rows = rows_for(R, ids.numel())
    eager = []
    for i in range(2):
        ctrs = [counter_at(c + i) for _ in ranks]
        eager.append(tp_each(ranks, streams, lambda m: m.sample_tokens(rows, T, c0, c1, seed=SEED, counter=ctrs[ranks.index(m)], return_stats=True)))
    ctrs = [counter_at(c) for _ in ranks]
    outs = [[torch.full_like(e, -7) for e in eager[0][0]] for _ in ranks]
    graphs = []
    try:
        for r, (m, s) in enumerate(zip(ranks, streams)):           # capturing enqueues nothing: one rank after the other
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                abi.check(lib.mmada_graph_begin(abi.stream_ptr()), "graph_begin")
                rc = lib.mmada_head_sample(m._handle, rows.data_ptr(), R, c0, c1, T, SEED, ctrs[r].data_ptr(), *[o.data_ptr() for o in outs[r]],
                                           abi.stream_ptr())
                if rc:
                    lib.mmada_graph_abort(abi.stream_ptr())
                abi.check(rc, "mmada_head_sample under capture")
                gr = C.c_void_p()
                abi.check(lib.mmada_graph_end(abi.stream_ptr(), C.byref(gr)), "graph_end")
                graphs.append(gr)
        replays = []
        for _ in range(2):
            for gr, s in zip(graphs, streams):                      # every rank's replay is enqueued before the host waits
                with torch.cuda.stream(s):
                    abi.check(lib.mmada_graph_launch(gr, abi.stream_ptr()), "graph_launch")
            torch.cuda.synchronize()
            replays.append([[o.clone() for o in outs[r]] for r in range(2)])
    finally:
        torch.cuda.synchronize()
        for gr in graphs:
            lib.mmada_graph_destroy(gr)
    clean(ranks)
    for r in range(2):
        assert int(ctrs[r]) == c + 2
        for i in range(2):
            for a, b, z in zip(replays[i][r], eager[i][r], replays[i][0]):
                assert torch.equal(a, b), f"rank {r}: replay {i} is not the eager call at counter c + {i}"
                assert torch.equal(a, z), f"rank {r} against rank 0, replay {i}"
    assert not torch.equal(replays[0][0][0], replays[1][0][0])
    after = tp_each(ranks, streams, lambda m: m.top_logprobs(rows, 3, c0, c1))       # eager calls go on behind the replays
    clean(ranks)
    assert torch.equal(after[0][0], after[1][0])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_text_select_sampled_on_tp2_commits_the_draw_by_the_rule(group2):
    ranks, streams, ids = group2
    lib = abi.lib()
    mask = int(ranks[0].config.get("mask_token_id", synth.MASK))
    Bf, L = ids.shape
    B, ts, T = 2, 10, 16
    masked = torch.zeros(B, T, dtype=torch.bool)
    masked[0, [0, 3, 4, 7, 8, 12, 15]] = True
    masked[1, [1, 2, 9]] = True
    seq = ids[:B].clone()
    seq[:, ts:ts + T][masked.to(DEV)] = mask           # the commit reads the mask from the ids it is given
    rows = (torch.arange(B)[:, None] * L + ts + torch.arange(T)[None, :]).flatten().int().to(DEV)
    k = [3, 0]
    c, temp = 9, 0.7
    k_dev = torch.tensor(k, dtype=torch.int32, device=DEV)
    got = [seq.clone() for _ in ranks]
    scratch = [torch.empty(B * T * 16, dtype=torch.uint8, device=DEV) for _ in ranks]
    ctr_draw, ctr_sel = [counter_at(c) for _ in ranks], [counter_at(c) for _ in ranks]

    def one(m):
        r = ranks.index(m)
        drawn = m.sample_tokens(rows, temp, seed=SEED, counter=ctr_draw[r])
        abi.check(lib.mmada_text_select_sampled(m._handle, rows.data_ptr(), B, T, temp, SEED, ctr_sel[r].data_ptr(), got[r].data_ptr(), L, ts,
                                                k_dev.data_ptr(), scratch[r].data_ptr(), abi.stream_ptr()), "mmada_text_select_sampled")
        return drawn

    res = tp_each(ranks, streams, one)
    clean(ranks)
    assert torch.equal(got[0], got[1]), "both ranks commit the same ids"
    for r, (x0, lp, _) in enumerate(res):
        assert int(ctr_sel[r]) == c + 1
        want = seq.clone()    # the commit rule: masked positions only, confidence descending, then position ascending, k[b] winners
        conf = torch.where(masked.to(DEV), lp.view(B, T).double(), torch.full((B, T), float("-inf"), dtype=torch.float64, device=DEV))
        for b in range(B):
            order = sorted(range(T), key=lambda t: (-float(conf[b, t]), t))
            for t in order[:k[b]]:
                want[b, ts + t] = int(x0[b * T + t])
        assert torch.equal(got[r], want), f"rank {r}: not the draw of sample_tokens committed by the rule"
    changed = got[0] != seq
    assert int(changed[0].sum()) == 3 and int(changed[1].sum()) == 0


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def on_threads(ranks, streams, fn):
    """fn(rank model) on a host thread per rank, each on the rank's stream: for loops that read the host between steps (a rank's
    hand-off spins until its peers' launches arrive, so one thread must not run the ranks one after the other)."""
    out, err = [None] * len(ranks), [None] * len(ranks)
    cur = torch.cuda.current_stream()

    def run(i):
        try:
            torch.cuda.set_device(DEV)
            streams[i].wait_stream(cur)
            with torch.cuda.stream(streams[i]):
                out[i] = fn(ranks[i])
        except BaseException as e:   # noqa: BLE001  (re-raised below, on the test's thread)
            err[i] = e

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(ranks))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for e in err:
        if e is not None:
            raise e
    return out


@pytest.fixture(scope="module")
def small2():
    job = tiny_job()
    L = job["input_ids"].shape[1]
    ranks, streams = tp_group(synth.CFG_TINY, tiny_sd(), 2, 2 * ((L + 7) // 8 * 8))
    yield ranks, streams
    torch.cuda.synchronize()
    for m in ranks:
        m.disconnect_tp()


def test_generate_ti2ti_tp2_with_both_device_samplers(small2):
    """The README settings' samplers (temperature 1.0, text_temperature 0.7) on the device under TP = 2: the ranks' trajectories are
    identical, and the replayed run (graph=True) is the eager one."""
    from mmada_parallel_amd.generators.parallel_generator import _ti2ti_steps

    ranks, streams = small2
    job = tiny_job()
    ids0 = job["input_ids"].to(DEV)
    ts, te = job["text_start"], job["text_end"]

    def run(graph, seed):
        def steps(m):
            last = None
            for _, ids, _ in _ti2ti_steps(m, ids0, ts, te, job["image_start"], job["seq_len"], job["newline_every"], text_steps=6,
                                          timesteps=3, temperature=1.0, text_temperature=0.7, cfg_scale=0.0, cfg_img=4.0,
                                          uncon_text=job["uncon_text"], uncon_image=job["uncon_image"], text_sampler="device",
                                          image_sampler="device", sampler_seed=seed, graph=graph):
                last = ids
            return last.clone()

        out = on_threads(ranks, streams, steps)
        clean(ranks)
        assert torch.equal(out[0], out[1]), "ranks end with identical ids"
        return out[0]

    eager = run(False, 1234)
    assert not bool((eager[0, ts:te] == synth.MASK).any())
    assert torch.equal(run(True, 1234), eager), "graph=True equals eager"
    assert not torch.equal(run(False, 1235), eager), "another seed draws another run"


def test_generate_image_and_interleave_tp2_with_device_samplers(small2):
    from mmada_parallel_amd.generators.image_generation_generator import generate_image
    from test_gpu_m_sample import interleave
    from test_gpu_t2i_mmu_sample import g_kwargs

    ranks, streams = small2
    job = t2i_job(side=4)
    kw = g_kwargs(job, timesteps=4, temperature=1.0, cfg_scale=2.0)
    runs = {}
    for graph in (False, True):
        res = on_threads(ranks, streams, lambda m: generate_image(m, job["prompt"], image_sampler="device", sampler_seed=77, graph=graph,
                                                                  **kw).clone())
        clean(ranks)
        assert torch.equal(res[0], res[1]), f"generate_image(graph={graph}): ranks end with identical ids"
        runs[graph] = res[0]
    assert torch.equal(runs[True], runs[False]), "generate_image: graph=True equals eager"
    runs = {}
    for graph in (False, True):
        res = on_threads(ranks, streams, lambda m: interleave(m, text_sampler="device", text_temperature=0.7, sampler_seed=77, graph=graph))
        clean(ranks)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), f"interleave_generate(graph={graph}): ranks agree"
        runs[graph] = res[0]
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1]), "interleave_generate: graph=True equals eager"
