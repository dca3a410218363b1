"""Scoring under tensor parallelism: mmada_head_logprobs on a connected handle (csrc/tp_comm.hip: tp_head_logprobs).  The launch's
256-column tiles are split over the ranks (tp.score_tile_slice), each rank's EPI_ROWSTAT launch writes the records of its tiles
into a published buffer, the ranks hand off, and every rank joins every row in the fold order of the one-rank head.

The ranks of a group are handles of ONE process on one device (helpers.tp_group / tp_each, see tests/test_gpu_tp.py): nothing
may synchronise the host before every rank's work is enqueued."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, PARITY_REPORT, tiny_sd, tp_each, tp_group
from mmada_parallel_amd import abi, synth, tp as tp_plan
from mmada_parallel_amd.tp_link import connect_local_group
from test_gpu_score import LSE_TOL   # the bound of the one-rank head against float64 (derived there)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
os.environ.setdefault("MMADA_TP_TIMEOUT_S", "8")
V = synth.CFG_TINY["vocab_size"]
Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
NAMES = ("logprob", "lse", "argmax", "max")
RANGES = ((0, V), (synth.TEXT_VOCAB, synth.TEXT_VOCAB + synth.CODEBOOK), (1000, 2237))
SCORE_ROUND = 1280   # rows per round of the published record buffers (csrc/tp_comm.hip)


@pytest.fixture(scope="module")
def tiny_tp1():
    from mmada_parallel_amd import LLaDAForMultiModalGeneration

    return LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(synth.CFG_TINY), tiny_sd(), device=DEV)


class single_rank_group:
    """A connected ONE-rank group (tp_allow_single_rank): every line of the tensor-parallel path with no peer."""

    def __init__(self, cfg, sd, transport, max_rows):
        self.cfg, self.sd, self.transport, self.max_rows = cfg, sd, transport, max_rows

    def __enter__(self):
        from mmada_parallel_amd import LLaDAForMultiModalGeneration

        lib = abi.lib()
        self.m = m = LLaDAForMultiModalGeneration.from_state_dict(synth.full_config(self.cfg), self.sd, device=DEV, tp_rank=0, tp_size=1)
        abi.check(lib.mmada_set_option(b"tp_allow_single_rank", 1), "set_option")
        try:
            connect_local_group([m], self.max_rows, transport=self.transport)
            assert m._comm_in_library and m.tp_collective == self.transport and m.comm_status()["mode"] == self.transport
        except Exception:
            self.__exit__(None, None, None)
            raise
        return m

    def __exit__(self, *exc):
        abi.lib().mmada_set_option(b"tp_allow_single_rank", 0)
        torch.cuda.synchronize()
        self.m.disconnect_tp()
        assert not self.m._comm_in_library
        return False


def targets_for(R, seed, lo=0, hi=V):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi, (R,), generator=g)
    t[::7] = -100                      # ignored rows
    if R > 3:
        t[3] = V + 5                   # outside the vocabulary: -inf, like any target outside the column range
    return t.to(DEV)


def same_bits(got, want, what):
    for a, b, name in zip(got, want, NAMES):
        assert a.dtype == b.dtype and torch.equal(a, b), f"{what}: {name} differs ({int((a != b).sum())} of {a.numel()} rows)"


def fixture_ids():
    return torch.from_numpy(Z["main_ids"]).to(DEV)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["pull", "copy", "rccl"])
def test_single_rank_group_scores_the_bits_of_the_plain_model(tiny_tp1, transport):
    ids = fixture_ids()
    B, L = ids.shape
    tiny_tp1.forward_body(ids)
    with single_rank_group(synth.CFG_TINY, tiny_sd(), transport, B * ((L + 7) // 8 * 8)) as m:
        m.forward_body(ids)
        for c0, c1 in RANGES:
            for R in (1, 5, 61, B * L):
                rows = torch.arange(B * L, dtype=torch.int32, device=DEV)[:R] if R > 1 else torch.tensor([77], dtype=torch.int32, device=DEV)
                t = targets_for(R, R + c0)
                want = tiny_tp1.token_logprobs(rows, t, c0, c1, return_stats=True)
                got = m.token_logprobs(rows, t, c0, c1, return_stats=True)
                torch.cuda.synchronize()
                same_bits(got, want, f"{transport}, cols [{c0},{c1}), R={R}")
                assert bool((got[0][t < 0] == 0).all())
        assert m.comm_status()["error"] == 0


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_result_is_independent_of_rank_count_and_transport():
    cfg = synth.CFG_PEAKED
    Vp = cfg["vocab_size"]
    sd = synth.synthetic_state_dict(cfg, seed=5, device=DEV)
    head = sd["model.transformer.ff_out.weight"]
    # a planted tie across ranks: two equal head rows, one in rank 0's tiles of every split (below 66 tiles = column 16896),
    # one in the upper half of the vocabulary; the row that reads them (below) is a multiple of that head row
    c_lo, c_hi = 1000, 263 * 256 + 5
    head[c_hi] = head[c_lo]
    g = torch.Generator().manual_seed(17)
    B, L = 2, 61
    ids = torch.randint(0, 126000, (B, L), generator=g).to(DEV)
    Lp = (L + 7) // 8 * 8
    R = B * L
    rows = torch.arange(R, dtype=torch.int32, device=DEV)
    ranges = ((0, Vp), (0, Vp - 100), (1000, 2237))       # whole tiles only; a partial last tile; five tiles (fewer than 8 ranks)
    targets = {}
    for c0, c1 in ranges:
        edge = []
        for k in (2, 4, 8):                              # first and last column of every rank's range, for every split
            for r in range(k):
                t0, t1 = tp_plan.score_tile_slice(c1 - c0, r, k)
                if t1 > t0:
                    edge += [c0 + t0 * 256, min(c1, c0 + t1 * 256) - 1]
        edge = sorted(set(edge))
        assert len(edge) <= R - 16 and c1 - 1 in edge
        t = targets_for(R, 100 + c0, c0, c1).cpu()
        t[16:16 + len(edge)] = torch.tensor(edge)
        targets[(c0, c1)] = t.to(DEV)

    results = {}
    xn_ref = planted = None
    for k in (1, 2, 4, 8):
        if k == 1:
            ctx = single_rank_group(cfg, sd, "pull", B * Lp)
            ranks, streams = [ctx.__enter__()], [torch.cuda.current_stream()]
        else:
            ctx = None
            ranks, streams = tp_group(cfg, sd, k, B * Lp)
        try:
            tp_each(ranks, streams, lambda m: m.forward_body(ids))
            if xn_ref is None:   # the one-rank group's normalised stream, with two planted rows, becomes every rank's
                xn_ref = ranks[0].debug_buffer(0).clone()
                xn_ref[5].zero_()                                              # every logit 0: a tie across ALL tiles and ranks
                xn_ref[9] = (head[c_lo].float() * 40.0).to(torch.bfloat16)     # the two equal head rows win by a wide margin
            for transport in ("pull", "copy"):
                if transport == "copy":
                    for m in ranks:
                        m.set_transport("copy")

                def one(m):
                    m.debug_buffer(0).copy_(xn_ref)
                    return [m.token_logprobs(rows, targets[rg], rg[0], rg[1], return_stats=True) for rg in ranges]

                out = tp_each(ranks, streams, one)
                for m in ranks:
                    status = m.comm_status()
                    assert status["mode"] == transport and status["error"] == 0, status
                for r, res in enumerate(out):
                    results[(k, transport, r)] = res
            if planted is None:   # the materialised logits of the planted row, from the same library
                ranks[0].debug_buffer(0).copy_(xn_ref)
                planted = ranks[0].head_rows(rows[9:10], 0, Vp)[0].clone()
                torch.cuda.synchronize()
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
        del ranks, streams
        torch.cuda.empty_cache()
    ref = results[(1, "pull", 0)]
    for key, res in results.items():
        for rg, got, want in zip(ranges, res, ref):
            same_bits(got, want, f"tp={key[0]} {key[1]} rank {key[2]}, cols {rg}")
    # the planted rows: the lowest column wins a tie, also when the tie spans ranks; and the reference itself is sane
    (lp, lse, arg, mx), (_, _, arg_p, _), (_, _, arg_s, _) = ref
    assert arg[5].item() == 0 and mx[5].item() == 0.0 and arg_p[5].item() == 0 and arg_s[5].item() == 1000
    assert arg[9].item() == c_lo and arg_p[9].item() == c_lo
    assert planted[c_lo] == planted[c_hi] == planted.max() and mx[9].item() == float(planted[c_lo])
    assert int((planted == planted.max()).sum()) == 2, "the tie is between the two planted columns only"
    t_full = targets[ranges[0]]
    inside = (t_full >= 0) & (t_full < Vp)
    assert bool(torch.isfinite(lp[inside]).all()) and bool((lp[t_full < 0] == 0).all()) and bool(torch.isinf(lp[t_full >= Vp]).all())


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_tp2_against_materialised_logits_of_the_same_rank():
    ids = fixture_ids()
    B, L = ids.shape
    ranks, streams = tp_group(synth.CFG_TINY, tiny_sd(), 2, B * ((L + 7) // 8 * 8))
    tp_each(ranks, streams, lambda m: m.forward_body(ids))
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    for c0, c1 in RANGES:
        t = targets_for(B * L, 31 + c0)
        out = tp_each(ranks, streams, lambda m: (m.head_rows(rows, c0, c1), m.token_logprobs(rows, t, c0, c1, return_stats=True)))
        for r, (logits, (lp, lse, arg, mx)) in enumerate(out):    # the logic of test_gpu_score.check_against_logits
            what = f"rank {r}, cols [{c0},{c1})"
            lf = logits.float()
            assert torch.equal(mx, lf.max(1).values), f"{what}: max"
            assert torch.equal(arg.long(), lf.argmax(1) + c0), f"{what}: arg-max"
            lse64 = torch.logsumexp(logits.double(), 1)
            assert float(lse64.abs().max()) < 32.0
            err = float((lse.double() - lse64).abs().max())
            print(f"{what}: max |lse - float64| = {err:.3e}")
            assert err < LSE_TOL, f"{what}: lse off by {err:.3e}"
            inside = (t >= c0) & (t < c1)
            x_t = lf.gather(1, (t - c0).clamp(0, c1 - c0 - 1)[:, None])[:, 0]
            want = torch.where(t < 0, torch.zeros_like(lse), torch.where(inside, x_t - lse, torch.full_like(lse, float("-inf"))))
            assert torch.equal(lp, want), f"{what}: target logit / log-probability"
        assert torch.equal(out[0][0], out[1][0])
        same_bits(out[1][1], out[0][1], f"rank 1 against rank 0, cols [{c0},{c1})")
    for m in ranks:
        assert m.comm_status()["error"] == 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_reuse_the_published_buffers():
    """Three calls enqueued on every rank with no forward (and no host synchronisation) between them, five rounds of the two
    published buffers in all: each result equals that of the same call made on its own."""
    ids = fixture_ids()[:1].repeat(24, 1)
    ids[:, 3] = torch.arange(24, device=DEV) + 40
    B, L = ids.shape
    max_rows = B * ((L + 7) // 8 * 8)
    assert B * L > SCORE_ROUND and max_rows > SCORE_ROUND, "the first call must need two rounds"
    ranks, streams = tp_group(synth.CFG_TINY, tiny_sd(), 2, max_rows)
    tp_each(ranks, streams, lambda m: m.forward_body(ids))
    calls = []
    for i, R in enumerate((B * L, 700, SCORE_ROUND + 9)):
        g = torch.Generator().manual_seed(50 + i)
        rows = torch.randperm(B * L, generator=g)[:R].to(torch.int32).to(DEV)
        calls.append((rows, targets_for(R, 60 + i), *RANGES[i]))
    score = lambda m, c: m.token_logprobs(c[0], c[1], c[2], c[3], return_stats=True)   # noqa: E731
    alone = [tp_each(ranks, streams, lambda m: score(m, c)) for c in calls]
    together = tp_each(ranks, streams, lambda m: [score(m, c) for c in calls])
    for m in ranks:
        assert m.comm_status()["error"] == 0
    for r in range(2):
        for i in range(3):
            same_bits(together[r][i], alone[i][r], f"rank {r}, call {i} back to back against alone")
            same_bits(alone[i][r], alone[i][0], f"rank {r} against rank 0, call {i}")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
# model.score under TP = 2 against TP = 1 on the fixture's ids and labels, per-token NLL in fp32.  The head adds nothing (tests 1
# and 2: the same bits on the same normalised rows); the difference is that of the forward, whose ranks round their partial
# sums to bf16 (tests/test_gpu_tp.py).  Measured on MI355X (profiles/score_tp_parity.txt); the limits are measured + 10 %, the
# convention of tests/test_gpu_parity_depth.py.
# Measured: 81 labelled tokens, mean NLL 12.38: max |difference| 1.575e-2, mean 4.01e-3, max relative to the mean NLL 1.27e-3.
MEASURED = dict(max_abs=0.0157470703125, mean_abs=0.0040125787994008, max_rel_to_mean_nll=0.001271963404347467)


def test_score_tp2_against_tp1(tiny_tp1):
    ids, lab = fixture_ids(), torch.from_numpy(Z["main_labels"]).to(DEV)
    B, L = ids.shape
    want = tiny_tp1.score(ids, lab)
    ranks, streams = tp_group(synth.CFG_TINY, tiny_sd(), 2, B * ((L + 7) // 8 * 8))
    got = tp_each(ranks, streams, lambda m: m.score(ids, lab))
    for m in ranks:
        assert m.comm_status()["error"] == 0
    assert got[0].dtype == torch.float32 and torch.equal(got[0], got[1]), "ranks agree bit for bit"
    valid = lab != -100
    assert bool((got[0][~valid] == 0).all()) and bool(torch.isfinite(got[0]).all())
    diff = (got[0] - want).abs()[valid].double()
    fig = dict(max_abs=float(diff.max()), mean_abs=float(diff.mean()), max_rel_to_mean_nll=float(diff.max() / want[valid].double().mean()))
    print("score TP=2 vs TP=1:", fig, "labelled tokens", int(valid.sum()), "mean NLL", float(want[valid].mean()))
    out_dir = os.path.dirname(PARITY_REPORT)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "score_tp_parity.txt"), "w") as f:
        f.write("model.score on the tiny model, TP = 2 (in-process group, pull transport) vs TP = 1, MI355X, per-token NLL fp32\n")
        f.write(f"labelled tokens {int(valid.sum())}, mean NLL (TP = 1) {float(want[valid].mean())!r}\n")
        for k, v in fig.items():
            f.write(f"{k} {v!r}\n")
    for k, v in fig.items():
        assert MEASURED[k] is not None, f"no measured bound recorded for {k} (first GPU run: {fig})"
        assert v <= MEASURED[k] * 1.1, f"{k}: {v} against measured {MEASURED[k]} + 10 %"


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_forward_labels_on_a_single_rank_group_equals_the_plain_model(tiny_tp1):
    n = Z["main_len"].tolist()
    ids_l = [Z["main_ids"][b, :n[b]].tolist() for b in range(3)]
    lab_l = [Z["main_labels"][b, :n[b]].tolist() for b in range(3)]
    tt = torch.from_numpy(Z["t"])
    B, L = Z["main_ids"].shape

    def same(a, b, what):
        if isinstance(a, dict):
            assert sorted(a) == sorted(b), what
            for k in a:
                same(a[k], b[k], f"{what}[{k}]")
        elif isinstance(a, (tuple, list)):
            assert len(a) == len(b), what
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, f"{what}[{i}]")
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what

    with single_rank_group(synth.CFG_TINY, tiny_sd(), "pull", B * ((L + 7) // 8 * 8)) as m:
        for kw in (dict(), dict(t=tt), dict(compute_separate_losses=False), dict(return_dict=True),
                   dict(return_dict=True, compute_separate_losses=False)):
            want = tiny_tp1(ids_l, labels=lab_l, **kw)
            got = m(ids_l, labels=lab_l, **kw)
            torch.cuda.synchronize()
            same(got, want, f"forward(labels=..., {kw})")
        ids, lab = fixture_ids(), torch.from_numpy(Z["main_labels"]).to(DEV)
        assert torch.equal(m.score(ids, lab), tiny_tp1.score(ids, lab))
        assert m.comm_status()["error"] == 0


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_rows_beyond_the_comms_capacity_are_refused():
    ids = fixture_ids()[:2, :40].contiguous()
    B, L = ids.shape
    max_rows = B * L                                       # L = 40: no pad rows, the comm holds exactly the forward's rows
    ranks, streams = tp_group(synth.CFG_TINY, tiny_sd(), 2, max_rows)
    tp_each(ranks, streams, lambda m: m.forward_body(ids))
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    t = targets_for(B * L, 5)
    before = tp_each(ranks, streams, lambda m: m.token_logprobs(rows, t, return_stats=True))
    too_many = torch.zeros(max_rows + 1, dtype=torch.int32, device=DEV)
    for m in ranks:                                        # refused on the host, before anything is enqueued
        with pytest.raises(abi.MmadaError, match=f"exceed the {max_rows} rows this handle's comm was created for"):
            m.token_logprobs(too_many, torch.zeros(max_rows + 1, dtype=torch.long, device=DEV))
    torch.cuda.synchronize()
    after = tp_each(ranks, streams, lambda m: m.token_logprobs(rows, t, return_stats=True))   # the hand-off counters still agree
    for r, m in enumerate(ranks):
        assert m.comm_status()["error"] == 0
        same_bits(after[r], before[r], f"rank {r} after the refused call")
