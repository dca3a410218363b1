"""Sampling on the GPU: mmada_head_sample / model.sample_tokens (the EPI_ROWSAMPLE epilogue of the head GEMM and
rowsample_combine_kernel), mmada_text_select_sampled and generate_ti2ti(text_sampler="device").  The draw is the first-index arg-max
of logits + T * g over the repo's own logits (head_rows) and the device's own noise (mmada_probe_gumbel), its log-probability and
statistics are the scoring head's (token_logprobs): everything is exact but the accuracy of g itself, which has a derived bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, NOISY_CASES, STUB_CB, STUB_TEXT_VOCAB, ReplayCpuRng, tiny_job, tiny_sd
from mmada_parallel_amd import abi, synth
from mmada_parallel_amd.abi import MmadaError
from test_gpu_score import head8b, tiny_model   # noqa: F401  (the same fixtures: the tiny model, one 8B-width block + full head)
from test_gpu_score_tp import single_rank_group

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = synth.CFG_TINY["vocab_size"]
Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
SEED = 0x0123456789abcdef
TEMPS = (0.0, 0.7, 100.0)
RANGES = [(40, 48), (512, 512 + 259), (512 + 256, 512 + 259), (1000, 1000 + 1237), (synth.TEXT_VOCAB, synth.TEXT_VOCAB + synth.CODEBOOK), (0, V)]


def probe(seed, counter, row0, R, col0, N, words=True, g=True):
    """mmada_probe_gumbel: (words as int64 [R, N], g fp32 [R, N]) of rows row0.. and columns col0.."""
    w = torch.empty((R, N), dtype=torch.int32, device=DEV) if words else None
    gg = torch.empty((R, N), dtype=torch.float32, device=DEV) if g else None
    abi.check(abi.lib().mmada_probe_gumbel(seed, counter, row0, R, col0, N, abi.ptr(w), abi.ptr(gg), abi.stream_ptr()), "mmada_probe_gumbel")
    return (w.long() & 0xFFFFFFFF) if words else None, gg


def g_float64(words):
    """-log(-log(u)) in float64 on the exact u = (2 * (word >> 9) + 1) / 2^24."""
    u = (2 * (words >> 9) + 1).double() * 2.0 ** -24
    return -torch.log(-torch.log(u))


def g_bound_ratio(g, g64):
    return float(((g.double() - g64).abs() / (2.0 ** -21 * (1.0 + g64.abs()))).max())


def counter_at(c):
    return torch.tensor([c], dtype=torch.int64, device=DEV)


def draw(model, rows, T, c0, c1, seed, c):
    ctr = counter_at(c)
    out = model.sample_tokens(rows, T, c0, c1, seed=seed, counter=ctr, return_stats=True)
    torch.cuda.synchronize()
    assert int(ctr) == c + 1, "the counter advances by one per call"
    return out


def keys_of(logits, T, g):
    """fadd_rn(x, fmul_rn(T, g)): a separate torch multiply and add (no alpha=, no fused multiply-add)."""
    tg = torch.tensor(T, dtype=torch.float32, device=DEV) * g
    return logits.float() + tg


def check_draw(model, rows, c0, c1, temps=TEMPS, seed=SEED, c=7, what=""):
    """ids = first-index arg-max of the keys; logprobs / lse / argmax / max = the scoring head's.  Returns {T: outputs}."""
    R, N = rows.numel(), c1 - c0
    logits = model.head_rows(rows, c0, c1)
    _, g = probe(seed, c, 0, R, c0, N, words=False)
    _, lse_ref, arg_ref, max_ref = model.token_logprobs(rows, torch.full((R,), -1, device=DEV), c0, c1, return_stats=True)
    outs = {}
    for T in temps:
        ids, lp, lse, arg, mx = outs[T] = draw(model, rows, T, c0, c1, seed, c)
        want = (keys_of(logits, T, g).argmax(1) + c0).int()
        print(f"{what}: R={R} cols [{c0},{c1}) T={T}: rows with a wrong id {int((ids != want).sum())}, draws that are the arg-max "
              f"{int((ids == arg).sum())}")
        assert torch.equal(ids, want), f"{what} T={T}: ids are not the arg-max of logits + T * g"
        assert torch.equal(lp, model.token_logprobs(rows, ids.long(), c0, c1)), f"{what} T={T}: log-probability of the draw"
        assert torch.equal(lse, lse_ref) and torch.equal(arg, arg_ref) and torch.equal(mx, max_ref), f"{what} T={T}: lse / argmax / max"
        if T == 0:
            assert torch.equal(ids, arg), f"{what}: T = 0 is the arg-max"
    return outs


def tiny_rows(R, B, L):
    return torch.arange(B * L, dtype=torch.int32, device=DEV)[:R] if R > 1 else torch.tensor([77], dtype=torch.int32, device=DEV)


def test_probe_words_equal_the_host_and_g_is_within_the_bound():
    lib = abi.lib()
    R, N, row0, col0, c = 64, 1237, 3, 1001, (1 << 32) + 5        # an odd first column, a counter above 2^32
    words, g = probe(SEED, c, row0, R, col0, N)
    host = torch.tensor([[lib.mmada_sample_word(SEED, c, row0 + r, col0 + k) for k in range(N)] for r in range(R)], dtype=torch.int64)
    assert torch.equal(words.cpu(), host)
    ratio = g_bound_ratio(g, g_float64(words))
    print(f"probe g against float64 on [{R}, {N}]: worst |g - g64| / (2^-21 (1 + |g64|)) = {ratio:.3f}")
    assert ratio <= 1.0


def test_g_is_accurate_for_every_value_of_u():
    """Every one of the 2^23 values of u through the device's g (the probe's enumeration mode: element i takes the word i << 9):
    |g - g64| <= 2^-21 (1 + |g64|), g64 = -log(-log(u)) in float64 on the exact u.

    Why this bound.  g = -log(L), L = -log(u), both logarithms in fp32 with an error of at most 2 ulp, i.e. a relative error of at
    most 2 * 2^-23 = 2^-22 (an ulp is at most 2^-23 of the value).  u is exact, so L carries a relative error delta <= 2^-22; the
    outer logarithm turns a relative error of its argument into an ABSOLUTE error of its result, log(L (1 + delta)) - log(L) =
    log1p(delta) ~ delta <= 2^-22, and adds its own 2 ulp, at most 2^-22 |g|.  Together 2^-22 (1 + |g|); the bound is twice that."""
    n = 1 << 23
    words, g = probe(0, 0, -1, 1 << 11, 0, 1 << 12)
    assert torch.equal(words.view(-1), torch.arange(n, device=DEV) << 9)
    g64 = g_float64(words)
    assert bool(torch.isfinite(g).all()) and float(g.min()) < -2.8 and float(g.max()) > 16.6
    ratio = g_bound_ratio(g, g64)
    print(f"all 2^23 values of u: worst |g - g64| / (2^-21 (1 + |g64|)) = {ratio:.3f}, worst |g - g64| = {float((g.double() - g64).abs().max()):.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("c0, c1", RANGES)
def test_tiny_model_draw_is_the_argmax_of_the_key(tiny_model, c0, c1):
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    assert V == 526 * 256
    tiny_model.forward_body(ids)
    for R in (1, 5, 61, B * L):       # R = 1, not a multiple of 8, every row
        outs = check_draw(tiny_model, tiny_rows(R, B, L), c0, c1, what=f"tiny R={R}")
        for T in TEMPS:
            assert int(outs[T][0].min()) >= c0 and int(outs[T][0].max()) < c1


def test_tiny_model_counter_seed_subrange_and_window(tiny_model):
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    tiny_model.forward_body(ids)
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    R, c, T = B * L, 41, 100.0
    a = draw(tiny_model, rows, T, 0, V, SEED, c)
    again = draw(tiny_model, rows, T, 0, V, SEED, c)
    for x, y in zip(a, again):
        assert torch.equal(x, y), "the counter reset to c repeats the bits"
    nxt = draw(tiny_model, rows, T, 0, V, SEED, c + 1)
    other = draw(tiny_model, rows, T, 0, V, SEED ^ 0x55, c)
    hi = draw(tiny_model, rows, T, 0, V, SEED, c + (1 << 32))
    for b, name in ((nxt, "the next counter"), (other, "another seed"), (hi, "a counter 2^32 further")):
        differ = float((a[0] != b[0]).float().mean())
        print(f"{name}: {differ:.3f} of the rows draw another token")
        assert differ > 0.5, name
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])          # lse / argmax do not depend on the noise

    # the model's own counter: created at 0, advanced by the library
    tiny_model._sample_counter = None
    first = tiny_model.sample_tokens(rows, 0.7, seed=SEED)
    assert int(tiny_model.sample_counter) == 1
    tiny_model.sample_tokens(rows, 0.7, seed=SEED)
    assert int(tiny_model.sample_counter) == 2
    assert torch.equal(first[0], draw(tiny_model, rows, 0.7, 0, V, SEED, 0)[0])

    # a draw on a sub-range is the arg-max of the WHOLE vocabulary's keys restricted to the range
    c0, c1 = 1000, 1000 + 1237
    _, g = probe(SEED, c, 0, R, 0, V, words=False)
    keys = keys_of(tiny_model.head_rows(rows, 0, V), 0.7, g)
    sub = draw(tiny_model, rows, 0.7, c0, c1, SEED, c)
    assert torch.equal(sub[0], (keys[:, c0:c1].argmax(1) + c0).int())
    del keys, g

    # windowed forward: rows inside the consumed window
    tiny_model.forward_body(ids, consumed=(20, 50))
    try:
        wrows = (torch.arange(B)[:, None] * L + torch.arange(20, 50)[None, :]).flatten().int().to(DEV)
        check_draw(tiny_model, wrows, 0, V, what="tiny windowed")
        check_draw(tiny_model, wrows, 1000, 1000 + 1237, what="tiny windowed, odd range")
    finally:
        tiny_model.forward_body(ids)


def test_planted_ties(tiny_model):
    """A zeroed row of the resident stream: every logit of the row is 0 — one tie across all column tiles, waves and lanes."""
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    tiny_model.forward_body(ids)
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    Lp = (L + 7) // 8 * 8
    view = tiny_model._stream_view().view(-1, tiny_model.config.d_model)
    tied = [5, Lp + 17]                                             # stream rows of (b = 0, l = 5) and (b = 1, l = 17)
    trow = [5, L + 17]
    for r in tied:
        view[r].zero_()
    try:
        for c0, c1 in ((0, V), (1000, 1000 + 1237), (512 + 256, 512 + 259), (4096 + 8, 4096 + 8 + 2048)):
            outs = check_draw(tiny_model, rows, c0, c1, temps=(0.0, 0.7), c=3, what="planted ties")
            _, g = probe(SEED, 3, 0, B * L, c0, c1 - c0, words=False)
            for r in trow:
                assert bool((tiny_model.head_rows(rows[r:r + 1], c0, c1) == 0).all())
                assert int(outs[0.0][0][r]) == c0, "T = 0 on an all-equal row: the first column"
                assert int(outs[0.7][0][r]) == c0 + int(g[r].argmax()), "T > 0 on an all-equal row: the arg-max of g"
    finally:
        tiny_model.forward_body(ids)


def test_8b_head_configurations_memory_and_graph(head8b):
    model = head8b
    lib = abi.lib()
    gen = torch.Generator().manual_seed(11)
    L = 700                                       # not a multiple of any tile height (320 / 256 / 160 / 192 / 128)
    ids = torch.randint(0, 126000, (1, L), generator=gen).to(DEV)
    model.forward_body(ids)
    rows = torch.arange(L, dtype=torch.int32, device=DEV)
    c, T = 11, 0.7
    ref = check_draw(model, rows, 0, model.vocab, temps=(T,), c=c, what="8B head")[T]      # once, under the planner's pick
    try:
        for code in (-1, 0, 1, 2, 3, 1128, 1256, 1320):
            abi.check(lib.mmada_set_option(b"gemm_config", code), "set_option")
            got = draw(model, rows, T, 0, model.vocab, SEED, c)
            for a, b, name in zip(got, ref, ("ids", "logprobs", "lse", "argmax", "max")):
                assert torch.equal(a, b), f"gemm_config {code}: {name} differ from the planner's pick"
    finally:
        lib.mmada_set_option(b"gemm_config", -1)

    # memory: the record buffer is 32 bytes per row and tile + 4 per row, and torch allocates the outputs only
    own = lib.mmada_score_buffer_bytes(model._handle)
    assert 0 < own <= (L + 7) // 8 * 8 * (526 * 32 + 4), own
    ctr = counter_at(c)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    out = model.sample_tokens(rows, T, seed=SEED, counter=ctr)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated(DEV) - before
    print(f"sample at R={L}: torch peak +{grew} B, library record buffer {own} B (logits would be {L * model.vocab * 2} B)")
    assert grew < L * model.vocab * 2 // 10 and lib.mmada_score_buffer_bytes(model._handle) == own
    del out

    # a captured call draws fresh noise on every replay: the counter lives in device memory
    eager = [draw(model, rows, T, 0, model.vocab, SEED, c + i) for i in range(2)]
    ctr = counter_at(c)
    outs = [torch.full_like(e, -7) for e in eager[0]]
    replays = []
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        abi.check(lib.mmada_graph_begin(abi.stream_ptr()), "graph_begin")
        rc = lib.mmada_head_sample(model._handle, rows.data_ptr(), L, 0, model.vocab, T, SEED, ctr.data_ptr(), *[o.data_ptr() for o in outs],
                                   abi.stream_ptr())
        if rc:
            lib.mmada_graph_abort(abi.stream_ptr())
        abi.check(rc, "mmada_head_sample under capture")
        gr = C.c_void_p()
        abi.check(lib.mmada_graph_end(abi.stream_ptr(), C.byref(gr)), "graph_end")
        for _ in range(2):
            abi.check(lib.mmada_graph_launch(gr, abi.stream_ptr()), "graph_launch")
            side.synchronize()
            replays.append([o.clone() for o in outs])
        lib.mmada_graph_destroy(gr)
    torch.cuda.current_stream().wait_stream(side)
    assert int(ctr) == c + 2
    for i in range(2):
        for a, b in zip(replays[i], eager[i]):
            assert torch.equal(a, b), f"replay {i} is not the eager call at counter c + {i}"
    assert not torch.equal(replays[0][0], replays[1][0])


def test_text_select_sampled_commits_by_the_rule(tiny_model):
    lib = abi.lib()
    mask = int(tiny_model.config.get("mask_token_id", synth.MASK))
    gen = torch.Generator().manual_seed(5)
    B, L, ts, T = 2, 40, 10, 16
    ids = torch.randint(0, 2000, (B, L), generator=gen)
    masked = torch.zeros(B, T, dtype=torch.bool)
    masked[0, [0, 3, 4, 7, 8, 12, 15]] = True
    masked[1, [1, 2, 9]] = True
    ids[:, ts:ts + T][masked] = mask
    ids = ids.to(DEV)
    tiny_model.forward_body(ids)
    rows = (torch.arange(B)[:, None] * L + ts + torch.arange(T)[None, :]).flatten().int().to(DEV)
    k = [3, 0]
    c, temp = 9, 0.7
    x0, lp, *_ = draw(tiny_model, rows, temp, 0, V, SEED, c)
    # the commit rule: masked positions only, confidence descending, then position ascending, k[b] winners
    want = ids.clone()
    conf = torch.where(masked.to(DEV), lp.view(B, T).double(), torch.full((B, T), float("-inf"), dtype=torch.float64, device=DEV))
    for b in range(B):
        order = sorted(range(T), key=lambda t: (-float(conf[b, t]), t))
        for t in order[:k[b]]:
            assert bool(masked[b, t])
            want[b, ts + t] = int(x0[b * T + t])
    got = ids.clone()
    ctr = counter_at(c)
    scratch = torch.empty(B * T * 16, dtype=torch.uint8, device=DEV)
    k_dev = torch.tensor(k, dtype=torch.int32, device=DEV)
    abi.check(lib.mmada_text_select_sampled(tiny_model._handle, rows.data_ptr(), B, T, temp, SEED, ctr.data_ptr(), got.data_ptr(), L, ts,
                                            k_dev.data_ptr(), scratch.data_ptr(), abi.stream_ptr()), "mmada_text_select_sampled")
    torch.cuda.synchronize()
    assert int(ctr) == c + 1
    assert torch.equal(got, want)
    changed = (got != ids)
    assert int(changed[0].sum()) == 3 and int(changed[1].sum()) == 0, "k = [3, 0]: three commits in row 0, row 1 untouched"
    assert bool((changed[:, ts:ts + T] <= masked.to(DEV)).all()) and not bool(changed[:, :ts].any()) and not bool(changed[:, ts + T:].any())


def _generate(model, job, **kw):
    from mmada_parallel_amd import generate_ti2ti

    args = dict(text_steps=8, timesteps=4, temperature=0.0, text_temperature=0.7, cfg_scale=0.0, cfg_img=4.0,
                uncon_text=job["uncon_text"], uncon_image=job["uncon_image"], return_state=True)
    args.update(kw)
    return generate_ti2ti(model, job["input_ids"].to(DEV), job["text_start"], job["text_end"], job["image_start"], job["seq_len"],
                          job["newline_every"], **args)


def test_generate_ti2ti_with_the_device_sampler(tiny_model):
    job = tiny_job()
    ts, te = job["text_start"], job["text_end"]
    calls = []
    orig = tiny_model.head_rows

    def spy(rows, c0, c1, out=None):
        calls.append((rows.numel(), c1 - c0))
        return orig(rows, c0, c1, out=out)

    tiny_model.head_rows = spy
    try:
        a = _generate(tiny_model, job, text_sampler="device", sampler_seed=1234)
    finally:
        del tiny_model.head_rows
    assert calls and all(width == synth.CODEBOOK for _, width in calls), "text_sampler='device' never materialises text logits"
    b = _generate(tiny_model, job, text_sampler="device", sampler_seed=1234)
    c = _generate(tiny_model, job, text_sampler="device", sampler_seed=1235)
    assert torch.equal(a[2], b[2]) and a[1] == b[1], "the same seed repeats the run"
    assert not torch.equal(a[2][:, ts:te], c[2][:, ts:te]), "another seed draws another text"
    assert int((a[2][0, ts:te] == synth.MASK).sum()) == 0 and len(a[1]) == te - ts


def test_generate_ti2ti_torch_sampler_still_reproduces_the_recording(tiny_model):
    from mmada_parallel_amd import generate_ti2ti
    from test_gpu_model import _stubbed

    name = "noisy_both"
    z = np.load(os.path.join(GOLDEN, "sampler_noisy.npz"))
    calls_ref = torch.from_numpy(z[name + "_calls"])
    job, kw = tiny_job(), NOISY_CASES[name]
    stub = _stubbed(tiny_model, int(z[name + "_seed"]), STUB_TEXT_VOCAB + STUB_CB)
    gen = torch.Generator().manual_seed(int(z[name + "_gen_seed"]))
    generate_ti2ti(stub, job["input_ids"].to(DEV), job["text_start"], job["text_end"], job["image_start"], job["seq_len"],
                   job["newline_every"], uncon_text=job["uncon_text"], uncon_image=job["uncon_image"], tokenizer=None,
                   text_vocab_size=STUB_TEXT_VOCAB, codebook_size=STUB_CB, generator=gen, rng=ReplayCpuRng(), text_sampler="torch", **kw)
    got = torch.cat(stub.calls, 0)
    assert got.shape == calls_ref.shape and torch.equal(got, calls_ref)


def test_refusals(tiny_model):
    job = tiny_job()
    for kw, match in ((dict(text_sampler="device"), "sampler_seed"),
                      (dict(text_sampler="device", sampler_seed=1, text_temperature=0.0), "text_temperature"),
                      (dict(text_sampler="device", sampler_seed=1, remasking="random"), "low_confidence"),
                      (dict(text_sampler="gpu", sampler_seed=1), "text_sampler")):
        with pytest.raises(ValueError, match=match):
            _generate(tiny_model, job, **kw)

    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    rows = torch.arange(8, dtype=torch.int32, device=DEV)
    # a forward resident in micro-batched lanes: row indices would restart per lane
    os.environ["MMADA_MICROBATCH"] = "1"
    try:
        tiny_model.forward_body(ids)
        assert tiny_model._resident.split is not None
        with pytest.raises(NotImplementedError, match="lanes"):
            tiny_model.sample_tokens(rows, 0.7, seed=1)
        with pytest.raises(ValueError, match="lanes"):
            _generate(tiny_model, dict(job, input_ids=job["input_ids"].repeat(2, 1)), text_sampler="device", sampler_seed=1)
    finally:
        os.environ.pop("MMADA_MICROBATCH", None)
        tiny_model.forward_body(ids)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            tiny_model.sample_tokens(rows, bad, seed=1)
    ctr = counter_at(0)
    out = [torch.empty(8, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32)]
    rc = abi.lib().mmada_head_sample(tiny_model._handle, rows.data_ptr(), 8, 0, V, float("inf"), 1, ctr.data_ptr(), out[0].data_ptr(),
                                     out[1].data_ptr(), None, None, None, abi.stream_ptr())
    assert rc != 0 and b"finite" in abi.lib().mmada_last_error() and int(ctr) == 0

    with single_rank_group(synth.CFG_TINY, tiny_sd(), "pull", B * ((L + 7) // 8 * 8)) as m:
        m.forward_body(ids)
        out = [torch.empty(8, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32)]
        ctr = counter_at(0)
        rc = abi.lib().mmada_head_sample(m._handle, rows.data_ptr(), 8, 0, V, 0.7, 1, ctr.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                         None, None, None, abi.stream_ptr())
        with pytest.raises(MmadaError, match="one rank"):
            abi.check(rc, "mmada_head_sample")
        assert b"vocabulary-parallel" in abi.lib().mmada_last_error() and int(ctr) == 0
        with pytest.raises(NotImplementedError, match="one rank"):
            m.sample_tokens(rows, 0.7, seed=1)
        with pytest.raises(ValueError, match="one rank"):
            _generate(m, job, text_sampler="device", sampler_seed=1)
        assert m.comm_status()["error"] == 0
