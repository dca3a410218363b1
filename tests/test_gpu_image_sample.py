"""The image step sampled on the GPU: mmada_image_sample (image_row_kernel's Gumbel-max draw beside its statistics),
mmada_image_commit_sampled (the re-mask noise computed in the commit), mmada_probe_normal, and generate_ti2ti(image_sampler="device")
with its hipGraph replay.  Everything is equality — against torch's own bf16 ops, the device's own noise (mmada_probe_gumbel /
mmada_probe_normal), mmada_image_probs, mmada_image_commit and the row head — except the accuracy of z itself, which has a derived
bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, NOISY_CASES, STUB_CB, STUB_TEXT_VOCAB, ReplayCpuRng, bits, tiny_job, tiny_sd
from mmada_parallel_amd import abi, synth
from mmada_parallel_amd.generators.parallel_generator import TorchRng, _ti2ti_steps
from test_gpu_kernels import handle   # noqa: F401  (a tiny handle: the sampler entry points only need its cfg)
from test_gpu_score import tiny_model   # noqa: F401
from test_gpu_score_tp import single_rank_group
from test_image_sample_host import IMAGE_COUNTER, Z_TOL, mirror_normal_words, z_float64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0123456789abcdef
Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
# (B, N, CB, cfg_scale, cfg_img, col0, quant): one 16-byte chunk with almost every thread idle; the production codebook at an odd
# row count; the LDS limit with an odd col0; quantised logits with many equal l
CASES = [(1, 5, 8, 0.0, 0.0, 0, None), (2, 100, 8192, 2.5, 4.0, 126356, None), (1, 3, 16384, 0.0, 4.0, 1001, None),
         (3, 16, 512, 3.0, 4.0, 2, 2)]


def st():
    return abi.stream_ptr()


def dev_i64(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


_INPUTS = {}


def image_inputs(B, N, CB, quant):
    """Seeded logits as in test_gpu_kernels.py::test_image_probs_bit_exact, made once per shape: (cond, unc_text, unc_img) on the CPU
    and on the device."""
    key = (B, N, CB, quant)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(N + CB)
        c = torch.randn(B, N, CB, generator=g) * 1.5
        if quant:
            c = (c * quant).round() / quant
        c = c.to(torch.bfloat16)
        ut = (c.float() + torch.randn(B, N, CB, generator=g) * 0.5).to(torch.bfloat16)
        ui = (c.float() + torch.randn(B, N, CB, generator=g) * 0.5).to(torch.bfloat16)
        _INPUTS[key] = ((c, ut, ui), tuple(t.to(DEV) for t in (c, ut, ui)))
    return _INPUTS[key]


def combined_logits(c, ut, ui, cs, ci):
    """generators/parallel_generator.py:282-289 with torch's own bf16 ops on the CPU, as test_oracle_golden.py::
    test_image_probs_against_torch_ops does; a null unconditional input drops its term."""
    il = c
    if cs != 0.0 and ut is not None:
        il = il + cs * (c - ut)
    if ci != 0.0 and ui is not None:
        il = il + ci * (c - ui)
    return il


def image_sample(h, cd, utd, uid, B, N, CB, cs, ci, col0, seed, counter, stats=False):
    """mmada_image_sample: (sampled int32 [B, N], p_sel bf16 [B, N]) and, with stats, (argmax, pmax) too."""
    sampled = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    p_sel = torch.empty((B, N), dtype=torch.bfloat16, device=DEV)
    am = torch.full((B, N), -7, dtype=torch.int32, device=DEV) if stats else None
    pm = torch.empty((B, N), dtype=torch.bfloat16, device=DEV) if stats else None
    abi.check(abi.lib().mmada_image_sample(h, cd.data_ptr(), abi.ptr(utd), abi.ptr(uid), B, N, CB, cs, ci, col0, seed, counter.data_ptr(),
                                           sampled.data_ptr(), p_sel.data_ptr(), abi.ptr(am), abi.ptr(pm), st()), "mmada_image_sample")
    return (sampled, p_sel, am, pm) if stats else (sampled, p_sel)


def probe_gumbel(seed, counter, R, col0, N):
    g = torch.empty((R, N), dtype=torch.float32, device=DEV)
    abi.check(abi.lib().mmada_probe_gumbel(seed, counter, 0, R, col0, N, None, g.data_ptr(), st()), "mmada_probe_gumbel")
    return g


def probe_normal(seed, counter, row0, R):
    """mmada_probe_normal: (words int64 [R, 2], z fp32 [R], z bf16 [R])."""
    w = torch.empty((R, 2), dtype=torch.int32, device=DEV)
    z = torch.empty(R, dtype=torch.float32, device=DEV)
    zb = torch.empty(R, dtype=torch.bfloat16, device=DEV)
    abi.check(abi.lib().mmada_probe_normal(seed, counter, row0, R, w.data_ptr(), z.data_ptr(), zb.data_ptr(), st()), "mmada_probe_normal")
    return w.long() & 0xFFFFFFFF, z, zb


def test_probe_words_and_z():
    """The device's words equal the host mirror, the bf16 output is torch's rounding of the fp32 one, and |z - z64| <= 2^-17 over 2^16
    rows at a counter above 2^32, z64 = sqrt(-2 log u1) cos(2 pi u2) in float64 on the exact u.

    Why this bound.  It assumes logf and cosf are off by at most 2 ulp, as test_gpu_sample.py::test_g_is_accurate_for_every_value_of_u
    does for logf.  u1 is exact, so logf(u1) carries a relative error of at most 2^-22; the product with -2 is exact; the square root
    halves that and adds its own rounding, 2^-24: the radius has a relative error below 2^-22.  The angle is the product of the fp32
    constant 2 pi (relative error 2^-25.1) and the exact u2, rounded once: an absolute error below 2 pi * 2^-23.  The cosine's slope is
    at most 1, so that is also the error it passes on, and cosf adds at most 2^-22 of its own (2 ulp of a value below 1):
    |error of the cosine| <= 2 pi * 2^-23 + 2^-22 = 9.9e-7.  The radius is at most sqrt(48 ln 2) = 5.77, so the product is off by at
    most 5.77 * 9.9e-7 + 2^-22 * 5.77 + its own rounding 2^-24 * 5.77 = 7.4e-6 < 2^-17 = 7.63e-6, absolute."""
    lib = abi.lib()
    R, row0, c = 1 << 16, 3, (1 << 32) + 5
    words, z, zb = probe_normal(SEED, c, row0, R)
    r = np.arange(row0, row0 + R, dtype=np.uint64)
    w0, w1 = mirror_normal_words(SEED, c, r)
    assert np.array_equal(words.cpu().numpy(), np.stack([w0, w1], 1).astype(np.int64)), "the device's words are not the mirror's"
    assert torch.equal(bits(zb), bits(z.to(torch.bfloat16))), "z_bf16 is not the bf16 rounding of z"
    err = np.abs(z.cpu().double().numpy() - z_float64(w0, w1))
    host = np.array([lib.mmada_sample_normal(SEED, c, int(x)) for x in r[:4096]], dtype=np.float64)
    print(f"device z against float64 Box-Muller on {R} rows: worst |z - z64| = {err.max():.3e} (limit {Z_TOL:.3e}); against the host's "
          f"fp32 z on 4096 rows: worst {np.abs(z[:4096].cpu().double().numpy() - host).max():.3e}")
    assert bool(torch.isfinite(z).all()) and err.max() <= Z_TOL
    # only some outputs requested
    only = torch.empty(8, dtype=torch.bfloat16, device=DEV)
    abi.check(lib.mmada_probe_normal(SEED, c, row0, 8, None, None, only.data_ptr(), st()), "mmada_probe_normal")
    assert torch.equal(bits(only), bits(zb[:8]))


@pytest.mark.parametrize("B,N,CB,cs,ci,col0,quant", CASES)
def test_draw_is_the_argmax_of_the_key(handle, B, N, CB, cs, ci, col0, quant):
    (c, ut, ui), (cd, utd, uid) = image_inputs(B, N, CB, quant)
    cnt = IMAGE_COUNTER + 3
    ctr = dev_i64(cnt)
    g = probe_gumbel(SEED, cnt, B * N, col0, CB).cpu()
    variants = [(True, True), (False, True), (True, False), (False, False)] if cs != 0.0 and ci != 0.0 else [(True, True), (False, False)]
    first = None
    for has_t, has_i in variants:
        l = combined_logits(c, ut if has_t else None, ui if has_i else None, cs, ci).float().view(B * N, CB)
        want = (l + g).argmax(1).int().view(B, N)          # the CPU's arg-max: the first index on equal keys
        sampled, _ = image_sample(handle, cd, utd if has_t else None, uid if has_i else None, B, N, CB, cs, ci, col0, SEED, ctr)
        wrong = int((sampled.cpu() != want).sum())
        print(f"B={B} N={N} CB={CB} col0={col0} unc_text={has_t} unc_img={has_i}: rows with a wrong draw {wrong}, draws that are the "
              f"arg-max of l {int((want == l.argmax(1).int().view(B, N)).sum())} of {B * N}")
        assert wrong == 0, "sampled is not the first-index arg-max of l + g"
        assert int(ctr) == cnt, "mmada_image_sample must not write the counter"
        first = sampled if first is None else first
    if B * N * CB >= 1 << 12:
        other_c, _ = image_sample(handle, cd, utd, uid, B, N, CB, cs, ci, col0, SEED, dev_i64(cnt + 1))
        other_s, _ = image_sample(handle, cd, utd, uid, B, N, CB, cs, ci, col0, SEED ^ 0x55, ctr)
        assert not torch.equal(first, other_c), "another counter changes some draw"
        assert not torch.equal(first, other_s), "another seed changes some draw"


@pytest.mark.parametrize("B,N,CB,cs,ci,col0,quant", CASES)
def test_outputs_agree_with_image_probs(handle, B, N, CB, cs, ci, col0, quant):
    _, (cd, utd, uid) = image_inputs(B, N, CB, quant)
    probs = torch.empty(B, N, CB, dtype=torch.bfloat16, device=DEV)
    am_ref = torch.empty(B, N, dtype=torch.int32, device=DEV)
    pm_ref = torch.empty(B, N, dtype=torch.bfloat16, device=DEV)
    abi.check(abi.lib().mmada_image_probs(handle, cd.data_ptr(), utd.data_ptr(), uid.data_ptr(), B, N, CB, cs, ci, probs.data_ptr(),
                                          am_ref.data_ptr(), pm_ref.data_ptr(), st()), "mmada_image_probs")
    ctr = dev_i64(IMAGE_COUNTER)
    sampled, p_sel, am, pm = image_sample(handle, cd, utd, uid, B, N, CB, cs, ci, col0, SEED, ctr, stats=True)
    assert int(sampled.min()) >= 0 and int(sampled.max()) < CB
    assert torch.equal(bits(p_sel), bits(probs.gather(-1, sampled.long()[..., None]).squeeze(-1))), "p_sel is not probs[sampled]"
    assert torch.equal(am, am_ref) and torch.equal(bits(pm), bits(pm_ref)), "argmax_out / pmax_out differ from mmada_image_probs"
    bare, p_bare = image_sample(handle, cd, utd, uid, B, N, CB, cs, ci, col0, SEED, ctr)          # null for both: accepted
    assert torch.equal(bare, sampled) and torch.equal(bits(p_bare), bits(p_sel))


def commit_inputs(case):
    """The inputs of test_gpu_kernels.py::test_image_commit_bit_exact."""
    g = torch.Generator().manual_seed({"fresh": 1, "half_known": 2, "all_known": 3, "one_unknown": 4}[case])
    B, N, L = 2, 256, 400
    pos = torch.sort(torch.randperm(L - 10, generator=g)[:N]).values + 5
    ids = torch.randint(0, 1000, (B, L), generator=g)
    known = {"fresh": 0, "half_known": N // 2, "all_known": N, "one_unknown": N - 1}[case]
    for b in range(B):
        perm = torch.randperm(N, generator=g)
        ids[b, pos] = synth.MASK
        kn = pos[perm[:known]]
        ids[b, kn] = synth.TEXT_VOCAB + torch.randint(0, synth.CODEBOOK, (known,), generator=g)
    sampled = torch.randint(0, synth.CODEBOOK, (B, N), generator=g, dtype=torch.int32)
    # bf16 probabilities from a coarse set -> massive ties in the log-confidence (stable order matters)
    p = (torch.randint(1, 40, (B, N), generator=g).float() / 4096).to(torch.bfloat16)
    return B, N, L, ids.to(DEV), pos.to(torch.int32).to(DEV), sampled.to(DEV), p.to(DEV)


def commit_by_value(h, ids, B, L, pos, N, sampled, p, noise, temp, mlen):
    out = ids.clone()
    abi.check(abi.lib().mmada_image_commit(h, out.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p.data_ptr(), noise.data_ptr(),
                                           temp, mlen.data_ptr(), synth.TEXT_VOCAB, synth.CODEBOOK, st()), "mmada_image_commit")
    return out


def commit_sampled(h, ids, B, L, pos, N, sampled, p, temp_dev, seed, ctr, mlen):
    out = ids.clone()
    abi.check(abi.lib().mmada_image_commit_sampled(h, out.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p.data_ptr(),
                                                   temp_dev.data_ptr(), seed, ctr.data_ptr(), mlen.data_ptr(), synth.TEXT_VOCAB,
                                                   synth.CODEBOOK, st()), "mmada_image_commit_sampled")
    return out


@pytest.mark.parametrize("case", ["fresh", "half_known", "all_known", "one_unknown"])
def test_commit_sampled_is_image_commit_on_the_probed_noise(handle, case):
    B, N, L, ids, pos, sampled, p = commit_inputs(case)
    c = IMAGE_COUNTER + 11
    noise = [probe_normal(SEED, c + i, 0, B * N)[2].view(B, N) for i in range(2)]
    assert not torch.equal(noise[0], noise[1])
    differs = 0
    for temp in (0.37, 0.0):
        temp_dev = torch.tensor([temp], dtype=torch.float32, device=DEV)
        for mlen_v in (-1, 0, 1, 17, N // 2, N + 5):
            mlen = torch.tensor([mlen_v], dtype=torch.int32, device=DEV)
            ctr = dev_i64(c)
            got = commit_sampled(handle, ids, B, L, pos, N, sampled, p, temp_dev, SEED, ctr, mlen)
            want = commit_by_value(handle, ids, B, L, pos, N, sampled, p, noise[0], temp, mlen)
            assert torch.equal(got, want), f"{case} temp={temp} mlen={mlen_v}"
            assert int(ctr) == c + 1, "the counter reads c + 1 after the call"
            again = commit_sampled(handle, ids, B, L, pos, N, sampled, p, temp_dev, SEED, ctr, mlen)      # draws the noise of c + 1
            assert torch.equal(again, commit_by_value(handle, ids, B, L, pos, N, sampled, p, noise[1], temp, mlen)), "second call"
            assert int(ctr) == c + 2
            differs += int(temp != 0.0 and not torch.equal(got, again))
    if case in ("fresh", "half_known"):
        assert differs > 0, "with a temperature the noise of another counter re-masks other positions"


def test_capture_replays_draw_fresh_noise(handle):
    """mmada_image_sample + mmada_image_commit_sampled captured once and replayed twice: replay i is the eager pair at counter c + i,
    and the temperature tensor, rewritten between the replays, takes effect."""
    lib = abi.lib()
    B, N, CB, cs, ci, col0 = 2, 100, 8192, 2.5, 4.0, synth.TEXT_VOCAB
    _, (cd, utd, uid) = image_inputs(B, N, CB, None)
    L = 140
    gen = torch.Generator().manual_seed(17)
    pos = (torch.sort(torch.randperm(L - 10, generator=gen)[:N]).values + 5).to(torch.int32).to(DEV)
    ids0 = torch.randint(0, 1000, (B, L), generator=gen).to(DEV)
    ids0[:, pos.long()] = synth.MASK
    mlen = torch.tensor([40], dtype=torch.int32, device=DEV)
    c, temps = IMAGE_COUNTER + 100, (0.37, 0.9)

    def eager(cnt, temp):
        ctr = dev_i64(cnt)
        sampled, p_sel = image_sample(handle, cd, utd, uid, B, N, CB, cs, ci, col0, SEED, ctr)
        out = commit_sampled(handle, ids0, B, L, pos, N, sampled, p_sel, torch.tensor([temp], dtype=torch.float32, device=DEV), SEED, ctr, mlen)
        torch.cuda.synchronize()
        assert int(ctr) == cnt + 1
        return sampled, p_sel, out

    want = [eager(c + i, temps[i]) for i in range(2)]
    stale = eager(c + 1, temps[0])
    assert torch.equal(stale[0], want[1][0]) and not torch.equal(stale[2], want[1][2]), "the temperature must show in the commit"

    ctr = dev_i64(c)
    temp_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    ids = ids0.clone()
    sampled = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    p_sel = torch.zeros((B, N), dtype=torch.bfloat16, device=DEV)
    replays = []
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        abi.check(lib.mmada_graph_begin(st()), "graph_begin")
        rc = lib.mmada_image_sample(handle, cd.data_ptr(), utd.data_ptr(), uid.data_ptr(), B, N, CB, cs, ci, col0, SEED, ctr.data_ptr(),
                                    sampled.data_ptr(), p_sel.data_ptr(), None, None, st())
        rc = rc or lib.mmada_image_commit_sampled(handle, ids.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p_sel.data_ptr(),
                                                  temp_dev.data_ptr(), SEED, ctr.data_ptr(), mlen.data_ptr(), synth.TEXT_VOCAB,
                                                  synth.CODEBOOK, st())
        if rc:
            lib.mmada_graph_abort(st())
        abi.check(rc, "image sample + commit under capture")
        gr = C.c_void_p()
        abi.check(lib.mmada_graph_end(st(), C.byref(gr)), "graph_end")
        assert lib.mmada_graph_num_nodes(gr) == 3          # the draw, the commit, the counter's increment
        for i in range(2):
            ids.copy_(ids0)
            temp_dev.fill_(temps[i])
            abi.check(lib.mmada_graph_launch(gr, st()), "graph_launch")
            side.synchronize()
            replays.append((sampled.clone(), p_sel.clone(), ids.clone()))
        lib.mmada_graph_destroy(gr)
    torch.cuda.current_stream().wait_stream(side)
    assert int(ctr) == c + 2
    for i in range(2):
        for a, b, name in zip(replays[i], want[i], ("sampled", "p_sel", "ids")):
            assert torch.equal(a, b), f"replay {i}: {name} is not the eager pair's at counter c + {i}"
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[0][2], replays[1][2])


def test_draw_equals_the_row_head_on_the_same_logits(tiny_model):
    """T = 1 makes T * g exact, so mmada_head_sample over the codebook columns and mmada_image_sample on head_rows of the same rows
    maximise the same fp32 keys: equal in every row."""
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    tiny_model.forward_body(ids)
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    c0, c1 = synth.TEXT_VOCAB, synth.TEXT_VOCAB + synth.CODEBOOK
    s, c = SEED ^ 0xabc, IMAGE_COUNTER + 5
    ctr = dev_i64(c)
    head_ids = tiny_model.sample_tokens(rows, 1.0, c0, c1, seed=s, counter=ctr)[0]
    logits = tiny_model.head_rows(rows, c0, c1)
    sampled, _ = image_sample(tiny_model._handle, logits, None, None, 1, B * L, synth.CODEBOOK, 0.0, 0.0, c0, s, dev_i64(c))
    assert int(ctr) == c + 1
    print(f"{B * L} rows: draws that are the arg-max of the logits {int((sampled.view(-1) == logits.float().argmax(1).int()).sum())}")
    assert torch.equal(head_ids - c0, sampled.view(-1))


class SpyRng(TorchRng):
    def __init__(self):
        self.calls = []

    def rand(self, *a):
        self.calls.append("rand")
        return super().rand(*a)

    def randn(self, *a):
        self.calls.append("randn")
        return super().randn(*a)

    def multinomial(self, *a):
        self.calls.append("multinomial")
        return super().multinomial(*a)


README = dict(text_steps=8, timesteps=4, temperature=1.0, text_temperature=0.7, cfg_scale=0.0, cfg_img=4.0)


def _generate(model, job, **kw):
    from mmada_parallel_amd import generate_ti2ti

    args = dict(README, uncon_text=job["uncon_text"], uncon_image=job["uncon_image"], return_state=True)
    args.update(kw)
    return generate_ti2ti(model, job["input_ids"].to(DEV), job["text_start"], job["text_end"], job["image_start"], job["seq_len"],
                          job["newline_every"], **args)


def _steps(model, job, **kw):
    """The generator core, step by step: (final ids, [sampled ids of every image step])."""
    args = dict(README, uncon_text=job["uncon_text"], uncon_image=job["uncon_image"])
    args.update(kw)
    sampled, ids = [], None
    with torch.no_grad():
        for _step, ids, info in _ti2ti_steps(model, job["input_ids"].to(DEV), job["text_start"], job["text_end"], job["image_start"],
                                             job["seq_len"], job["newline_every"], **args):
            if info["sampled"] is not None:
                sampled.append(info["sampled"].clone())
    return ids.clone(), sampled


def image_positions(job):
    span = job["input_ids"][0, job["image_start"]:job["image_start"] + job["seq_len"] + job["seq_len"] // job["newline_every"]]
    return (span != synth.NEW_LINE).nonzero().flatten() + job["image_start"]


def test_generate_ti2ti_with_both_samplers_on_the_device(tiny_model):
    """At the README temperatures with both samplers on the device nothing is drawn on the host, a seed repeats the run, and the
    image span ends as the reference's rule leaves it: the last step's mask_len is floor(N cos(pi / 2)) = -1 in fp32 and the rule's
    floor of 1 re-masks exactly one position (mask_len_schedule; the read-out fills it, as the reference does) — every other
    position holds a codebook token."""
    job = tiny_job()
    pos = image_positions(job)
    assert pos.numel() == job["seq_len"]
    dev = dict(text_sampler="device", image_sampler="device")
    spy = SpyRng()
    a = _generate(tiny_model, job, sampler_seed=1234, rng=spy, **dev)
    assert spy.calls == [], f"torch draws on the device path: {spy.calls}"
    b = _generate(tiny_model, job, sampler_seed=1234, **dev)
    c = _generate(tiny_model, job, sampler_seed=1235, **dev)
    assert torch.equal(a[2], b[2]) and a[1] == b[1], "the same seed repeats the run"
    assert not torch.equal(a[2][0, pos], c[2][0, pos]), "another seed draws another image"
    img = a[2][0, pos]
    left = int((img == synth.MASK).sum())
    print(f"image span at the end: {left} of {pos.numel()} positions still masked (the reference's floor of one)")
    assert left == 1, "exactly the one position the mask_len rule re-masks on the last step stays masked"
    tok = img[img != synth.MASK]
    assert int(tok.min()) >= synth.TEXT_VOCAB and int(tok.max()) < synth.TEXT_VOCAB + synth.CODEBOOK
    assert len(a[0]) == job["seq_len"] and all(0 <= v < synth.CODEBOOK for v in a[0]), "no mask token in the returned image"
    assert [v for v, t in zip(a[0], img.tolist()) if t != synth.MASK] == (tok - synth.TEXT_VOCAB).tolist()


def test_generate_ti2ti_replays_sampled_steps_as_graphs(tiny_model):
    job = tiny_job()
    for kw in (dict(text_sampler="device", image_sampler="device"), dict(text_sampler="torch", text_temperature=0.0, image_sampler="device")):
        eager_ids, eager_sampled = _steps(tiny_model, job, sampler_seed=77, graph=False, **kw)
        before = tiny_model.graph_replays
        graph_ids, graph_sampled = _steps(tiny_model, job, sampler_seed=77, graph=True, **kw)
        replays = tiny_model.graph_replays - before
        print(f"{kw}: {replays} step replays, {len(graph_sampled)} image steps")
        assert replays > 0, "a step at temperature > 0 with device-side draws is captured and replayed"
        assert torch.equal(graph_ids, eager_ids), "the replayed run's ids are not the eager run's"
        assert len(graph_sampled) == len(eager_sampled) == 4
        for i, (x, y) in enumerate(zip(graph_sampled, eager_sampled)):
            assert torch.equal(x, y), f"image step {i}: sampled ids differ between the replayed and the eager run"
        assert not torch.equal(eager_sampled[0], eager_sampled[1])


def test_temperature_zero_with_the_device_text_sampler_replays_too(tiny_model):
    """temperature == 0 with text_sampler="device": the one randn the reference still draws per image step (multiplied by 0) is drawn
    ahead of the step's launches, so the step is captured without it and torch's stream sees the same draws, eager or replayed."""
    job = tiny_job()
    runs = []
    for graph in (False, True):
        spy = SpyRng()
        before = tiny_model.graph_replays
        ids, sampled = _steps(tiny_model, job, temperature=0.0, text_sampler="device", sampler_seed=5, graph=graph, rng=spy)
        runs.append((ids, sampled, spy.calls, tiny_model.graph_replays - before))
    assert runs[0][3] == 0 and runs[1][3] > 0
    assert runs[0][2] == runs[1][2] == ["randn"] * 4, "one randn per image step, nothing else, in both runs"
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))


def test_refusals(tiny_model):
    job = tiny_job()
    for kw, match in ((dict(image_sampler="device", sampler_seed=1, temperature=0.0), "temperature > 0"),
                      (dict(image_sampler="device"), "sampler_seed"),
                      (dict(image_sampler="gpu", sampler_seed=1), "image_sampler")):
        with pytest.raises(ValueError, match=match):
            _generate(tiny_model, job, **kw)
    ids = torch.from_numpy(Z["main_ids"])
    B, L = ids.shape
    with single_rank_group(synth.CFG_TINY, tiny_sd(), "pull", B * ((L + 7) // 8 * 8)) as m:
        with pytest.raises(ValueError, match="image_sampler='device' needs one rank"):
            _generate(m, job, image_sampler="device", sampler_seed=1)


def test_torch_sampler_passed_explicitly_still_reproduces_the_recording(tiny_model):
    from mmada_parallel_amd import generate_ti2ti
    from test_gpu_model import _stubbed

    name = "noisy_img"
    z = np.load(os.path.join(GOLDEN, "sampler_noisy.npz"))
    calls_ref = torch.from_numpy(z[name + "_calls"])
    job, kw = tiny_job(), NOISY_CASES[name]
    stub = _stubbed(tiny_model, int(z[name + "_seed"]), STUB_TEXT_VOCAB + STUB_CB)
    gen = torch.Generator().manual_seed(int(z[name + "_gen_seed"]))
    generate_ti2ti(stub, job["input_ids"].to(DEV), job["text_start"], job["text_end"], job["image_start"], job["seq_len"],
                   job["newline_every"], uncon_text=job["uncon_text"], uncon_image=job["uncon_image"], tokenizer=None,
                   text_vocab_size=STUB_TEXT_VOCAB, codebook_size=STUB_CB, generator=gen, rng=ReplayCpuRng(), image_sampler="torch", **kw)
    got = torch.cat(stub.calls, 0)
    assert got.shape == calls_ref.shape and torch.equal(got, calls_ref)
