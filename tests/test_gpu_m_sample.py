"""The M samplers drawn on the GPU: mmada_image_sample_m (image_row_kernel<true>'s Gumbel-max draw beside its statistics),
mmada_image_commit_m_sampled (the Gumbel re-mask noise computed in the commit), mmada_text_draw_cfg (the text draw on the CFG-combined
logits), and interleave_generate / t2i_generate with image_sampler="device" / text_sampler="device" and the hipGraph replay.  Every
check is equality — against torch's own bf16 ops, the device's own noise (mmada_probe_gumbel), mmada_image_probs_m,
mmada_image_commit_m, mmada_text_select_cfg and the row head — except the host mirror of the re-mask noise, whose logf may differ
from the device's within the bound test_m_sample_host.py states."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import GOLDEN, M_CASES, M_SHAPE, M_T2I_SHAPE, bits, m_t2i_job, stub_logits, tiny_sd
from mmada_parallel_amd import abi, synth
from mmada_parallel_amd.generators.interleave_generator import cosine_schedule, get_num_transfer_tokens, interleave_generate
from mmada_parallel_amd.generators.parallel_generator import mask_len_schedule
from mmada_parallel_amd.generators.t2i_generator import t2i_generate, t2i_generate_decoding_stepwise
from test_gpu_image_sample import dev_i64, image_inputs, probe_gumbel, st
from test_gpu_kernels import handle   # noqa: F401  (a tiny handle: the sampler entry points only need its cfg)
from test_gpu_score import tiny_model   # noqa: F401
from test_gpu_score_tp import single_rank_group
from test_image_sample_host import IMAGE_COUNTER, NORMAL_KEY_XOR
from test_m_sample_host import g_tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0123456789abcdef
Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
# (B, N, CB, image_cfg, col0, quant): one 16-byte chunk with almost every thread idle; the production codebook at an odd row count
# with col0 & 3 == 1; the LDS limit with an odd col0; quantised logits with many equal l (key ties)
CASES = [(1, 5, 8, 0.0, 0, None), (2, 100, 8192, 3.5, 126349, None), (1, 3, 16384, 4.0, 1001, None), (3, 16, 512, 3.5, 2, 2)]


def m_logits(c, u, cfg):
    """modeling_mmada.py:216 with torch's own bf16 ops on the CPU: every op rounds to bf16."""
    return (1 + cfg) * c - cfg * u


def sample_m(h, cd, ud, B, N, CB, cfg, col0, seed, counter, stats=False):
    sampled = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    p_sel = torch.empty((B, N), dtype=torch.bfloat16, device=DEV)
    am = torch.full((B, N), -7, dtype=torch.int32, device=DEV) if stats else None
    pm = torch.empty((B, N), dtype=torch.bfloat16, device=DEV) if stats else None
    abi.check(abi.lib().mmada_image_sample_m(h, cd.data_ptr(), ud.data_ptr(), B, N, CB, cfg, col0, seed, counter.data_ptr(),
                                             sampled.data_ptr(), p_sel.data_ptr(), abi.ptr(am), abi.ptr(pm), st()), "mmada_image_sample_m")
    return (sampled, p_sel, am, pm) if stats else (sampled, p_sel)


def probe_remask(seed, counter, R):
    """The device's fp32 g_remask of rows 0 .. R - 1: the Gumbel value of column 0 under the key seed ^ NORMAL_KEY_XOR."""
    return probe_gumbel(seed ^ NORMAL_KEY_XOR, counter, R, 0, 1).view(R)


def commit_m(h, ids, B, L, pos, N, sampled, p, gumbel, temp, mlen, tv):
    out = ids.clone()
    abi.check(abi.lib().mmada_image_commit_m(h, out.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p.data_ptr(), gumbel.data_ptr(),
                                             temp, mlen.data_ptr(), tv, st()), "mmada_image_commit_m")
    return out


def commit_m_sampled(h, ids, B, L, pos, N, sampled, p, temp_dev, seed, ctr, mlen, tv, want_sampled=True):
    out = ids.clone()
    s_out = torch.full((B, N), -7, dtype=torch.int32, device=DEV) if want_sampled else None
    abi.check(abi.lib().mmada_image_commit_m_sampled(h, out.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p.data_ptr(),
                                                     temp_dev.data_ptr(), seed, ctr.data_ptr(), mlen.data_ptr(), tv, abi.ptr(s_out), st()),
              "mmada_image_commit_m_sampled")
    return out, s_out


def replay_image_step(h, il_c, il_u, B, N, CB, cfg, tv, seed, counter, ids, pos, temp, mlen_v):
    """An image step recomputed from the documented parts: the draw at `counter`, then mmada_image_commit_m on the probed Gumbel
    values with the temperature by value.  Returns (ids after the step, the ids it committed from)."""
    sampled, p_sel = sample_m(h, il_c, il_u, B, N, CB, cfg, tv, seed, dev_i64(counter))
    gumbel = probe_remask(seed, counter, B * N).to(torch.bfloat16).view(B, N)
    mlen = torch.tensor([mlen_v], dtype=torch.int32, device=DEV)
    L = ids.shape[1]
    cur = ids[:, pos.long()]
    committed_from = torch.where(cur == synth.MASK, sampled.long(), cur - tv)
    return commit_m(h, ids, B, L, pos, N, sampled, p_sel, gumbel, temp, mlen, tv), committed_from


# ------------------------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("B,N,CB,cfg,col0,quant", CASES)
def test_draw_is_the_argmax_of_the_key(handle, B, N, CB, cfg, col0, quant):
    (c, u, _), (cd, ud, _) = image_inputs(B, N, CB, quant)
    cnt = IMAGE_COUNTER + 3
    ctr = dev_i64(cnt)
    g = probe_gumbel(SEED, cnt, B * N, col0, CB).cpu()
    l = m_logits(c, u, cfg).float().view(B * N, CB)
    keys = l + g
    want = keys.argmax(1).int().view(B, N)          # the CPU's arg-max: the first index on equal keys
    sampled, _ = sample_m(handle, cd, ud, B, N, CB, cfg, col0, SEED, ctr)
    tied = int((keys == keys.max(1, keepdim=True).values).sum(1).gt(1).sum())
    print(f"B={B} N={N} CB={CB} cfg={cfg} col0={col0}: rows with a wrong draw {int((sampled.cpu() != want).sum())}, rows whose best key "
          f"is tied {tied}, draws that are the arg-max of l {int((want == l.argmax(1).int().view(B, N)).sum())} of {B * N}")
    assert torch.equal(sampled.cpu(), want), "sampled is not the first-index arg-max of l + g"
    assert int(ctr) == cnt, "mmada_image_sample_m must not write the counter"
    again, _ = sample_m(handle, cd, ud, B, N, CB, cfg, col0, SEED, dev_i64(cnt))
    assert torch.equal(again, sampled), "the same counter repeats the draw"
    if B * N * CB >= 1 << 12:
        other, _ = sample_m(handle, cd, ud, B, N, CB, cfg, col0, SEED, dev_i64(cnt + 1))
        assert not torch.equal(other, sampled), "another counter changes some draw"


@pytest.mark.parametrize("B,N,CB,cfg,col0,quant", CASES)
def test_outputs_agree_with_image_probs_m(handle, B, N, CB, cfg, col0, quant):
    _, (cd, ud, _) = image_inputs(B, N, CB, quant)
    probs = torch.empty(B, N, CB, dtype=torch.bfloat16, device=DEV)
    am_ref = torch.empty(B, N, dtype=torch.int32, device=DEV)
    pm_ref = torch.empty(B, N, dtype=torch.bfloat16, device=DEV)
    abi.check(abi.lib().mmada_image_probs_m(handle, cd.data_ptr(), ud.data_ptr(), B, N, CB, cfg, probs.data_ptr(), am_ref.data_ptr(),
                                            pm_ref.data_ptr(), st()), "mmada_image_probs_m")
    ctr = dev_i64(IMAGE_COUNTER)
    sampled, p_sel, am, pm = sample_m(handle, cd, ud, B, N, CB, cfg, col0, SEED, ctr, stats=True)
    assert int(sampled.min()) >= 0 and int(sampled.max()) < CB
    assert torch.equal(bits(p_sel), bits(probs.gather(-1, sampled.long()[..., None]).squeeze(-1))), "p_sel is not probs[sampled]"
    assert torch.equal(am, am_ref) and torch.equal(bits(pm), bits(pm_ref)), "argmax_out / pmax_out differ from mmada_image_probs_m"
    bare, p_bare = sample_m(handle, cd, ud, B, N, CB, cfg, col0, SEED, ctr)          # null for both: accepted
    assert torch.equal(bare, sampled) and torch.equal(bits(p_bare), bits(p_sel))


# --------------------------------------------------------------------------------------------------------------------- 3
def commit_inputs_m(case, N=64):
    """The four cases of test_gpu_image_sample.commit_inputs (fresh, half known, all known, one unknown) at N = 64, B = 2."""
    g = torch.Generator().manual_seed({"fresh": 1, "half_known": 2, "all_known": 3, "one_unknown": 4}[case])
    B, L = 2, 100
    pos = torch.sort(torch.randperm(L - 10, generator=g)[:N]).values + 5
    ids = torch.randint(0, 1000, (B, L), generator=g)
    known = {"fresh": 0, "half_known": N // 2, "all_known": N, "one_unknown": N - 1}[case]
    for b in range(B):
        perm = torch.randperm(N, generator=g)
        ids[b, pos] = synth.MASK
        ids[b, pos[perm[:known]]] = synth.TEXT_VOCAB + torch.randint(0, synth.CODEBOOK, (known,), generator=g)
    sampled = torch.randint(0, synth.CODEBOOK, (B, N), generator=g, dtype=torch.int32)
    # bf16 probabilities from a coarse set, p == 0 included -> the clamp at 1e-20 and massive ties at the cut-off
    p = (torch.randint(0, 40, (B, N), generator=g).float() / 4096).to(torch.bfloat16)
    return B, N, L, ids.to(DEV), pos.to(torch.int32).to(DEV), sampled.to(DEV), p.to(DEV)


@pytest.mark.parametrize("case", ["fresh", "half_known", "all_known", "one_unknown"])
def test_commit_m_sampled_is_image_commit_m_on_the_probed_noise(handle, case):
    B, N, L, ids, pos, sampled, p = commit_inputs_m(case)
    tv = synth.TEXT_VOCAB
    c = IMAGE_COUNTER + 11
    g32 = [probe_remask(SEED, c + i, B * N) for i in range(2)]
    noise = [g.to(torch.bfloat16).view(B, N) for g in g32]
    assert not torch.equal(noise[0], noise[1])
    cur = ids[:, pos.long()]
    want_sampled = torch.where(cur == synth.MASK, sampled.long(), cur - tv).int()
    differs = 0
    for temp in (0.6, 0.0):
        temp_dev = torch.tensor([temp], dtype=torch.float32, device=DEV)
        for mlen_v in (-1, 0, 1, 17, N // 2, N + 5):
            mlen = torch.tensor([mlen_v], dtype=torch.int32, device=DEV)
            ctr = dev_i64(c)
            got, s_out = commit_m_sampled(handle, ids, B, L, pos, N, sampled, p, temp_dev, SEED, ctr, mlen, tv)
            assert torch.equal(got, commit_m(handle, ids, B, L, pos, N, sampled, p, noise[0], temp, mlen, tv)), f"{case} temp={temp} mlen={mlen_v}"
            assert torch.equal(s_out, want_sampled), "sampled_out is not where(unknown, sampled_in, ids - text_vocab)"
            assert int(ctr) == c + 1, "the counter reads c + 1 after the call"
            again, _ = commit_m_sampled(handle, ids, B, L, pos, N, sampled, p, temp_dev, SEED, ctr, mlen, tv, want_sampled=False)
            assert torch.equal(again, commit_m(handle, ids, B, L, pos, N, sampled, p, noise[1], temp, mlen, tv)), "second call"
            assert int(ctr) == c + 2
            differs += int(temp != 0.0 and not torch.equal(got, again))
    if case in ("fresh", "half_known"):
        assert differs > 0, "with a temperature the noise of another counter re-masks other positions"
    lib = abi.lib()
    host = np.array([lib.mmada_sample_remask_gumbel(SEED, c, r) for r in range(B * N)], dtype=np.float64)
    dev = g32[0].cpu().double().numpy()
    ratio = float((np.abs(host - dev) / g_tol(dev)).max())
    print(f"{case}: host mirror against the probe on {B * N} rows: worst |difference| / (2^-21 (1 + |g|)) = {ratio:.3f}")
    assert ratio <= 1.0


# --------------------------------------------------------------------------------------------------------------------- 4
TEXT_CASES = [(1, 3, 8, 8, 0.0, 0.7), (1, 5, 1003, 1008, 1.5, 0.7), (2, 4, 134656, 134656, 2.0, 1.0), (1, 4, 1003, 1008, 1.5, 0.0)]


def text_inputs(B, T, V, ld):
    g = torch.Generator().manual_seed(V + T)
    c = (torch.randn(B * T, V, generator=g) * 2.0).to(torch.bfloat16)
    u = (c.float() + torch.randn(B * T, V, generator=g) * 0.7).to(torch.bfloat16)
    cp, up = torch.full((B * T, ld), 1e4, dtype=torch.bfloat16), torch.full((B * T, ld), 1e4, dtype=torch.bfloat16)   # a pad that would win
    cp[:, :V], up[:, :V] = c, u
    return c, u, cp, up


def text_draw(h, cd, ud, cfg, B, T, V, ld, temp, seed, ctr):
    x0 = torch.full((B * T,), -7, dtype=torch.int32, device=DEV)
    rc = abi.lib().mmada_text_draw_cfg(h, cd.data_ptr(), ud.data_ptr(), cfg, B, T, V, ld, temp, seed, ctr.data_ptr(), x0.data_ptr(), st())
    return rc, x0


@pytest.mark.parametrize("B,T,V,ld,cfg,temp", TEXT_CASES)
def test_text_draw_is_the_argmax_of_the_key(handle, B, T, V, ld, cfg, temp):
    c, u, cp, up = text_inputs(B, T, V, ld)
    if temp == 0.0:   # two equal maxima per row, the lower column must win: one below a 16-byte chunk boundary, one in the tail
        for r in range(B * T):
            lo, hi = 17 + r, V - 1 - r
            for t in (c, u, cp, up):
                t[r, lo] = t[r, hi] = 30.0
    comb = c + cfg * (u - c)                       # :173 with torch's own bf16 ops on the CPU
    cnt = 41
    ctr = dev_i64(cnt)
    g = probe_gumbel(SEED, cnt, B * T, 0, V).cpu()
    want = (comb.float() + torch.tensor(temp, dtype=torch.float32) * g).argmax(1).int()
    rc, x0 = text_draw(handle, cp.to(DEV), up.to(DEV), cfg, B, T, V, ld, temp, SEED, ctr)
    abi.check(rc, "mmada_text_draw_cfg")
    print(f"B={B} T={T} V={V} ld={ld} cfg={cfg} T={temp}: rows with a wrong draw {int((x0.cpu() != want).sum())}, draws that are the "
          f"arg-max of the combined logits {int((want == comb.float().argmax(1).int()).sum())} of {B * T}")
    assert torch.equal(x0.cpu(), want), "x0 is not the first-index arg-max of comb + T * g"
    assert int(ctr) == cnt + 1, "the counter reads c + 1 after the call"
    if temp == 0.0:
        assert x0.cpu().tolist() == [17 + r for r in range(B * T)], "the lower of two equal maxima wins"
    else:
        rc, other = text_draw(handle, cp.to(DEV), up.to(DEV), cfg, B, T, V, ld, temp, SEED, ctr)     # the noise of c + 1
        abi.check(rc, "mmada_text_draw_cfg")
        g1 = probe_gumbel(SEED, cnt + 1, B * T, 0, V).cpu()
        assert torch.equal(other.cpu(), (comb.float() + torch.tensor(temp, dtype=torch.float32) * g1).argmax(1).int())
        assert int(ctr) == cnt + 2


def test_text_draw_refuses_a_bad_temperature_and_leaves_the_counter(handle):
    B, T, V, ld = 1, 3, 8, 8
    _, _, cp, up = text_inputs(B, T, V, ld)
    ctr = dev_i64(9)
    for bad in (float("inf"), float("nan"), -0.5):
        rc, x0 = text_draw(handle, cp.to(DEV), up.to(DEV), 1.5, B, T, V, ld, bad, SEED, ctr)
        assert rc != 0 and b"not a finite value >= 0" in abi.lib().mmada_last_error(), bad
        torch.cuda.synchronize()
        assert int(ctr) == 9 and bool((x0 == -7).all()), "a refused call launches nothing"


# --------------------------------------------------------------------------------------------------------------------- 5
def test_draws_equal_the_row_head_on_the_same_logits(tiny_model):
    """With no guidance the combined logits are the head's own bf16 logits, so the head's draw (mmada_head_sample) and these kernels
    maximise the same fp32 keys: equal in every row, for the image draw (T = 1) and the text draw (T = 0.7)."""
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    V = tiny_model.vocab
    tiny_model.forward_body(ids)
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    c0, c1 = synth.TEXT_VOCAB, synth.TEXT_VOCAB + synth.CODEBOOK
    s, c = SEED ^ 0xabc, IMAGE_COUNTER + 5
    head_ids = tiny_model.sample_tokens(rows, 1.0, c0, c1, seed=s, counter=dev_i64(c))[0]
    logits = tiny_model.head_rows(rows, c0, c1)
    sampled, _ = sample_m(tiny_model._handle, logits, logits, 1, B * L, synth.CODEBOOK, 0.0, c0, s, dev_i64(c))
    assert torch.equal(head_ids - c0, sampled.view(-1)), "image draw"
    head_ids = tiny_model.sample_tokens(rows, 0.7, seed=s, counter=dev_i64(7))[0]
    full = tiny_model.head_rows(rows, 0, V)
    rc, x0 = text_draw(tiny_model._handle, full, full, 0.0, 1, B * L, V, V, 0.7, s, dev_i64(7))
    abi.check(rc, "mmada_text_draw_cfg")
    print(f"{B * L} rows: text draws that are the arg-max of the logits {int((x0 == full.float().argmax(1).int()).sum())}")
    assert torch.equal(head_ids, x0), "text draw"


# --------------------------------------------------------------------------------------------------------------------- 6
def test_capture_replays_draw_fresh_noise(handle):
    """mmada_image_sample_m + mmada_image_commit_m_sampled captured once on a side stream and launched three times: launch i is the
    eager pair at counter c + i, and the counter ends at c + 3."""
    lib = abi.lib()
    B, N, CB, cfg, tv = 2, 100, 8192, 3.5, synth.TEXT_VOCAB
    _, (cd, ud, _) = image_inputs(B, N, CB, None)
    L = 140
    gen = torch.Generator().manual_seed(17)
    pos = (torch.sort(torch.randperm(L - 10, generator=gen)[:N]).values + 5).to(torch.int32).to(DEV)
    ids0 = torch.randint(0, 1000, (B, L), generator=gen).to(DEV)
    ids0[:, pos.long()] = synth.MASK
    mlen = torch.tensor([40], dtype=torch.int32, device=DEV)
    temp_dev = torch.tensor([0.6], dtype=torch.float32, device=DEV)
    c = IMAGE_COUNTER + 100

    def eager(cnt):
        ctr = dev_i64(cnt)
        sampled, p_sel = sample_m(handle, cd, ud, B, N, CB, cfg, tv, SEED, ctr)
        out, s_out = commit_m_sampled(handle, ids0, B, L, pos, N, sampled, p_sel, temp_dev, SEED, ctr, mlen, tv)
        torch.cuda.synchronize()
        assert int(ctr) == cnt + 1
        return sampled, p_sel, out, s_out

    want = [eager(c + i) for i in range(3)]
    ctr = dev_i64(c)
    ids = ids0.clone()
    sampled = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    p_sel = torch.zeros((B, N), dtype=torch.bfloat16, device=DEV)
    s_out = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    replays = []
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        abi.check(lib.mmada_graph_begin(st()), "graph_begin")
        rc = lib.mmada_image_sample_m(handle, cd.data_ptr(), ud.data_ptr(), B, N, CB, cfg, tv, SEED, ctr.data_ptr(), sampled.data_ptr(),
                                      p_sel.data_ptr(), None, None, st())
        rc = rc or lib.mmada_image_commit_m_sampled(handle, ids.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p_sel.data_ptr(),
                                                    temp_dev.data_ptr(), SEED, ctr.data_ptr(), mlen.data_ptr(), tv, s_out.data_ptr(), st())
        if rc:
            lib.mmada_graph_abort(st())
        abi.check(rc, "image sample + commit under capture")
        gr = C.c_void_p()
        abi.check(lib.mmada_graph_end(st(), C.byref(gr)), "graph_end")
        assert lib.mmada_graph_num_nodes(gr) == 3          # the draw, the commit, the counter's increment
        for i in range(3):
            ids.copy_(ids0)
            abi.check(lib.mmada_graph_launch(gr, st()), "graph_launch")
            side.synchronize()
            replays.append((sampled.clone(), p_sel.clone(), ids.clone(), s_out.clone()))
        lib.mmada_graph_destroy(gr)
    torch.cuda.current_stream().wait_stream(side)
    assert int(ctr) == c + 3
    for i in range(3):
        for a, b, name in zip(replays[i], want[i], ("sampled", "p_sel", "ids", "sampled_out")):
            assert torch.equal(a, b), f"launch {i}: {name} is not the eager pair's at counter c + {i}"
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[1][2], replays[2][2])


# --------------------------------------------------------------------------------------------------------------------- 7
class Tok:
    bos_token_id = 126080

    def __len__(self):
        return synth.TEXT_VOCAB


class RaisingRng:
    def __getattr__(self, name):
        raise AssertionError(f"rng.{name} touched on the device path")


M_TINY = dict(P=6, N=16, T=16, text_steps=8, image_steps=4, image_cfg=3.5, text_cfg=1.5, image_temperature=1.0)
M_CFG = SimpleNamespace(model=SimpleNamespace(mmada=SimpleNamespace(num_vq_tokens=M_TINY["N"], codebook_size=synth.CODEBOOK)),
                        dataset=SimpleNamespace(preprocessing=SimpleNamespace(max_seq_length=M_TINY["T"])))


def m_prompts():
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 1000, (M_TINY["P"],), generator=g), torch.randint(0, 1000, (M_TINY["P"],), generator=g)


def interleave(model, **kw):
    inp, unc = m_prompts()
    args = dict(text_cfg=M_TINY["text_cfg"], image_cfg=M_TINY["image_cfg"], text_steps=M_TINY["text_steps"], image_steps=M_TINY["image_steps"],
                image_temperature=M_TINY["image_temperature"], reserved_token_mapping={"<|soi|>": synth.BOI, "<|eoi|>": synth.EOI},
                config=M_CFG, uni_prompting=SimpleNamespace(text_tokenizer=Tok()), image_sampler="device")
    args.update(kw)
    img, text = interleave_generate(model, inp, unc, **args)
    torch.cuda.synchronize()
    return img.clone(), text.clone()


def test_interleave_device_sampler_repeats_with_its_seed_and_never_asks_torch(tiny_model, monkeypatch):
    def no_probs(*a):
        raise AssertionError("mmada_image_probs_m called: the [N, CB] probabilities must not exist on the device path")

    torch.cuda.reset_peak_memory_stats()
    torch_run = interleave(tiny_model, image_sampler="torch")
    peak_torch = torch.cuda.max_memory_allocated()
    monkeypatch.setattr(abi.lib(), "mmada_image_probs_m", no_probs, raising=False)
    torch.cuda.reset_peak_memory_stats()
    a = interleave(tiny_model, sampler_seed=1234, rng=RaisingRng())
    peak_dev = torch.cuda.max_memory_allocated()
    b = interleave(tiny_model, sampler_seed=1234)
    c = interleave(tiny_model, sampler_seed=1235)
    print(f"peak torch memory: torch sampler {peak_torch} B, device sampler {peak_dev} B")
    assert a[0].dtype == torch_run[0].dtype and a[0].shape == torch_run[0].shape == (1, M_TINY["N"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the same seed repeats the run"
    assert not torch.equal(a[0], c[0]), "another seed draws another image"
    assert int(a[0].min()) >= 0 and int(a[0].max()) < synth.CODEBOOK and a[1].shape == (1, M_TINY["T"])
    d = interleave(tiny_model, sampler_seed=1234, rng=RaisingRng(), text_sampler="device", text_temperature=0.7)
    e = interleave(tiny_model, sampler_seed=1234, text_sampler="device", text_temperature=0.7)
    assert torch.equal(d[0], e[0]) and torch.equal(d[1], e[1]) and not torch.equal(d[1], a[1])


def test_interleave_device_text_sampler_beside_the_torch_image_sampler(tiny_model):
    """text_sampler="device" alone: the text draw never asks `rng`, the image step still takes the reference's draws from it (so
    the run repeats with the rng's seed and changes with it), and such a run is not captured."""
    from oracle.interleave_oracle import SeededRng

    class ImageOnlyRng(SeededRng):
        def text_gumbel_argmax(self, *a):
            raise AssertionError("rng.text_gumbel_argmax touched with text_sampler='device'")

    kw = dict(image_sampler="torch", text_sampler="device", text_temperature=0.7, sampler_seed=5, graph=True)
    before = tiny_model.graph_replays
    rng = ImageOnlyRng(3)
    a = interleave(tiny_model, rng=rng, **kw)
    assert rng.n == 2 * M_TINY["image_steps"], "one multinomial and one uniform draw per image step"
    b = interleave(tiny_model, rng=ImageOnlyRng(3), **kw)
    c = interleave(tiny_model, rng=ImageOnlyRng(4), **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    assert a[0].dtype == torch.int64 and a[0].shape == (1, M_TINY["N"]) and tiny_model.graph_replays == before


@pytest.mark.parametrize("text_temperature", [0.0, 0.7])
def test_interleave_teacher_forced_from_the_trace(tiny_model, text_temperature):
    """Every recorded step recomputed from its recorded input with the documented parts: the text draw at counter i and
    mmada_text_select_cfg, the image draw at counter 2^62 + j and mmada_image_commit_m on the probed Gumbel values with the step's
    temperature by value — the result is the next recorded input (the returned ids after the last step)."""
    lib, h = abi.lib(), tiny_model._handle
    P, N, T, steps = M_TINY["P"], M_TINY["N"], M_TINY["T"], M_TINY["text_steps"]
    CB, tv, V = synth.CODEBOOK, synth.TEXT_VOCAB, tiny_model.vocab
    seed, trace = 4321, []
    kw = dict(text_sampler="device", text_temperature=0.7) if text_temperature else {}
    img, text = interleave(tiny_model, sampler_seed=seed, trace=trace, **kw)
    assert len(trace) == steps
    L = trace[0].shape[1]
    text_start, img_start = L - T, P + 1
    img_steps = sorted(set(torch.linspace(steps // 4, steps - 1, M_TINY["image_steps"]).round().int().tolist()))
    assert len(img_steps) == 4
    mlen = mask_len_schedule(N, steps, cosine_schedule)
    k = get_num_transfer_tokens(trace[0][:1, text_start:] == synth.MASK, steps)
    pos = torch.arange(img_start, img_start + N, dtype=torch.int32, device=DEV)
    ar = torch.arange(text_start, L, dtype=torch.int32, device=DEV)
    text_rows, img_rows = torch.cat([ar, ar + L]), torch.cat([pos, pos + L])
    scratch = torch.empty(T * 16, dtype=torch.uint8, device=DEV)
    last_sampled = None
    for i, rec in enumerate(trace):
        both = rec.to(DEV)
        assert torch.equal(both[1, P:], both[0, P:]), "the uncond row carries the cond row's tail"
        tiny_model.forward_body(both)
        ids = both[0:1].clone()
        tl = tiny_model.head_rows(text_rows, 0, V)
        x0 = None
        if text_temperature:
            rc, x0 = text_draw(h, tl[:T], tl[T:], M_TINY["text_cfg"], 1, T, V, V, text_temperature, seed, dev_i64(i))
            abi.check(rc, "mmada_text_draw_cfg")
        k_i = k[:, i].to(device=DEV, dtype=torch.int32).contiguous()
        abi.check(lib.mmada_text_select_cfg(h, tl[:T].data_ptr(), tl[T:].data_ptr(), M_TINY["text_cfg"], abi.ptr(x0), 1, T, V, V,
                                            ids.data_ptr(), L, text_start, k_i.data_ptr(), scratch.data_ptr(), st()), "mmada_text_select_cfg")
        if i in img_steps:
            il = tiny_model.head_rows(img_rows, tv, tv + CB)
            temp = M_TINY["image_temperature"] * (1.0 - 1.0 * (i + 1) / steps)
            ids, last_sampled = replay_image_step(h, il[:N], il[N:], 1, N, CB, M_TINY["image_cfg"], tv, seed,
                                                  IMAGE_COUNTER + img_steps.index(i), ids, pos, temp, mlen[i])
        nxt = trace[i + 1][0:1].to(DEV) if i + 1 < steps else None
        if nxt is not None:
            assert torch.equal(ids, nxt), f"step {i}: the recomputed step is not the next recorded input"
        else:
            assert torch.equal(ids[:, text_start:], text), "last step: text ids"
    assert torch.equal(last_sampled, img), "the returned image ids are the ids the last image step committed from"


@pytest.mark.parametrize("text_temperature", [0.0, 0.7])
def test_interleave_replays_steps_as_graphs(tiny_model, text_temperature):
    kw = dict(text_sampler="device", text_temperature=0.7) if text_temperature else {}
    eager = interleave(tiny_model, sampler_seed=77, graph=False, **kw)
    before = tiny_model.graph_replays
    replayed = interleave(tiny_model, sampler_seed=77, graph=True, **kw)
    replays = tiny_model.graph_replays - before
    print(f"text_temperature={text_temperature}: {replays} step replays of {M_TINY['text_steps']} steps")
    assert replays > 0, "a step with device-side draws is captured and replayed"
    assert torch.equal(replayed[0], eager[0]) and torch.equal(replayed[1], eager[1]), "the replayed run's ids are not the eager run's"
    before = tiny_model.graph_replays
    interleave(tiny_model, image_sampler="torch", graph=True, **({"text_temperature": 0.7} if text_temperature else {}))
    assert tiny_model.graph_replays == before, "a run that draws from torch stays eager"


def test_interleave_torch_sampler_passed_explicitly_reproduces_the_recording(tiny_model):
    from oracle.interleave_oracle import SeededRng
    from test_gpu_model import _stubbed

    name = "m_noisy"
    z = np.load(os.path.join(GOLDEN, "m_traj.npz"))
    sh, kw = M_SHAPE, dict(M_CASES[name])
    seed = int(z[name + "_seed"])
    V = sh["text_vocab"] + sh["CB"]
    stub = _stubbed(tiny_model, seed, V)
    calls = []

    def fb(ids, consumed=None):
        stub.n += 1
        calls.append(ids.cpu().clone())
        stub._cur = stub_logits(seed, stub.n, ids.shape[0], ids.shape[1], V).to(DEV)

    stub.forward_body = fb

    class StubTok:
        bos_token_id = sh["bos"]

        def __len__(self):
            return sh["text_vocab"]

    cfgobj = SimpleNamespace(model=SimpleNamespace(mmada=SimpleNamespace(num_vq_tokens=sh["N"], codebook_size=sh["CB"])),
                             dataset=SimpleNamespace(preprocessing=SimpleNamespace(max_seq_length=sh["T"])))
    img, text = interleave_generate(stub, torch.from_numpy(z[name + "_inp"]), torch.from_numpy(z[name + "_unc"]),
                                    reserved_token_mapping={"<|soi|>": sh["soi"], "<|eoi|>": sh["eoi"]}, config=cfgobj,
                                    uni_prompting=SimpleNamespace(text_tokenizer=StubTok()), rng=SeededRng(seed), image_sampler="torch",
                                    text_sampler="torch", **kw)
    assert torch.equal(torch.stack(calls, 0), torch.from_numpy(z[name + "_calls"]))
    assert torch.equal(img.cpu(), torch.from_numpy(z[name + "_img"])) and torch.equal(text.cpu(), torch.from_numpy(z[name + "_text"]))


# --------------------------------------------------------------------------------------------------------------------- 8
class T2iTok:
    def __len__(self):
        return M_T2I_SHAPE["text_vocab"]


def t2i(model, B, guidance, known, **kw):
    sh = M_T2I_SHAPE
    inp, unc = m_t2i_job(5, B, known)
    inp = inp.to(DEV)
    out = t2i_generate(model, input_ids=inp, uncond_input_ids=unc if guidance else None, temperature=1.0, timesteps=4, guidance_scale=guidance,
                       seq_len=sh["N"], mask_token_id=sh["mask_id"], resolution=sh["resolution"], codebook_size=sh["CB"],
                       uni_prompting=SimpleNamespace(text_tokenizer=T2iTok()), image_sampler="device", **kw)
    torch.cuda.synchronize()
    return out, inp


@pytest.mark.parametrize("B,guidance,known", [(2, 3.5, 0), (1, 0, 3)])
def test_t2i_generate_device_sampler(tiny_model, B, guidance, known):
    sh = M_T2I_SHAPE
    N, CB, tv, steps, seed = sh["N"], sh["CB"], sh["text_vocab"], 4, 99
    trace = []
    a, a_in = t2i(tiny_model, B, guidance, known, sampler_seed=seed, rng=RaisingRng(), trace=trace)
    b, b_in = t2i(tiny_model, B, guidance, known, sampler_seed=seed)
    c, _ = t2i(tiny_model, B, guidance, known, sampler_seed=seed + 1)
    assert torch.equal(a, b) and torch.equal(a_in, b_in) and not torch.equal(a, c)
    start = m_t2i_job(5, B, known)[0]
    assert not torch.equal(a_in.cpu(), start), "input_ids is updated in place"
    assert a.shape == (B, N) and int(a.min()) >= 0 and int(a.max()) < CB
    # teacher-forced: each recorded input through the documented parts gives the next one; the last one gives input_ids
    L = start.shape[1]
    i0 = L - (N + 1)
    pos = torch.arange(i0, i0 + N, dtype=torch.int32, device=DEV)
    rows1 = (torch.arange(B, dtype=torch.int32, device=DEV)[:, None] * L + pos[None, :]).reshape(-1)
    rows = torch.cat([rows1, rows1 + B * L]) if guidance else rows1
    mlen = mask_len_schedule(N, steps, cosine_schedule)
    temp, sampled = 1.0, None
    assert len(trace) == steps
    for step, rec in enumerate(trace):
        assert rec.shape[0] == (2 * B if guidance else B)
        both = rec.to(DEV)
        tiny_model.forward_body(both)
        il = tiny_model.head_rows(rows, tv, tv + CB)
        il_c, il_u = (il[:B * N], il[B * N:]) if guidance else (il, il)
        temp = temp * (1.0 - 1.0 * (step + 1) / steps)
        ids, sampled = replay_image_step(tiny_model._handle, il_c, il_u, B, N, CB, float(guidance), tv, seed, IMAGE_COUNTER + step,
                                         both[:B].clone(), pos, temp, mlen[step])
        nxt = trace[step + 1][:B].to(DEV) if step + 1 < steps else a_in
        assert torch.equal(ids, nxt), f"step {step}: the recomputed step is not the next recorded input"
    assert torch.equal(sampled, a), "the returned ids are the ids the last step committed from"


# --------------------------------------------------------------------------------------------------------------------- 9
def test_refusals_on_a_connected_group():
    ids = torch.from_numpy(Z["main_ids"])
    B, L = ids.shape
    sh = M_T2I_SHAPE
    with single_rank_group(synth.CFG_TINY, tiny_sd(), "pull", B * ((L + 7) // 8 * 8)) as m:
        with pytest.raises(ValueError, match="image_sampler='device' needs one rank"):
            interleave(m, sampler_seed=1)
        with pytest.raises(ValueError, match="text_sampler='device' needs one rank"):
            interleave(m, image_sampler="torch", text_sampler="device", text_temperature=0.7, sampler_seed=1)
        with pytest.raises(ValueError, match="image_sampler='device' needs one rank"):
            t2i(m, 1, 0, 0, sampler_seed=1)
        inp, _ = m_t2i_job(5, 1, 0)
        with pytest.raises(ValueError, match="image_sampler='device' needs one rank"):
            next(t2i_generate_decoding_stepwise(m, input_ids=inp.to(DEV), seq_len=sh["N"], mask_token_id=sh["mask_id"],
                                                resolution=sh["resolution"], codebook_size=sh["CB"], image_sampler="device", sampler_seed=1,
                                                uni_prompting=SimpleNamespace(text_tokenizer=T2iTok())))
