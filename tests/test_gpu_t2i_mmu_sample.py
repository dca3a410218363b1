"""generate_image and mmu_generate drawn on the GPU: mmada_image_sample_g (mmada_image_sample_m with a temperature),
mmada_image_commit_g_sampled (mmada_image_commit_g with the Gumbel re-mask noise computed in the kernel), generate_image with
image_sampler="device" and its hipGraph replay, mmu_generate / mmu_generate_fast with text_sampler="device".  Every check is
equality: against torch's own bf16 ops on the CPU, the device's own noise (mmada_probe_gumbel), mmada_image_probs_m,
mmada_image_sample_m, mmada_image_commit_g, mmada_text_select_cfg and the row head (sample_tokens)."""
import itertools
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, bits, t2i_job, tiny_sd
from mmada_parallel_amd import abi, synth
from mmada_parallel_amd.generators.image_generation_generator import generate_image, keep_schedule
from mmada_parallel_amd.generators.interleave_generator import get_num_transfer_tokens
from mmada_parallel_amd.generators.mmu_generator import mmu_generate, mmu_generate_fast
from test_gpu_image_sample import dev_i64, image_inputs, probe_gumbel, st
from test_gpu_kernels import handle   # noqa: F401  (a tiny handle: the sampler entry points only need its cfg)
from test_gpu_m_sample import RaisingRng, m_logits, probe_remask, sample_m
from test_gpu_score import tiny_model   # noqa: F401
from test_gpu_score_tp import single_rank_group
from test_image_sample_host import IMAGE_COUNTER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0123456789abcdef
Z = np.load(os.path.join(GOLDEN, "loss_tiny.npz"))
TV, CBK = synth.TEXT_VOCAB, synth.CODEBOOK


def sample_g(h, cd, ud, B, N, CB, cfg, temp, col0, seed, counter, stats=True):
    """mmada_image_sample_g: (rc, sampled, p_sel, argmax, pmax); the outputs are pre-filled, so a refused call shows."""
    sampled = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    p_sel = torch.full((B, N), -7.0, dtype=torch.bfloat16, device=DEV)
    am = torch.full((B, N), -7, dtype=torch.int32, device=DEV) if stats else None
    pm = torch.full((B, N), -7.0, dtype=torch.bfloat16, device=DEV) if stats else None
    rc = abi.lib().mmada_image_sample_g(h, cd.data_ptr(), ud.data_ptr(), B, N, CB, cfg, temp, col0, seed, counter.data_ptr(),
                                        sampled.data_ptr(), p_sel.data_ptr(), abi.ptr(am), abi.ptr(pm), st())
    return rc, sampled, p_sel, am, pm


def probs_m(h, cd, ud, B, N, CB, cfg):
    probs = torch.empty(B, N, CB, dtype=torch.bfloat16, device=DEV)
    am = torch.empty(B, N, dtype=torch.int32, device=DEV)
    pm = torch.empty(B, N, dtype=torch.bfloat16, device=DEV)
    abi.check(abi.lib().mmada_image_probs_m(h, cd.data_ptr(), ud.data_ptr(), B, N, CB, cfg, probs.data_ptr(), am.data_ptr(), pm.data_ptr(),
                                            st()), "mmada_image_probs_m")
    return probs, am, pm


def key_argmax(l, temp, g):
    """First-index arg-max of l + T * g as two torch fp32 ops on the CPU (no fused multiply-add)."""
    tg = torch.tensor(temp, dtype=torch.float32) * g
    return (l.float() + tg).argmax(-1)


# --------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("N", [1, 5, 67])
@pytest.mark.parametrize("CB", [8, 264, 8192])
def test_sample_g_is_the_argmax_of_the_key_with_image_probs_m_statistics(handle, N, CB):
    (c, u, _), (cd, ud, _) = image_inputs(1, N, CB, None)
    cnt = IMAGE_COUNTER + 7
    wrong = 0
    for cfg in (0.0, 3.5):
        l = m_logits(c, u, cfg).view(N, CB)
        probs, am_ref, pm_ref = probs_m(handle, cd, ud, 1, N, CB, cfg)
        for col0 in (TV, 1001, 7):                     # col0 & 3 == 0, 1, 3
            g = probe_gumbel(SEED, cnt, N, col0, CB).cpu()
            for temp in (0.5, 1.0, 2.0, 8.0):
                ctr = dev_i64(cnt)
                rc, sampled, p_sel, am, pm = sample_g(handle, cd, ud, 1, N, CB, cfg, temp, col0, SEED, ctr)
                abi.check(rc, "mmada_image_sample_g")
                want = key_argmax(l, temp, g).int().view(1, N)
                wrong += int((sampled.cpu() != want).sum())
                what = f"N={N} CB={CB} cfg={cfg} col0={col0} T={temp}"
                assert torch.equal(sampled.cpu(), want), f"{what}: sampled is not the first-index arg-max of l + T * g"
                assert torch.equal(bits(p_sel), bits(probs.gather(-1, sampled.long()[..., None]).squeeze(-1))), f"{what}: p_sel"
                assert torch.equal(am, am_ref) and torch.equal(bits(pm), bits(pm_ref)), f"{what}: argmax / pmax"
                assert int(ctr) == cnt, "mmada_image_sample_g must not write the counter"
                if temp == 1.0:
                    s_m, p_m, am_m, pm_m = sample_m(handle, cd, ud, 1, N, CB, cfg, col0, SEED, ctr, stats=True)
                    assert torch.equal(sampled, s_m) and torch.equal(bits(p_sel), bits(p_m)), f"{what}: not mmada_image_sample_m's draw"
                    assert torch.equal(am, am_m) and torch.equal(bits(pm), bits(pm_m))
                rc, bare, p_bare, _, _ = sample_g(handle, cd, ud, 1, N, CB, cfg, temp, col0, SEED, ctr, stats=False)   # null for both
                assert rc == 0 and torch.equal(bare, sampled) and torch.equal(bits(p_bare), bits(p_sel))
    print(f"N={N} CB={CB}: rows with a wrong draw over 24 (cfg, col0, T) combinations: {wrong}")


@pytest.mark.parametrize("N,CB", [(1, 8), (5, 264), (67, 8192)])
def test_sample_g_at_temperature_0_takes_the_lowest_of_equal_maxima(handle, N, CB):
    (c, u, _), _ = image_inputs(1, N, CB, None)
    c, u = c.clone(), u.clone()
    lo = [(3 * r) % (CB // 2) for r in range(N)]
    for r in range(N):
        for t in (c, u):                                   # equal inputs -> equal combined logits at both places
            t[0, r, lo[r]] = t[0, r, CB - 1 - (r % 3)] = 30.0
    cd, ud = c.to(DEV), u.to(DEV)
    for cfg in (0.0, 3.5):
        ctr = dev_i64(5)
        rc, sampled, p_sel, am, pm = sample_g(handle, cd, ud, 1, N, CB, cfg, 0.0, TV + 1, SEED, ctr)
        abi.check(rc, "mmada_image_sample_g")
        assert sampled.view(-1).tolist() == lo and torch.equal(sampled, am), "T = 0: the plain first-index arg-max"
        assert torch.equal(bits(p_sel), bits(pm)) and int(ctr) == 5


def test_sample_g_refuses_bad_arguments_and_writes_nothing(handle):
    _, (cd, ud, _) = image_inputs(1, 5, 264, None)
    ctr = dev_i64(9)
    for temp, cb, match in ((-0.5, 264, b"not a finite value >= 0"), (float("inf"), 264, b"not a finite value >= 0"),
                            (float("nan"), 264, b"not a finite value >= 0"), (1.0, 260, b"multiple of 8 and <= 16384"),
                            (1.0, 0, b"multiple of 8 and <= 16384"), (1.0, 16384 + 8, b"multiple of 8 and <= 16384")):
        rc, sampled, p_sel, am, pm = sample_g(handle, cd, ud, 1, 5, cb, 3.5, temp, TV, SEED, ctr)
        assert rc != 0 and match in abi.lib().mmada_last_error(), (temp, cb)
        torch.cuda.synchronize()
        assert bool((sampled == -7).all()) and bool((am == -7).all()) and bool((p_sel == -7).all()) and bool((pm == -7).all())
        assert int(ctr) == 9


# --------------------------------------------------------------------------------------------------------------------- 2
def test_sample_g_draws_what_the_row_head_draws(tiny_model):
    """Without guidance the combined logits are the head's own bf16 logits, so mmada_head_sample and this kernel maximise the same
    fp32 keys."""
    ids = torch.from_numpy(Z["main_ids"]).to(DEV)
    B, L = ids.shape
    tiny_model.forward_body(ids)
    rows = torch.arange(B * L, dtype=torch.int32, device=DEV)
    logits = tiny_model.head_rows(rows, TV, TV + CBK)
    for temp in (0.7, 1.0):
        s, c = SEED ^ 0xabc, IMAGE_COUNTER + 5
        head_ids = tiny_model.sample_tokens(rows, temp, TV, TV + CBK, seed=s, counter=dev_i64(c))[0]
        rc, sampled, _, _, _ = sample_g(tiny_model._handle, logits, logits, 1, B * L, CBK, 0.0, temp, TV, s, dev_i64(c), stats=False)
        abi.check(rc, "mmada_image_sample_g")
        assert torch.equal(sampled.view(-1) + TV, head_ids), f"T={temp}"


# --------------------------------------------------------------------------------------------------------------------- 3
def commit_g(h, ids, B, L, pos, N, sampled, p, gumbel, temp, keep, tv):
    out = ids.clone()
    abi.check(abi.lib().mmada_image_commit_g(h, out.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p.data_ptr(), gumbel.data_ptr(),
                                             temp, keep.data_ptr(), tv, st()), "mmada_image_commit_g")
    return out


def commit_g_sampled(h, ids, B, L, pos, N, sampled, p, temp, seed, ctr, keep, tv):
    out = ids.clone()
    abi.check(abi.lib().mmada_image_commit_g_sampled(h, out.data_ptr(), B, L, pos.data_ptr(), N, sampled.data_ptr(), p.data_ptr(), temp,
                                                     seed, ctr.data_ptr(), keep.data_ptr(), tv, st()), "mmada_image_commit_g_sampled")
    return out


def commit_inputs_g(case, N):
    g = torch.Generator().manual_seed({"all_unknown": 1, "some_known": 2, "none_unknown": 3}[case] * 10007 + N)
    B, L = 2, N + 20
    pos = torch.sort(torch.randperm(L - 10, generator=g)[:N]).values + 5
    ids = torch.randint(0, 1000, (B, L), generator=g)
    known = {"all_unknown": 0, "some_known": N // 2, "none_unknown": N}[case]
    for b in range(B):
        perm = torch.randperm(N, generator=g)
        ids[b, pos] = synth.MASK
        ids[b, pos[perm[:known]]] = TV + torch.randint(0, CBK, (known,), generator=g)
    sampled = torch.randint(0, CBK, (B, N), generator=g, dtype=torch.int32)
    # bf16 probabilities from a coarse set, p == 0 included -> the clamp at 1e-20 and many ties at the cut-off
    p = (torch.randint(0, 40, (B, N), generator=g).float() / 4096).to(torch.bfloat16)
    return B, L, N - known, ids.to(DEV), pos.to(torch.int32).to(DEV), sampled.to(DEV), p.to(DEV)


@pytest.mark.parametrize("N", [1, 4, 64, 1024])
@pytest.mark.parametrize("case", ["all_unknown", "some_known", "none_unknown"])
def test_commit_g_sampled_is_image_commit_g_on_the_probed_noise(handle, case, N):
    B, L, unknown, ids, pos, sampled, p = commit_inputs_g(case, N)
    c = IMAGE_COUNTER + 21
    noise = [probe_remask(SEED, c + i, B * N).to(torch.bfloat16).view(B, N) for i in range(2)]
    assert not torch.equal(noise[0], noise[1])
    differs = 0
    for temp, keep_v in itertools.product((0.6, 1.0, 8.0), (0, 1, unknown - 1, unknown + 3)):
        keep = torch.tensor([keep_v], dtype=torch.int32, device=DEV)
        ctr = dev_i64(c)
        got = commit_g_sampled(handle, ids, B, L, pos, N, sampled, p, temp, SEED, ctr, keep, TV)
        assert torch.equal(got, commit_g(handle, ids, B, L, pos, N, sampled, p, noise[0], temp, keep, TV)), f"temp={temp} keep={keep_v}"
        assert int(ctr) == c + 1, "the counter advances by exactly 1 per call"
        if case == "none_unknown":
            assert torch.equal(got, ids), "with no unknown slot no id changes"
        again = commit_g_sampled(handle, ids, B, L, pos, N, sampled, p, temp, SEED, ctr, keep, TV)   # the noise of c + 1
        assert torch.equal(again, commit_g(handle, ids, B, L, pos, N, sampled, p, noise[1], temp, keep, TV)), "second call"
        assert int(ctr) == c + 2
        differs += int(not torch.equal(got, again))
    print(f"{case} N={N}: (temperature, keep_n) combinations whose two counters re-mask other positions: {differs} of 12")
    if case != "none_unknown" and N >= 64:
        assert differs > 0, "the noise of another counter re-masks other positions"


# --------------------------------------------------------------------------------------------------------------------- 4
def g_kwargs(job, **kw):
    out = dict(seq_len=job["seq_len"], newline_every=job["newline_every"], uncon_ids=job["uncon_ids"], code_start=job["code_start"])
    out.update(kw)
    return out


def linear_schedule(t):
    """1 - t: with it 4 slots over 8 timesteps keep 3, 3, 2, 2, 1, 1, 1, 0 (floor(4 * (1 - (step + 1) / 8)) floored at 1, 0 on the last
    step); the default cosine schedule gives 3, 3, 3, 2, 2, 1, 1, 0.  Either empties a mask of 4 within four steps, because a step
    keeps at most unknown - 1 slots masked."""
    return 1.0 - t


EARLY = [3, 3, 2, 2, 1, 1, 1, 0]


def reference_image_loop(model, job, timesteps, temperature, cfg, seed, schedule=None):
    """generate_image's device path rebuilt from parts that exist without it: forward_body, head_rows on every slot, torch's bf16
    combine on the CPU, the probed noise, mmada_image_probs_m and mmada_image_commit_g.  Returns the ids before every step (and,
    with guidance, the unconditional ids of every step) and the ids after the last."""
    h = model._handle
    x = job["prompt"].to(DEV).clone()
    L = x.shape[1]
    slots = (x[0] == synth.MASK).nonzero()[:, 0]
    N, off = int(slots.numel()), model.vocab - CBK
    pos = slots.to(torch.int32).contiguous()
    keep = keep_schedule(N, timesteps, *([schedule] if schedule else []))
    cs, uncon = job["code_start"], job["uncon_ids"].to(DEV)
    U = uncon.shape[1]
    seen = []
    for step in range(timesteps):
        cnt = IMAGE_COUNTER + step
        seen.append(x.cpu().clone())
        model.forward_body(x)
        cond = model.head_rows(pos, off, off + CBK)
        unc = cond
        if cfg > 0:
            unc_ids = torch.cat((uncon, x[:, cs - 2:]), dim=1).contiguous()
            seen.append(unc_ids.cpu().clone())
            model.forward_body(unc_ids)
            unc = model.head_rows((pos - (cs - 2) + U).contiguous(), off, off + CBK)
        l = m_logits(cond.cpu(), unc.cpu(), cfg) if cfg > 0 else cond.cpu()
        g = probe_gumbel(seed, cnt, N, off, CBK).cpu()
        sampled = key_argmax(l, temperature, g).to(torch.int32).view(1, N).to(DEV)
        probs, _, _ = probs_m(h, cond, unc, 1, N, CBK, float(cfg) if cfg > 0 else 0.0)
        p = probs.gather(-1, sampled.long()[..., None]).squeeze(-1).contiguous()
        gumbel = probe_remask(seed, cnt, N).to(torch.bfloat16).view(1, N)
        x = commit_g(h, x, 1, L, pos, N, sampled, p, gumbel, float(temperature), torch.tensor([keep[step]], dtype=torch.int32, device=DEV), off)
    return seen, x


@pytest.mark.parametrize("side,timesteps,cfg,temperature", [(4, 5, 0.0, 1.0), (4, 5, 2.0, 0.6), (2, 8, 2.0, 1.0), (2, 8, 0.0, 0.6)])
def test_generate_image_device_sampler_is_the_loop_of_its_parts(tiny_model, side, timesteps, cfg, temperature):
    job = t2i_job(side=side)
    seed, trace = 4321, []
    early = dict(noise_schedule=linear_schedule) if side == 2 else {}      # the job that empties its mask early
    vq = generate_image(tiny_model, job["prompt"], **g_kwargs(job, timesteps=timesteps, temperature=temperature, cfg_scale=cfg,
                                                              image_sampler="device", sampler_seed=seed, trace=trace, rng=RaisingRng(),
                                                              **early))
    seen, x = reference_image_loop(tiny_model, job, timesteps, temperature, cfg, seed, early.get("noise_schedule"))
    assert len(trace) == len(seen) == timesteps * (2 if cfg > 0 else 1), "all timesteps run, no early exit"
    for i, (a, b) in enumerate(zip(trace, seen)):
        assert torch.equal(a, b), f"model call {i}: the ids are not the loop's"
    want = x[0, job["code_start"]:-2]
    want = want[want != synth.NEW_LINE].view(1, job["seq_len"])
    assert torch.equal(vq, want) and not bool((vq == synth.MASK).any())
    assert int(vq.min()) >= tiny_model.vocab - CBK and int(vq.max()) < tiny_model.vocab   # every slot was filled
    if side == 2:   # 4 slots, 8 timesteps: the mask is empty well before the end, the remaining steps change nothing
        assert keep_schedule(4, 8, linear_schedule) == EARLY
        stride = 2 if cfg > 0 else 1
        empty_from = [i for i in range(timesteps) if not bool((trace[i * stride] == synth.MASK).any())]
        print(f"the input of step {empty_from[0] if empty_from else None} is the first without a masked slot")
        assert empty_from and empty_from[0] <= 6, "nothing is unknown after step 5"
        for i in empty_from:
            assert torch.equal(trace[i * stride], x.cpu()), "a step with nothing unknown is a no-op"


# --------------------------------------------------------------------------------------------------------------------- 5
def test_generate_image_device_sampler_repeats_replays_and_leaves_the_default_alone(tiny_model, monkeypatch):
    job = t2i_job(side=4)
    timesteps = 6
    kw = g_kwargs(job, timesteps=timesteps, temperature=1.0, cfg_scale=2.0)

    def no_probs(*a):
        raise AssertionError("mmada_image_probs_m called: the [n, CB] probabilities must not exist on the device path")

    with monkeypatch.context() as mp:
        mp.setattr(abi.lib(), "mmada_image_probs_m", no_probs, raising=False)
        a = generate_image(tiny_model, job["prompt"], image_sampler="device", sampler_seed=77, rng=RaisingRng(), graph=False, **kw)
        b = generate_image(tiny_model, job["prompt"], image_sampler="device", sampler_seed=77, graph=False, **kw)
        c = generate_image(tiny_model, job["prompt"], image_sampler="device", sampler_seed=78, graph=False, **kw)
        before = tiny_model.graph_replays
        r = generate_image(tiny_model, job["prompt"], image_sampler="device", sampler_seed=77, rng=RaisingRng(), graph=True, **kw)
        torch.cuda.synchronize()
        replays = tiny_model.graph_replays - before
    print(f"{replays} step replays of {timesteps} steps, {tiny_model.graph_nodes.get(('generate_image',))} nodes")
    assert torch.equal(a, b) and not torch.equal(a, c), "the same seed repeats the run, another seed draws another image"
    assert replays == timesteps - 1, "graph_replays counts every graph launch: the first step runs eagerly, every later one launches"
    assert torch.equal(r, a), "the replayed run's ids are not the eager run's"
    # the default path: the same result with the new keywords absent, at their defaults, and whatever `graph` says
    for temperature in (0.0, 1.0):
        kw_t = dict(kw, temperature=temperature)
        outs = []
        before = tiny_model.graph_replays
        for extra in ({}, dict(image_sampler="torch", sampler_seed=None, graph=None), dict(image_sampler="torch", sampler_seed=5, graph=True)):
            torch.manual_seed(1234)
            outs.append(generate_image(tiny_model, job["prompt"], **kw_t, **extra))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"temperature={temperature}"
        assert tiny_model.graph_replays == before, "the torch path is never captured"
    # refusals
    for extra, match in ((dict(image_sampler="device", sampler_seed=1, temperature=0.0), "image_sampler='device' needs temperature > 0"),
                         (dict(image_sampler="device"), "image_sampler='device' needs sampler_seed"),
                         (dict(image_sampler="gpu", sampler_seed=1), "image_sampler='gpu'")):
        with pytest.raises(ValueError, match=match):
            generate_image(tiny_model, job["prompt"], **dict(kw, **extra))


# --------------------------------------------------------------------------------------------------------------------- 6
MMU = dict(max_new_tokens=16, steps=8, block_length=8)
MMU_TEMP = 0.7


def mmu_idx(B=2):
    return torch.randint(0, 1000, (B, 9), generator=torch.Generator().manual_seed(2))


def reference_mmu_loop(model, idx, cfg, seed):
    """mmu_generate's device path rebuilt from parts that exist without it.  Guidance: head_rows, torch's bf16 combine on the CPU,
    the probed noise, mmada_text_select_cfg with that x0_in.  No guidance: sample_tokens, then the commit rule in torch — the k
    masked positions of the block with the highest log-probability, the lowest position on a tie."""
    lib, h = abi.lib(), model._handle
    B, P = idx.shape
    BL, V = MMU["block_length"], model.vocab
    L = P + MMU["max_new_tokens"]
    nblocks = MMU["max_new_tokens"] // BL
    steps = MMU["steps"] // nblocks
    x = torch.full((B, L), synth.MASK, dtype=torch.long, device=DEV)
    x[:, :P] = idx.to(DEV)
    scratch = torch.empty(B * BL * 16, dtype=torch.uint8, device=DEV)
    seen, cnt = [], 0
    for nb in range(nblocks):
        start = P + nb * BL
        k = get_num_transfer_tokens((x[:, start:start + BL] == synth.MASK).cpu(), steps)            # [B, steps]
        rows = (torch.arange(B, dtype=torch.int32, device=DEV)[:, None] * L + start
                + torch.arange(BL, dtype=torch.int32, device=DEV)[None, :]).reshape(-1).contiguous()
        for i in range(steps):
            if cfg > 0:
                un_x = x.clone()
                un_x[:, :P] = synth.MASK
                both = torch.cat([x, un_x], dim=0).contiguous()
                seen.append(both.cpu().clone())
                model.forward_body(both)
                lg = model.head_rows(torch.cat([rows, rows + B * L]), 0, V)
                cond, unc = lg[:B * BL], lg[B * BL:]
                cc, uc = cond.cpu(), unc.cpu()
                comb = uc + float(cfg + 1) * (cc - uc)                                              # bf16 tensor ops (:666)
                g = probe_gumbel(seed, cnt, B * BL, 0, V).cpu()
                x0 = key_argmax(comb, MMU_TEMP, g).to(torch.int32).to(DEV).contiguous()
                k_i = k[:, i].to(device=DEV, dtype=torch.int32).contiguous()
                abi.check(lib.mmada_text_select_cfg(h, unc.data_ptr(), cond.data_ptr(), float(cfg + 1), x0.data_ptr(), B, BL, V, V,
                                                    x.data_ptr(), L, start, k_i.data_ptr(), scratch.data_ptr(), st()), "mmada_text_select_cfg")
            else:
                seen.append(x.cpu().clone())
                model.forward_body(x)
                tok, lp = model.sample_tokens(rows, MMU_TEMP, seed=seed, counter=dev_i64(cnt))[:2]
                tok, lp = tok.view(B, BL).cpu(), lp.view(B, BL).cpu().double()
                blk = x[:, start:start + BL].cpu()
                lp[blk != synth.MASK] = -float("inf")
                order = torch.sort(lp, dim=1, descending=True, stable=True).indices                # the lowest position on a tie
                for b in range(B):
                    take = [int(t) for t in order[b, :int(k[b, i])] if blk[b, t] == synth.MASK]
                    x[b, start + torch.tensor(take, dtype=torch.long)] = tok[b, take].long().to(DEV)
            cnt += 1
    return seen, x


@pytest.mark.parametrize("cfg", [0.0, 1.5])
def test_mmu_generate_device_sampler_is_the_loop_of_its_parts(tiny_model, cfg):
    idx = mmu_idx()
    seed, trace = 99, []
    kw = dict(MMU, temperature=MMU_TEMP, cfg_scale=cfg, text_sampler="device")
    a = mmu_generate(tiny_model, idx, sampler_seed=seed, rng=RaisingRng(), trace=trace, **kw)
    seen, x = reference_mmu_loop(tiny_model, idx, cfg, seed)
    assert len(trace) == len(seen) == MMU["steps"]
    for i, (s, t) in enumerate(zip(trace, seen)):
        assert torch.equal(s, t), f"step {i}: the ids are not the loop's"
    assert torch.equal(a, x) and not bool((a == synth.MASK).any()) and torch.equal(a[:, :9].cpu(), idx)
    b = mmu_generate(tiny_model, idx, sampler_seed=seed, **kw)
    assert torch.equal(a, b), "the same seed repeats the run"


@pytest.mark.parametrize("cfg", [0.0, 1.5])
def test_mmu_generate_device_sampler_seeds_and_the_fast_variant(tiny_model, cfg):
    # one block of 32 committed in one step: the returned block is the 64 draws of that step
    one = dict(max_new_tokens=32, steps=1, block_length=32, temperature=MMU_TEMP, cfg_scale=cfg, text_sampler="device")
    idx = mmu_idx()
    d1 = mmu_generate(tiny_model, idx, sampler_seed=1, rng=RaisingRng(), **one)[:, 9:]
    d2 = mmu_generate(tiny_model, idx, sampler_seed=2, rng=RaisingRng(), **one)[:, 9:]
    assert d1.numel() == 64 and not bool((d1 == synth.MASK).any()) and not torch.equal(d1, d2), "two seeds draw differently"
    # mmu_generate_fast: a block that ends in eot_token in every row ends the run, the later blocks stay masked
    idx1 = mmu_idx(1)
    kw = dict(MMU, temperature=MMU_TEMP, cfg_scale=cfg, text_sampler="device", sampler_seed=7)
    full = mmu_generate(tiny_model, idx1, **kw)
    stop = mmu_generate_fast(tiny_model, idx1, eot_token=int(full[0, 9 + 7]), rng=RaisingRng(), **kw)
    assert torch.equal(stop[:, :17], full[:, :17]) and bool((stop[:, 17:] == synth.MASK).all())
    other = mmu_generate_fast(tiny_model, idx1, eot_token=-5, **kw)          # never met: every block runs
    assert torch.equal(other, full)


def test_refusals(tiny_model, monkeypatch):
    idx = mmu_idx()
    for extra, match in ((dict(text_sampler="device", sampler_seed=1, temperature=0.0), "text_sampler='device' needs temperature > 0"),
                         (dict(text_sampler="device", temperature=0.7), "text_sampler='device' needs sampler_seed"),
                         (dict(text_sampler="gpu", sampler_seed=1, temperature=0.7), "text_sampler='gpu'")):
        with pytest.raises(ValueError, match=match):
            mmu_generate(tiny_model, idx, **dict(MMU, **extra))
    with pytest.raises(ValueError, match="text_sampler='device' needs sampler_seed"):
        mmu_generate_fast(tiny_model, idx, text_sampler="device", temperature=0.7, **MMU)
    monkeypatch.setenv("MMADA_MICROBATCH", "1")
    with pytest.raises(ValueError, match="text_sampler='device' needs a forward without micro-batched lanes"):
        mmu_generate(tiny_model, idx, text_sampler="device", temperature=0.7, sampler_seed=1, **MMU)
    monkeypatch.delenv("MMADA_MICROBATCH")
    job = t2i_job(side=4)
    L = job["prompt"].shape[1] + job["uncon_ids"].shape[1]
    with single_rank_group(synth.CFG_TINY, tiny_sd(), "pull", 2 * ((L + 7) // 8 * 8)) as m:
        with pytest.raises(ValueError, match="image_sampler='device' needs one rank"):
            generate_image(m, job["prompt"], **g_kwargs(job, timesteps=4, temperature=1.0, image_sampler="device", sampler_seed=1))
        with pytest.raises(ValueError, match="text_sampler='device' needs one rank"):
            mmu_generate(m, idx, text_sampler="device", temperature=0.7, sampler_seed=1, **MMU)
