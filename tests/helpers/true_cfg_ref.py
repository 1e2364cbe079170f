"""True CFG restated (DESIGN.md section 4 "True CFG"): the combine of FluxCFGPipeline's loop, noise_pred = neg + true_cfg * (pos - neg)
on bf16 tensors, as the three roundings torch performs; two named WRONG variants that tests must tell apart from it; the Euler step on
the result; and the engine's CFG loop issued from Python, one launch at a time (GPU), with the combine written as the literal torch
expression and the step taken by scheduler.step.  tests/golden/g18_true_cfg.safetensors holds the reference's own results."""
import torch

BF = torch.bfloat16
SCALES = (1.5, 3.3, 7.0, 30.0)


def bits(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    """equal bit for bit, NaNs compared by position (a NaN's payload and sign are not part of the contract)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def differing(a, b):
    """number of elements that differ (NaN against NaN counts as equal)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return int(((bits(a) != bits(b)) & ~(na & nb)).sum())


def combine(neg, pos, g):
    """d = bf16(f32(pos) - f32(neg));  m = bf16(f32(g) f32(d));  v = bf16(f32(neg) + f32(m)) -- every torch op of the reference's line
    rounds on its own and the Python float takes part as fp32"""
    g32 = torch.tensor(g, dtype=torch.float32)
    d = (pos.float() - neg.float()).to(BF)
    m = (g32 * d.float()).to(BF)
    return (neg.float() + m.float()).to(BF)


def combine_scale_in_bf16(neg, pos, g):
    """WRONG: the scale rounded to bf16 before it multiplies (3.3 -> 3.296875)"""
    return combine(neg, pos, float(torch.tensor(g, dtype=torch.float32).to(BF)))


def combine_single_rounding(neg, pos, g):
    """WRONG: the three ops in fp32 with one rounding at the end"""
    return (neg.float() + torch.tensor(g, dtype=torch.float32) * (pos.float() - neg.float())).to(BF)


def euler_step(v, lat, sigmas, i):
    """FlowMatchEulerDiscreteScheduler.step on bf16 tensors: x' = bf16(f32(x) + bf16(dsigma f32(v))), dsigma = sigma_{i+1} - sigma_i in
    fp32 and then ROUNDED TO BF16 -- a 0-dim fp32 tensor times a bf16 tensor is computed in bf16's type
    (scheduling_flow_match_euler_discrete.py:319-330)"""
    ds = (sigmas[i + 1].float() - sigmas[i].float()).to(BF).float()
    return (lat.float() + (ds * v.float()).to(BF).float()).to(BF)


def loop(pipe, latents, masked_image_latents, prompt_embeds, pooled, neg_embeds, neg_pooled, grid, true_cfg, guidance_scale=30.0,
         on_step=None, per_step=None):
    """The reference's CFG loop on the engine's forward (GPU): per step one ses.run on [negative; positive] with both halves of xin
    holding [latents | masked_image_latents], the combine as the reference writes it, scheduler.step.  Call after a pipeline call at
    this geometry: pipe.scheduler then holds the call's timesteps.  on_step(i, latents) -> latents or None: a step callback."""
    from tests.helpers.plain_loop import mod_table
    from textflux_amd import ops
    tr, sch = pipe.transformer, pipe.scheduler
    B, S, C = latents.shape
    T = prompt_embeds.shape[1]
    timesteps = sch.timesteps
    ses = tr.session(2 * B, S, T)
    ses.set_conditioning(torch.cat([neg_embeds, prompt_embeds], dim=0).to("cuda", BF), torch.zeros(T, 3),
                         pipe._prepare_latent_image_ids(B, *grid, "cuda", BF))
    mod = mod_table(pipe, timesteps, 2 * B, torch.cat([neg_pooled, pooled], dim=0), guidance_scale)
    lat = latents.to("cuda", BF).contiguous().clone()
    mil = masked_image_latents.to("cuda", BF).contiguous()
    sch._step_index = None
    sch._begin_index = None
    for i, t in enumerate(timesteps):
        ses.xin.copy_(torch.cat([torch.cat([lat, mil], dim=2)] * 2))
        noise_pred = ses.run(mod[i]).clone()
        neg_noise_pred, noise_pred = noise_pred.chunk(2)
        noise_pred = neg_noise_pred + true_cfg * (noise_pred - neg_noise_pred)
        lat = sch.step(noise_pred, t, lat, return_dict=False)[0]
        if on_step is not None:
            new = on_step(i, lat)
            lat = lat if new is None else new.to("cuda", BF)
        if per_step is not None:
            per_step.append(lat.clone())
    return lat


def launch_loop(pipe, latents, masked_image_latents, prompt_embeds, pooled, neg_embeds, neg_pooled, grid, true_cfg, sampler="euler",
                guidance_scale=30.0, amo_noise=None, keep=None, change=None, per_step=None):
    """The launches of tfx_dit_step_run_ex3 with a tfx_step_cfg, issued one by one from Python (GPU): per step tfx_dit_forward on 2B
    (ses.run), ops.cfg_combine over the two halves of its output into the first, the sampler's own op on B samples (mirrored into
    the first half of xin), the blend when given, and the copy of the new latents into the second half of xin.  Call after a pipeline
    call: pipe.scheduler then holds the call's timesteps, begin_index and tables.  sampler: "euler" | "amo" | "multistep".  keep:
    dict(x0, noise, mask) -- ops.known_region_blend; change: dict(x0, noise, hold, last) -- ops.change_map_blend."""
    from tests.helpers.change_map_ref import cut_table
    from tests.helpers.keep_known_ref import keep_sigma
    from tests.helpers.plain_loop import mod_table
    from textflux_amd import ops
    tr, sch = pipe.transformer, pipe.scheduler
    B, S, C = latents.shape
    T = prompt_embeds.shape[1]
    begin = sch.begin_index or 0
    timesteps = sch.timesteps[begin:]
    n = len(timesteps)
    ses = tr.session(2 * B, S, T)
    ses.set_conditioning(torch.cat([neg_embeds, prompt_embeds], dim=0).to("cuda", BF), torch.zeros(T, 3),
                         pipe._prepare_latent_image_ids(B, *grid, "cuda", BF))
    coef = sch.coef_table("cuda", BF)
    assert coef.shape[0] == n
    mod = mod_table(pipe, timesteps, 2 * B, torch.cat([neg_pooled, pooled], dim=0), guidance_scale)
    scale = torch.tensor([true_cfg], dtype=torch.float32, device="cuda")
    lat = latents.to("cuda", BF).contiguous().clone()
    hist = torch.full_like(lat, float("nan"))
    mil = masked_image_latents.to("cuda", BF).contiguous()
    first, second = ses.xin[:B], ses.xin[B:]
    for half in (first, second):
        ops.scatter_cols_(lat, half, 0)
        ops.scatter_cols_(mil, half, C)
    known = keep if keep is not None else change
    if known is not None:
        sig = keep_sigma(sch._sigmas_host, begin).cuda()
    if change is not None:
        cut, hold = cut_table(n, change["last"]).cuda(), change["hold"].cuda().contiguous()
    for i in range(n):
        out = ses.run(mod[i])
        v = ops.cfg_combine(out[:B], out[B:], scale, out=out[:B])
        if sampler == "amo":
            ops.amo_step_(v, lat, coef, amo_noise[i].to("cuda", torch.float32).contiguous(), step=i, xin=first)
        elif sampler == "multistep":
            ops.multistep_step_(v, lat, coef, hist, step=i, xin=first)
        else:
            ops.euler_step_(v, lat, coef, step=i, xin=first)
        if keep is not None:
            ops.known_region_blend(lat, keep["x0"], keep["noise"], keep["mask"], sig, step=i, xin=first)
        if change is not None:
            ops.change_map_blend(lat, change["x0"], change["noise"], hold, cut, sig, step=i, xin=first)
        ops.copy_rows_(first[:, :, :C], second[:, :, :C])
        if per_step is not None:
            per_step.append(lat.clone())
    return lat
