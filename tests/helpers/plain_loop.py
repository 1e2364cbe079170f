"""The denoising loop restated from public pieces, one Python-issued launch at a time: FluxTransformer2DModel.session / temb /
modulation, DitSession.set_conditioning / run, ops.scatter_cols_ / euler_step_ / amo_step_.  The pipeline issues every step through
the library's tfx_dit_step_run (textflux_amd/step_loop.py); this is the independent composition its results are compared with,
bit for bit.  GPU only."""
import torch

BF = torch.bfloat16


def mod_table(pipe, timesteps, B, pooled, guidance_scale, dsigma=None):
    """[n, B, mod_len] modulation rows of all steps, rows ordered (step, sample); timesteps [n] or [n, B].  dsigma ([n] or [n, B]):
    the rows grow by EULER_PAD columns holding the step's Euler coefficient (DitSession.run(..., euler=True)).  The table is built
    as the pipeline builds its own, so a mistake in the row order or the dsigma layout would be shared: what guards the table are
    the oracle trajectories (per-step MAE against g5_pipeline and against each sample's own oracle run); this helper guards the
    launches behind it."""
    from textflux_amd.transformer import EULER_PAD
    tr = pipe.transformer
    t = timesteps.detach().float().cpu()
    n = t.shape[0]
    t = t.view(n, -1).expand(n, B)
    t_rows = torch.tensor([pipe._timestep_chain(x, BF) for x in t.reshape(-1)], dtype=torch.float32).cuda()
    g_rows = torch.full((n * B,), float((torch.full([1], guidance_scale).to(BF) * 1000).float()), dtype=torch.float32, device="cuda")
    mod = tr.modulation(tr.temb(t_rows, g_rows, pooled.to("cuda", BF).repeat(n, 1))).view(n, B, tr.mod_len)
    if dsigma is None:
        return mod
    modx = torch.empty(n, B, tr.mod_len + EULER_PAD, dtype=BF, device="cuda")
    modx[:, :, :tr.mod_len] = mod
    modx[:, :, tr.mod_len:] = dsigma.to("cuda", BF).reshape(n, -1, 1).expand(n, B, 1)
    return modx


def plain_loop(pipe, latents, masked_image_latents, prompt_embeds, pooled_prompt_embeds, grid, guidance_scale=30.0, fused=False,
               amo_noise=None, forward=None, per_step=None):
    """The latents after every step of pipe.scheduler's current schedule -- call after a pipeline call at this geometry: the
    scheduler then holds the call's timesteps and coefficients.  grid: (h2, w2) of the latent grid.  fused: the Euler update in
    proj_out's epilogue (ses.run(modx[i], euler=True)) instead of the scheduler kernel; amo_noise: the AMO sampler's eps per step.
    forward(ses, mod_i, i) -> model output replaces the whole forward ses.run(mod_i) (unfused forms).  per_step: a list that
    receives a clone of the latents after every step."""
    from textflux_amd import ops
    tr, sch = pipe.transformer, pipe.scheduler
    B, S, C = latents.shape
    T = prompt_embeds.shape[1]
    n = len(sch.timesteps)
    ses = tr.session(B, S, T)
    ses.set_conditioning(prompt_embeds.to("cuda", BF), torch.zeros(T, 3), pipe._prepare_latent_image_ids(B, *grid, "cuda", BF))
    coef = sch.coef_table("cuda", BF)
    mod = mod_table(pipe, sch.timesteps, B, pooled_prompt_embeds, guidance_scale, coef[:n] if fused else None)
    lat = latents.to("cuda", BF).contiguous().clone()
    ops.scatter_cols_(lat, ses.xin, 0)
    ops.scatter_cols_(masked_image_latents.to("cuda", BF).contiguous(), ses.xin, C)
    for i in range(n):
        if fused:
            ses.run(mod[i], euler=True)
            lat = ses.xin[:, :, :C].clone()
        else:
            v = forward(ses, mod[i], i) if forward is not None else ses.run(mod[i])
            if amo_noise is not None:
                ops.amo_step_(v, lat, coef, amo_noise[i].to("cuda", torch.float32).contiguous(), step=i, xin=ses.xin)
            else:
                ops.euler_step_(v, lat, coef, step=i, xin=ses.xin)
        if per_step is not None:
            per_step.append(lat.clone())
    return lat


def mixed_fused_loop(pipe, latents, masked_image_latents, prompt_embeds, pooled_prompt_embeds, grids, n, guidance_scale=30.0):
    """call_mixed restated: sample b has the latent grid grids[b] = (h2, w2), latents[b] [1, S_b, C] and masked_image_latents[b]
    [1, S_b, *]; rows padded to T + S a multiple of 256, every sample on its own sigma schedule (per_sample_schedules), the fused
    Euler step per Python-issued forward.  Returns the final latents [S_b, C] per sample."""
    from textflux_amd.pipeline import per_sample_schedules
    tr = pipe.transformer
    B, T, C = len(grids), prompt_embeds.shape[1], latents[0].shape[-1]
    S_b = [h2 * w2 for h2, w2 in grids]
    S = (T + max(S_b) + 255) // 256 * 256 - T
    ses = tr.session(B, S, T, mixed=True)
    ses.set_conditioning(prompt_embeds.to("cuda", BF), torch.zeros(T, 3), [pipe._prepare_latent_image_ids(1, h2, w2, "cuda", BF) for h2, w2 in grids])
    tabs = per_sample_schedules(pipe.scheduler, S_b, n)
    modx = mod_table(pipe, tabs["timesteps"].t(), B, pooled_prompt_embeds, guidance_scale, tabs["dsigma"].t())
    for b in range(B):
        ses.xin[b, :S_b[b], :C].copy_(latents[b][0].to("cuda", BF))
        ses.xin[b, :S_b[b], C:].copy_(masked_image_latents[b][0].to("cuda", BF))
    for i in range(n):
        ses.run(modx[i], euler=True)
    return [ses.xin[b, :S_b[b], :C].clone() for b in range(B)]
