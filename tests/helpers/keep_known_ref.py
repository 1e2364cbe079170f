"""torch-CPU restatement of known-region sampling (include/textflux_hip.h: tfx_known_region_blend, tfx_keep_mask_pack; DESIGN.md
section 4 "Known-region sampling"), written from the specification with no code shared with the package: every op in fp32 on bf16
operands, rounded to bf16 on its own.

    scale_noise(x0, s, n) = bf16( bf16(s n) + bf16( bf16(1 - s) x0 ) )          s = bf16(sigma); s < 0 stands for "x0 itself"
    blend(x, p, m)        = bf16( bf16( bf16(1 - m) p ) + bf16(m x) )
    keep_sigma(sigmas, b) = [bf16(sigma_{b+1}), ..., bf16(sigma_{n-1}), -1]      sigmas fp32 [n + 1], the last one 0

tests/golden/g16_keep_known.safetensors holds what the reference computes for the same inputs (tests/test_keep_known_cpu.py compares).
`loop` is the GPU side: the pipeline's denoising loop issued from Python, one forward, one sampler op and one blend per step."""
import torch

BF = torch.bfloat16


def _r(t):
    """fp32 -> the nearest bf16 value (ties to even), as fp32"""
    return t.to(BF).float()


def scale_noise(x0, sigma, noise):
    """x0, noise bf16; sigma a float (already bf16-exact or not: it is rounded here, as `sigmas.to(dtype=sample.dtype)` does)"""
    s = _r(torch.tensor(float(sigma), dtype=torch.float32))
    if float(s) < 0:
        return x0.clone()
    a = _r(s * noise.float())
    u = _r(1.0 - s)
    b = _r(u * x0.float())
    return (a + b).to(BF)


def blend(x, x0, noise, mask, sigma):
    """the whole kernel: x' = (1 - m) scale_noise(x0, sigma, noise) + m x"""
    p = scale_noise(x0, sigma, noise).float()
    m = mask.float()
    w = _r(1.0 - m)
    c = _r(w * p)
    d = _r(m * x.float())
    return (c + d).to(BF)


def keep_sigma(sigmas, begin=0):
    """sigmas fp32 [n + 1] (closing 0 included) -> fp32 [n - begin]"""
    s = torch.as_tensor(sigmas, dtype=torch.float32)[begin:]
    tab = _r(s[1:].clone())
    tab[-1] = -1.0
    return tab


def get_timesteps(n, strength):
    """(t_start, steps)"""
    t_start = int(max(n - min(n * strength, n), 0))
    return t_start, n - t_start


def mask_pack(mask_u8, mode=0, grow=0, C=64):
    """mask_u8 uint8 [B, H, W] -> bf16 [B, (H/16)(W/16), C]; mode 0 nearest, 1 cover with `grow` latent pixels"""
    B, H, W = mask_u8.shape
    h, w = H // 8, W // 8
    on = mask_u8 >= 128
    if mode == 0:
        assert grow == 0
        lat = on[:, ::8, ::8]
    else:
        blocks = on.view(B, h, 8, w, 8).any(dim=4).any(dim=2)
        lat = torch.zeros_like(blocks)
        for ly in range(h):
            for lx in range(w):
                lat[:, ly, lx] = blocks[:, max(ly - grow, 0):ly + grow + 1, max(lx - grow, 0):lx + grow + 1].flatten(1).any(dim=1)
    lat = lat.to(BF)                                                   # [B, h, w]
    out = torch.empty(B, (h // 2) * (w // 2), C, dtype=BF)
    for ty in range(h // 2):
        for tx in range(w // 2):
            for py in range(2):
                for px in range(2):
                    out[:, ty * (w // 2) + tx, py * 2 + px::4] = lat[:, 2 * ty + py, 2 * tx + px, None]
    return out


def loop(pipe, latents, masked_image_latents, prompt_embeds, pooled_prompt_embeds, grid, x0, noise, mask, sampler="euler",
         guidance_scale=30.0, amo_noise=None, per_step=None):
    """The engine's loop with the blend, issued from Python (GPU): per step ses.run -> the sampler's op -> ops.known_region_blend.
    Call after a pipeline call: pipe.scheduler then holds the call's timesteps, begin_index and tables.  sampler: "euler" (the
    unfused kernel), "fused" (the update in proj_out's epilogue, the blend on xin's columns), "amo", "multistep".  mask None: no
    blend (a strength-only call).  Returns the final latents; per_step receives a clone after every step."""
    from tests.helpers.plain_loop import mod_table
    from textflux_amd import ops
    tr, sch = pipe.transformer, pipe.scheduler
    B, S, C = latents.shape
    T = prompt_embeds.shape[1]
    begin = sch.begin_index or 0
    timesteps = sch.timesteps[begin:]
    n = len(timesteps)
    ses = tr.session(B, S, T)
    ses.set_conditioning(prompt_embeds.to("cuda", BF), torch.zeros(T, 3), pipe._prepare_latent_image_ids(B, *grid, "cuda", BF))
    coef = sch.coef_table("cuda", BF)
    assert coef.shape[0] == n
    sig = keep_sigma(sch._sigmas_host, begin).cuda()
    mod = mod_table(pipe, timesteps, B, pooled_prompt_embeds, guidance_scale, coef[:n] if sampler == "fused" else None)
    lat = latents.to("cuda", BF).contiguous().clone()
    hist = torch.full_like(lat, float("nan"))
    ops.scatter_cols_(lat, ses.xin, 0)
    ops.scatter_cols_(masked_image_latents.to("cuda", BF).contiguous(), ses.xin, C)
    for i in range(n):
        if sampler == "fused":
            ses.run(mod[i], euler=True)
            if mask is not None:
                ops.known_region_blend(ses.xin[:, :, :C], x0, noise, mask, sig, step=i)
            lat = ses.xin[:, :, :C].clone()
        else:
            v = ses.run(mod[i])
            if sampler == "amo":
                ops.amo_step_(v, lat, coef, amo_noise[i].to("cuda", torch.float32).contiguous(), step=i, xin=ses.xin)
            elif sampler == "multistep":
                ops.multistep_step_(v, lat, coef, hist, step=i, xin=ses.xin)
            else:
                ops.euler_step_(v, lat, coef, step=i, xin=ses.xin)
            if mask is not None:
                ops.known_region_blend(lat, x0, noise, mask, sig, step=i, xin=ses.xin)
        if per_step is not None:
            per_step.append(lat.clone())
    return lat
