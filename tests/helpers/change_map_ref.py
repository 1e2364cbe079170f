"""numpy / torch-CPU restatement of change-map sampling (include/textflux_hip.h: tfx_change_map_pack, tfx_change_map_blend; DESIGN.md
section 4 "Change-map sampling"), written from the specification with no code shared with the package: every op in fp32 on bf16
operands, rounded to bf16 on its own.

    hold(map)             = 255 - g, g the map at every 8th pixel (nearest) or its maximum over the latent pixel's neighbourhood (cover)
    cut(n)[i]             = the largest byte q with NOT bf16(q / 255) > (arange(n, dtype=bf16) / n)[i]       ("free": cut[n - 1] = 255)
    k                     = hold[row, col & 3] > cut[i] ? 1 : 0
    blend(x, p, k)        = bf16( bf16(p k) + bf16( x bf16(1 - k) ) )        p = scale_noise(x0, s, noise), s < 0: x0 itself
                            cut[i] >= 255: x stays as it is, bit for bit

tests/golden/g17_change_map.safetensors holds what the reference computes for the same inputs (tests/test_change_map_cpu.py compares).
`loop` is the GPU side: the pipeline's denoising loop issued from Python, one forward, one sampler op and one blend per step."""
import torch

BF = torch.bfloat16


def _r(t):
    """fp32 -> the nearest bf16 value (ties to even), as fp32"""
    return t.to(BF).float()


def scale_noise(x0, sigma, noise):
    s = _r(torch.tensor(float(sigma), dtype=torch.float32))
    if float(s) < 0:
        return x0.clone()
    a = _r(s * noise.float())
    u = _r(1.0 - s)
    b = _r(u * x0.float())
    return (a + b).to(BF)


def cut_table(n, last="keep"):
    """int32 [n].  The two sides of the reference's comparison, evaluated with its own expressions; cut is read off, not derived."""
    thr = torch.arange(n, dtype=BF) / n
    lev = (torch.arange(256, dtype=torch.float32) / 255).to(BF)
    cut = []
    for i in range(n):
        held = [bool(lev[q] > thr[i]) for q in range(256)]
        free = [q for q in range(256) if not held[q]]
        c = max(free) if free else -1
        assert all(held[q] == (q > c) for q in range(256)), (n, i)
        cut.append(c)
    if last == "free":
        cut[-1] = 255
    else:
        assert last == "keep"
    return torch.tensor(cut, dtype=torch.int32)


def hold_mask(hold, cut_i, C=64):
    """hold uint8 [.., 4], one cut entry -> k as bf16 [.., C]: column c reads byte c & 3"""
    k = (hold.to(torch.int32) > int(cut_i)).to(BF)
    return k.repeat(*([1] * (hold.dim() - 1)), C // 4)


def blend(x, x0, noise, hold, cut_i, sigma):
    """the whole kernel for one step: x bf16 [.., C], hold uint8 [.., 4]"""
    if int(cut_i) >= 255:
        return x.clone()
    p = scale_noise(x0, sigma, noise).float()
    k = hold_mask(hold, cut_i, x.shape[-1]).float()
    e = _r(p * k)
    w = _r(1.0 - k)
    d = _r(x.float() * w)
    return (e + d).to(BF)


def keep_sigma(sigmas, begin=0):
    """sigmas fp32 [n + 1] (closing 0 included) -> fp32 [n - begin]: bf16(sigma_{i+1}), the last entry -1 = the original itself"""
    s = torch.as_tensor(sigmas, dtype=torch.float32)[begin:]
    tab = _r(s[1:].clone())
    tab[-1] = -1.0
    return tab


def run_blends(step_latents, x0, noise, hold, sigmas, begin=0, last="keep"):
    """the whole loop's blends on the CPU: step_latents[i] = the latents behind step i's sampler update -> what each step leaves"""
    n = len(step_latents)
    sig, cut = keep_sigma(sigmas, begin), cut_table(n, last)
    assert sig.numel() == n
    return [blend(step_latents[i], x0, noise, hold, cut[i], sig[i]) for i in range(n)]


def pack(map_u8, mode=0, grow=0):
    """map uint8 [B, H, W] -> hold uint8 [B, (H/16)(W/16), 4]; mode 0 nearest, 1 cover (maximum) with `grow` latent pixels"""
    B, H, W = map_u8.shape
    h, w = H // 8, W // 8
    m = map_u8.to(torch.int32)
    if mode == 0:
        assert grow == 0
        g = m[:, ::8, ::8]
    else:
        blocks = m.view(B, h, 8, w, 8).amax(dim=4).amax(dim=2)
        g = torch.zeros_like(blocks)
        for ly in range(h):
            for lx in range(w):
                g[:, ly, lx] = blocks[:, max(ly - grow, 0):ly + grow + 1, max(lx - grow, 0):lx + grow + 1].flatten(1).amax(dim=1)
    out = torch.empty(B, (h // 2) * (w // 2), 4, dtype=torch.uint8)
    for ty in range(h // 2):
        for tx in range(w // 2):
            for py in range(2):
                for px in range(2):
                    out[:, ty * (w // 2) + tx, py * 2 + px] = (255 - g[:, 2 * ty + py, 2 * tx + px]).to(torch.uint8)
    return out


def loop(pipe, latents, masked_image_latents, prompt_embeds, pooled_prompt_embeds, grid, x0, noise, hold, last="keep", sampler="euler",
         guidance_scale=30.0, amo_noise=None, per_step=None):
    """The engine's loop with the change-map blend, issued from Python (GPU): per step ses.run -> the sampler's op ->
    ops.change_map_blend.  Call after a pipeline call: pipe.scheduler then holds the call's timesteps, begin_index and tables.
    sampler: "euler" (the unfused kernel), "fused" (the update in proj_out's epilogue, the blend on xin's columns), "amo",
    "multistep".  Returns the final latents; per_step receives a clone after every step."""
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
    cut = cut_table(n, last).cuda()
    hold = hold.cuda().contiguous()
    mod = mod_table(pipe, timesteps, B, pooled_prompt_embeds, guidance_scale, coef[:n] if sampler == "fused" else None)
    lat = latents.to("cuda", BF).contiguous().clone()
    hist = torch.full_like(lat, float("nan"))
    ops.scatter_cols_(lat, ses.xin, 0)
    ops.scatter_cols_(masked_image_latents.to("cuda", BF).contiguous(), ses.xin, C)
    for i in range(n):
        if sampler == "fused":
            ses.run(mod[i], euler=True)
            ops.change_map_blend(ses.xin[:, :, :C], x0, noise, hold, cut, sig, step=i)
            lat = ses.xin[:, :, :C].clone()
        else:
            v = ses.run(mod[i])
            if sampler == "amo":
                ops.amo_step_(v, lat, coef, amo_noise[i].to("cuda", torch.float32).contiguous(), step=i, xin=ses.xin)
            elif sampler == "multistep":
                ops.multistep_step_(v, lat, coef, hist, step=i, xin=ses.xin)
            else:
                ops.euler_step_(v, lat, coef, step=i, xin=ses.xin)
            ops.change_map_blend(lat, x0, noise, hold, cut, sig, step=i, xin=ses.xin)
        if per_step is not None:
            per_step.append(lat.clone())
    return lat
