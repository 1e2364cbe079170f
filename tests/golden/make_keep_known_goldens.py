#!/usr/bin/env python3
"""Generate tests/golden/g16_keep_known.safetensors by IMPORTING the reference (as make_goldens.py does; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_keep_known_goldens.py

What known-region sampling is pinned to, all on torch-CPU bf16 tensors, data only:
  * FlowMatchEulerDiscreteScheduler.scale_noise and the blend line of FluxInpaintPipeline's loop
    (pipeline_flux_inpaint.py:974-984) on [2, 6, 64] tensors, a 5-step shifted grid with the mu of a 96-token image,
    set_begin_index 0 and 2, every step including the last, one binary and one soft mask (values 0, 0.25, 0.5, 1);
  * FluxInpaintPipeline.get_timesteps for n in {1, 4, 30} x strength in {0, 0.01, 0.3, 0.5, 0.6, 1};
  * _pack_latents(F.interpolate(mask).repeat(1, 16, 1, 1)) (prepare_mask_latents :615, :656-662) for a 32 x 48 mask whose
    edges are not multiples of 8.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference/diffusers/src")
sys.dont_write_bytecode = True

import numpy as np
import torch
import transformers.utils as tu

tu.FLAX_WEIGHTS_NAME = "flax_model.msgpack"  # removed in transformers 5.x; the reference imports it

from safetensors.torch import save_file

import diffusers  # the reference, 0.32.0.dev0
from diffusers import FlowMatchEulerDiscreteScheduler
from diffusers.pipelines.flux.pipeline_flux_inpaint import FluxInpaintPipeline, calculate_shift

OUT = os.path.dirname(os.path.abspath(__file__))
assert diffusers.__version__ == "0.32.0.dev0"
torch.set_grad_enabled(False)
BF = torch.bfloat16
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
N, TOKENS, SHAPE = 5, 96, (2, 6, 64)
STRENGTH_N, STRENGTHS = (1, 4, 30), (0.0, 0.01, 0.3, 0.5, 0.6, 1.0)


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


def scheduler(n=N):
    s = FlowMatchEulerDiscreteScheduler(**SCHED)
    mu = calculate_shift(TOKENS, s.config.base_image_seq_len, s.config.max_image_seq_len, s.config.base_shift, s.config.max_shift)
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cpu", mu=mu)
    return s, mu


class _Pipe:
    """get_timesteps reads self.scheduler only"""
    get_timesteps = FluxInpaintPipeline.get_timesteps


def main():
    out = {}
    x0, noise = rnd(SHAPE, 1), rnd(SHAPE, 2)
    x0.view(-1)[:4] = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=BF)        # signed zeros where the last step copies x0
    noise.view(-1)[:4] = torch.tensor([0.0, 0.0, -0.0, -0.0], dtype=BF)
    g = torch.Generator().manual_seed(3)
    binary = (torch.rand(SHAPE, generator=g) < 0.5).to(BF)
    soft = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, SHAPE, generator=g)].to(BF)
    out.update(x0=x0, noise=noise, mask_binary=binary, mask_soft=soft)
    sch, mu = scheduler()
    out["mu"] = torch.tensor([mu], dtype=torch.float64)
    out["sigmas"] = sch.sigmas.clone()
    out["timesteps"] = sch.timesteps.clone()
    for begin in (0, 2):
        sch, _ = scheduler()
        sch.set_begin_index(begin)
        timesteps = sch.timesteps[begin:]
        # img2img start: before the first step scale_noise reads sigmas[begin_index]
        out[f"b{begin}_start"] = sch.scale_noise(x0, timesteps[:1].repeat(SHAPE[0]), noise)
        for i, t in enumerate(timesteps):
            lat = rnd(SHAPE, 10 + i)
            v = rnd(SHAPE, 20 + i, 0.5)
            lat = sch.step(v, t, lat, return_dict=False)[0]               # moves step_index on, as the loop does
            proper = x0
            if i < len(timesteps) - 1:
                proper = sch.scale_noise(proper, torch.tensor([timesteps[i + 1]]), noise)
            out[f"b{begin}_s{i}_latents"] = lat
            out[f"b{begin}_s{i}_proper"] = proper.clone()
            for name, m in (("binary", binary), ("soft", soft)):
                out[f"b{begin}_s{i}_blend_{name}"] = (1 - m) * proper + m * lat          # :984
    rows = []
    for n in STRENGTH_N:
        for st in STRENGTHS:
            p = _Pipe()
            p.scheduler, _ = scheduler(n)
            ts, steps = p.get_timesteps(n, st, "cpu")
            assert len(ts) == steps or steps == 0
            rows.append([n, int(round(st * 100)), p.scheduler.begin_index, steps])
    out["get_timesteps"] = torch.tensor(rows, dtype=torch.int32)                      # (n, 100 strength, t_start, steps)
    # the latent mask: a 32 x 48 pixel mask [1, 1, H, W] of 0 / 1 whose rectangle's edges are not multiples of 8
    H, W = 32, 48
    pix = torch.zeros(1, 1, H, W)
    pix[:, :, 5:19, 11:37] = 1.0
    pix[:, :, 24, 40] = 1.0                                                            # a lone pixel ON the sampling lattice
    pix[:, :, 25, 1] = 1.0                                                             # and one off it
    small = torch.nn.functional.interpolate(pix, size=(H // 8, W // 8)).to(BF)
    packed = FluxInpaintPipeline._pack_latents(small.repeat(1, 16, 1, 1), 1, 16, H // 8, W // 8)
    out["mask_pixels_u8"] = (pix[0, 0] * 255).to(torch.uint8)
    out["mask_packed"] = packed
    out = {k: v.contiguous() for k, v in out.items()}
    path = os.path.join(OUT, "g16_keep_known.safetensors")
    save_file(out, path)
    print(f"g16_keep_known: {len(out)} tensors, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
