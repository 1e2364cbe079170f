#!/usr/bin/env python3
"""Generate tests/golden/g17_change_map.safetensors by IMPORTING the reference (as make_keep_known_goldens.py does; build container
only); the community pipeline file is loaded by path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_change_map_goldens.py

What change-map sampling is pinned to, all from the reference's own code on torch-CPU bf16 tensors, data only
(FluxDifferentialImg2ImgPipeline, examples/community/pipeline_flux_differential_img2img.py):
  * mask_processor.preprocess -> prepare_mask_latents (:918-934) for a 32 x 48 grey map with a ramp and lone pixels on and off the
    sampling lattice, and for a 128 x 128 map that carries every byte 0..255 once on the lattice;
  * masks = original_mask > mask_thresholds (:936-938) of both for n in {1, 3, 5, 30}, and for n = 4 after strength 0.5 (:892);
  * the loop body :972-985 on [2, 6, 64] tensors over a 5-step shifted grid, set_begin_index 0 and 2, every step including the last,
    signed zeros planted in x0, noise and the latents, mask bytes on both sides of the bf16 ties (85 / 86 at n = 3, 51 / 52 at n = 5).
The reference HOLDS where its mask is high: its mask byte is the hold byte, 255 - our change map."""
import importlib.util
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference/diffusers/src")
sys.dont_write_bytecode = True

import numpy as np
import PIL.Image
import torch
import transformers.utils as tu

tu.FLAX_WEIGHTS_NAME = "flax_model.msgpack"  # removed in transformers 5.x; the reference imports it

from safetensors.torch import save_file

import diffusers  # the reference, 0.32.0.dev0
from diffusers import FlowMatchEulerDiscreteScheduler
from diffusers.image_processor import VaeImageProcessor

spec = importlib.util.spec_from_file_location(
    "pipeline_flux_differential_img2img", "/root/reference/diffusers/examples/community/pipeline_flux_differential_img2img.py")
community = importlib.util.module_from_spec(spec)
spec.loader.exec_module(community)
Pipe, calculate_shift = community.FluxDifferentialImg2ImgPipeline, community.calculate_shift

OUT = os.path.dirname(os.path.abspath(__file__))
assert diffusers.__version__ == "0.32.0.dev0"
torch.set_grad_enabled(False)
BF = torch.bfloat16
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
N, TOKENS, SHAPE = 5, 96, (2, 6, 64)
MASK_N = (1, 3, 5, 30)


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


def scheduler(n=N):
    s = FlowMatchEulerDiscreteScheduler(**SCHED)
    mu = calculate_shift(TOKENS, s.config.base_image_seq_len, s.config.max_image_seq_len, s.config.base_shift, s.config.max_shift)
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cpu", mu=mu)
    return s, mu


class _Stub:
    """what prepare_mask_latents and get_timesteps read of the pipeline: the scale factor and mask processor of its __init__ (:224-234),
    the VAE's two constants (used on the masked image, which is given as 16-channel latents here and not recorded), the scheduler"""
    vae_scale_factor = 16
    vae = types.SimpleNamespace(config=types.SimpleNamespace(shift_factor=0.1159, scaling_factor=0.3611))
    mask_processor = VaeImageProcessor(vae_scale_factor=16, vae_latent_channels=16, do_normalize=False, do_binarize=False,
                                       do_convert_grayscale=True)
    _pack_latents = staticmethod(Pipe._pack_latents)
    prepare_mask_latents = Pipe.prepare_mask_latents
    get_timesteps = Pipe.get_timesteps


def original_mask(hold_u8):
    """the reference's :918-934 for a grey PIL image of its mask bytes [H, W] -> packed [1, (H/16)(W/16), 64] bf16"""
    H, W = hold_u8.shape
    p = _Stub()
    m = p.mask_processor.preprocess(PIL.Image.fromarray(hold_u8.numpy(), mode="L"), height=H, width=W, resize_mode="default", crops_coords=None)
    packed, _ = p.prepare_mask_latents(m, torch.zeros(1, 16, H // 8, W // 8), 1, 16, 1, H, W, BF, "cpu", None)
    return packed


def masks_of(om, n):
    thresholds = torch.arange(n, dtype=om.dtype) / n                                  # :936
    thresholds = thresholds.reshape(-1, 1, 1, 1).to("cpu")                            # :937
    return om > thresholds                                                             # :938  [n, B, S, 64]


def main():
    out = {}
    # ---- the 32 x 48 map, in OUR polarity (255 = free); the reference sees 255 - map
    H, W = 32, 48
    cmap = torch.zeros(H, W, dtype=torch.uint8)
    cmap[:, :] = (torch.arange(W) * 255 // (W - 1)).to(torch.uint8)[None, :]          # a ramp over the width
    cmap[8:24, 0:8] = 170                                                              # 255 - 85: the n = 3 tie
    cmap[8:24, 8:16] = 169                                                             # 255 - 86
    cmap[24, 40] = 0                                                                   # a lone pixel ON the sampling lattice
    cmap[25, 1] = 255                                                                  # and one off it
    cmap[7, 23] = 255                                                                  # off the lattice, seen only by cover
    out["map_u8"] = cmap
    om = original_mask(255 - cmap)
    out["map_original_mask"] = om
    # ---- every byte once on the lattice: 128 x 128 -> 16 x 16 latent pixels, latent pixel (ly, lx) holds byte 16 ly + lx
    q = torch.zeros(128, 128, dtype=torch.uint8)
    q[::8, ::8] = torch.arange(256, dtype=torch.uint8).view(16, 16)
    q[1::8, 1::8] = 255                                                                # off the lattice: nearest must not see it
    om256 = original_mask(q)
    out["bytes_hold_u8"] = q
    out["bytes_original_mask4"] = om256[:, :, :4].contiguous()                        # channel 0's four patch positions
    runs = [(str(n), n) for n in MASK_N]
    p = _Stub()
    p.scheduler, _ = scheduler(4)
    _, n_run = p.get_timesteps(4, 0.5, "cpu")                                          # :892
    assert n_run == 2
    runs.append(("4s50", n_run))
    for name, n in runs:
        out[f"map_masks_n{name}"] = masks_of(om, n)[:, 0].to(torch.uint8)              # [n, 6, 64]
        out[f"bytes_masks_n{name}"] = masks_of(om256, n)[:, 0, :, :4].to(torch.uint8)  # [n, 64, 4]
    # ---- the loop body on [2, 6, 64]
    x0, noise = rnd(SHAPE, 1), rnd(SHAPE, 2)
    g = torch.Generator().manual_seed(3)
    hold = torch.randint(0, 256, (2, 6, 4), generator=g).to(torch.uint8)
    hold[0, 0] = torch.tensor([255, 255, 0, 0], dtype=torch.uint8)                     # columns 0..15: held where c & 2
    hold[0, 1] = torch.tensor([85, 86, 84, 170], dtype=torch.uint8)                    # both sides of the n = 3 ties
    hold[0, 2] = torch.tensor([171, 169, 51, 52], dtype=torch.uint8)                   # ... and of n = 5's first
    hold[1, 0] = torch.tensor([102, 103, 153, 154], dtype=torch.uint8)
    hold[1, 1] = torch.tensor([204, 205, 0, 1], dtype=torch.uint8)
    zsign = lambda bit: torch.tensor([-0.0 if c & bit else 0.0 for c in range(16)], dtype=BF)
    x0[0, 0, :16] = zsign(4)                                                           # signed zeros: every combination of held (c & 2),
    noise[0, 0, :16] = zsign(8)                                                        # latent sign (c & 1), x0 sign and noise sign
    om_loop = (hold.float() / 255).to(BF).repeat(1, 1, 16)                             # what preprocess -> prepare_mask_latents make of it
    assert torch.equal(om_loop[0, 0, :4], (torch.tensor([255, 255, 0, 0]).float() / 255).to(BF))
    out.update(x0=x0, noise=noise, loop_hold_u8=hold, loop_original_mask=om_loop)
    sch, mu = scheduler()
    out["mu"] = torch.tensor([mu], dtype=torch.float64)
    out["sigmas"] = sch.sigmas.clone()
    out["timesteps"] = sch.timesteps.clone()
    for begin in (0, 2):
        sch, _ = scheduler()
        sch.set_begin_index(begin)
        timesteps = sch.timesteps[begin:]
        num_inference_steps = len(timesteps)
        masks = masks_of(om_loop, num_inference_steps)                                 # [n, 2, 6, 64], as the reference's
        for i, t in enumerate(timesteps):
            latents = rnd(SHAPE, 10 + i)
            noise_pred = rnd(SHAPE, 20 + i, 0.5)
            latents_dtype = latents.dtype
            latents = sch.step(noise_pred, t, latents, return_dict=False)[0]          # :972
            latents[0, 0, :16] = zsign(1)
            out[f"b{begin}_s{i}_latents"] = latents.clone()
            image_latent = x0                                                          # :975
            if i < len(timesteps) - 1:                                                 # :977
                noise_timestep = timesteps[i + 1]
                image_latent = sch.scale_noise(x0, torch.tensor([noise_timestep]), noise)
                mask = masks[i].to(latents_dtype)                                      # :984
                latents = image_latent * mask + latents * (1 - mask)                   # :985
            out[f"b{begin}_s{i}_out"] = latents.clone()
            out[f"b{begin}_s{i}_image_latent"] = image_latent.clone()
    out = {k: v.contiguous() for k, v in out.items()}
    path = os.path.join(OUT, "g17_change_map.safetensors")
    save_file(out, path)
    print(f"g17_change_map: {len(out)} tensors, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
