"""What change-map sampling (FluxFillPipeline.__call__: change_map) costs beside the plain call and beside keep_known,
measured on whole pipeline calls of a random-init full-depth model (latents out: no text encoders, no VAE decode) at the headline geometry
(1024 x 1024, batch 8), step graphs, calls of 4 steps, arms alternating call by call in ONE process, device events, median of 20 calls
per arm:

    plain           fused Euler, the default call (masked_image_latents and latents given)
    keep            the same with keep_known=True and image_latents given: tfx_known_region_blend behind every step's fused update,
                    plus one tfx_keep_mask_pack per call
    change          the same with change_map=dict(dilate, feather) and image_latents given: tfx_change_map_blend behind every step's
                    fused update, plus the dilate, the feather and one tfx_change_map_pack per call

The forward is the same in all arms.  From bytes the change-map blend reads 4 B of hold bytes per token where keep_known reads 128 B of
mask, beside a ~440 ms step: an expectation; this tool is the measurement.  It measures COST only: the latents of random weights say
nothing about image quality, and no dilate, feather, mode, grow or last is recommended here.

    python tools/change_map_cost.py [--iters 20] [--warmup 2] [--steps 4] [--out profiles/change_map_cost.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textflux_amd.pipeline import FluxFillPipeline
from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
from textflux_amd.transformer import FluxTransformer2DModel
from textflux_amd.vae import AutoencoderKL

BF = torch.bfloat16
ARMS = ("plain", "keep", "change")
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
T_TXT = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="timed calls per arm")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--layers", default="19,38", help="double,single blocks (full depth by default)")
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--dilate", type=int, default=16)
    ap.add_argument("--feather", type=int, default=4)
    ap.add_argument("--eager", action="store_true", help="the eager step loop instead of captured step graphs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    nd, ns = (int(v) for v in a.layers.split(","))
    tr = FluxTransformer2DModel(in_channels=384, out_channels=64, num_layers=nd, num_single_layers=ns, num_attention_heads=a.heads,
                                guidance_embeds=True)
    tr.init_random_(seed=1, device=dev)
    vae = AutoencoderKL(sample_size=1024).init_random_(seed=2, device=dev)      # the pipeline's geometry constants; never run here
    pipe = FluxFillPipeline(scheduler=FlowMatchEulerDiscreteScheduler(**SCHED), vae=vae, text_encoder=None, tokenizer=None,
                            text_encoder_2=None, tokenizer_2=None, transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_graph(not a.eager)
    B, H, W = a.batch, a.size, a.size
    S = (H // 16) * (W // 16)
    g = torch.Generator().manual_seed(0)
    mask = torch.zeros(B, H, W, dtype=torch.uint8)
    mask[:, H // 4: H // 2, W // 8: 7 * W // 8] = 255
    common = dict(masked_image_latents=torch.cat([torch.randn(B, S, 64, generator=g), (torch.randn(B, S, 256, generator=g) > 0).float()], -1).to(BF).to(dev),
                  prompt_embeds=(torch.randn(B, T_TXT, tr.config.joint_attention_dim, generator=g) * 0.1).to(BF).to(dev),
                  pooled_prompt_embeds=torch.randn(B, tr.config.pooled_projection_dim, generator=g).to(BF).to(dev),
                  latents=torch.randn(B, S, 64, generator=g).to(BF).to(dev), height=H, width=W, guidance_scale=30.0, output_type="latent",
                  num_inference_steps=a.steps)
    x0 = torch.randn(B, S, 64, generator=g).to(BF).to(dev)
    mask_dev = mask.to(dev)
    cm = dict(dilate=a.dilate, feather=a.feather)
    kw = {"plain": common,
          "keep": dict(common, keep_known=True, image_latents=x0, mask_image=mask_dev),
          "change": dict(common, change_map=cm, image_latents=x0, mask_image=mask_dev)}

    def run(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipe(**kw[name]).images
        e1.record()
        e1.synchronize()
        ms_ = e0.elapsed_time(e1)
        print(f"  {name}: {ms_:.1f} ms", file=sys.stderr, flush=True)
        return ms_, out

    outs = {}
    for _ in range(a.warmup):
        for name in ARMS:
            outs[name] = run(name)[1]
    ms = {name: [] for name in ARMS}
    for _ in range(a.iters):                         # alternating: drift of the board (clock, temperature) hits every arm alike
        for name in ARMS:
            ms[name].append(run(name)[0])
    med = lambda v: sorted(v)[len(v) // 2]
    call = {n: med(v) for n, v in ms.items()}
    from textflux_amd import ops
    from textflux_amd.paste_back import alpha_mask
    hold = ops.change_map_pack(alpha_mask(mask_dev, a.dilate, a.feather), "nearest", 0)
    never = (hold == 255)[:, :, :, None].expand(B, S, 4, 16).transpose(2, 3).reshape(B, S, 64)      # column c reads byte c & 3
    res = {"layers": [nd, ns], "heads": a.heads, "steps": a.steps, "iters": a.iters, "warmup": a.warmup,
           "batch": B, "height": H, "width": W, "image_tokens": S, "loop": "eager" if a.eager else "graph",
           "device": torch.cuda.get_device_name(0), "weights": "random-init", "change_map": cm,
           "ms_per_call": {n: {"median": call[n], "min": min(v), "max": max(v)} for n, v in ms.items()},
           "ms_per_step": {n: call[n] / a.steps for n in ARMS},
           "change_minus_plain_ms_per_step": (call["change"] - call["plain"]) / a.steps,
           "change_minus_keep_ms_per_step": (call["change"] - call["keep"]) / a.steps,
           "keep_minus_plain_ms_per_step": (call["keep"] - call["plain"]) / a.steps,
           "spread_of_one_arm_ms_per_step": max((max(ms[n]) - min(ms[n])) / a.steps for n in ARMS),
           "blend_side_input_bytes_per_token": {"keep": 128, "change": 4},
           "hold_bytes_distinct": int(hold.unique().numel()),
           "never_released_equal_image_latents": bool(torch.equal(outs["change"][never], x0[never])),
           "change_latents_differ_from_plain": not bool(torch.equal(outs["change"], outs["plain"])),
           "change_latents_differ_from_keep": not bool(torch.equal(outs["change"], outs["keep"]))}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
