"""What true CFG (FluxFillPipeline.__call__: negative_prompt_embeds, true_cfg) costs beside the plain call, measured on
whole pipeline calls of a random-init full-depth model (latents out: no text encoders, no VAE) with step graphs, arms alternating call by
call in ONE process, device events, median of 20 calls per arm, at the headline geometry (1024 x 1024, batch 8) and at the reference's
own entry point (576 x 512, batch 1):

    plain_B     unfused Euler at batch B (the sampler a CFG call runs; the default call fuses the update into proj_out)
    cfg_B       the same call with negative embeds and true_cfg = 3.3: one forward on 2B, tfx_cfg_combine, the update on B
    plain_2B    unfused Euler at batch 2B                                          -> what the doubled forward alone costs

The expectation, which this tool exists to replace by a measurement: cfg_B = plain_2B + one pass over the model output (4 MB at the
headline geometry), and at batch 1 less than twice plain_B because batch 2 fills the chip better.  It measures COST only: the latents of
random weights say nothing about image quality, and no true_cfg is recommended here.  No threshold is set.

Sessions are kept per transformer object, so the B and the 2B arms run on two objects that share one set of weights.

    python tools/true_cfg_cost.py [--iters 20] [--warmup 2] [--steps 4] [--out profiles/true_cfg_cost.json]"""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textflux_amd.pipeline import FluxFillPipeline
from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
from textflux_amd.transformer import FluxTransformer2DModel

BF = torch.bfloat16
ARMS = ("plain_B", "cfg_B", "plain_2B")
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
T_TXT = 512


class _VaeCfg:       # output_type "latent" with masked_image_latents given: only the VAE's config is consulted
    class config:
        block_out_channels = (128, 256, 512, 512)
        latent_channels = 16
        scaling_factor, shift_factor = 0.3611, 0.1159


def make_pipe(tr, eager):
    pipe = FluxFillPipeline(scheduler=FlowMatchEulerDiscreteScheduler(**SCHED), vae=_VaeCfg(), text_encoder=None, tokenizer=None,
                            text_encoder_2=None, tokenizer_2=None, transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_graph(not eager)
    pipe.fuse_euler_step = False
    return pipe


def measure(tr, B, H, W, a):
    """the three arms at one geometry -> the result dict"""
    dev = tr.device
    tr2 = copy.copy(tr)                                  # the same weights, a session of its own
    tr._session = tr2._session = None
    pipes = {"plain_B": make_pipe(tr, a.eager), "cfg_B": make_pipe(tr2, a.eager), "plain_2B": make_pipe(tr2, a.eager)}
    S = (H // 16) * (W // 16)
    g = torch.Generator().manual_seed(0)
    c = tr.config

    def call_kw(n):
        return dict(masked_image_latents=torch.cat([torch.randn(n, S, 64, generator=g), (torch.randn(n, S, 256, generator=g) > 0).float()], -1).to(BF).to(dev),
                    prompt_embeds=(torch.randn(n, T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF).to(dev),
                    pooled_prompt_embeds=torch.randn(n, c.pooled_projection_dim, generator=g).to(BF).to(dev),
                    latents=torch.randn(n, S, 64, generator=g).to(BF).to(dev), height=H, width=W, guidance_scale=30.0, output_type="latent",
                    num_inference_steps=a.steps)

    one, two = call_kw(B), call_kw(2 * B)
    neg = dict(negative_prompt_embeds=(torch.randn(B, T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF).to(dev),
               negative_pooled_prompt_embeds=torch.randn(B, c.pooled_projection_dim, generator=g).to(BF).to(dev), true_cfg=3.3)
    kw = {"plain_B": one, "cfg_B": dict(one, **neg), "plain_2B": two}

    def run(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipes[name](**kw[name]).images
        e1.record()
        e1.synchronize()
        ms_ = e0.elapsed_time(e1)
        print(f"  {H}x{W} {name}: {ms_:.1f} ms", file=sys.stderr, flush=True)
        return ms_, out

    outs = {}
    for _ in range(a.warmup):
        for name in ARMS:
            outs[name] = run(name)[1]
    ms = {name: [] for name in ARMS}
    for _ in range(a.iters):                             # alternating: drift of the board (clock, temperature) hits every arm alike
        for name in ARMS:
            ms[name].append(run(name)[0])
    med = lambda v: sorted(v)[len(v) // 2]
    step = {n: med(v) / a.steps for n, v in ms.items()}
    return {"batch": B, "height": H, "width": W, "image_tokens": S, "sessions": {"plain_B": B, "cfg_B": 2 * B, "plain_2B": 2 * B},
            "ms_per_call": {n: {"median": med(v), "min": min(v), "max": max(v)} for n, v in ms.items()},
            "ms_per_step": step,
            "cfg_over_plain_B": step["cfg_B"] / step["plain_B"],
            "cfg_minus_plain_2B_ms_per_step": step["cfg_B"] - step["plain_2B"],
            "spread_of_one_arm_ms_per_step": max((max(v) - min(v)) / a.steps for v in ms.values()),
            "model_output_bytes": B * S * 64 * 2,
            "cfg_latents_differ_from_plain": not bool(torch.equal(outs["cfg_B"], outs["plain_B"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="timed calls per arm")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--geometries", default="8x1024x1024,1x576x512", help="comma-separated BxHxW; every one runs at B and 2B")
    ap.add_argument("--layers", default="19,38", help="double,single blocks (full depth by default)")
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--eager", action="store_true", help="the eager step loop instead of captured step graphs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    nd, ns = (int(v) for v in a.layers.split(","))
    tr = FluxTransformer2DModel(in_channels=384, out_channels=64, num_layers=nd, num_single_layers=ns, num_attention_heads=a.heads,
                                guidance_embeds=True)
    tr.init_random_(seed=1, device=dev)
    res = {"layers": [nd, ns], "heads": a.heads, "steps": a.steps, "iters": a.iters, "warmup": a.warmup, "true_cfg": 3.3,
           "loop": "eager" if a.eager else "graph", "sampler": "euler, unfused (all arms)", "device": torch.cuda.get_device_name(0),
           "weights": "random-init", "geometries": []}
    for spec in a.geometries.split(","):
        B, H, W = (int(v) for v in spec.split("x"))
        res["geometries"].append(measure(tr, B, H, W, a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
