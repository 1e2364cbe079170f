"""What the second-order multistep sampler (FlowMatchMultistepScheduler) costs per step beside the Euler forms, measured on whole
pipeline calls of a random-init full-depth model (latents in, latents out: no text encoders, no VAE) at the headline geometry
(1024 x 1024, batch 8), arms alternating call by call in ONE process, device events, median of 20 calls per arm:

    euler_fused     the default: the Euler update in proj_out's epilogue
    euler_unfused   fuse_euler_step = False: proj_out stores the model output, the scheduler kernel updates the latents
    multistep       unfused as well: tfx_multistep_step reads the model output and the history, writes the latents, xin and the history

The forward is the same in all three; what differs is one launch and a few passes over [B, S, 64] bf16 per step.  The calls are
short (--steps 4) so that twenty of each fit into a few minutes; the per-step difference does not depend on the number of steps.
This measures COST only: the latents of random weights say nothing about image quality, and no step count is recommended here.

    python tools/multistep_cost.py [--iters 20] [--warmup 2] [--steps 4] [--layers 19,38] [--out profiles/multistep_cost.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textflux_amd.pipeline import FluxFillPipeline
from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
from textflux_amd.transformer import FluxTransformer2DModel

BF = torch.bfloat16
ARMS = ("euler_fused", "euler_unfused", "multistep")
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
T_TXT = 512


class _VaeCfg:       # output_type "latent" with injected masked_image_latents: only the VAE's config is consulted
    class config:
        block_out_channels = (128, 256, 512, 512)
        latent_channels = 16
        scaling_factor, shift_factor = 0.3611, 0.1159


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="timed calls per arm")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
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
    euler = FlowMatchEulerDiscreteScheduler(**SCHED)
    scheds = {"euler_fused": euler, "euler_unfused": euler, "multistep": FlowMatchMultistepScheduler.from_config(euler.config)}
    pipe = FluxFillPipeline(scheduler=euler, vae=_VaeCfg(), text_encoder=None, tokenizer=None, text_encoder_2=None, tokenizer_2=None,
                            transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_graph(not a.eager)
    B, H, W = a.batch, a.size, a.size
    S = (H // 16) * (W // 16)
    g = torch.Generator().manual_seed(0)
    kw = dict(latents=torch.randn(B, S, 64, generator=g).to(BF).to(dev),
              masked_image_latents=torch.cat([torch.randn(B, S, 64, generator=g), (torch.randn(B, S, 256, generator=g) > 0).float()], -1).to(BF).to(dev),
              prompt_embeds=(torch.randn(B, T_TXT, tr.config.joint_attention_dim, generator=g) * 0.1).to(BF).to(dev),
              pooled_prompt_embeds=torch.randn(B, tr.config.pooled_projection_dim, generator=g).to(BF).to(dev),
              height=H, width=W, num_inference_steps=a.steps, guidance_scale=30.0, output_type="latent")

    def run(name):
        pipe.scheduler, pipe.fuse_euler_step = scheds[name], name == "euler_fused"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipe(**kw).images
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
    res = {"layers": [nd, ns], "heads": a.heads, "steps": a.steps, "iters": a.iters, "warmup": a.warmup, "batch": B, "height": H, "width": W,
           "image_tokens": S, "loop": "eager" if a.eager else "graph", "device": torch.cuda.get_device_name(0), "weights": "random-init",
           "ms_per_call": {n: {"median": call[n], "min": min(v), "max": max(v)} for n, v in ms.items()},
           "ms_per_step": {n: call[n] / a.steps for n in ARMS},
           "multistep_minus_euler_fused_ms_per_step": (call["multistep"] - call["euler_fused"]) / a.steps,
           "multistep_minus_euler_unfused_ms_per_step": (call["multistep"] - call["euler_unfused"]) / a.steps,
           "euler_unfused_minus_fused_ms_per_step": (call["euler_unfused"] - call["euler_fused"]) / a.steps,
           "spread_of_one_arm_ms_per_step": max((max(v) - min(v)) / a.steps for v in ms.values()),
           "euler_unfused_latents_equal_fused": bool(torch.equal(outs["euler_unfused"], outs["euler_fused"])),
           "multistep_latents_differ_from_euler": not bool(torch.equal(outs["multistep"], outs["euler_fused"]))}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
