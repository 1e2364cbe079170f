"""Cost and effect of the first-block step cache (FluxFillPipeline.enable_step_cache), measured on whole pipeline calls of a random-init
full-depth model (latents in, latents out: no text encoders, no VAE), arms alternating call by call in ONE process, device events:

    off      the cache disabled: the plain loop, the baseline
    armed    threshold 0: never skips -- what arming costs (x0 copy, metric, store: four to five passes over [B, S, D] bf16, and one
             host read of the metric per step)
    skip     skip_steps = every second step from step 4 on -- the cost of a skipped step, and the latent MAE against `off`

Geometries: the headline (1024 x 1024, batch 8, 30 Euler steps) for all three arms, 576 x 512 batch 1 for off / skip.  Every arm is
timed in two blocks so that the spread between blocks is on record.  The MAE is a mechanism check on RANDOM weights, not image
quality, and no skip rate at any threshold is claimed here: both are properties of a real checkpoint.

    python tools/step_cache_ab.py [--geom headline,small] [--iters 5] [--warmup 3] [--layers 19,38] [--out profiles/step_cache_ab.json]

Per-kernel split of the armed arm (a run of its own):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/step_cache_ab.py --one armed --geom headline --iters 1 --warmup 1"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textflux_amd.pipeline import FluxFillPipeline
from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
from textflux_amd.transformer import FluxTransformer2DModel

BF = torch.bfloat16
GEOMS = {"headline": (8, 1024, 1024, ("off", "armed", "skip")), "small": (1, 576, 512, ("off", "skip"))}     # B, height, width, arms
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
T_TXT = 512


class _VaeCfg:       # output_type "latent" with injected masked_image_latents: only the VAE's config is consulted
    class config:
        block_out_channels = (128, 256, 512, 512)
        latent_channels = 16
        scaling_factor, shift_factor = 0.3611, 0.1159


def arm(pipe, name, steps):
    if name == "off":
        pipe.disable_step_cache()
    elif name == "armed":
        pipe.enable_step_cache(0.0)
    else:
        pipe.enable_step_cache(0.0, skip_steps=range(4, steps, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geom", default="headline,small")
    ap.add_argument("--iters", type=int, default=5, help="timed calls per arm and block (two blocks per arm)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--layers", default="19,38", help="double,single blocks (full depth by default)")
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--eager", action="store_true", help="the eager step loop instead of captured step graphs")
    ap.add_argument("--one", choices=["off", "armed", "skip"], default=None, help="run ONE arm only (under a profiler)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    nd, ns = (int(v) for v in a.layers.split(","))
    tr = FluxTransformer2DModel(in_channels=384, out_channels=64, num_layers=nd, num_single_layers=ns, num_attention_heads=a.heads,
                                guidance_embeds=True)
    tr.init_random_(seed=1, device=dev)
    pipe = FluxFillPipeline(scheduler=FlowMatchEulerDiscreteScheduler(**SCHED), vae=_VaeCfg(), text_encoder=None, tokenizer=None,
                            text_encoder_2=None, tokenizer_2=None, transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_graph(not a.eager)
    res = {"layers": [nd, ns], "heads": a.heads, "steps": a.steps, "iters_per_block": a.iters, "blocks": 2, "warmup": a.warmup,
           "loop": "eager" if a.eager else "graph", "device": torch.cuda.get_device_name(0), "weights": "random-init", "geometries": {}}
    for geom in a.geom.split(","):
        B, H, W, arms = GEOMS[geom]
        arms = [a.one] if a.one else list(arms)
        S = (H // 16) * (W // 16)
        g = torch.Generator().manual_seed(0)
        kw = dict(latents=torch.randn(B, S, 64, generator=g).to(BF).to(dev),
                  masked_image_latents=torch.cat([torch.randn(B, S, 64, generator=g), (torch.randn(B, S, 256, generator=g) > 0).float()], -1).to(BF).to(dev),
                  prompt_embeds=(torch.randn(B, T_TXT, tr.config.joint_attention_dim, generator=g) * 0.1).to(BF).to(dev),
                  pooled_prompt_embeds=torch.randn(B, tr.config.pooled_projection_dim, generator=g).to(BF).to(dev),
                  height=H, width=W, num_inference_steps=a.steps, guidance_scale=30.0, output_type="latent")

        def run(name):
            arm(pipe, name, a.steps)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = pipe(**kw).images
            e1.record()
            e1.synchronize()
            ms_ = e0.elapsed_time(e1)
            print(f"  {geom} {name}: {ms_:.1f} ms", file=sys.stderr, flush=True)
            return ms_, out

        outs = {}
        for _ in range(a.warmup):
            for name in arms:
                outs[name] = run(name)[1]
        ms = {name: [[], []] for name in arms}
        for block in range(2):
            for _ in range(a.iters):                     # alternating: drift of the board (clock, temperature) hits every arm alike
                for name in arms:
                    ms[name][block].append(run(name)[0])
        med = lambda v: sorted(v)[len(v) // 2]
        entry = {"batch": B, "height": H, "width": W, "image_tokens": S,
                 "ms_per_call": {n: {"median": med(v[0] + v[1]), "block_medians": [med(v[0]), med(v[1])], "min": min(v[0] + v[1]),
                                     "max": max(v[0] + v[1])} for n, v in ms.items()}}
        call = {n: entry["ms_per_call"][n]["median"] for n in arms}
        skipped = len(range(4, a.steps, 2))
        if "off" in call:
            entry["full_step_ms"] = call["off"] / a.steps
        if "off" in call and "armed" in call:
            entry["arming_ms_per_step"] = (call["armed"] - call["off"]) / a.steps
            entry["arming_share_of_a_step"] = (call["armed"] - call["off"]) / call["off"]
            entry["armed_latents_equal_off"] = bool(torch.equal(outs["armed"], outs["off"]))
        if "off" in call and "skip" in call and skipped:
            base = call["armed"] if "armed" in call else call["off"]       # the skip arm is armed too: its computed steps cost the armed step
            step = base / a.steps
            entry["skipped_steps"] = skipped
            entry["skipped_step_ms"] = step - (base - call["skip"]) / skipped
            entry["skipped_step_share_of_a_full_step"] = entry["skipped_step_ms"] / step
            entry["skipped_step_baseline_arm"] = "armed" if "armed" in call else "off"
            entry["skip_over_off_time"] = call["skip"] / call["off"]
            entry["latent_mae_skip_vs_off"] = (outs["skip"].float() - outs["off"].float()).abs().mean().item()
            entry["latent_mean_abs_off"] = outs["off"].float().abs().mean().item()
            entry["report_skipped"] = [i for i, r in enumerate(pipe.step_cache_report) if r["skipped"]] if arms[-1] == "skip" else None
        res["geometries"][geom] = entry
        print(geom, json.dumps(entry), flush=True)
        tr._session = None                               # the next geometry's workspace replaces this one
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
