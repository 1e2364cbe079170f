#!/usr/bin/env python3
"""Generate tests/golden/g18_true_cfg.safetensors by IMPORTING the reference (as make_keep_known_goldens.py does; build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_true_cfg_goldens.py

What true CFG is pinned to, all on torch-CPU bf16 tensors, data only:
  * the combine of FluxCFGPipeline's loop (examples/community/pipeline_flux_with_cfg.py:808) on [2, 6, 64] Gaussian tensors with
    planted special values -- the four sign combinations of zero, +-inf on either side, NaN, a bf16 subnormal -- for true_cfg in
    {1.5, 3.3, 7.0, 30.0}.  The loop body is not a function, so the line itself is read from the reference's file, checked to be the
    line this was written against, and executed on the tensors;
  * FlowMatchEulerDiscreteScheduler.step on that result, on g16's 5-step shifted grid (the mu of a 96-token image), every step;
  * the order of the doubled batch: the reference's two torch.cat lines (:739-740), executed on index rows.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REFERENCE = "/root/reference/diffusers"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REFERENCE, "src"))
sys.dont_write_bytecode = True

import numpy as np
import torch
import transformers.utils as tu

tu.FLAX_WEIGHTS_NAME = "flax_model.msgpack"  # removed in transformers 5.x; the reference imports it

from safetensors.torch import save_file

import diffusers  # the reference, 0.32.0.dev0
from diffusers import FlowMatchEulerDiscreteScheduler
from diffusers.pipelines.flux.pipeline_flux_inpaint import calculate_shift

OUT = os.path.dirname(os.path.abspath(__file__))
assert diffusers.__version__ == "0.32.0.dev0"
torch.set_grad_enabled(False)
BF = torch.bfloat16
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
N, TOKENS, SHAPE = 5, 96, (2, 6, 64)
SCALES = (1.5, 3.3, 7.0, 30.0)
COMBINE = "noise_pred = neg_noise_pred + true_cfg * (noise_pred - neg_noise_pred)"
CAT = ("prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)",
       "pooled_prompt_embeds = torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds], dim=0)")


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


def scheduler(n=N):
    s = FlowMatchEulerDiscreteScheduler(**SCHED)
    mu = calculate_shift(TOKENS, s.config.base_image_seq_len, s.config.max_image_seq_len, s.config.base_shift, s.config.max_shift)
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cpu", mu=mu)
    return s


def reference_lines():
    """the reference's own lines, stripped; each must stand in the file exactly once"""
    src = [l.strip() for l in open(os.path.join(REFERENCE, "examples", "community", "pipeline_flux_with_cfg.py"))]
    for line in (COMBINE,) + CAT:
        assert src.count(line) == 1, line
    return COMBINE, CAT


def main():
    combine, cat = reference_lines()
    out = {}
    neg, pos = rnd(SHAPE, 1, 0.5), rnd(SHAPE, 2, 0.5)
    inf, nan, sub = float("inf"), float("nan"), 2.0 ** -130         # 2^-130: a bf16 subnormal (the smallest normal is 2^-126)
    planted_neg = [0.0, 0.0, -0.0, -0.0, inf, -inf, 1.0, 1.0, inf, inf, nan, 1.0, sub, 1.0, sub, -sub]
    planted_pos = [0.0, -0.0, 0.0, -0.0, 1.0, 1.0, inf, -inf, inf, -inf, 1.0, nan, 1.0, sub, sub, sub]
    neg.view(-1)[:len(planted_neg)] = torch.tensor(planted_neg, dtype=torch.float32).to(BF)
    pos.view(-1)[:len(planted_pos)] = torch.tensor(planted_pos, dtype=torch.float32).to(BF)
    assert float(neg.view(-1)[12]) == sub                            # the subnormal survived the conversion
    out.update(neg=neg, pos=pos, scales=torch.tensor(SCALES, dtype=torch.float64))
    sch = scheduler()
    out["sigmas"] = sch.sigmas.clone()
    out["timesteps"] = sch.timesteps.clone()
    for k, g in enumerate(SCALES):
        env = dict(neg_noise_pred=neg, noise_pred=pos, true_cfg=g)
        exec(combine, {}, env)                                       # :808, the Python float as the reference passes it
        v = env["noise_pred"]
        assert v.dtype == BF
        out[f"g{k}_combined"] = v
        sch = scheduler()
        for i, t in enumerate(sch.timesteps):
            lat = rnd(SHAPE, 10 + i)
            out[f"g{k}_s{i}_latents"] = sch.step(v, t, lat, return_dict=False)[0]
    for i in range(N):
        out[f"s{i}_latents_in"] = rnd(SHAPE, 10 + i)
    # the doubled batch: rows named by index, negative b = b, positive b = 100 + b
    env = dict(torch=torch, negative_prompt_embeds=torch.tensor([[0], [1]], dtype=torch.int32),
               prompt_embeds=torch.tensor([[100], [101]], dtype=torch.int32),
               negative_pooled_prompt_embeds=torch.tensor([[0], [1]], dtype=torch.int32),
               pooled_prompt_embeds=torch.tensor([[100], [101]], dtype=torch.int32))
    for line in cat:
        exec(line, {}, env)
    out["cat_prompt_embeds"], out["cat_pooled"] = env["prompt_embeds"], env["pooled_prompt_embeds"]
    out = {k: v.contiguous() for k, v in out.items()}
    path = os.path.join(OUT, "g18_true_cfg.safetensors")
    save_file(out, path)
    print(f"g18_true_cfg: {len(out)} tensors, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
