#!/usr/bin/env python3
"""LoRA variant of run_inference.py: base FLUX.1-Fill-dev transformer + TextFlux LoRA merged at load (reference:
run_inference_lora.py:44-73: lora_state_dict(..., return_alphas=True) + load_lora_into_transformer).  Like the
reference, --scheduler is parsed but the sampler is chosen by the module-level `scheduler_name`.
Not in the reference: --lora_runtime keeps the adapter unmerged (FluxTransformer2DModel.attach_lora: its strength can change per call,
it can be unloaded) and --lora_scale sets its strength; the defaults are the merged path at strength 1."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import run_inference as base
from textflux_amd.pipeline import FluxFillPipeline
from textflux_amd.transformer import FluxTransformer2DModel

LORA = os.environ.get("TEXTFLUX_LORA", "./models/textflux-lora-beta")
scheduler_name = "default"
LORA_ADAPTER = "textflux"


def load_flux_pipeline(lora_runtime: bool = False, lora_scale: float = 1.0):
    if base.PIPE is None:
        transformer = FluxTransformer2DModel.from_pretrained(base.BASE, subfolder="transformer", torch_dtype=torch.bfloat16)
        state_dict, network_alphas = FluxFillPipeline.lora_state_dict(LORA, return_alphas=True)
        if lora_runtime:
            FluxFillPipeline.load_lora_into_transformer(state_dict, network_alphas, transformer, adapter_name=LORA_ADAPTER, runtime=True)
            transformer.set_adapters([LORA_ADAPTER], [lora_scale])
        elif lora_scale != 1.0:
            from textflux_amd import lora
            lora.merge_lora_into_transformer(state_dict, network_alphas, transformer, scale=lora_scale)
        else:
            FluxFillPipeline.load_lora_into_transformer(state_dict, network_alphas, transformer)
        base.PIPE = FluxFillPipeline.from_pretrained(base.BASE, transformer=transformer, torch_dtype=torch.bfloat16).to("cuda")
    return base.PIPE


def build_parser():
    ap = argparse.ArgumentParser(description="Flux Text Generation CLI (LoRA)")
    ap.add_argument("--image", type=str, required=True)
    ap.add_argument("--mask", type=str, required=True)
    ap.add_argument("--words", type=str, required=True)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--guidance-scale", type=float, default=30)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--scheduler", type=str, default="default", help="parsed but unused, as in the reference (:538)")
    ap.add_argument("--lora_runtime", action="store_true", help="keep the LoRA as an unmerged runtime adapter instead of merging it at load")
    ap.add_argument("--lora_scale", type=float, default=1.0, help="strength of the LoRA (1.0 = as trained)")
    ap.add_argument("--multistep", action="store_true", help="sample with the second-order multistep sampler (not in the reference)")
    base.add_known_region_args(ap)
    base.add_step_cache_args(ap)
    base.add_paste_back_args(ap)
    base.add_ocr_args(ap)
    base.add_candidates_args(ap)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    paste_back = base.paste_back_from_args(a)
    known = base.known_region_from_args(a)
    ocr = base.ocr_from_args(a)
    base.scheduler_name = "multistep" if a.multistep else scheduler_name
    candidates = base.candidates_from_args(a)
    pipe = base.apply_step_cache_args(a, load_flux_pipeline(a.lora_runtime, a.lora_scale))
    if candidates is not None:
        base.process_candidates(a.image, a.mask, a.words, a.steps, a.guidance_scale, a.seed, pipe, candidates, ocr, paste_back=paste_back,
                                known=known)
        base.report_step_cache(pipe)
        print("\nProcessing completed successfully!")
        return
    base.process_normal_mode(a.image, a.mask, a.words, a.steps, a.guidance_scale, a.seed, pipe=pipe, paste_back=paste_back,
                             **(dict(known=known) if known else {}), **(dict(ocr=ocr) if ocr else {}))
    base.report_step_cache(pipe)
    print("\nProcessing completed successfully!")


if __name__ == "__main__":
    main()
