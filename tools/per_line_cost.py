#!/usr/bin/env python3
"""What a multi-line scene costs on each of its five paths (DESIGN.md section 4 "Per-line edits"), on one GPU, in ONE process:

    canvas            today's multi-line canvas: all lines rendered onto a full-size glyph image stacked with the scene
    region            today's paste_back region: the bounding box of ALL lines together
    per_line          paste_back per_line: one single-line strip edit per line, each through its own region
    per_line_color    the same with color_match
    per_line_rectify  per_line with rectify: a slanted line is edited upright (DESIGN.md section 4 "Rectified lines"); on a scene
                      without a slanted line it is per_line

Scenes: glyph.synthetic_case(1024, 1024, multiline=True) (two lines, 768 and 512 px wide), a 2048 x 1536 photo with two lines in
opposite corners, neither wider than a quarter of the photo, and ("slanted", not in the default set) that photo with its second line
turned by 25 degrees.  Full depth, random weights (as bench.py), 30 Euler steps, step graphs
on; random stand-ins for the prompt embeddings (no text encoder runs: it costs the same in every arm).  The arms alternate, each
`--reps` times after one warm-up pass; the wall clock of the whole run_items call is recorded (device synchronised on both sides),
and device-event timings of the two colour-matching kernels at each scene's first line's region.  Every run goes into the output
file, which is rewritten after each of them; an arm's "spread" is max - min of its own runs, and a difference between two arms'
medians smaller than the larger of their spreads is reported as "no difference".

The first two arms are the same commit's unchanged paths.  Image content on random weights says nothing about quality; this tool
claims none.

    python tools/per_line_cost.py [--scenes 1024 2048 slanted] [--steps 30] [--reps 2] [--layers 19 38] [--out profiles/per_line_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

ARMS = {"canvas": None, "region": dict(region={}), "per_line": dict(per_line=True), "per_line_color": dict(per_line=True, color_match=True),
        "per_line_rectify": dict(per_line=True, rectify=True)}


def scenes(which):
    from PIL import Image
    from textflux_amd import glyph
    out = {}
    if "1024" in which:
        out["1024x1024"] = glyph.synthetic_case(1024, 1024, multiline=True)
    if "2048" in which:
        scene, _, words = glyph.synthetic_case(2048, 1536, multiline=True)
        m = np.zeros((1536, 2048), np.uint8)
        m[128:224, 128:640] = 255                 # 512 x 96, top left
        m[1312:1408, 1472:1920] = 255             # 448 x 96, bottom right
        out["2048x1536"] = (scene, Image.fromarray(m).convert("RGB"), words)
    if "slanted" in which:
        import math
        from PIL import ImageDraw
        scene, _, words = glyph.synthetic_case(2048, 1536, multiline=True)
        im = Image.new("L", (2048, 1536), 0)
        d = ImageDraw.Draw(im)
        d.rectangle((128, 128, 639, 223), fill=255)                              # 512 x 96, top left, level
        c, s = math.cos(math.radians(25)), math.sin(math.radians(25))
        d.polygon([(1600 + u * c - v * s, 1200 + u * s + v * c) for u, v in ((-224, -48), (224, -48), (224, 48), (-224, 48))], fill=255)
        out["2048x1536_slanted"] = (scene, im.convert("RGB"), words)             # 448 x 96 at 25 degrees, bottom right
    return out


def token_arithmetic(scene, mask, words, warp=None):
    """Image tokens of every arm's pipeline calls, from the preparation alone (warp: the pipeline's warp_affine, for the rectified arm)."""
    from textflux_amd import batch_driver as bd
    from textflux_amd import per_line as pl
    item = dict(image="s", mask="m", text="\n".join(words))
    load = lambda p: scene if p == "s" else mask
    cfg = lambda pb: None if pb is None else bd._paste_back_cfg(pb)
    out = {}
    for arm, pb in ARMS.items():
        if pb is not None and pb.get("per_line"):
            works = pl.prepare_lines(0, item, load, True, None, cfg(pb), warp=warp if pb.get("rectify") else None)
        else:
            works = [bd.prepare_item(0, item, load, device_compose=True, **({} if pb is None else dict(paste_back=cfg(pb))))]
        toks = [bd.image_tokens(w.size) for w in works]
        out[arm] = dict(sizes=[list(w.size) for w in works], image_tokens=toks, attention_sum_n2=sum(t * t for t in toks))
    return out


def kernel_times(scene, mask, words, iters=20, warmup=3):
    from paste_back_cost import timed
    from textflux_amd import batch_driver as bd
    from textflux_amd import ops
    from textflux_amd import paste_back as pb
    from textflux_amd import per_line as pl
    w = pl.prepare_lines(0, dict(image="s", mask="m", text="\n".join(words)), lambda p: scene if p == "s" else mask, True, None,
                         bd._paste_back_cfg(dict(per_line=True)))[0]
    reg = w.region
    crop = torch.from_numpy(np.ascontiguousarray(w.orig_scene[reg.y0:reg.y1, reg.x0:reg.x1]))[None].cuda()
    grey = torch.from_numpy(pb.grey_of(w.orig_mask[reg.y0:reg.y1, reg.x0:reg.x1]))[None].cuda()
    alpha = pb.alpha_mask(grey)
    ring = pb.ring_mask(alpha)
    lut = torch.arange(256, dtype=torch.uint8, device="cuda").expand(1, 3, 256).contiguous()
    return dict(shape=list(crop.shape), ring_pixels=int((ring != 0).sum()),
                masked_moments=timed(lambda: ops.masked_moments(crop, crop, ring), iters, warmup),
                overlay_lut=timed(lambda: ops.overlay_lut(crop, crop, alpha, lut), iters, warmup))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", nargs="*", default=["1024", "2048"], choices=["1024", "2048", "slanted"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--layers", type=int, nargs=2, default=[19, 38])
    ap.add_argument("--arms", nargs="*", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "per_line_cost.json"))
    a = ap.parse_args()
    from mixed_batch_ab import build_pipe
    from textflux_amd import batch_driver
    dev = torch.device("cuda", 0)
    pipe = build_pipe(a.layers, dev)
    out = dict(steps=a.steps, reps=a.reps, layers=a.layers, device=torch.cuda.get_device_name(0), weights="random-init", step_graphs=True,
               scenes={})

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for name, (scene, mask, words) in scenes(a.scenes).items():
        sc = out["scenes"][name] = dict(words=words, arithmetic=token_arithmetic(scene, mask, words, pipe.warp_affine),
                                        kernels=kernel_times(scene, mask, words), runs={arm: [] for arm in a.arms})
        item = [dict(image="s", mask="m", text="\n".join(words))]
        load = lambda p: scene if p == "s" else mask

        def run(arm):
            torch.cuda.synchronize()
            t0 = time.time()
            res = batch_driver.run_items(item, pipe, None, batch_size=8, num_inference_steps=a.steps, seed=42, device=dev, loader=load,
                                         save=lambda i, img: None, paste_back=ARMS[arm])
            torch.cuda.synchronize()
            if res["failed"]:
                raise SystemExit(f"{name} / {arm}: failed")
            return time.time() - t0

        for arm in a.arms:                         # warm-up: kernels loaded, sessions made and step graphs captured for every geometry
            sc.setdefault("warmup_seconds", {})[arm] = run(arm)
            print(f"{name} warm-up {arm}: {sc['warmup_seconds'][arm]:.2f} s", flush=True)
            flush()
        for rep in range(a.reps):
            for arm in a.arms:                     # alternating: drift of the machine hits every arm alike
                sc["runs"][arm].append(run(arm))
                print(f"{name} rep {rep} {arm}: {sc['runs'][arm][-1]:.2f} s", flush=True)
                flush()
        summary = {arm: dict(median_s=float(np.median(r)), spread_s=max(r) - min(r)) for arm, r in sc["runs"].items()}
        for arm, s in summary.items():
            for base in ("canvas", "region"):
                if base in summary and arm != base:
                    d = s["median_s"] - summary[base]["median_s"]
                    s[f"vs_{base}"] = "no difference" if abs(d) <= max(s["spread_s"], summary[base]["spread_s"]) else f"{d:+.2f} s"
        sc["summary"] = summary
        print(name, json.dumps(summary), flush=True)
        flush()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
