"""What paste-back costs beside the VAE decode it follows (DESIGN.md section 4 "Paste-back"), in ONE process, device events:

    alpha_mask   binarise + dilate (2 window passes) + feather (6 window passes) of a [B, H, W] uint8 mask
    paste        resample of the edit to the original's size (two passes), alpha_mask, overlay
    vae_decode   AutoencoderKL.decode_nhwc of the same batch (random-init weights, production configuration)

Default: 1024 x 1024 scenes, batch 8, the edit 1024 x 832 (a canvas crop: the resample is part of the cost), dilate 16, feather 4,
median of 20 after 3 warm-up calls.  No threshold hangs on these numbers: the path is opt-in and not part of bench.py.

    python tools/paste_back_cost.py [--batch 8] [--size 1024] [--iters 20] [--out profiles/paste_back_cost.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textflux_amd import paste_back as pb
from textflux_amd.vae import AutoencoderKL


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dilate", type=int, default=pb.DILATE)
    ap.add_argument("--feather", type=int, default=pb.FEATHER)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    B, S = a.batch, a.size
    g = torch.Generator().manual_seed(0)
    orig = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    edit = torch.randint(0, 256, (B, S * 13 // 16, S, 3), generator=g, dtype=torch.uint8).to(dev)
    mask = torch.zeros(B, S, S, dtype=torch.uint8)
    mask[:, S // 3: 2 * S // 3, S // 8: 7 * S // 8] = 255
    mask = mask.to(dev)
    vae = AutoencoderKL().init_random_(seed=7, device=dev)
    z = (torch.randn(B, S // 8, S // 8, 16, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    res = {"batch": B, "height": S, "width": S, "edit_size": list(edit.shape[1:3]), "dilate": a.dilate, "feather": a.feather,
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "vae_weights": "random-init"}
    res["alpha_mask"] = timed(lambda: pb.alpha_mask(mask, a.dilate, a.feather), a.iters, a.warmup)
    res["paste"] = timed(lambda: pb.paste(orig, edit, mask, a.dilate, a.feather), a.iters, a.warmup)
    res["vae_decode"] = timed(lambda: vae.decode_nhwc(z), a.iters, a.warmup)
    res["paste_over_vae_decode"] = res["paste"]["median_ms"] / res["vae_decode"]["median_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
