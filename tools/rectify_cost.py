"""What rectifying a slanted line costs beside the paste and the VAE decode it sits between (DESIGN.md section 4 "Rectified lines"), in
ONE process, device events:

    warp_forward    scene -> upright: the [rh, rw] crop of the oriented rectangle, sampled from the whole scene (ops.warp_affine_u8)
    warp_mask       the same warp of the scene's RGB mask (the preparation runs both)
    warp_backward   upright -> scene: the rectangle's bounding window, sampled from the upright result, with coverage
    paste           today's unrectified paste on that same window (resample of an edit, alpha_mask, overlay)
    paste_rect      the rectified paste on it (resample to (rh, rw), warp_backward, alpha_mask, overlay)
    vae_decode      AutoencoderKL.decode_nhwc of the strip's canvas: the glyph strip stacked on the upright crop (random-init weights)

Default: a 1024 x 256 line at 25 degrees in the middle of a 2048 x 1536 scene, batch 1, dilate 16, feather 4, median of 20 after 3
warm-up calls outside the timed window.  No threshold hangs on these numbers: the path is opt-in and not part of bench.py.

    python tools/rectify_cost.py [--angle 25] [--iters 20] [--out profiles/rectify_cost.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from paste_back_cost import timed
from textflux_amd import ops
from textflux_amd import paste_back as pb
from textflux_amd import rectify as rc
from textflux_amd.vae import AutoencoderKL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, nargs=2, default=[2048, 1536], metavar=("W", "H"))
    ap.add_argument("--line", type=int, nargs=2, default=[1024, 256], metavar=("RW", "RH"), help="the oriented rectangle's size")
    ap.add_argument("--angle", type=float, default=25.0)
    ap.add_argument("--dilate", type=int, default=pb.DILATE)
    ap.add_argument("--feather", type=int, default=pb.FEATHER)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    (W, H), (rw, rh) = a.scene, a.line
    rect = rc.Rect(W // 2, H // 2, rw, rh, a.angle, rw, rh)
    x0, y0, x1, y1 = rc.rect_window(rect, (W, H))
    fwd, back = rc.matrices(rect, (x0, y0))
    fwd_d, back_d = (torch.from_numpy(m).to(dev) for m in (rc.matrices(rect)[0], back))
    g = torch.Generator().manual_seed(0)
    scene = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    # the mask: a bar along the rectangle's axis, inset by the rectangle's margin on every side
    yy, xx = np.mgrid[0:H, 0:W]
    c, s = math.cos(math.radians(a.angle)), math.sin(math.radians(a.angle))
    u, v = (xx - rect.cx) * c + (yy - rect.cy) * s, -(xx - rect.cx) * s + (yy - rect.cy) * c
    margin = 2 * pb.halo(a.dilate, a.feather)
    m = np.where((np.abs(u) <= rw / 2 - margin) & (np.abs(v) <= rh / 2 - margin), 255, 0).astype(np.uint8)
    mask_rgb = torch.from_numpy(np.repeat(m[None, :, :, None], 3, 3)).to(dev).contiguous()
    window = scene[:, y0:y1, x0:x1].contiguous()
    wmask = torch.from_numpy(np.ascontiguousarray(m[None, y0:y1, x0:x1])).to(dev)
    strip = int(rw * 0.1667)
    canvas = ((rw // 32) * 32, ((rh + strip) // 32) * 32)
    upright = torch.randint(0, 256, (1, canvas[1] - canvas[1] * strip // (rh + strip), canvas[0], 3), generator=g, dtype=torch.uint8).to(dev)
    flat_edit = torch.randint(0, 256, (1, (y1 - y0) * 13 // 16, x1 - x0, 3), generator=g, dtype=torch.uint8).to(dev)
    vae = AutoencoderKL().init_random_(seed=7, device=dev)
    z = (torch.randn(1, canvas[1] // 8, canvas[0] // 8, 16, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    res = {"scene": [W, H], "rect": [rw, rh], "angle": a.angle, "window": [x1 - x0, y1 - y0], "canvas": list(canvas), "dilate": a.dilate,
           "feather": a.feather, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "vae_weights": "random-init"}
    t = lambda fn: timed(fn, a.iters, a.warmup)
    res["warp_forward"] = t(lambda: ops.warp_affine_u8(scene, fwd_d, (rh, rw)))
    res["warp_mask"] = t(lambda: ops.warp_affine_u8(mask_rgb, fwd_d, (rh, rw)))
    up = ops.resample_u8(upright, (rh, rw))
    res["warp_backward"] = t(lambda: ops.warp_affine_u8(up, back_d, (y1 - y0, x1 - x0), coverage=True))
    res["paste"] = t(lambda: pb.paste(window, flat_edit, wmask, a.dilate, a.feather))
    res["paste_rect"] = t(lambda: pb.paste(window, upright, wmask, a.dilate, a.feather, rect=rect, origin=(x0, y0)))
    res["vae_decode"] = t(lambda: vae.decode_nhwc(z))
    both = res["warp_forward"]["median_ms"] + res["warp_mask"]["median_ms"] + res["warp_backward"]["median_ms"]
    res["warps_over_vae_decode"] = both / res["vae_decode"]["median_ms"]
    res["paste_rect_over_paste"] = res["paste_rect"]["median_ms"] / res["paste"]["median_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
