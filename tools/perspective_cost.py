"""What cutting a line through a homography costs beside the affine (rectified) cut of the same size, the paste and the VAE decode it
sits between (DESIGN.md section 4 "Perspective lines"), in ONE process, device events, the arms ALTERNATING: every round runs each arm
once, so a drift of the clocks falls on all of them alike.

    persp_forward    scene -> upright: the [rh, rw] crop of the quad, sampled from the whole scene (ops.warp_perspective_u8)
    persp_mask       the same warp of the scene's RGB mask (the preparation runs both)
    persp_backward   upright -> scene: the footprint's bounding window, sampled from the upright result, with coverage
    paste_quad       the whole perspective paste on that window (resample to (rh, rw), persp_backward, alpha_mask, overlay)
    affine_forward, affine_mask, affine_backward, paste_rect
                     tools/rectify_cost.py's arms at the same crop size: the yardstick (a level oriented rectangle of rw x rh at the same
                     place; the backward warp and the paste on ITS window)
    vae_decode       AutoencoderKL.decode_nhwc of the strip's canvas: the glyph strip stacked on the upright crop (random-init weights)

Default: a 1024 x 256 line with a 2:1 taper (its far side 128 tall) in the middle of a 2048 x 1536 scene, batch 1, dilate 16, feather 4,
pad 0, median of 20 rounds after 3 warm-up calls of every arm outside the timed window.  No threshold hangs on these numbers: the path is
opt-in and not part of bench.py.

    python tools/perspective_cost.py [--taper 2] [--iters 20] [--out profiles/perspective_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textflux_amd import glyph, ops
from textflux_amd import paste_back as pb
from textflux_amd import perspective as ps
from textflux_amd import rectify as rc
from textflux_amd.vae import AutoencoderKL


def timed_alternating(arms, iters, warmup):
    """{name: {median_ms, min_ms, max_ms}}: `warmup` untimed calls of every arm, then `iters` rounds of one timed call per arm."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(iters):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    out = {}
    for name, v in ms.items():
        v.sort()
        out[name] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, nargs=2, default=[2048, 1536], metavar=("W", "H"))
    ap.add_argument("--line", type=int, nargs=2, default=[1024, 256], metavar=("L", "T"), help="the line's length and its near side's height")
    ap.add_argument("--taper", type=float, default=2.0, help="near side / far side")
    ap.add_argument("--dilate", type=int, default=pb.DILATE)
    ap.add_argument("--feather", type=int, default=pb.FEATHER)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    (W, H), (L, T) = a.scene, a.line
    cx, cy, far = W // 2, H // 2, T / a.taper
    drawn = [(cx - L // 2, cy - T // 2), (cx + L // 2, cy - far / 2), (cx + L // 2, cy + far / 2), (cx - L // 2, cy + T // 2)]
    m = glyph.fill_polygon(H, W, drawn)[:, :, 0]
    quad = ps.select_quad(rc.mask_points(m), a.dilate, a.feather, pad=0.0, min_side=96, max_side=1 << 30)
    if quad is None:
        raise SystemExit("no padding serves this quad: lower --taper")
    rw, rh = quad.rw, quad.rh
    x0, y0, x1, y1 = ps.quad_window(quad, (W, H))
    fwd_d, back_d = (torch.from_numpy(v).to(dev) for v in (ps.matrices(quad)[0], ps.matrices(quad, (x0, y0))[1]))
    rect = rc.Rect(cx, cy, rw, rh, 0.0, rw, rh)
    a0, b0, a1, b1 = rc.rect_window(rect, (W, H))
    afwd_d, aback_d = (torch.from_numpy(v).to(dev) for v in (rc.matrices(rect)[0], rc.matrices(rect, (a0, b0))[1]))
    g = torch.Generator().manual_seed(0)
    scene = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    mask_rgb = torch.from_numpy(np.repeat(m[None, :, :, None], 3, 3)).to(dev).contiguous()
    window, wmask = scene[:, y0:y1, x0:x1].contiguous(), torch.from_numpy(np.ascontiguousarray(m[None, y0:y1, x0:x1])).to(dev)
    awindow, amask = scene[:, b0:b1, a0:a1].contiguous(), torch.from_numpy(np.ascontiguousarray(m[None, b0:b1, a0:a1])).to(dev)
    strip = int(rw * 0.1667)
    canvas = ((rw // 32) * 32, ((rh + strip) // 32) * 32)
    upright = torch.randint(0, 256, (1, canvas[1] - canvas[1] * strip // (rh + strip), canvas[0], 3), generator=g, dtype=torch.uint8).to(dev)
    up = ops.resample_u8(upright, (rh, rw))
    vae = AutoencoderKL().init_random_(seed=7, device=dev)
    z = (torch.randn(1, canvas[1] // 8, canvas[0] // 8, 16, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    res = {"scene": [W, H], "line": [L, T], "taper": a.taper, "crop": [rw, rh], "inner": [quad.ox, quad.oy, quad.iw, quad.ih],
           "window": [x1 - x0, y1 - y0], "affine_window": [a1 - a0, b1 - b0], "canvas": list(canvas), "dilate": a.dilate, "feather": a.feather,
           "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "vae_weights": "random-init"}
    res.update(timed_alternating({
        "persp_forward": lambda: ops.warp_perspective_u8(scene, fwd_d, (rh, rw)),
        "affine_forward": lambda: ops.warp_affine_u8(scene, afwd_d, (rh, rw)),
        "persp_mask": lambda: ops.warp_perspective_u8(mask_rgb, fwd_d, (rh, rw)),
        "affine_mask": lambda: ops.warp_affine_u8(mask_rgb, afwd_d, (rh, rw)),
        "persp_backward": lambda: ops.warp_perspective_u8(up, back_d, (y1 - y0, x1 - x0), coverage=True),
        "affine_backward": lambda: ops.warp_affine_u8(up, aback_d, (b1 - b0, a1 - a0), coverage=True),
        "paste_quad": lambda: pb.paste(window, upright, wmask, a.dilate, a.feather, rect=quad, origin=(x0, y0)),
        "paste_rect": lambda: pb.paste(awindow, upright, amask, a.dilate, a.feather, rect=rect, origin=(a0, b0)),
        "vae_decode": lambda: vae.decode_nhwc(z),
    }, a.iters, a.warmup))
    med = lambda k: res[k]["median_ms"]
    # per destination pixel, since the two backward windows differ in size
    px_q, px_r = (x1 - x0) * (y1 - y0), (a1 - a0) * (b1 - b0)
    res["persp_forward_over_affine_forward"] = med("persp_forward") / med("affine_forward")
    res["persp_backward_over_affine_backward_per_pixel"] = (med("persp_backward") / px_q) / (med("affine_backward") / px_r)
    res["paste_quad_over_paste_rect_per_pixel"] = (med("paste_quad") / px_q) / (med("paste_rect") / px_r)
    res["persp_backward_over_vae_decode"] = med("persp_backward") / med("vae_decode")
    res["persp_warps_over_vae_decode"] = (med("persp_forward") + med("persp_mask") + med("persp_backward")) / med("vae_decode")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
