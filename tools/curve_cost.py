"""What cutting a line through a control grid costs beside the affine (rectified) cut of the same size, the paste and the VAE decode it
sits between (DESIGN.md section 4 "Curved lines").  Device events; the arms of one step ALTERNATE in one process: every round runs the
grid arm and the affine arm of the same crop size once, so a drift of the clocks falls on both alike.  No figure is fixed in advance:
the yardstick is the affine arm of the same run.

    forward     scene -> upright: the [rh, rw] crop of the ribbon, sampled from the whole scene (ops.warp_grid_u8), beside
                ops.warp_affine_u8 into a level rectangle of rw x rh at the same place
    backward    upright -> scene: the footprint's bounding window, sampled from the upright result, with coverage, beside the affine
                warp back on ITS window (per destination pixel, since the two windows differ in size)
    paste       the whole paste on that window (resample to (rh, rw), the backward GRID BUILT ON THE HOST, the warp, alpha_mask, overlay)
                beside paste(rect=Rect)
    vae         AutoencoderKL.decode_nhwc of the strip's canvas: the glyph strip stacked on the upright crop (random-init weights)

Every step is a child process of its own under its own time limit; the parent never opens the device, and after a step that fails or
runs out of time it starts nothing more.  Default: a 1024 x 256 line on an arc of radius 1200 in a 2048 x 1536 scene, batch 1, dilate 16,
feather 4, pad 0, median of 20 rounds after 3 warm-up calls of every arm outside the timed window.  The path is opt-in and not part of
bench.py.

    python tools/curve_cost.py [--radius 1200] [--iters 20] [--out profiles/curve_cost.json]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = ("forward", "backward", "paste", "vae")


def timed_alternating(arms, iters, warmup):
    """{name: {median_ms, min_ms, max_ms}}: `warmup` untimed calls of every arm, then `iters` rounds of one timed call per arm."""
    import torch
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


def plan(a):
    """The line's mask, its Ribbon and window, and the level rectangle of the same crop size with its window (host only)."""
    from textflux_amd import curve as cv
    from textflux_amd import glyph
    from textflux_amd import paste_back as pb                                    # imported here, so that host_plan_ms times the plan alone
    from textflux_amd import rectify as rc
    (W, H), (L, T), R = a.scene, a.line, a.radius
    half = L / (2.0 * R)
    sag = R * (1.0 - math.cos(half))
    cx, cy = W / 2.0, H / 2.0 - sag / 2.0 + R
    ang = np.linspace(-math.pi / 2 - half, -math.pi / 2 + half, 256)
    outer = [(cx + (R + T / 2) * math.cos(t), cy + (R + T / 2) * math.sin(t)) for t in ang]
    inner = [(cx + (R - T / 2) * math.cos(t), cy + (R - T / 2) * math.sin(t)) for t in ang[::-1]]
    m = glyph.fill_polygon(H, W, outer + inner)[:, :, 0]
    t0 = time.perf_counter()
    rb = cv.select_ribbon(rc.mask_points(m), a.dilate, a.feather, pad=0.0, min_side=96, max_side=1 << 30)
    host_plan_ms = (time.perf_counter() - t0) * 1e3
    if rb is None or not cv.is_curved(rb.line):
        raise SystemExit("this line is not served by the curved path: change --radius or --line")
    win = cv.ribbon_window(rb, (W, H))
    rect = rc.Rect(W // 2, H // 2, rb.rw, rb.rh, 0.0, rb.rw, rb.rh)
    return m, rb, win, rect, rc.rect_window(rect, (W, H)), host_plan_ms


def child(a):
    import torch
    from textflux_amd import curve as cv
    from textflux_amd import ops
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    dev = torch.device("cuda")
    (W, H) = a.scene
    m, rb, (x0, y0, x1, y1), rect, (a0, b0, a1, b1), host_plan_ms = plan(a)
    rw, rh = rb.rw, rb.rh
    g = torch.Generator().manual_seed(0)
    strip = int(rw * 0.1667)
    canvas = ((rw // 32) * 32, ((rh + strip) // 32) * 32)
    res = {"crop": [rw, rh], "shift": rb.shift, "r_min": rb.line.r_min, "window": [x1 - x0, y1 - y0], "affine_window": [a1 - a0, b1 - b0],
           "canvas": list(canvas), "host_plan_ms": host_plan_ms, "device": torch.cuda.get_device_name(0)}
    if a.step == "vae":
        from textflux_amd.vae import AutoencoderKL
        vae = AutoencoderKL().init_random_(seed=7, device=dev)
        z = (torch.randn(1, canvas[1] // 8, canvas[0] // 8, 16, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        arms = {"vae_decode": lambda: vae.decode_nhwc(z)}
        res["vae_weights"] = "random-init"
    else:
        scene = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        upright = torch.randint(0, 256, (1, canvas[1] - canvas[1] * strip // (rh + strip), canvas[0], 3), generator=g, dtype=torch.uint8).to(dev)
        if a.step == "forward":
            fwd_d, afwd_d = torch.from_numpy(cv.forward_grid(rb)).to(dev), torch.from_numpy(rc.matrices(rect)[0]).to(dev)
            arms = {"grid_forward": lambda: ops.warp_grid_u8(scene, fwd_d, rb.shift, (rh, rw)),
                    "affine_forward": lambda: ops.warp_affine_u8(scene, afwd_d, (rh, rw))}
        elif a.step == "backward":
            t0 = time.perf_counter()
            back = cv.backward_grid(rb, (x0, y0), (y1 - y0, x1 - x0))
            res["host_backward_grid_ms"] = (time.perf_counter() - t0) * 1e3
            back_d, aback_d = torch.from_numpy(back).to(dev), torch.from_numpy(rc.matrices(rect, (a0, b0))[1]).to(dev)
            up = ops.resample_u8(upright, (rh, rw))
            arms = {"grid_backward": lambda: ops.warp_grid_u8(up, back_d, rb.shift, (y1 - y0, x1 - x0), coverage=True),
                    "affine_backward": lambda: ops.warp_affine_u8(up, aback_d, (b1 - b0, a1 - a0), coverage=True)}
        else:
            window, wmask = scene[:, y0:y1, x0:x1].contiguous(), torch.from_numpy(np.ascontiguousarray(m[None, y0:y1, x0:x1])).to(dev)
            awindow, amask = scene[:, b0:b1, a0:a1].contiguous(), torch.from_numpy(np.ascontiguousarray(m[None, b0:b1, a0:a1])).to(dev)
            arms = {"paste_ribbon": lambda: pb.paste(window, upright, wmask, a.dilate, a.feather, rect=rb, origin=(x0, y0)),
                    "paste_rect": lambda: pb.paste(awindow, upright, amask, a.dilate, a.feather, rect=rect, origin=(a0, b0))}
    res.update(timed_alternating(arms, a.iters, a.warmup))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, nargs=2, default=[2048, 1536], metavar=("W", "H"))
    ap.add_argument("--line", type=int, nargs=2, default=[1024, 256], metavar=("L", "T"), help="the line's arc length and thickness")
    ap.add_argument("--radius", type=float, default=1200.0, help="the radius of the line's centre arc")
    ap.add_argument("--dilate", type=int, default=16)
    ap.add_argument("--feather", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step_timeout", type=int, default=240, help="seconds one step's process may take")
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run this one step in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step is not None:
        return child(a)
    res = {"scene": a.scene, "line": a.line, "radius": a.radius, "dilate": a.dilate, "feather": a.feather, "iters": a.iters, "warmup": a.warmup}
    passed = [x for x in sys.argv[1:]]
    for step in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + passed, capture_output=True, text=True,
                               timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} ran out of its {a.step_timeout} s: nothing more is started")
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"step {step} failed with exit status {p.returncode}: nothing more is started")
        res.update(json.loads(lines[-1][len("RESULT "):]))
    med = lambda k: res[k]["median_ms"]
    px_g, px_a = res["window"][0] * res["window"][1], res["affine_window"][0] * res["affine_window"][1]
    res["grid_forward_over_affine_forward"] = med("grid_forward") / med("affine_forward")
    res["grid_backward_over_affine_backward_per_pixel"] = (med("grid_backward") / px_g) / (med("affine_backward") / px_a)
    res["paste_ribbon_over_paste_rect_per_pixel"] = (med("paste_ribbon") / px_g) / (med("paste_rect") / px_a)
    res["grid_backward_over_vae_decode"] = med("grid_backward") / med("vae_decode")
    res["paste_ribbon_over_vae_decode"] = med("paste_ribbon") / med("vae_decode")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
