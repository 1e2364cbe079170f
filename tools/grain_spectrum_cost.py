"""What the grain spectrum match costs beside the white grain match and today's paste of the same window, and beside the VAE decode it
follows (DESIGN.md section 4 "Grain spectrum").  The scene, the window, the timing (device events, arms ALTERNATING in one process,
median of --iters rounds after --warmup calls of every arm) and the process discipline are tools/grain_cost.py's: every step is a child
process of its own under its own time limit, the parent never opens the device, and after a step that fails or runs out of time it
starts nothing more.  No figure is fixed in advance: the yardsticks are the white-grain and plain arms of the same run.

    paste       three arms on the line's window: paste() without the key, paste(grain=True) and paste(grain=dict(spectrum=True)) (three
                ops.highpass_hist_step instead of two ops.highpass_hist, grain_shape and grain_shaped_gains on the host, ops.grain_shaped
                instead of ops.grain).  The events bracket the host's part too: the device waits for the gains.
    vae         AutoencoderKL.decode_nhwc of the strip's canvas (random-init weights)

The scene's noise is white, so the shape the estimator finds (part of the output) is near (0, 0); the kernels do the same work for every
shape.  The path is opt-in and not part of bench.py.

    python tools/grain_spectrum_cost.py [--scene_sigma 4] [--iters 20] [--out profiles/grain_spectrum_cost.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grain_cost  # noqa: E402  (the same scene, window and timing)

STEPS = ("paste", "vae")


def child(a):
    import torch
    from textflux_amd import paste_back as pb
    dev = torch.device("cuda")
    (W, H) = a.scene
    m, reg = grain_cost.plan(a)
    rw, rh = reg.x1 - reg.x0, reg.y1 - reg.y0
    g = torch.Generator().manual_seed(0)
    strip = int(rw * 0.1667)
    canvas = ((rw // 32) * 32, ((rh + strip) // 32) * 32)
    res = {"window": [rw, rh], "canvas": list(canvas), "device": torch.cuda.get_device_name(0)}
    if a.step == "vae":
        from textflux_amd.vae import AutoencoderKL
        vae = AutoencoderKL().init_random_(seed=7, device=dev)
        z = (torch.randn(1, canvas[1] // 8, canvas[0] // 8, 16, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        arms = {"vae_decode": lambda: vae.decode_nhwc(z)}
        res["vae_weights"] = "random-init"
    else:
        from textflux_amd import ops
        scene = (128 + a.scene_sigma * torch.randn(1, H, W, 3, generator=g)).round().clamp(0, 255).to(torch.uint8).to(dev)
        window = scene[:, reg.y0:reg.y1, reg.x0:reg.x1].contiguous()
        edit = torch.full((1, rh, rw, 3), 124, dtype=torch.uint8).to(dev)
        wmask = torch.from_numpy(np.ascontiguousarray(m[None, reg.y0:reg.y1, reg.x0:reg.x1])).to(dev)
        origin = (reg.x0, reg.y0)
        paste = lambda **kw: pb.paste(window, edit, wmask, a.dilate, a.feather, **kw)
        arms = {"paste_plain": lambda: paste(), "paste_grain": lambda: paste(grain=True, origin=origin),
                "paste_grain_spectrum": lambda: paste(grain=dict(spectrum=True), origin=origin)}
        alpha = pb.alpha_mask(wmask, a.dilate, a.feather)
        ring = pb.ring_mask(alpha, pb.RING)
        h1, h2 = ops.highpass_hist_step(window, ring, 255, 255, 1), ops.highpass_hist_step(window, ring, 255, 255, 2)
        shape = pb.grain_shape(h1, h2, dict(spectrum=True))
        gains = pb.grain_shaped_gains(h1, ops.highpass_hist_step(arms["paste_plain"](), alpha, 255, 255, 1), shape, dict(spectrum=True))
        res.update(shape=shape[0].tolist(), gains=gains[0].tolist())
    res.update(grain_cost.timed_alternating(arms, a.iters, a.warmup))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, nargs=2, default=[2048, 1536], metavar=("W", "H"))
    ap.add_argument("--line", type=int, nargs=2, default=[1024, 256], metavar=("L", "T"), help="the line's length and thickness")
    ap.add_argument("--dilate", type=int, default=16)
    ap.add_argument("--feather", type=int, default=4)
    ap.add_argument("--scene_sigma", type=float, default=4.0, help="standard deviation of the scene's noise in grey levels")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step_timeout", type=int, default=240, help="seconds one step's process may take")
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run this one step in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step is not None:
        return child(a)
    res = {"scene": a.scene, "line": a.line, "dilate": a.dilate, "feather": a.feather, "scene_sigma": a.scene_sigma,
           "iters": a.iters, "warmup": a.warmup}
    for step in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + sys.argv[1:], capture_output=True, text=True,
                               timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} ran out of its {a.step_timeout} s: nothing more is started")
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"step {step} failed with exit status {p.returncode}: nothing more is started")
        res.update(json.loads(lines[-1][len("RESULT "):]))
    med = lambda k: res[k]["median_ms"]
    res["paste_grain_spectrum_over_paste_grain"] = med("paste_grain_spectrum") / med("paste_grain")
    res["paste_grain_spectrum_over_paste_plain"] = med("paste_grain_spectrum") / med("paste_plain")
    res["paste_grain_spectrum_over_vae_decode"] = med("paste_grain_spectrum") / med("vae_decode")
    res["paste_grain_over_vae_decode"] = med("paste_grain") / med("vae_decode")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
