"""What the keyed paste costs beside today's paste of the same window and the VAE decode it follows (DESIGN.md section 4 "Keyed paste").
Device events; the two paste arms ALTERNATE in one process: every round runs paste(keyed=...) and the same paste() call without the key
once, so a drift of the clocks falls on both alike.  Report-only: no figure is fixed in advance and no threshold is set; the yardsticks
are the plain arm of the same run (that path does not change with the key) and the decode.

    paste       the whole paste on the line's window (alpha_mask, ops.overlay, then ring_mask, ops.highpass_hist and the histogram's way
                to the host for the scene's noise level, ops.change_metric, ops.hysteresis -- one launch and one read-back per round --,
                ops.mask_dilate, ops.mask_feather, ops.overlay) beside the plain paste (alpha_mask, ops.overlay).  The events bracket
                the host's part too: the device waits for the thresholds, and the host for every round's word.
    vae         AutoencoderKL.decode_nhwc of the strip's canvas: the glyph strip stacked on the window's crop (random-init weights)

The scene is the grain match's: a flat grey plus Gaussian noise of --scene_sigma grey levels in a window of the same size.  The edit is
the clean grey with dark bars drawn across the line (--bars of them, a "text"), so the key has strokes to keep and background to give
back; the noise level, the thresholds, the hysteresis' round count and the share of the mask that keeps the scene's byte are part of the
output.  Every step is a child process of its own under its own time limit; the parent never opens the device, and after a step that
fails or runs out of time it starts nothing more.  Default: a 1024 x 256 line in a 2048 x 1536 scene, batch 1, dilate 16, feather 4, pad
0, the default keyed configuration, median of 20 rounds after 3 warm-up calls of every arm outside the timed window.  The path is opt-in
and not part of bench.py.

    python tools/keyed_paste_cost.py [--scene_sigma 4] [--bars 24] [--iters 20] [--out profiles/keyed_paste_cost.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = ("paste", "vae")


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
    """The line's mask and the window (the region of the per-line path, pad 0) it is pasted into (host only)."""
    from textflux_amd import paste_back as pb
    (W, H), (L, T) = a.scene, a.line
    m = np.zeros((H, W), np.uint8)
    m[(H - T) // 2:(H - T) // 2 + T, (W - L) // 2:(W - L) // 2 + L] = 255
    return m, pb.select_region(m, a.dilate, a.feather, pad=0.0, min_side=96, max_side=1 << 30)


def child(a):
    import torch
    from textflux_amd import paste_back as pb
    dev = torch.device("cuda")
    (W, H) = a.scene
    m, reg = plan(a)
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
        edit = torch.full((1, rh, rw, 3), 124, dtype=torch.uint8)
        (L, T), x0, y0 = a.line, (rw - a.line[0]) // 2, (rh - a.line[1]) // 2
        for k in range(a.bars):                          # upright bars a sixteenth of the line's thickness wide, spread over its length
            x = x0 + (2 * k + 1) * L // (2 * a.bars)
            edit[:, y0 + T // 8:y0 + T - T // 8, x:x + max(T // 16, 1)] = 30
        edit = edit.to(dev)
        wmask = torch.from_numpy(np.ascontiguousarray(m[None, reg.y0:reg.y1, reg.x0:reg.x1])).to(dev)
        arms = {"paste_keyed": lambda: pb.paste(window, edit, wmask, a.dilate, a.feather, keyed=True),
                "paste_plain": lambda: pb.paste(window, edit, wmask, a.dilate, a.feather)}
        alpha = pb.alpha_mask(wmask, a.dilate, a.feather)
        sigma = float(pb.keyed_sigma(ops.highpass_hist(window, pb.ring_mask(alpha, pb.RING)))[0])
        lo_eff, hi_eff = pb.keyed_levels(True, sigma)
        plain = arms["paste_plain"]()
        marks, rounds = ops.hysteresis(ops.change_metric(plain, window), lo_eff, hi_eff, rounds=True)
        key = pb.change_key(window, plain, True, sigma)
        inside = wmask >= 128
        res.update(sigma_scene=sigma, lo_eff=lo_eff, hi_eff=hi_eff, hysteresis_rounds=rounds, marked_pixels=int((marks == 255).sum()),
                   mask_pixels=int(inside.sum()), mask_share_keeping_the_scene=float(((key == 0) & inside).sum()) / float(inside.sum()))
    res.update(timed_alternating(arms, a.iters, a.warmup))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, nargs=2, default=[2048, 1536], metavar=("W", "H"))
    ap.add_argument("--line", type=int, nargs=2, default=[1024, 256], metavar=("L", "T"), help="the line's length and thickness")
    ap.add_argument("--dilate", type=int, default=16)
    ap.add_argument("--feather", type=int, default=4)
    ap.add_argument("--scene_sigma", type=float, default=4.0, help="standard deviation of the scene's noise in grey levels")
    ap.add_argument("--bars", type=int, default=24, help="dark bars the edit draws across the line")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step_timeout", type=int, default=240, help="seconds one step's process may take")
    ap.add_argument("--step", choices=STEPS, default=None, help="(internal) run this one step in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step is not None:
        return child(a)
    res = {"scene": a.scene, "line": a.line, "dilate": a.dilate, "feather": a.feather, "scene_sigma": a.scene_sigma, "bars": a.bars,
           "iters": a.iters, "warmup": a.warmup}
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
    res["paste_keyed_over_paste_plain"] = med("paste_keyed") / med("paste_plain")
    res["paste_keyed_over_vae_decode"] = med("paste_keyed") / med("vae_decode")
    res["paste_plain_over_vae_decode"] = med("paste_plain") / med("vae_decode")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
