"""What read-back costs beside the VAE decode of the same batch (DESIGN.md section 4 "Read-back").  Device events; the two arms ALTERNATE
in one process: every round reads the lines once and decodes the batch once, so a drift of the clocks falls on both alike.  Report-only:
no figure is fixed in advance and no threshold is set; the yardstick is the decode of the same run.

    read        TextRecognizer.read of --lines line crops of 48 x 320 with their targets: the crops' way to the device, tfx_ocr_resize_norm,
                the 61 launches of the recogniser's forward, tfx_ctc_rows, tfx_ctc_score and the decode's way back to the host
                (seeded 'en' weights: the cost does not depend on what the weights say; --lang ch for the 6625-class head)
    forward     the recogniser's forward alone on the resized batch (no host traffic inside the events)
    vae         AutoencoderKL.decode_nhwc of a [lines, 6, 40, 16] latent: the same 48 x 320 pixels per line (random-init weights)

The measuring process is a child of its own under a time limit; the parent never opens the device, and after a child that fails or runs
out of time it starts nothing more.  Default: eight lines, median of 20 rounds after 3 warm-up calls of every arm outside the timed
window.  The path is opt-in and not part of bench.py.

    python tools/ocr_cost.py [--lines 8] [--lang en] [--dict tests/golden/en_dict.txt] [--iters 20] [--out profiles/ocr_cost.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


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


def child(a):
    import torch
    from textflux_amd import ocr
    from textflux_amd.vae import AutoencoderKL
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    crops = [rng.integers(0, 256, (48, 320, 3), dtype=np.uint8) for _ in range(a.lines)]
    n_class = ocr.N_CLASS[a.lang]
    if a.lang == "en":
        chars_path = a.dict
    else:                                                # no character list of that size ships here: numbered stand-ins, the cost is the same
        chars_path = os.path.join(a.tmp, "chars.txt")
        with open(chars_path, "w") as f:
            f.write("\n".join(f"c{i}" for i in range(n_class - 2)) + "\n")
    rec = ocr.TextRecognizer(ocr.create_predictor(None, a.lang, device=dev), chars_path, (3, 48, 320), a.lines)
    targets = ["".join(rec.chars[1 + (7 * i + j) % 60] for j in range(12)) for i in range(a.lines)] if a.lang == "en" else [""] * a.lines
    x = torch.randn(a.lines, 48, 320, 3, device=dev).clamp(-1, 1)
    vae = AutoencoderKL().init_random_(seed=7, device=dev)
    z = (torch.randn(a.lines, 6, 40, 16, generator=torch.Generator().manual_seed(0)) * 0.5).to(torch.bfloat16).to(dev)
    arms = {"read": lambda: rec.read(crops, targets), "forward": lambda: rec.predictor(x), "vae_decode": lambda: vae.decode_nhwc(z)}
    res = {"device": torch.cuda.get_device_name(0), "classes": n_class, "vae_weights": "random-init", "ocr_weights": "seeded"}
    res.update(timed_alternating(arms, a.iters, a.warmup))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=8)
    ap.add_argument("--lang", choices=("en", "ch"), default="en")
    ap.add_argument("--dict", default=os.path.join(REPO, "tests", "golden", "en_dict.txt"), help="the 'en' character list")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step_timeout", type=int, default=240, help="seconds the measuring process may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    ap.add_argument("--tmp", default=None, help="(internal)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import tempfile
    res = {"lines": a.lines, "line_size": [48, 320], "lang": a.lang, "iters": a.iters, "warmup": a.warmup}
    with tempfile.TemporaryDirectory() as tmp:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tmp", tmp] + sys.argv[1:], capture_output=True,
                               text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"the measuring process ran out of its {a.step_timeout} s")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"the measuring process failed with exit status {p.returncode}")
    res.update(json.loads(lines[-1][len("RESULT "):]))
    med = lambda k: res[k]["median_ms"]
    res["read_over_vae_decode"] = med("read") / med("vae_decode")
    res["forward_over_vae_decode"] = med("forward") / med("vae_decode")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
