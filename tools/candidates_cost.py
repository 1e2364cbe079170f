"""What best-of-N costs through the batch driver (DESIGN.md section 4 "Candidates").  Device events around whole run_items calls; the
three arms ALTERNATE in one process, so a drift of the clocks falls on all alike.  Report-only: no figure is fixed in advance and no
threshold is set.

    loop        what a caller does without the key: N run_items runs of the item with seeds s .. s + N - 1, each with ocr= (N batches of
                one, N reads of the final image)
    candidates  one run with candidates=N (one batch of N, one gather launch and one read for all of them, the winner alone is converted)
    pruned      one run with candidates=dict(n=N, prune=dict(at=steps // 3, keep=1)): steps // 3 steps on N samples, N previews decoded and
                read, the rest of the schedule on one sample -- (N p + K (n - p)) / (N n) of the unpruned steps

and, beside them, the two ways to read eight 48 x 320 lines that lie in device images:

    read          today's route: ocr.crop_line per line, then TextRecognizer.read, which takes every crop to the host and back
    read_device   TextRecognizer.read_device: one table upload, one gather launch, no crop leaves the device

Full depth, random weights (as bench.py), Euler, step graphs on, random stand-ins for the prompt embeddings (no text encoder runs: it
costs the same in every arm), seeded 'en' recogniser weights -- the cost does not depend on what the weights say, and no statement about
WHICH candidate wins is made.  The measuring process is a child of its own under a time limit; the parent never opens the device, and
after a child that fails or runs out of time it starts nothing more.  Default: N = 4, 30 steps, a 512 x 512 scene (a 512 x 576 canvas:
1152 image tokens), median of 20 rounds after one warm-up round outside the timed window.  The path is opt-in and not part of bench.py.

    python tools/candidates_cost.py [--n 4] [--steps 30] [--iters 20] [--out profiles/candidates_cost.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def child(a):
    import torch
    from mixed_batch_ab import build_pipe
    from ocr_cost import timed_alternating
    from textflux_amd import batch_driver, glyph
    from textflux_amd import candidates as cd
    from textflux_amd import ocr
    dev = torch.device("cuda", 0)
    pipe = build_pipe(a.layers, dev)
    scene, mask, words = glyph.synthetic_case(a.scene[0], a.scene[1])
    item = dict(image="s", mask="m", text=words[0])
    load = lambda p: scene if p == "s" else mask
    cfg = dict(weights=None, lang="en", dict_path=a.dict)
    reader = ocr.make_reader(ocr.ocr_cfg(cfg), dev)
    real = ocr.make_reader
    ocr.make_reader = lambda c, device="cuda": reader          # one recogniser for every run: its construction is not what is compared
    p = max(1, a.steps // 3)
    size = batch_driver.prepare_item(0, item, load).size

    def run(seed=42, **kw):
        res = batch_driver.run_items([item], pipe, None, batch_size=max(8, a.n), num_inference_steps=a.steps, seed=seed, device=dev, loader=load,
                                     save=lambda i, img: None, ocr=cfg, **kw)
        if res["failed"]:
            raise SystemExit(f"the run failed: {res}")
        return res

    arms = {"loop": lambda: [run(seed=42 + k) for k in range(a.n)],
            "candidates": lambda: run(candidates=a.n),
            "pruned": lambda: run(candidates=dict(n=a.n, prune=dict(at=p, keep=1)))}
    res = {"device": torch.cuda.get_device_name(0), "weights": "random-init", "ocr_weights": "seeded", "layers": a.layers, "step_graphs": True,
           "pipeline_size": list(size), "image_tokens": batch_driver.image_tokens(size), "prune_at": p,
           "pruned_share_of_steps": cd.pruned_steps(a.n, a.steps, p, 1)}
    try:
        res["runs"] = timed_alternating(arms, a.iters, 1)
        # the reads alone: eight lines of 48 x 320 inside device images
        rng = np.random.default_rng(0)
        images = torch.from_numpy(rng.integers(0, 256, (8, 64, 352, 3), dtype=np.uint8)).to(dev)
        m = np.zeros((64, 352), np.uint8)
        m[8:57, 16:337] = 255                                   # the minimum-area rectangle of 49 x 321 pixels is a 48 x 320 crop
        lines = [(b, m) for b in range(8)]
        targets = ["".join(reader.chars[1 + (7 * i + j) % 60] for j in range(12)) for i in range(8)]
        assert tuple(ocr.crop_line(images[0], m).shape) == (48, 320, 3)
        res["reads"] = timed_alternating({"read": lambda: reader.read([ocr.crop_line(images[b], s) for b, s in lines], targets),
                                          "read_device": lambda: reader.read_device(images, lines, targets)}, a.iters, 3)
    finally:
        ocr.make_reader = real
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4, help="candidates per edit")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--scene", type=int, nargs=2, default=[512, 512], metavar=("W", "H"))
    ap.add_argument("--layers", type=int, nargs=2, default=[19, 38])
    ap.add_argument("--dict", default=os.path.join(REPO, "tests", "golden", "en_dict.txt"), help="the 'en' character list")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step_timeout", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"n": a.n, "steps": a.steps, "scene": a.scene, "iters": a.iters, "warmup_rounds": 1}
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], capture_output=True, text=True,
                           timeout=a.step_timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measuring process ran out of its {a.step_timeout} s")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"the measuring process failed with exit status {p.returncode}")
    res.update(json.loads(lines[-1][len("RESULT "):]))
    med = lambda k: res["runs"][k]["median_ms"]
    res["candidates_over_loop"] = med("candidates") / med("loop")
    res["pruned_over_loop"] = med("pruned") / med("loop")
    res["pruned_over_candidates"] = med("pruned") / med("candidates")
    res["read_device_over_read"] = res["reads"]["read_device"]["median_ms"] / res["reads"]["read"]["median_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
