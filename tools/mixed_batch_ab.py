#!/usr/bin/env python3
"""A/B of mixed-geometry batching (batch_driver.run_items mixed_pad) on one GPU: a 16-item list of about six geometries goes through
run_items several times in ONE process, alternating between

    mixed_pad = 0      same-geometry batches only (the plan and the code path without the feature), and
    a sweep of caps    items of different sizes share a batch while at most that share of its transformer rows is padding
                       (FluxFillPipeline.call_mixed: rows padded to the longest sample, per-sample lengths in attention).

Per arm: images/s (wall clock of the whole run_items call, device synchronised on both sides: VAE, planning, session set-up and
graph captures included -- that is what a caller pays), the share of transformer rows that were padding, the number of batches,
of DiT sessions created and of step graphs captured.  Writes profiles/mixed_batch_ab.json and prints one summary line per arm.

    python tools/mixed_batch_ab.py [--steps 8] [--reps 2] [--caps 0.12 0.2 0.35] [--batch_size 8] [--layers 19 38] [--scenes six|distinct]

The model is the FLUX.1-Fill architecture with random weights (as bench.py), the prompts' embeddings are random stand-ins (no text
encoder is run: it costs the same in every arm), scenes and masks are synthetic."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (scene width, height) x count: with the glyph strip on top and the callers' rounding to multiples of 32 these become six pipeline
# geometries between 576 x 512 and 1024 x 1024, in the proportions of a list where small scenes dominate
SCENES = [((576, 416), 4), ((512, 480), 3), ((640, 512), 3), ((768, 512), 2), ((1024, 672), 2), ((1024, 848), 2)]
# --scenes distinct: sixteen scenes of sixteen sizes -- the regime of a real annos.json, where same-geometry batching means batches of one
DISTINCT = [((512 + 32 * (i % 8), 384 + 32 * ((3 * i) % 11)), 1) for i in range(12)] + [((1024, 640 + 64 * i), 1) for i in range(4)]


def build_pipe(layers, dev):
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
    from textflux_amd.transformer import FluxTransformer2DModel
    from textflux_amd.vae import AutoencoderKL
    tr = FluxTransformer2DModel(in_channels=384, out_channels=64, num_layers=layers[0], num_single_layers=layers[1],
                                guidance_embeds=True).init_random_(seed=1234, device=dev)
    vae = AutoencoderKL().init_random_(seed=7, device=dev)
    sch = FlowMatchEulerDiscreteScheduler(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256,
                                          max_image_seq_len=4096, shift=3.0)
    pipe = FluxFillPipeline(scheduler=sch, vae=vae, text_encoder=None, tokenizer=None, text_encoder_2=None, tokenizer_2=None,
                            transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_graph(True)
    g = torch.Generator().manual_seed(42)
    pe1 = (torch.randn(1, 512, 4096, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    pooled1 = torch.randn(1, 768, generator=g).to(torch.bfloat16).to(dev)

    def encode_prompt(prompt=None, prompt_2=None, device=None, max_sequence_length=512, **kw):
        if kw.get("prompt_embeds") is not None:      # the pipeline calls passing the embeddings through
            return kw["prompt_embeds"], kw.get("pooled_prompt_embeds"), torch.zeros(512, 3, device=dev)
        n = 1 if isinstance(prompt, str) else len(prompt)
        return pe1.expand(n, -1, -1).contiguous(), pooled1.expand(n, -1).contiguous(), torch.zeros(512, 3, device=dev)

    pipe.encode_prompt = encode_prompt
    pipe.encodes_locally = True
    return pipe


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--caps", type=float, nargs="*", default=[0.12, 0.2, 0.35])
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--layers", type=int, nargs=2, default=[19, 38])
    ap.add_argument("--scenes", choices=["six", "distinct"], default="six", help="six geometries (default) or sixteen distinct ones")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mixed_batch_ab.json"))
    a = ap.parse_args()
    from PIL import Image
    from textflux_amd import _lib as L
    from textflux_amd import batch_driver, transformer
    dev = torch.device("cuda", 0)
    pipe = build_pipe(a.layers, dev)

    # ---- the item list: synthetic scenes / masks behind a loader keyed by the "path"
    rng = np.random.RandomState(0)
    store, items = {}, []
    for (w, h), count in (SCENES if a.scenes == "six" else DISTINCT):
        for _ in range(count):
            k = len(items)
            store[f"scene{k}"] = Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8))
            m = np.zeros((h, w, 3), dtype=np.uint8)
            m[h // 3: 2 * h // 3, w // 8: 7 * w // 8] = 255
            store[f"mask{k}"] = Image.fromarray(m)
            items.append(dict(image=f"scene{k}", mask=f"mask{k}", text=f"WORD{k}"))
    order = np.random.RandomState(1).permutation(len(items))       # geometries arrive interleaved, as in a real list
    items = [items[i] for i in order]
    loader = lambda p: store[p]

    # ---- counters: sessions created, step graphs captured
    counts = dict(sessions=0, captures=0)
    init0 = transformer.DitSession.__init__

    def init1(self, *args, **kw):
        counts["sessions"] += 1
        return init0(self, *args, **kw)

    transformer.DitSession.__init__ = init1
    lib = L.lib()
    cap0 = lib.tfx_dit_step_capture_ex3

    class _Lib:       # the pipeline's graph loop calls lib.tfx_dit_step_capture_ex3: count it on the way through
        def __getattr__(self, name):
            return getattr(lib, name)

        def tfx_dit_step_capture_ex3(self, *args):
            counts["captures"] += 1
            return cap0(*args)

    L._lib = _Lib()

    def plan_stats(cap):
        works = [batch_driver.prepare_item(i, it, loader, device_compose=bool(getattr(pipe, "supports_device_compose", False)))
                 for i, it in enumerate(items)]
        plan = batch_driver.plan_batches(works, a.batch_size, cap, text_tokens=512)
        rows = valid = 0
        for b in plan:
            lens = [512 + batch_driver.image_tokens(w.size) for w in b.items]
            n = (max(lens) + 255) // 256 * 256 if b.mixed else max(lens)
            rows += n * len(lens)
            valid += sum(lens)
        return dict(batches=len(plan), mixed_batches=sum(b.mixed for b in plan), pad_fraction=1 - valid / rows,
                    geometries=sorted({w.size for w in works}), batch_sizes=[len(b.items) for b in plan])

    def run(cap):
        pipe.transformer._session = None           # every arm starts without a session: set-up and captures are part of its cost
        counts.update(sessions=0, captures=0)
        torch.cuda.synchronize()
        t0 = time.time()
        res = batch_driver.run_items(items, pipe, None, batch_size=a.batch_size, num_inference_steps=a.steps, seed=42, device=dev,
                                     loader=loader, save=lambda i, img: None, mixed_pad=cap)
        torch.cuda.synchronize()
        dt = time.time() - t0
        if res["failed"]:
            raise SystemExit(f"cap {cap}: items {res['failed']} failed")
        return dict(seconds=dt, images_per_s=len(items) / dt, sessions=counts["sessions"], captures=counts["captures"])

    arms = [0.0] + [c for c in a.caps if c > 0]
    out = dict(items=len(items), scenes=a.scenes, steps=a.steps, batch_size=a.batch_size, layers=a.layers, arms={})
    for cap in arms:
        out["arms"][str(cap)] = dict(plan_stats(cap), runs=[])
    run(arms[-1])                                   # warm-up: kernels loaded, LDS limits set, allocator pools filled
    for rep in range(a.reps):
        for cap in arms:                            # alternating: drift of the box hits every arm alike
            r = run(cap)
            out["arms"][str(cap)]["runs"].append(r)
            print(f"rep {rep} cap {cap}: {r['images_per_s']:.3f} images/s, {r['seconds']:.2f} s, {r['sessions']} sessions, "
                  f"{r['captures']} captures", flush=True)
    base = np.median([r["images_per_s"] for r in out["arms"]["0.0"]["runs"]])
    for cap in arms:
        arm = out["arms"][str(cap)]
        arm["images_per_s"] = float(np.median([r["images_per_s"] for r in arm["runs"]]))
        arm["vs_cap_0"] = arm["images_per_s"] / base
        print(f"cap {cap}: {arm['images_per_s']:.3f} images/s ({arm['vs_cap_0']:.3f} x cap 0), pad fraction {arm['pad_fraction']:.3f}, "
              f"{arm['batches']} batches ({arm['mixed_batches']} mixed), captures {arm['runs'][-1]['captures']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, default=str)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
