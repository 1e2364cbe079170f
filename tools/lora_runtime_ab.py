"""Cost of RUNTIME (unmerged) LoRA adapters against the merged path, measured on the DiT forward: two random-init full-depth models in
ONE process -- `merged` (the adapter folded into the weights at load: the default path, the baseline) and `runtime` (the same adapter
attached, FluxTransformer2DModel.attach_lora) -- alternating forward by forward, timed with device events.  Geometries: the headline
(1024 x 1024, batch 8: S = 4096, T = 512) and 576 x 512 batch 1 (S = 1152, T = 512).  The adapter is TextFlux's: rank 128 on the twelve
target patterns of scripts/train_lora.py (every attention / feed-forward Linear of the double blocks, to_q / to_k / to_v of the single
blocks).  Next to the measured ratio the tool prints the FLOP overhead the shapes imply (tail + down projection).

    python tools/lora_runtime_ab.py [--geom headline,small] [--iters 20] [--warmup 3] [--layers 19,38] [--out profiles/lora_runtime_ab.json]

Per-kernel split (a run of its own, one configuration per process so that the statistics are that configuration's):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/lora_runtime_ab.py --one merged|runtime|none --geom headline --iters 3
(`none`: no adapter at all -- its kernel names / counts are the parent commit's launch sequence.)"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from textflux_amd import lora as lora_mod
from textflux_amd.transformer import FluxTransformer2DModel

BF = torch.bfloat16
GEOMS = {"headline": (8, 4096, 512, 64), "small": (1, 1152, 512, 32)}          # B, S, T, latent row width (for the ids)
PATTERNS = ["attn.to_k", "attn.to_q", "attn.to_v", "attn.to_out.0", "attn.add_k_proj", "attn.add_q_proj", "attn.add_v_proj",
            "attn.to_add_out", "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2"]


def synthetic_adapter(model, rank, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    sd = {}
    for key, name, _ in model._fusion_map():
        if not key.startswith(("transformer_blocks.", "single_transformer_blocks.")) or not any(key.endswith("." + p) for p in PATTERNS):
            continue
        rows, k_in = model._rows_of(key), model.w[name + ".w"].shape[1]
        sd[f"transformer.{key}.lora_A.weight"] = (torch.randn(rank, k_in, generator=g, device=dev) * 0.02).to(BF)
        sd[f"transformer.{key}.lora_B.weight"] = (torch.randn(rows, rank, generator=g, device=dev) * 0.02).to(BF)
    return sd


def flop_overhead(model, rank):
    """(adapted-Linear FLOPs with the adapter) / (without) - 1 over the block Linears of one forward, per token: tail 2 N R per adapted
    segment's columns, down projection 2 K nseg R (the launch computes every segment's block)."""
    R = (rank + 127) // 128 * 128
    base = extra = 0
    info = model._lora["lin"]
    for k, t in model.w.items():
        if not k.endswith(".w") or not (k[0] in "ds" and k[1].isdigit()):
            continue
        N, K = t.shape
        base += 2 * N * K
        a = info.get(k[:-2])
        if a is not None and a["acat"] is not None:
            p = a["pack"]
            cols = sum((p.seg_cols if s + 1 < p.nseg else N - s * p.seg_cols) for s in range(p.nseg) if p.seg_mask >> s & 1)
            extra += 2 * cols * R + 2 * K * p.nseg * R
    return extra / base


def make_runner(model, geom, dev):
    B, S, T, w = GEOMS[geom]
    ses = model.session(B, S, T)
    g = torch.Generator().manual_seed(0)
    ids = torch.zeros(S, 3)
    ids[:, 1], ids[:, 2] = torch.arange(S) // w, torch.arange(S) % w
    ses.set_conditioning((torch.randn(B, T, model.config.joint_attention_dim, generator=g) * 0.1).to(BF).to(dev), torch.zeros(T, 3), ids)
    ses.xin.copy_(torch.randn(B, S, model.config.in_channels, generator=g).to(BF))
    t, gd = torch.full((B,), 500.0, device=dev), torch.full((B,), 29952.0, device=dev)
    mod = model.modulation(model.temb(t, gd, torch.randn(B, model.config.pooled_projection_dim, generator=g).to(BF).to(dev)))

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ses.run(mod)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geom", default="headline,small")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--layers", default="19,38", help="double,single blocks (full depth by default)")
    ap.add_argument("--one", choices=["merged", "runtime", "none"], default=None, help="run ONE configuration only (under a profiler)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    nd, ns = (int(v) for v in a.layers.split(","))
    kinds = [a.one] if a.one else ["merged", "runtime"]
    models = {}
    for kind in kinds:
        m = FluxTransformer2DModel(in_channels=384, out_channels=64, num_layers=nd, num_single_layers=ns, guidance_embeds=True)
        m.init_random_(seed=1, device=dev)
        if kind != "none":
            sd = synthetic_adapter(m, a.rank, dev)
            if kind == "merged":
                lora_mod.merge_lora_into_transformer(sd, None, m)
            else:
                m.attach_lora("textflux", sd)
        models[kind] = m
    res = {"rank": a.rank, "layers": [nd, ns], "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "geometries": {}}
    if "runtime" in models:
        res["flop_overhead_of_block_linears"] = flop_overhead(models["runtime"], a.rank)
    for geom in a.geom.split(","):
        runs = {k: make_runner(m, geom, dev) for k, m in models.items()}
        for _ in range(a.warmup):
            for r in runs.values():
                r()
        ms = {k: [] for k in runs}
        for _ in range(a.iters):                 # alternating: drift of the board (clock, temperature) hits both alike
            for k, r in runs.items():
                ms[k].append(r())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        entry = {"B_S_T": list(GEOMS[geom][:3]), "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()}}
        if "merged" in med and "runtime" in med:
            entry["runtime_over_merged"] = med["runtime"] / med["merged"]
        res["geometries"][geom] = entry
        print(geom, json.dumps(entry))
        for m in models.values():
            m._session = None                    # the next geometry's workspace replaces this one
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
