#!/usr/bin/env python3
"""Headline benchmark: images/sec of FluxFillPipeline.__call__ at 1024x1024, 30 Euler steps, bf16, batch 8 per GPU
(BASELINE.json metric; FLUX.1-Fill architecture, random-init weights, synthetic image/mask, injected prompt embeds).

    python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run, one rank per GPU)

One "step" = one full pipeline call on one batch: VAE encode of the masked image, 30 denoising steps of the 12 B-param
DiT (hand-written HIP: MFMA GEMMs, flash attention, fused norms / scheduler), VAE decode.  Inputs are resident in HBM
before the timed region.  Rank 0 prints ONE JSON line (contract in the task description).  A plain run does only what the
headline needs: set-up, W warm-up calls, K timed calls, the result line.

    --dump-outputs DIR : after the timed calls, the images the last timed call returned, as float32 / float64 .npy files under DIR
                         (a fixed, seeded sample of them when the whole batch would not fit in 48 MiB); inputs are seeded, so two
                         builds can be compared output for output
    --full             : also the untimed extras, each its own measurement, added to the same line:
      roofline     : MFMA roofline of the dominant kernel (gemm8p), measured live with HIP events on its launch stream, the attention
                     kernel forms of one eager call, one call with the attention score bound ignored, the pil-vs-pt output delta and
                     the live MFMA-only peak probe
      cpu_baseline : the CPU oracle (plain PyTorch restatement, `oracle/`) timed LIVE on this box's host cores: BASELINE config 1 in full
                     (576x512, 4 steps, fp32, 57 blocks: ~2 min in a subprocess that overlaps model init / warm-up and ends before the
                     timed region) + a bounded block sample at the GPU workload's own token count
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

D, T_TXT = 3072, 512
MFMA_PEAK_TFLOPS = 2500.0  # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md


def dit_flops(S: int) -> float:
    """Algorithmic FLOPs of one transformer forward for one image."""
    N = S + T_TXT
    return 57 * (24 * D * D * N + 4 * N * N * D) + 2 * (384 * D * S + 4096 * D * T_TXT + 64 * D * S)


def _cpu_budget() -> int:
    """Host CPUs this process may use: its affinity mask, capped by OMP_NUM_THREADS when that is set (on a shared host both can be
    far below os.cpu_count(), and a thread pool sized by the machine's count only slows itself down)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        n = min(n, int(os.environ.get("OMP_NUM_THREADS", n)))
    except ValueError:
        pass
    return max(1, n)


def cpu_baseline(height, width, steps, budget_s=25.0):
    """Oracle double + single block (full width, fp32) at this workload's token count, timed on the host cores and
    extrapolated: s/img = steps * (19 t_double + 38 t_single).  A reported baseline, not a target."""
    from oracle import flux_oracle as fo
    from oracle import pipeline_oracle as po
    S = (height // 16) * (width // 16)
    # pick the thread count that is actually fastest on this box for the dominant op shape (oversubscribing every
    # logical CPU is several times slower than ~1 thread per physical core on large hosts); ~2 s of calibration
    ncpu = _cpu_budget()
    xa, wa = torch.randn(S + T_TXT, D), torch.randn(4 * D, D)
    best_t, best_n = float("inf"), ncpu
    for nthr in sorted({ncpu, max(1, ncpu // 2), max(1, ncpu // 4), min(ncpu, 64), min(ncpu, 32)}, reverse=True):
        torch.set_num_threads(nthr)
        torch.nn.functional.linear(xa, wa)
        t1 = time.time()
        torch.nn.functional.linear(xa, wa)
        dt = time.time() - t1
        if dt < best_t:
            best_t, best_n = dt, nthr
    torch.set_num_threads(best_n)
    del xa, wa
    cfg = fo.FluxConfig(num_layers=1, num_single_layers=1)
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(s, generator=g) * 0.02 for k, s in fo.state_dict_shapes(cfg).items()
          if k.startswith(("transformer_blocks.0", "single_transformer_blocks.0"))}
    hidden, enc, temb = torch.randn(1, S, D, generator=g), torch.randn(1, T_TXT, D, generator=g), torch.randn(1, D, generator=g)
    ids = torch.cat([torch.zeros(T_TXT, 3), po.latent_image_ids(height // 16, width // 16)], 0)
    cos, sin = fo.flux_pos_embed(ids)
    t0 = time.time()
    with torch.no_grad():
        fo.double_block(sd, "transformer_blocks.0", 24, hidden, enc, temb, cos, sin)  # warm-up (thread pool, allocs)
        t1 = time.time()
        fo.double_block(sd, "transformer_blocks.0", 24, hidden, enc, temb, cos, sin)
        t_d = time.time() - t1
        joint = torch.cat([enc, hidden], 1)
        t2 = time.time()
        fo.single_block(sd, "single_transformer_blocks.0", 24, joint, temb, cos, sin)
        t_s = time.time() - t2
        # fill the rest of the budget with repeats in the model's own 1 : 2 ratio of block kinds and take the means (a single timing of
        # a 1-2 s block on a shared host is noisy): about 10-20 s of host work in all
        reps = int(max(0, min(6, (0.6 * budget_s - (time.time() - t0)) // max(t_d + 2 * t_s, 1e-3))))
        td, ts = [t_d], [t_s]
        for _ in range(reps):
            t1 = time.time()
            fo.double_block(sd, "transformer_blocks.0", 24, hidden, enc, temb, cos, sin)
            td.append(time.time() - t1)
            for _ in range(2):
                t2 = time.time()
                fo.single_block(sd, "single_transformer_blocks.0", 24, joint, temb, cos, sin)
                ts.append(time.time() - t2)
        t_d, t_s = sum(td) / len(td), sum(ts) / len(ts)
    s_img = steps * (19 * t_d + 38 * t_s)
    return {"value": 1.0 / s_img, "unit": "images/sec", "cores": best_n, "kind": "port",
            "sample": f"oracle/flux_oracle.py fp32: {len(td)} double-block ({t_d:.2f} s mean) + {len(ts)} single-block ({t_s:.2f} s mean) executions at full "
                      f"width (D=3072, N={S + T_TXT}, B=1) after warm-up on {best_n} threads (fastest of a 5-point sweep; {ncpu} CPUs available); "
                      f"extrapolated s/img = {steps} x (19 t_d + 38 t_s) = {s_img:.0f} s (VAE/text encoders excluded); "
                      f"sample wall {time.time() - t0:.0f} s"}


def cpu_baseline_c1(steps=4):
    """BASELINE.md section 3 / BASELINE.json config 1, as specified: SL512 (576 x 512, S = 1152, N = 1664), batch 1, 4 Euler
    steps, fp32, guidance 30, the FULL 19 + 38 block model on the host cores (oracle/pipeline_oracle.denoise), embeddings /
    latents injected.  ~50 GB of host RAM and minutes of CPU time: run once per round with `bench.py --cpu-baseline-c1`
    and committed under profiles/; a `bench.py --full` line carries the bounded sample above plus this record."""
    from oracle import flux_oracle as fo
    from oracle import pipeline_oracle as po
    # BASELINE.md asks for set_num_threads(os.cpu_count()); on this box's 256 logical CPUs (SMT) that oversubscription is
    # pathologically slow (a first attempt did not finish one forward in 20 minutes), so the thread count is the fastest of
    # a short sweep on the dominant op shape, as in cpu_baseline() above, within the CPUs this process may use
    ncpu = _cpu_budget()
    xa, wa = torch.randn(1664, D), torch.randn(4 * D, D)
    best_t, best_n = float("inf"), ncpu
    for nthr in sorted({max(1, ncpu // 2), max(1, ncpu // 4), min(ncpu, 64), min(ncpu, 32)}, reverse=True):
        torch.set_num_threads(nthr)
        torch.nn.functional.linear(xa, wa)
        t1 = time.time()
        torch.nn.functional.linear(xa, wa)
        if time.time() - t1 < best_t:
            best_t, best_n = time.time() - t1, nthr
    torch.set_num_threads(best_n)
    print(f"[c1] {best_n} threads", file=sys.stderr, flush=True)
    cfg = fo.FluxConfig()
    one = fo.seeded_state_dict(fo.FluxConfig(num_layers=1, num_single_layers=1), 0)
    sd = {}
    for k, v in one.items():     # every layer gets its own copy of the seeded block (47.6 GB resident, streamed per forward)
        if k.startswith("transformer_blocks.0."):
            for i in range(cfg.num_layers):
                sd[f"transformer_blocks.{i}." + k[len("transformer_blocks.0."):]] = v.clone()
        elif k.startswith("single_transformer_blocks.0."):
            for j in range(cfg.num_single_layers):
                sd[f"single_transformer_blocks.{j}." + k[len("single_transformer_blocks.0."):]] = v.clone()
        else:
            sd[k] = v
    H, W = 576, 512
    S = (H // 16) * (W // 16)
    g = torch.Generator().manual_seed(1)
    lat = torch.randn(1, S, 64, generator=g)
    mil = torch.cat([torch.randn(1, S, 64, generator=g), (torch.randn(1, S, 256, generator=g) > 0).float()], -1)
    pe, pooled = torch.randn(1, T_TXT, 4096, generator=g) * 0.1, torch.randn(1, 768, generator=g)
    print("[c1] weights resident", file=sys.stderr, flush=True)
    with torch.no_grad():
        t0 = time.time()
        po.denoise(sd, cfg, lat, mil, pe, pooled, H // 16, W // 16, steps, 30.0, max_steps=1)      # warm-up forward
        t_warm = time.time() - t0
        print(f"[c1] warm-up forward {t_warm:.1f} s", file=sys.stderr, flush=True)
        t0 = time.time()
        po.denoise(sd, cfg, lat, mil, pe, pooled, H // 16, W // 16, steps, 30.0)
        t = time.time() - t0
    return {"config": "C1: SL512 576x512 (S=1152, N=1664), batch 1, 4 Euler steps, fp32, full 19+38-block model, oracle/pipeline_oracle.denoise",
            "threads": torch.get_num_threads(), "logical_cpus": os.cpu_count(), "warmup_forward_s": t_warm, "loop_s": t,
            "s_per_step": t / steps, "s_per_img": t, "images_per_sec": 1.0 / t,
            "cpu_tflops": steps * dit_flops(S) / t / 1e12}


def _transport():
    """What the collectives of this run travelled on: 'RCCL' for the nccl backend (the driver's launch), otherwise the backend's name."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return "RCCL"            # no group at N = 1 without a launcher: the string describes the N > 1 design
    return "RCCL" if dist.get_backend() == "nccl" else dist.get_backend()


DUMP_WHOLE_BYTES = 48 << 20    # --dump-outputs writes the whole batch up to this size, a sample of it above
DUMP_SAMPLE = 1 << 22          # elements of that sample (16 MiB of float32)


def dump_outputs(dirname, images, rank, world):
    """--dump-outputs: the images the last timed call returned (B x 3 x H x W, what a caller of pipe(output_type="pt") receives).
      images.npy               float32, the whole batch when it fits in DUMP_WHOLE_BYTES; otherwise
      images_sample.npy        float32, DUMP_SAMPLE elements of the flattened batch at sorted positions drawn with seed 0
      images_channel_mean.npy  float64 B x 3, every image's per-channel mean over ALL its pixels
    In a multi-GPU run, ranks other than 0 add _rank<r> to the names."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    sfx = "" if rank == 0 else f"_rank{rank}"
    x = images.detach()
    if x.numel() * 4 <= DUMP_WHOLE_BYTES:
        np.save(os.path.join(dirname, f"images{sfx}.npy"), x.float().cpu().numpy())
    else:
        idx = torch.randint(0, x.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
        np.save(os.path.join(dirname, f"images_sample{sfx}.npy"), x.reshape(-1)[idx.to(x.device)].float().cpu().numpy())
    np.save(os.path.join(dirname, f"images_channel_mean{sfx}.npy"),
            x.mean(dim=tuple(range(2, x.dim())), dtype=torch.float64).cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU per pipeline call")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--denoise-steps", type=int, default=30)
    ap.add_argument("--sampler", choices=["euler", "amo"], default="euler")
    ap.add_argument("--layers", type=int, nargs=2, default=[19, 38], help=argparse.SUPPRESS)  # debugging only
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pil-delta", action="store_true", help="skip the untimed output_type='pil' vs 'pt' comparison")
    ap.add_argument("--no-peak-probe", action="store_true", help="skip the live MFMA-only probes (tfx_mfma_peak_probe, ~5 s): profiler passes use it so that the probe kernels stay out of the trace")
    ap.add_argument("--no-attention-ab", action="store_true", help="skip the untimed call with the attention score bound ignored (attention_use_bound=0)")
    ap.add_argument("--cpu-baseline-c1", action="store_true", help="only run BASELINE config 1 on the host cores (minutes, ~50 GB RAM) and print it")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of per-step hipGraph replay")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE", help=argparse.SUPPRESS)  # tuning knobs (tfx_set_option)
    ap.add_argument("--no-text-encoders", action="store_true", help="inject fixed prompt embeddings instead of running T5-XXL / CLIP-L per call")
    ap.add_argument("--fp8", action="store_true", help="BASELINE config 5: e4m3 block linears on the fp8 MFMA (NOT the bf16 headline)")
    ap.add_argument("--full", action="store_true", help="also the untimed extras (live CPU baseline, roofline sample call, attention A/B, "
                    "pil delta, MFMA peak probe; the --no-* options above switch single ones off); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the images of the last timed call to DIR/<name>.npy (float32 / float64)")
    a = ap.parse_args()
    if a.cpu_baseline_c1:
        # (first the bounded sample of the GPU workload's own geometry -- one double + one single block at P1024's token count,
        # extrapolated -- while the host memory is still free, then C1 proper)
        sample = cpu_baseline(a.height, a.width, a.denoise_steps, budget_s=10.0)
        print(json.dumps({"cpu_baseline_c1": cpu_baseline_c1(), "workload_block_sample": sample}), flush=True)
        return

    from textflux_amd import distributed as tdist
    tdist.respawn_under_torchrun(a.gpus, __file__, sys.argv[1:])   # bare `python bench.py --gpus N`: one rank per GPU
    # cpu_baseline (rank 0 at N = 1 only): BASELINE.md section 3's C1 run, LIVE (round 6) -- its own process on the host cores, started
    # here so that its ~2 minutes (47.6 GB of fp32 weights, a warm-up forward, 4 steps) overlap the model initialisation and the UNTIMED
    # warm-up calls of this process; it is waited for BEFORE the timed region starts, so the timed calls have the host to themselves.
    c1_proc = None
    if int(os.environ.get("RANK", "0")) == 0 and a.gpus == 1 and a.full and not a.no_cpu_baseline:
        import subprocess
        c1_proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-baseline-c1"], stdout=subprocess.PIPE,
                                   stderr=subprocess.DEVNULL, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
        t_c1_start = time.time()
    from textflux_amd import ops
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler, StochasticRFOvershotDiscreteScheduler
    from textflux_amd.transformer import FluxTransformer2DModel
    from textflux_amd.vae import AutoencoderKL

    rank, world, local = tdist.init_from_env()
    for kv in a.option:
        name, _, val = kv.partition("=")
        ops.set_option(name, int(val))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus} "
                         "(or without a launcher: bench.py re-executes itself under torch.distributed.run)")
    dev = torch.device("cuda", local)
    B, H, W, n = a.batch, a.height, a.width, a.denoise_steps
    S = (H // 16) * (W // 16)
    full = a.layers == [19, 38]

    # ---- model: FLUX.1-Fill architecture, random-init on the device (no checkpoints offline).  Throughput depends on the VALUES in one
    # place only: the attention stream each block's q / k RMSNorm weights admit (reported as roofline.attention.modes, with the call time
    # of the other stream beside it); matrix-core power, and with it the clock, also depends on operand entropy -- random data is the worst case
    tr = FluxTransformer2DModel(in_channels=384, out_channels=64, num_layers=a.layers[0], num_single_layers=a.layers[1],
                                guidance_embeds=True).init_random_(seed=1234 + rank, device=dev)
    vae = AutoencoderKL().init_random_(seed=7, device=dev)
    sched_cfg = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256,
                     max_image_seq_len=4096, shift=3.0)
    if a.sampler == "euler":
        sch = FlowMatchEulerDiscreteScheduler(**sched_cfg)
    else:
        sch = StochasticRFOvershotDiscreteScheduler(**sched_cfg)
        sch.set_c(2.0)
        sch.set_overshot_func(lambda t, dt: t + dt)
    # text encoders at their real geometry (T5-XXL: 24 x d_model 4096 / 64 heads / d_ff 10240, 4.7 B parameters; CLIP-L: 12 x 768),
    # random-init; the tokenizers' vocabulary files are not available offline, so token ids come from a stand-in tokenizer
    # (host string processing is not what is measured).  Every rank holds a T5 (9.5 GB of 288 GB) and encodes the prompts of
    # ITS OWN images; the CLIP prompt is one fixed template for every image: rank 0 encodes it, RCCL broadcasts the pooled
    # embedding (multi-GPU) -- no rank does another rank's work, no rank waits for more than that broadcast.
    te = te2 = tok = tok2 = None
    use_te = not a.no_text_encoders
    if use_te:
        from types import SimpleNamespace

        class _Tok:
            def __init__(self, n, vocab):
                self.model_max_length, self.vocab = n, vocab

            def __call__(self, prompts, padding=None, max_length=None, truncation=None, return_tensors=None, **kw):
                rows = []
                for p in prompts:
                    gtok = torch.Generator().manual_seed(sum(p.encode()) % 100003)
                    n = min(max_length - 1, 20 + len(p) // 4)
                    r = torch.randint(3, self.vocab - 1, (max_length,), generator=gtok)
                    r[n] = self.vocab - 1           # EOS (largest id: CLIP's legacy pooling position)
                    r[n + 1:] = 0                   # padding
                    rows.append(r)
                return SimpleNamespace(input_ids=torch.stack(rows))

        tok, tok2 = _Tok(77, 49408), _Tok(512, 32128)
        from textflux_amd.text_encoders import CLIPTextModel, T5EncoderModel
        if rank == 0:
            te = CLIPTextModel(dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                    num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu",
                                    eos_token_id=2)).init_random_(seed=11, device=dev)
        te2 = T5EncoderModel(dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64,
                                  feed_forward_proj="gated-gelu")).init_random_(seed=12, device=dev)
    pipe = FluxFillPipeline(scheduler=sch, vae=vae, text_encoder=te, tokenizer=tok, text_encoder_2=te2,
                            tokenizer_2=tok2, transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_graph(not a.no_graph)
    if a.fp8:
        tr.enable_fp8()

    # ---- synthetic inputs, resident in HBM.  Conditioning is produced on rank 0 and broadcast over RCCL/xGMI
    g = torch.Generator().manual_seed(42)
    pe = pooled = None
    if rank == 0:
        pe = (torch.randn(1, T_TXT, 4096, generator=g) * 0.1).to(torch.bfloat16)
        pooled = torch.randn(1, 768, generator=g).to(torch.bfloat16)
    pe, pooled = tdist.broadcast_conditioning(pe, pooled, (1, T_TXT, 4096), (1, 768), torch.bfloat16, dev)
    pe, pooled = pe.expand(B, -1, -1).contiguous(), pooled.expand(B, -1).contiguous()
    gi = torch.Generator().manual_seed(100 + rank)
    image = torch.rand(B, 3, H, W, generator=gi).to(dev)
    mask = torch.zeros(B, 1, H, W, device=dev)
    mask[:, :, H // 4: 3 * H // 4, W // 8: 7 * W // 8] = 1.0
    gen = torch.Generator(device=dev).manual_seed(42 + rank)

    from textflux_amd import glyph
    prompts2 = [glyph.generate_prompt([f"WORD{rank}{i}"]) for i in range(B)]     # one T5 prompt per image, one fixed CLIP prompt

    def one_call():
        pe_c, pooled_c = pe, pooled
        if use_te:     # inside the timed region: the CLIP template on rank 0 -> RCCL broadcast; B T5-XXL prompts on every rank
            with torch.no_grad():
                pooled_c = pipe._get_clip_prompt_embeds([glyph.PROMPT_TEMPLATE2], 1, dev) if rank == 0 else None
                pooled_c = tdist.broadcast_tensor(pooled_c, (1, 768), torch.bfloat16, dev).expand(B, -1).contiguous()
                pe_c = pipe._get_t5_prompt_embeds(prompts2, 1, T_TXT, dev)
        return pipe(prompt_embeds=pe_c, pooled_prompt_embeds=pooled_c, image=image, mask_image=mask, height=H, width=W,
                    num_inference_steps=n, guidance_scale=30.0, generator=gen, output_type="pt").images

    for _ in range(a.warmup):
        one_call()
    torch.cuda.synchronize()
    c1_rec = None
    if c1_proc is not None:      # the host-side baseline finishes before anything is timed
        try:     # at most 6 minutes from its start, so that a --full run ends within 10 minutes
            c1_out, _ = c1_proc.communicate(timeout=max(1.0, 360.0 - (time.time() - t_c1_start)))
        except Exception:            # a host that cannot finish C1 in 6 minutes must not hold the GPU measurement
            c1_proc.kill()
            c1_out = ""
        try:
            c1_json = json.loads(c1_out.strip().splitlines()[-1])
            c1_rec = c1_json["cpu_baseline_c1"]
            c1_rec["workload_block_sample"] = c1_json.get("workload_block_sample")
            c1_rec["wall_s_incl_weights_and_warmup"] = time.time() - t_c1_start
        except Exception as e:   # reported, never fatal for the GPU measurement
            c1_rec = {"error": f"C1 subprocess: rc {c1_proc.returncode}, {type(e).__name__}: {e}"}
    tdist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.steps):
        out = one_call()
    torch.cuda.synchronize()
    own = time.perf_counter() - t0        # this rank's own K calls, before it waits for the others (diagnostics only)
    tdist.barrier()
    torch.cuda.synchronize()
    elapsed = tdist.max_over_ranks(time.perf_counter() - t0, dev)
    own_all = tdist.all_ranks(own, dev)
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, out, rank, world)
    # ---- --full only: untimed extras after the timed region, each a measurement of its own
    attn_modes, unbounded_s, pil_delta_ms, probe = {}, None, None, {}
    if a.full:
        # roofline sample: ONE MORE call, untimed and eager (the library's per-launch HIP events only see eager launches; a
        # replayed graph's kernels are not individually timed), so that the sample is every GEMM / attention launch of a whole
        # call -- 30 steps, VAE, text encoders -- not just the eager first step of a graph-replayed call
        pipe.enable_hip_graph(False)
        if rank == 0:
            ops.prof_enable(True)
        ops.attention_mode_counts(reset=True)
        one_call()
        torch.cuda.synchronize()
        ops.prof_enable(False)
        attn_modes = {k: v for k, v in ops.attention_mode_counts(reset=True).items() if v}     # which attention stream every launch of a call took
        pipe.enable_hip_graph(not a.no_graph)
        # the reference-free attention stream is selected per launch from the block's q / k RMSNorm weights (tfx_*_block.attn_score_bound);
        # what a checkpoint whose norm scales do NOT admit it would see: one untimed call (after one warm-up call that re-captures the step
        # graph) with the bound ignored -- every launch on the guarded kernel
        if rank == 0 and world == 1 and not a.no_attention_ab:
            ops.set_option("attention_use_bound", 0)
            tr._session = None                       # the captured step graphs hold the kernels chosen at capture
            one_call()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            one_call()
            torch.cuda.synchronize()
            unbounded_s = time.perf_counter() - t1
            ops.set_option("attention_use_bound", 1)
            tr._session = None
        # what the timed calls leave out of a17: output_type="pt" keeps the decoded images on the device; one untimed call with
        # output_type="pil" (device -> host copy + uint8 / PIL conversion of the batch) gives the difference
        if rank == 0 and not a.no_pil_delta:
            def timed(kind):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                with torch.no_grad():
                    pipe(prompt_embeds=pe, pooled_prompt_embeds=pooled, image=image, mask_image=mask, height=H, width=W,
                         num_inference_steps=1, guidance_scale=30.0, generator=gen, output_type=kind)
                torch.cuda.synchronize()
                return time.perf_counter() - t1
            timed("pt")
            t_pt, t_pil = min(timed("pt"), timed("pt")), min(timed("pil"), timed("pil"))
            pil_delta_ms = (t_pil - t_pt) * 1e3
        # the matrix-pipe rate this board sustains at its power cap on random operands (tfx_mfma_peak_probe, LIVE: the product library's own
        # MFMA-only kernel, ~2.5 s each): the denominator of roofline.frac_of_capped; bf16 and e4m3
        if rank == 0 and not a.no_peak_probe:
            gp = torch.Generator().manual_seed(5)
            rb = torch.randn(1 << 20, generator=gp)
            probe["bf16"] = ops.mfma_peak_probe(rb.to(torch.bfloat16).to(dev), fp8=False, seconds=2.5)
            try:
                probe["e4m3"] = ops.mfma_peak_probe(rb.to(torch.float8_e4m3fn).view(torch.uint8).to(dev), fp8=True, seconds=2.5)
            except Exception as e:
                probe["e4m3"] = {"error": f"{type(e).__name__}: {e}"}
    seen = tdist.ranks_seen(dev)   # ranks that answered an RCCL all-reduce
    # results travel to rank 0 the way the batch driver collects them (untimed here: `value` is generation throughput): a per-image
    # checksum of every rank's last call, gathered over RCCL -- rank 0 checks that every rank produced finite images
    sums = tdist.gather_to_rank0(out.float().mean(dim=(1, 2, 3)).contiguous())
    if rank == 0:
        assert len(sums) == world and all(torch.isfinite(x).all() for x in sums), "a rank returned non-finite images"

    if rank == 0:
        gemm_ms, gemm_fl, gemm_n = ops.prof_collect(2 if a.fp8 else 0)   # fp8 run: the e4m3 GEMM launches are the dominant kernel
        att_ms, att_fl, att_n = ops.prof_collect(1)
        total_images = world * B * a.steps
        ips = total_images / elapsed
        achieved = gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        # Counter- and power-derived fields cannot be collected by bench.py itself (rocprofv3 --pmc needs its own passes,
        # rocm-smi its own sustained loops): they are READ from the newest committed profile and say so -- "live": false,
        # the file, and the round it was collected in -- so that no future run can pass them off as measured by this run.
        def committed(stem):
            for rnd in ("r06", "r05", "r04", "r03", "r02"):
                fn = os.path.join(REPO, "profiles", f"{rnd}_{stem}.json")
                if os.path.exists(fn):
                    with open(fn) as f:
                        return json.load(f), f"profiles/{rnd}_{stem}.json", rnd
            return None, None, None

        traffic, traffic_note = None, None
        try:
            pmj, fn, rnd = committed("gemm_pmc_traffic")
            pm = pmj["shapes"][0]
            traffic = pm["hbm_bytes_per_launch"]
            traffic_note = {"live": False, "collected_in_round": rnd, "file": fn,
                            "what": (f"PMC FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE of the most expensive shape M={pm['M']} "
                                     f"N={pm['N']} K={pm['K']} (algorithmic bytes {pm['algorithmic_bytes']})")}
        except Exception:
            pass
        mfma_pmc = None
        try:  # matrix-pipe busy fraction of the DiT kernels from the committed SQ_VALU_MFMA_BUSY_CYCLES pass over this bench
            mu, fn, rnd = committed("mfma_util")
            mfma_pmc = {"dit_kernels": mu["dit_kernels_total"]["mfma_util"], "live": False, "collected_in_round": rnd,
                        "file": fn, "formula": mu["formula"]}
        except Exception:
            pass
        # the rate of a kernel that does nothing but MFMAs on random data at the board's power cap: measured by THIS run (probe above)
        pk = probe.get("e4m3" if a.fp8 else "bf16", {})
        power_peak = None
        if pk.get("tflops"):
            power_peak = {"tflops": pk["tflops"], "live": True, "kernel": "tfx::mfma_probe_kernel (tfx_mfma_peak_probe): the GEMM kernels' MFMA sections on "
                          "register-resident random N(0,1) operands, 8 waves per CU, nothing else", "seconds": pk["seconds"],
                          "tflops_first_launch": pk["tflops_first_launch"], "launches": pk["launches"],
                          "bf16": probe.get("bf16"), "e4m3": probe.get("e4m3")}
        rec = {
            "metric": "images/sec (whole node), 1024x1024 30-step FLUX-Fill" if (H, W, n) == (1024, 1024, 30) else
                      f"images/sec (whole node), {H}x{W} {n}-step FLUX-Fill",
            "value": ips, "unit": "images/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "fp8 (e4m3 operands, fp32 accumulate) block linears; bf16 elsewhere" if a.fp8 else "bf16", "data": ("synthetic (random-init FLUX.1-Fill / T5-XXL / CLIP-L architecture weights, random image, box mask; per call: "
                                      "8 T5 prompts + the CLIP template encoded by the HIP text encoders from stand-in token ids)") if use_te else
                                     ("synthetic (random-init FLUX.1-Fill-architecture weights, random image, box mask, "
                                      "injected random prompt embeddings; text encoders bypassed)"),
            "config": {"workload": f"{'P1024' if (H, W) == (1024, 1024) else f'{H}x{W}'}: FluxFillPipeline.__call__ {H}x{W}, {n} {a.sampler} steps, guidance 30, "
                                   f"batch {B}/GPU (S={S} image + 512 text tokens), "
                                   + ("T5-XXL (8 prompts per rank) + CLIP-L prompt encoding from stand-in token ids (no tokenizer vocabularies offline), " if use_te else "")
                                   + "VAE encode+decode included, output_type='pt' (decoded images stay in HBM: the D2H copy + uint8/PIL conversion "
                                     "of a17 is outside the timed region, see pil_output_delta_ms_per_call)"
                                   + ("" if full else f" [REDUCED MODEL {a.layers} - not a valid headline]")
                                   + (" [fp8 linears: BASELINE config 5 precision, not the bf16 headline]" if a.fp8 else ""),
                       "global_batch": world * B, "parallelism": f"dp{world} (batch shards; shared CLIP conditioning broadcast over {_transport()}, T5 prompts encoded per rank)"},
            "rccl_ranks_seen": seen, "process_group": tdist.group_info(),
            "elapsed_s": elapsed, "elapsed_per_rank_s": {"min": min(own_all), "max": max(own_all), "ranks": own_all,
                                                         "note": "each rank's own K calls up to its synchronize(), before the closing barrier"},
            "pil_output_delta_ms_per_call": pil_delta_ms,
            "sec_per_img_per_gpu": elapsed / (B * a.steps),
            "dit_algorithmic_tflops_per_gpu": dit_flops(S) * n * B * a.steps / elapsed / 1e12 if full else None,
            "roofline": {"bound": "mfma", "kernel": "tfx::gemm8pp_kernel (persistent MFMA GEMM, all epilogues; + gemm8p_kernel for K % 128 != 0)", "achieved": achieved,
                         "peak": MFMA_PEAK_TFLOPS * (2 if a.fp8 else 1), "unit": "TFLOP/s", "frac": achieved / (MFMA_PEAK_TFLOPS * (2 if a.fp8 else 1)),
                         "power_capped_peak": power_peak, "frac_of_capped": (achieved / power_peak["tflops"]) if power_peak else None,
                         "traffic": None if a.fp8 else traffic, "traffic_note": None if a.fp8 else traffic_note, "mfma_busy_pmc": None if a.fp8 else mfma_pmc, "launches": gemm_n, "avg_launch_ms": gemm_ms / max(gemm_n, 1),
                         "sample": "HIP events around every GEMM launch of one extra, untimed, eager call after the timed region (graph-replayed launches are not individually timed)",
                         "flops_per_launch": gemm_fl / max(gemm_n, 1),
                         "attention": {"achieved": att_fl / (att_ms * 1e-3) / 1e12 if att_ms > 0 else 0.0,
                                       "launches": att_n, "avg_launch_ms": att_ms / max(att_n, 1),
                                       "modes": attn_modes,
                                       "modes_note": "launches of the eager sample call by kernel form; w4_reference_free needs the block's score bound "
                                                     "(128 max|w_q| max|w_k| 128^-0.5 * 1.03) to satisfy bound*log2(e) + log2(N) + 24 <= 126, i.e. "
                                                     "max|w_q| max|w_k| <= 5.3 at N = 4608; init_random_ draws the norm weights as 1 + 0.1 randn",
                                       "call_s_with_bound": elapsed / a.steps,
                                       "call_s_bound_ignored": unbounded_s}},
        }
        peak = MFMA_PEAK_TFLOPS * (2 if a.fp8 else 1)
        rec["roofline"]["attention"]["frac"] = rec["roofline"]["attention"]["achieved"] / MFMA_PEAK_TFLOPS     # attention is bf16 in both modes
        # the number north_star's ">= 60 % MFMA utilisation on the DiT block" is written against: algorithmic DiT FLOPs of the timed
        # region (GEMMs + attention, text encoders / VAE / everything else counted as time but not as FLOPs) over the bf16 dense peak
        rec["roofline"]["dit_achieved"] = rec["dit_algorithmic_tflops_per_gpu"]
        rec["roofline"]["dit_frac"] = rec["dit_algorithmic_tflops_per_gpu"] / MFMA_PEAK_TFLOPS if full and not a.fp8 else None
        rec["cpu_baseline"] = None
        if c1_rec is not None and "error" not in c1_rec:       # rank 0 at N = 1 only
            rec["cpu_baseline"] = {
                "value": c1_rec["images_per_sec"], "unit": "images/sec", "cores": c1_rec["threads"], "kind": "port", "live": True,
                "sample": ("BASELINE.md section 3 / BASELINE.json config 1 (C1), run live by this bench in a host-side subprocess that finished before "
                           f"the timed region: {c1_rec['config']}; {c1_rec['loop_s']:.1f} s for the 4-step loop ({c1_rec['s_per_step']:.1f} s / step, "
                           f"{c1_rec['cpu_tflops']:.2f} TFLOP/s) on {c1_rec['threads']} threads (fastest of a sweep; {c1_rec['logical_cpus']} logical CPUs) after a "
                           f"{c1_rec['warmup_forward_s']:.1f} s warm-up forward; the reference's C1 is a DIFFERENT configuration from the GPU headline "
                           "(576x512, 4 steps, fp32, batch 1): a reported baseline, not a ratio's denominator"),
                "c1": {k: v for k, v in c1_rec.items() if k != "workload_block_sample"},
                "workload_block_sample": c1_rec.get("workload_block_sample")}
        elif c1_rec is not None:
            rec["cpu_baseline"] = {"value": None, "unit": "images/sec", "cores": None, "kind": "port", "live": True, "sample": c1_rec["error"]}
        if not a.full:      # a plain run measured none of these: its line carries the headline and the run's own bookkeeping
            for k in ("pil_output_delta_ms_per_call", "roofline", "cpu_baseline"):
                del rec[k]
        print(json.dumps(rec), flush=True)
    tdist.shutdown()


if __name__ == "__main__":
    main()
