"""GPU parity of the drop-in boundary: FluxFillPipeline.__call__, both samplers, VAE ends, LoRA merge -- against the
reference's golden trajectories (tests/golden/g5_pipeline, g9_vae) and the CPU oracle.

Tolerance statement (north_star "latent MAE <= 1e-3"): latents here are O(1); per denoising step the engine may differ
from the reference-in-bf16 by at most 1.5x the distance between the reference's own bf16 and fp32 runs, and from the
reference-in-fp32 by at most 1.25x that distance (both asserted per step)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as fo
from oracle import pipeline_oracle as po
from oracle import vae_oracle as vo

BF = torch.bfloat16
G3_CFG = fo.FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, joint_attention_dim=64,
                       pooled_projection_dim=32)
G9_VAE = dict(block_out_channels=(64, 64, 128, 128), layers_per_block=1, latent_channels=16, norm_num_groups=16)
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096,
             shift=3.0)


def mae(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().mean().item()


def python_issued_loop(pipe, g, **kw):
    """tests/helpers/plain_loop.py on the g5 inputs (8 x 8 latent grid): the loop as Python-issued launches, the side that stays
    independent of tfx_dit_step_run.  Call after a pipeline call: the scheduler holds its schedule."""
    from tests.helpers.plain_loop import plain_loop
    return plain_loop(pipe, g["latents"], g["masked_image_latents"], g["prompt_embeds"], g["pooled"], (8, 8), **kw)


def make_pipe(sname, vae_seed=900):
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler, StochasticRFOvershotDiscreteScheduler
    from textflux_amd.transformer import FluxTransformer2DModel
    from textflux_amd.vae import AutoencoderKL
    tr = FluxTransformer2DModel(in_channels=384, out_channels=64, num_layers=2, num_single_layers=2,
                                num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=32,
                                guidance_embeds=True).load_state_dict(fo.seeded_state_dict(G3_CFG, 7), device="cuda")
    vcfg = vo.VaeConfig(**G9_VAE)
    vae = AutoencoderKL(**G9_VAE).load_state_dict(vo.seeded_state_dict(vcfg, vae_seed), device="cuda")
    if sname == "euler":
        sch = FlowMatchEulerDiscreteScheduler(**SCHED)
    else:
        sch = StochasticRFOvershotDiscreteScheduler(**SCHED)
        sch.set_c(2.0)
        sch.set_overshot_func(lambda t, dt: t + dt)
    pipe = FluxFillPipeline(scheduler=sch, vae=vae, text_encoder=None, tokenizer=None, text_encoder_2=None,
                            tokenizer_2=None, transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    return pipe


@pytest.mark.parametrize("sname", ["euler", "amo"])
def test_call_latent_trajectory_matches_reference(golden, sname):
    g = golden("g5_pipeline")
    pipe = make_pipe(sname)
    steps = []

    def cb(p, i, t, kw):
        steps.append(kw["latents"].clone())
        return {}

    eps = [g[f"amo.eps{i}"] for i in range(4)] if sname == "amo" else None
    out = pipe(prompt_embeds=g["prompt_embeds"].to(BF).cuda(), pooled_prompt_embeds=g["pooled"].to(BF).cuda(),
               latents=g["latents"].to(BF).cuda(), masked_image_latents=g["masked_image_latents"].to(BF).cuda(),
               height=128, width=128, num_inference_steps=4, guidance_scale=30.0, output_type="latent",
               callback_on_step_end=cb, callback_on_step_end_tensor_inputs=["latents"], amo_noise=eps).images
    assert out.shape == (2, 64, 64) and out.dtype == BF
    for i in range(4):
        rb, rf = g[f"{sname}.bf16.step{i}"], g[f"{sname}.f32.step{i}"]
        gap = mae(rb, rf)
        e_b, e_f = mae(steps[i], rb), mae(steps[i], rf)
        print(f"{sname} step {i}: MAE vs ref-bf16 {e_b:.2e} vs ref-f32 {e_f:.2e} (ref bf16-vs-f32 {gap:.2e})")
        assert e_b <= 1.5 * gap + 1e-4 and e_f <= 1.25 * gap + 1e-4
    assert torch.equal(out, steps[-1])


def test_scheduler_objects_step_protocol(golden):
    """The drop-in scheduler classes driven the way the reference pipeline drives them (P:2098)."""
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler, StochasticRFOvershotDiscreteScheduler
    from textflux_amd.pipeline import calculate_shift
    import numpy as np
    g = golden("g4_sched")
    n, S = 6, 4096
    mu = calculate_shift(S, 256, 4096, 0.5, 1.15)
    e = FlowMatchEulerDiscreteScheduler(**SCHED)
    e.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=mu, device="cuda")
    assert torch.equal(e.sigmas.cpu(), g["euler.n6.S4096.sigmas"]) if "euler.n6.S4096.sigmas" in g else True
    x = g["traj.x0"].to(BF).cuda()
    for i, t in enumerate(e.timesteps):
        x = e.step(g[f"traj.v{i}"].to(BF).cuda(), t, x, return_dict=False)[0]
        assert torch.equal(x.cpu(), g[f"traj.euler.bf16.x{i}"])
    a = StochasticRFOvershotDiscreteScheduler(**SCHED)
    a.set_c(2.0)
    a.set_overshot_func(lambda t, dt: t + dt)
    a.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=mu, device="cuda")
    x = g["traj.x0"].to(BF).cuda()
    for i, t in enumerate(a.timesteps):
        x, x1 = a.step(g[f"traj.v{i}"].to(BF).cuda(), t, x, return_dict=False, noise=g[f"traj.amo.eps{i}"])
        assert torch.equal(x.cpu(), g[f"traj.amo.bf16.x{i}"])
    with pytest.raises(ValueError):
        e.step(x, 3, x)


def test_vae_ends_match_oracle(golden):
    from textflux_amd.vae import AutoencoderKL
    g = golden("g9_vae")
    vcfg = vo.VaeConfig(**G9_VAE)
    vae = AutoencoderKL(**G9_VAE).load_state_dict(vo.seeded_state_dict(vcfg, 900), device="cuda")
    post = vae.encode(g["x"].to(BF).cuda()).latent_dist
    assert mae(post.mean, g["enc.mean"]) <= 2e-2 * g["enc.mean"].abs().mean().item() + 1e-3
    dec = vae.decode(g["z"].to(BF).cuda(), return_dict=False)[0]
    assert mae(dec, g["dec.out"]) <= 2e-2 * g["dec.out"].abs().mean().item() + 1e-3


def test_call_with_image_and_mask_matches_oracle():
    """Full __call__ (preprocess -> VAE encode -> denoise -> VAE decode -> postprocess) with a CPU generator; the
    oracle is fed the same two draws (latents first, posterior eps second: SURVEY Appendix E)."""
    pipe = make_pipe("euler")
    H = W = 128
    gi = torch.Generator().manual_seed(5)
    image = (torch.randn(2, 3, H, W, generator=gi) * 0.3 + 0.5).clamp(0, 1)
    mask = torch.zeros(2, 1, H, W)
    mask[:, :, 32:96, 16:112] = 1.0
    pe, pooled = torch.randn(2, 16, 64, generator=gi), torch.randn(2, 32, generator=gi)
    gen = torch.Generator().manual_seed(99)
    out = pipe(prompt_embeds=pe.to(BF).cuda(), pooled_prompt_embeds=pooled.to(BF).cuda(), image=image, mask_image=mask,
               height=H, width=W, num_inference_steps=3, guidance_scale=30.0, generator=gen, output_type="np").images
    assert out.shape == (2, H, W, 3) and out.min() >= 0 and out.max() <= 1
    gen2 = torch.Generator().manual_seed(99)
    lat_noise = torch.randn((2, 16, 16, 16), generator=gen2, dtype=BF).float()
    post_eps = torch.randn((2, 16, 16, 16), generator=gen2, dtype=BF).float()
    vcfg = vo.VaeConfig(**G9_VAE)
    ref = po.fill_pipeline(fo.seeded_state_dict(G3_CFG, 7), G3_CFG, vo.seeded_state_dict(vcfg, 900), vcfg, image, mask,
                           pe, pooled, lat_noise, post_eps, 3, 30.0, output_type="np")
    err = (torch.from_numpy(out) - ref).abs().mean().item()
    print(f"image MAE vs fp32 oracle: {err:.3e}")
    assert err < 2e-2  # pixels in [0,1]; bf16 VAE + bf16 DiT vs fp32 oracle


def test_lora_merge_matches_oracle_with_premerged_weights(tmp_path):
    """Synthetic LoRA in the reference file format (a18): merged-at-load engine == oracle with W + (alpha/r) B A."""
    from safetensors.torch import save_file
    from textflux_amd.pipeline import FluxFillPipeline
    pipe = make_pipe("euler")
    sd = fo.seeded_state_dict(G3_CFG, 7)
    r, D = 16, 256
    gl = torch.Generator().manual_seed(3)
    targets = ["transformer_blocks.0.attn.to_q", "transformer_blocks.0.attn.add_k_proj", "transformer_blocks.1.attn.to_out.0",
               "transformer_blocks.1.ff.net.0.proj", "transformer_blocks.0.ff_context.net.2",
               "single_transformer_blocks.0.attn.to_v", "single_transformer_blocks.1.attn.to_k"]
    lora, merged = {}, dict(sd)
    for i, t in enumerate(targets):
        out_f, in_f = sd[t + ".weight"].shape
        A = torch.randn(r, in_f, generator=gl) * 0.2
        Bm = torch.randn(out_f, r, generator=gl) * 0.2
        alpha = float(r) if i % 2 == 0 else 8.0
        lora[f"transformer.{t}.lora_A.weight"], lora[f"transformer.{t}.lora_B.weight"] = A, Bm
        if i % 2:
            lora[f"transformer.{t}.alpha"] = torch.tensor(alpha)
        merged[t + ".weight"] = sd[t + ".weight"] + (alpha / r) * (Bm.to(BF).float() @ A.to(BF).float())
    path = tmp_path / "pytorch_lora_weights.safetensors"
    save_file(lora, str(path))
    lsd, alphas = FluxFillPipeline.lora_state_dict(str(tmp_path), return_alphas=True)
    assert len(alphas) == 3 and not any(k.endswith(".alpha") for k in lsd)
    n = FluxFillPipeline.load_lora_into_transformer(lsd, alphas, pipe.transformer)
    assert n == len(targets)
    g = torch.Generator().manual_seed(11)
    inp = dict(hidden_states=torch.randn(1, 64, 384, generator=g), encoder_hidden_states=torch.randn(1, 16, 64, generator=g),
               pooled_projections=torch.randn(1, 32, generator=g), timestep=torch.tensor([0.6]),
               guidance=torch.tensor([30.0]), img_ids=po.latent_image_ids(8, 8), txt_ids=torch.zeros(16, 3))
    tobf = lambda d: {k: (v.to(BF) if v.dtype == torch.float32 and k != "guidance" else v) for k, v in d.items()}
    ref_m = fo.transformer_forward(tobf(merged), G3_CFG, **tobf(inp))   # bf16-faithful oracle, pre-merged weights
    ref_0 = fo.transformer_forward(tobf(sd), G3_CFG, **tobf(inp))
    bf = lambda t: t.to(BF).cuda()
    got = pipe.transformer(hidden_states=bf(inp["hidden_states"]), encoder_hidden_states=bf(inp["encoder_hidden_states"]),
                           pooled_projections=bf(inp["pooled_projections"]), timestep=bf(inp["timestep"]),
                           guidance=inp["guidance"].cuda(), img_ids=inp["img_ids"], txt_ids=inp["txt_ids"],
                           return_dict=False)[0]
    e_m, e_0, delta = mae(got, ref_m), mae(got, ref_0), mae(ref_m, ref_0)
    print(f"LoRA: |got-merged| {e_m:.2e}  |got-unmerged| {e_0:.2e}  |merged-unmerged| {delta:.2e}")
    assert delta > 5 * e_m and e_0 > 3 * e_m and e_m < 2e-2 * ref_m.float().abs().mean().item()  # the merge is visible and lands on the merged oracle


@pytest.mark.parametrize("sname", ["euler", "amo"])
def test_hip_graph_replay_is_bit_identical_to_eager_loop(golden, sname):
    """One captured step graph (device-side step cursor) replayed for steps 1..n-1 == the eager step == the launch sequence issued
    from Python (Euler: fused into proj_out, the default; AMO: supplied noise)."""
    g = golden("g5_pipeline")
    eps = [g[f"amo.eps{i}"] for i in range(4)] if sname == "amo" else None
    kw = dict(prompt_embeds=g["prompt_embeds"].to(BF).cuda(), pooled_prompt_embeds=g["pooled"].to(BF).cuda(),
              latents=g["latents"].to(BF).cuda(), masked_image_latents=g["masked_image_latents"].to(BF).cuda(),
              height=128, width=128, num_inference_steps=4, guidance_scale=30.0, output_type="latent", amo_noise=eps)
    pipe = make_pipe(sname)
    eager = pipe(**kw).images
    pipe.enable_hip_graph(True)
    graphed = pipe(**kw).images          # captures
    again = pipe(**kw).images            # re-uses the cached graph
    assert torch.equal(eager, graphed) and torch.equal(eager, again)
    assert torch.equal(eager, python_issued_loop(pipe, g, fused=sname == "euler", amo_noise=eps))
    assert mae(graphed, g[f"{sname}.bf16.final"]) < 1e-3


def test_euler_update_in_proj_out_epilogue_is_bit_identical_to_the_scheduler_kernel(golden):
    """north_star's "flow-matching Euler step fused into the residual add": the final projection's gated-residual epilogue
    applies x' = x + bf16(dsigma * bf16(v)) in place on the latent columns of the x_embedder input (tfx_dit_desc.euler_gate;
    no scheduler launch, no copy of the new latents into the next step's input).  Same rounding points as
    FlowMatchEulerDiscreteScheduler.step (scheduling_flow_match_euler_discrete.py:319-330) applied to the stored model output:
    every step of the trajectory is bit-identical, eagerly, as a replayed step graph and issued launch by launch from Python."""
    g = golden("g5_pipeline")
    kw = dict(prompt_embeds=g["prompt_embeds"].to(BF).cuda(), pooled_prompt_embeds=g["pooled"].to(BF).cuda(),
              latents=g["latents"].to(BF).cuda(), masked_image_latents=g["masked_image_latents"].to(BF).cuda(),
              height=128, width=128, guidance_scale=30.0, output_type="latent")
    pipe = make_pipe("euler")
    outs = {}
    for n in (1, 2, 4):
        for fuse in (False, True):
            pipe.fuse_euler_step = fuse
            pipe.enable_hip_graph(False)
            outs[(n, fuse, "eager")] = pipe(num_inference_steps=n, **kw).images
            outs[(n, fuse, "python")] = python_issued_loop(pipe, g, fused=fuse)     # the same launches issued from Python (n = 1 never captures)
            pipe.enable_hip_graph(True)
            outs[(n, fuse, "graph")] = pipe(num_inference_steps=n, **kw).images
        ref = outs[(n, False, "eager")]
        for k, v in outs.items():
            if k[0] == n:
                assert torch.equal(v, ref), k
    assert mae(outs[(4, True, "graph")], g["euler.bf16.final"]) < 1e-3
    assert pipe.transformer._session.desc.euler_gate is not None        # the last call really ran fused


def test_step_callback_sees_the_python_issued_loops_latents_every_step(golden):
    """A step callback keeps the loop eager and unfused (graphs on or off) and is handed the live latents: every step's clone equals
    the Python-issued loop's latents after that step, bit for bit."""
    g = golden("g5_pipeline")
    pipe = make_pipe("euler").enable_hip_graph(True)
    steps = []
    out = pipe(prompt_embeds=g["prompt_embeds"].to(BF).cuda(), pooled_prompt_embeds=g["pooled"].to(BF).cuda(),
               latents=g["latents"].to(BF).cuda(), masked_image_latents=g["masked_image_latents"].to(BF).cuda(),
               height=128, width=128, num_inference_steps=4, guidance_scale=30.0, output_type="latent",
               callback_on_step_end=lambda p, i, t, kw: steps.append(kw["latents"].clone()) or {}).images
    mine = []
    python_issued_loop(pipe, g, per_step=mine)
    assert len(steps) == len(mine) == 4 and all(torch.equal(a, b) for a, b in zip(steps, mine)) and torch.equal(out, mine[-1])
    assert not pipe.transformer._session.graphs                       # nothing was captured


def test_hip_graph_amo_internal_noise_runs():
    pipe = make_pipe("amo").enable_hip_graph(True)
    gi = torch.Generator().manual_seed(1)
    out = pipe(prompt_embeds=torch.randn(1, 16, 64, generator=gi).to(BF).cuda(),
               pooled_prompt_embeds=torch.randn(1, 32, generator=gi).to(BF).cuda(),
               latents=torch.randn(1, 64, 64, generator=gi).to(BF).cuda(),
               masked_image_latents=torch.randn(1, 64, 320, generator=gi).to(BF).cuda(), height=128, width=128,
               num_inference_steps=5, guidance_scale=30.0, output_type="latent").images
    assert torch.isfinite(out.float()).all() and out.float().std().item() > 0.1


def test_fp8_call_matches_fp8_oracle_trajectory_and_graph_replay(golden):
    """BASELINE config 5 precision (fp8 block linears) through FluxFillPipeline.__call__: per-step latents against the
    oracle running the same e4m3 scheme (flux_oracle.fp8_block_linears) in bf16, under the bf16 criterion of the tests
    above; hipGraph replay stays bit-identical; the cost of fp8 against the reference's bf16 trajectory is printed and
    bounded (it is the scheme's property, not the kernels')."""
    g = golden("g5_pipeline")
    kw = dict(prompt_embeds=g["prompt_embeds"].to(BF).cuda(), pooled_prompt_embeds=g["pooled"].to(BF).cuda(),
              latents=g["latents"].to(BF).cuda(), masked_image_latents=g["masked_image_latents"].to(BF).cuda(),
              height=128, width=128, num_inference_steps=4, guidance_scale=30.0, output_type="latent")
    pipe = make_pipe("euler")
    pipe.transformer.enable_fp8()
    steps = []

    def cb(p, i, t, k):
        steps.append(k["latents"].clone())
        return {}

    out = pipe(callback_on_step_end=cb, callback_on_step_end_tensor_inputs=["latents"], **kw).images
    mine = []
    assert torch.equal(python_issued_loop(pipe, g, per_step=mine), out) and all(torch.equal(a, b) for a, b in zip(steps, mine))
    sd = {k: v.to(BF) for k, v in fo.seeded_state_dict(G3_CFG, 7).items()}
    with fo.fp8_block_linears():
        _, traj = po.denoise(sd, G3_CFG, g["latents"].to(BF), g["masked_image_latents"].to(BF), g["prompt_embeds"].to(BF),
                             g["pooled"].to(BF), 8, 8, 4, 30.0, scheduler="euler", sched_cfg=SCHED)
    for i in range(4):
        gap = mae(g[f"euler.bf16.step{i}"], g[f"euler.f32.step{i}"])
        e, cost = mae(steps[i], traj[i]), mae(steps[i], g[f"euler.bf16.step{i}"])
        print(f"fp8 step {i}: MAE vs fp8 oracle {e:.2e} (bf16 ref gap {gap:.2e}); vs reference bf16 {cost:.2e}")
        assert e <= 1.5 * gap + 1e-4
        assert cost <= 5e-2
    pipe.enable_hip_graph(True)
    graphed = pipe(**kw).images
    assert torch.equal(out, graphed)


@pytest.mark.parametrize("height,width", [(32, 32), (72, 57), (128, 96)])
def test_output_shape_follows_the_references_rounding(height, width):
    """The reference's own behavioural test (diffusers/tests/pipelines/flux/test_pipeline_flux_fill.py:153-165): a requested size that is
    not a multiple of vae_scale_factor * 2 = 16 is rounded DOWN -- (72, 57) -> (64, 48) -- by the image processor's resize and by
    prepare_latents alike; the call returns images of that size."""
    pipe = make_pipe("euler")
    gi = torch.Generator().manual_seed(6)
    image = (torch.randn(1, 3, 64, 64, generator=gi) * 0.3 + 0.5).clamp(0, 1)
    mask = torch.zeros(1, 1, 64, 64)
    mask[:, :, 16:48, 8:56] = 1.0
    pe, pooled = torch.randn(1, 16, 64, generator=gi), torch.randn(1, 32, generator=gi)
    out = pipe(prompt_embeds=pe.to(BF).cuda(), pooled_prompt_embeds=pooled.to(BF).cuda(), image=image, mask_image=mask, height=height,
               width=width, num_inference_steps=2, guidance_scale=30.0, generator=torch.Generator().manual_seed(1), output_type="np").images
    assert out.shape == (1, height - height % 16, width - width % 16, 3) and out.min() >= 0 and out.max() <= 1


def test_batch_of_identical_inputs_equals_the_single_call():
    """PipelineTesterMixin.test_inference_batch_single_identical (diffusers/tests/pipelines/test_pipelines_common.py:1057-1166, the
    reference asserts max difference < 1e-3 ... 1e-4 on np images): three copies of one input in a batch, each with its own generator
    seeded alike, give the single call's image -- here bit for bit."""
    pipe = make_pipe("euler")
    gi = torch.Generator().manual_seed(8)
    H = W = 64
    image = (torch.randn(1, 3, H, W, generator=gi) * 0.3 + 0.5).clamp(0, 1)
    mask = torch.zeros(1, 1, H, W)
    mask[:, :, 16:48, 8:56] = 1.0
    pe, pooled = torch.randn(1, 16, 64, generator=gi).to(BF).cuda(), torch.randn(1, 32, generator=gi).to(BF).cuda()
    kw = dict(height=H, width=W, num_inference_steps=3, guidance_scale=30.0, output_type="np")
    one = pipe(prompt_embeds=pe, pooled_prompt_embeds=pooled, image=image, mask_image=mask,
               generator=torch.Generator(device="cuda").manual_seed(3), **kw).images
    three = pipe(prompt_embeds=pe.repeat(3, 1, 1), pooled_prompt_embeds=pooled.repeat(3, 1), image=image.repeat(3, 1, 1, 1),
                 mask_image=mask.repeat(3, 1, 1, 1), generator=[torch.Generator(device="cuda").manual_seed(3) for _ in range(3)], **kw).images
    assert three.shape == (3, H, W, 3)
    for i in range(3):
        assert (three[i] == one[0]).all()


def test_callback_tensor_inputs_are_validated_and_delivered():
    """PipelineTesterMixin.test_callback_inputs (test_pipelines_common.py:1721-1790): only names in _callback_tensor_inputs are accepted;
    the callback receives exactly the requested tensors every step and may replace the latents (here: zero them at the last step)."""
    pipe = make_pipe("euler")
    gi = torch.Generator().manual_seed(9)
    lat = torch.randn(1, 16, 64, generator=gi).to(BF).cuda()
    mil = torch.randn(1, 16, 320, generator=gi).to(BF).cuda()
    pe, pooled = torch.randn(1, 16, 64, generator=gi).to(BF).cuda(), torch.randn(1, 32, generator=gi).to(BF).cuda()
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, latents=lat, masked_image_latents=mil, height=64, width=64,
              num_inference_steps=3, guidance_scale=30.0, output_type="latent")
    with pytest.raises(ValueError, match="callback_on_step_end_tensor_inputs"):
        pipe(callback_on_step_end=lambda *a: {}, callback_on_step_end_tensor_inputs=["latents", "not_a_tensor_input"], **kw)
    seen = []

    def cb(p, i, t, k):
        seen.append(sorted(k))
        if i == 2:
            return {"latents": torch.zeros_like(k["latents"])}
        return {}

    out = pipe(callback_on_step_end=cb, callback_on_step_end_tensor_inputs=["latents", "prompt_embeds"], **kw).images
    assert seen == [["latents", "prompt_embeds"]] * 3 and out.abs().sum().item() == 0
