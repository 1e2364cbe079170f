"""Known-region sampling on the GPU (DESIGN.md section 4 "Known-region sampling"): tfx_known_region_blend and tfx_keep_mask_pack
against the torch-CPU restatement of helpers/keep_known_ref.py (itself pinned to the reference by tests/test_keep_known_cpu.py), bit
for bit; tfx_dit_step_run_ex inside the pipeline against the same loop issued from Python, for every sampler, eager and captured,
with the fp8 linears and the step cache; and the pipeline's invariants.  Tiny model of tests/helpers/tiny_checkpoint.py, B = 2,
128 x 96 pixels (48 tokens), 4 steps.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import exact_inputs as X
from tests.helpers import keep_known_ref as R

BF = torch.bfloat16
B, H, W, N_STEPS = 2, 96, 128, 4
GRID = (H // 16, W // 16)
S = GRID[0] * GRID[1]


def bits(t):
    return t.contiguous().view(torch.int16)


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


# ----------------------------------------------------------------------------- tfx_known_region_blend alone
SIGMA = torch.tensor([0.90625, 0.5, -1.0, 0.0], dtype=torch.float32)        # bf16-exact; entry 2: "x0 itself"; entry 3: a true zero


def blend_inputs(rows, C, seed, soft):
    x, x0, noise = (X.arbitrary_bf16((rows, C), seed + k) for k in range(3))
    g = X.gen(seed + 3)
    if soft:
        mask = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (rows, C), generator=g)].to(BF)
    else:
        mask = (torch.rand(rows, C, generator=g) < 0.5).to(BF)
    for t, pattern in ((x, (0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0)), (x0, (0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 2.0, -2.0)),
                       (noise, (-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0))):
        t.view(-1)[:8] = torch.tensor(pattern, dtype=BF)                 # planted signed zeros under both mask values
    mask.view(-1)[:8] = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1], dtype=BF)
    return x, x0, noise, mask


@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
@pytest.mark.parametrize("device_step", [False, True], ids=["host_step", "step_ptr"])
@pytest.mark.parametrize("mirror", [False, True], ids=["no_xin", "xin"])
@pytest.mark.parametrize("rows,C,ldx", [(1, 8, 8), (3, 64, 384), (257, 64, 64), (192, 64, 384)],
                         ids=["one_chunk", "pitched", "grid_tail", "pitched_48_blocks"])
def test_blend_equals_the_restatement(rows, C, ldx, mirror, device_step, soft):
    from textflux_amd import ops
    x, x0, noise, mask = blend_inputs(rows, C, 11 * rows + C, soft)
    assert (rows * C // 8) % 256 != 0 or rows == 192
    sig = SIGMA.cuda()
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in range(len(SIGMA)):
        want = R.blend(x, x0, noise, mask, float(SIGMA[s]))
        pad = X.arbitrary_bf16((rows, ldx), 77).cuda()
        pad[:, :C] = x.cuda()
        xd = pad[:, :C]                                                  # a column view when ldx > C, the tensor itself otherwise
        pad0 = pad.clone()
        xin = X.arbitrary_bf16((rows, C + 16), 78).cuda() if mirror else None
        xin0 = xin.clone() if mirror else None
        cursor.fill_(s)
        got = ops.known_region_blend(xd, x0.cuda(), noise.cuda(), mask.cuda(), sig, step=(3 - s) if device_step else s,
                                     step_ptr=cursor if device_step else None, xin=xin)
        assert got is xd
        assert same(pad[:, :C], want), (s, "x")
        assert same(pad[:, C:], pad0[:, C:]), (s, "columns of x beyond C")
        if mirror:
            assert same(xin[:, :C], want) and same(xin[:, C:], xin0[:, C:]), (s, "xin")
    # the negative entry copies x0's bits where the mask is 0, which sigma = 0 does not (the planted -0 of x0 under a +0 noise)
    last, zero = R.blend(x, x0, noise, mask, -1.0), R.blend(x, x0, noise, mask, 0.0)
    assert not same(last, zero)


def test_blend_refusals():
    from textflux_amd import ops
    x, x0, noise, mask = (t.cuda() for t in blend_inputs(16, 64, 5, False))
    sig = SIGMA.cuda()
    keep = x.clone()
    for bad in (dict(x0=x), dict(noise=x), dict(mask=x)):
        with pytest.raises(RuntimeError, match="alias"):
            ops.known_region_blend(**dict(dict(x=x, x0=x0, noise=noise, mask=mask, keep_sigma=sig), **bad))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.known_region_blend(x[:, :12].contiguous(), x0[:, :12].contiguous(), noise[:, :12].contiguous(), mask[:, :12].contiguous(), sig)
    with pytest.raises(RuntimeError, match="ldxin"):
        ops.known_region_blend(x, x0, noise, mask, sig, xin=torch.zeros(16, 56, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="ldx"):
        ops.known_region_blend(torch.zeros(16, 68, dtype=BF, device="cuda")[:, :64], x0, noise, mask, sig)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.known_region_blend(torch.zeros(16, 72, dtype=BF, device="cuda")[:, 4:68], x0, noise, mask, sig)
    with pytest.raises(ValueError, match="outside the sigma table"):
        ops.known_region_blend(x, x0, noise, mask, sig, step=4)
    with pytest.raises(ValueError, match="contiguous and of x's shape"):
        ops.known_region_blend(x, x0[:8], noise, mask, sig)
    with pytest.raises(TypeError, match="bf16"):
        ops.known_region_blend(x, x0.float(), noise, mask, sig)
    with pytest.raises(TypeError, match="fp32"):
        ops.known_region_blend(x, x0, noise, mask, sig.double())
    empty = torch.zeros(0, 64, dtype=BF, device="cuda")
    assert ops.known_region_blend(empty, empty.clone(), empty.clone(), empty.clone(), sig) is empty
    assert torch.equal(x, keep)                                          # nothing was launched


# ----------------------------------------------------------------------------- tfx_keep_mask_pack alone
def pixel_mask(Hm, Wm, seed):
    """B = 2: sparse random 128s with 127s around them; 127 / 128 at the corners of 8 x 8 blocks, on and off the sampling lattice"""
    g = X.gen(seed)
    m = torch.where(torch.rand(2, Hm, Wm, generator=g) < 0.004, 128, 0).to(torch.uint8)
    m[torch.rand(2, Hm, Wm, generator=g) < 0.05] = 127
    m[0, 0, 0], m[0, 7, 7], m[0, 8, 8], m[0, 15, 15] = 128, 128, 127, 128
    m[1, 0, 0], m[1, Hm - 1, Wm - 1], m[1, Hm - 8, Wm - 8], m[1, 8, 0] = 127, 128, 127, 255
    return m


@pytest.mark.parametrize("mode,grow", [(0, 0), (1, 0), (1, 1), (1, 8)], ids=["nearest", "cover0", "cover1", "cover8"])
@pytest.mark.parametrize("Hm,Wm", [(16, 16), (32, 48), (64, 16)])
def test_keep_mask_pack_equals_the_restatement(Hm, Wm, mode, grow):
    from textflux_amd import ops
    m = pixel_mask(Hm, Wm, Hm + Wm)
    want = R.mask_pack(m, mode, grow)
    got = ops.keep_mask_pack(m.cuda(), 64, mode, grow)
    assert got.shape == (2, (Hm // 16) * (Wm // 16), 64) and got.dtype == BF
    assert same(got, want)
    assert set(got.float().unique().tolist()) <= {0.0, 1.0}
    assert same(ops.keep_mask_pack(m.cuda(), 64, {0: "nearest", 1: "cover"}[mode], grow), want)          # the mode by name
    if grow == 8:
        assert Hm // 8 <= 8 and (want.float().flatten(1).min(dim=1).values == 1).all()    # larger than the image: everything is masked


def test_keep_mask_pack_refusals():
    from textflux_amd import ops
    m = torch.zeros(1, 32, 48, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="grow must be 0"):
        ops.keep_mask_pack(m, 64, "nearest", 1)
    with pytest.raises(RuntimeError, match="outside 0..8"):
        ops.keep_mask_pack(m, 64, "cover", 9)
    with pytest.raises(RuntimeError, match="mode must be"):
        ops.keep_mask_pack(m, 64, 2, 0)
    with pytest.raises(ValueError, match="multiples of 16"):
        ops.keep_mask_pack(m[:, :24], 64)
    with pytest.raises(TypeError, match="uint8"):
        ops.keep_mask_pack(m.float(), 64)


# ----------------------------------------------------------------------------- the pipeline
def make_pipe(sname="euler", fp8=False):
    from tests.test_step_cache_gpu import make_pipe as base
    from textflux_amd.schedulers import FlowMatchMultistepScheduler
    pipe = base("amo" if sname == "amo" else "euler", fp8=fp8)
    if sname == "multistep":
        pipe.scheduler = FlowMatchMultistepScheduler.from_config(pipe.scheduler.config)
    if sname == "euler_unfused":
        pipe.fuse_euler_step = False
    return pipe


_inputs = {}


def inputs():
    """the call's tensors: drawn once, never modified"""
    if not _inputs:
        from tests.helpers import tiny_checkpoint as tc
        from tests.test_step_cache_gpu import T_TXT
        c = tc.TR_CFG
        g = torch.Generator().manual_seed(9)
        mask_u8 = torch.zeros(B, H, W, dtype=torch.uint8)
        mask_u8[:, :, W // 2:] = 255                                     # the right half is edited, the left half is known
        mask_u8[1, 40:56, 8:40] = 255                                    # and a block of sample 1's left half
        _inputs.update(
            call=dict(masked_image_latents=torch.cat([torch.randn(B, S, 64, generator=g), (torch.randn(B, S, 256, generator=g) > 0).float()], -1).to(BF).cuda(),
                      prompt_embeds=(torch.randn(B, T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF).cuda(),
                      pooled_prompt_embeds=torch.randn(B, c.pooled_projection_dim, generator=g).to(BF).cuda(),
                      height=H, width=W, num_inference_steps=N_STEPS, guidance_scale=30.0, output_type="latent"),
            latents=torch.randn(B, S, 64, generator=g).to(BF).cuda(),
            x0=torch.randn(B, S, 64, generator=g).to(BF).cuda(),
            mask_u8=mask_u8,
            amo_noise=[torch.randn(B, S, 64, generator=g) for _ in range(N_STEPS)])
        _inputs["mask"] = R.mask_pack(mask_u8, 0, 0).cuda()              # the restatement's, not the device kernel's
        assert 0 < _inputs["mask"].float().mean() < 1
    return _inputs


def call(pipe, latents=True, **kw):
    inp = inputs()
    if latents:
        kw.setdefault("latents", inp["latents"])
    out = pipe(**inp["call"], **kw).images
    assert out.shape == (B, S, 64) and torch.isfinite(out.float()).all()
    return out


def keep_kw(mask_u8=None, **kw):
    inp = inputs()
    return dict(dict(keep_known=True, image_latents=inp["x0"], mask_image=inp["mask_u8"] if mask_u8 is None else mask_u8), **kw)


def python_loop(pipe, sname, start=None, mask="default", per_step=None):
    inp = inputs()
    c = inp["call"]
    return R.loop(pipe, inp["latents"] if start is None else start, c["masked_image_latents"], c["prompt_embeds"], c["pooled_prompt_embeds"],
                  GRID, inp["x0"], inp["latents"], inp["mask"] if isinstance(mask, str) else mask,
                  sampler={"euler": "fused", "euler_unfused": "euler"}.get(sname, sname), amo_noise=inp["amo_noise"], per_step=per_step)


@pytest.mark.parametrize("sname", ["euler_unfused", "euler", "amo", "multistep"])
def test_step_run_ex_equals_the_python_issued_loop(sname):
    """eager, the captured graph (one for all steps, serving a second call), and the step cache that never skips"""
    pipe = make_pipe(sname)
    extra = dict(amo_noise=inputs()["amo_noise"]) if sname == "amo" else {}
    eager = call(pipe.enable_hip_graph(False), **keep_kw(), **extra)
    want = python_loop(pipe, sname)
    assert torch.equal(eager, want)
    plain = call(pipe, **extra)
    assert not torch.equal(plain, eager)                                # the blend does something
    ses = pipe.transformer._session
    assert not any(ses.graphs.values())
    graphed = call(pipe.enable_hip_graph(True), **keep_kw(), **extra)
    assert torch.equal(graphed, want)
    keys = [k for k, g in ses.graphs.items() if g]
    assert len(keys) == 1 and keys[0][-1] == "keep"
    assert torch.equal(call(pipe, **keep_kw(), **extra), want) and [k for k, g in ses.graphs.items() if g] == keys
    assert torch.equal(call(pipe, **extra), plain)                      # and the plain call still is the plain call, on a graph of its own
    for graph in (False, True):
        pipe.enable_hip_graph(graph)
        pipe.enable_step_cache(0.0)
        assert torch.equal(call(pipe, **keep_kw(), **extra), want), graph
        assert len(pipe.step_cache_report) == N_STEPS and not any(r["skipped"] for r in pipe.step_cache_report)
    pipe.enable_step_cache(0.0, skip_steps={2})                         # the cached tail ends in the same blend
    skipped = call(pipe, **keep_kw(), **extra)
    assert [r["skipped"] for r in pipe.step_cache_report] == [False, False, True, False]
    assert torch.equal(call(pipe.enable_hip_graph(False), **keep_kw(), **extra), skipped)
    known = inputs()["mask"] == 0
    assert torch.equal(skipped[known], inputs()["x0"][known])


@pytest.mark.parametrize("sname", ["euler", "multistep"])
def test_step_run_ex_with_fp8_linears(sname):
    pipe = make_pipe(sname, fp8=True)
    eager = call(pipe.enable_hip_graph(False), **keep_kw())
    assert torch.equal(eager, python_loop(pipe, sname))
    assert torch.equal(call(pipe.enable_hip_graph(True), **keep_kw()), eager)


@pytest.mark.parametrize("sname", ["euler_unfused", "euler", "amo", "multistep"])
def test_all_ones_mask_at_strength_1_is_the_plain_call(sname):
    pipe = make_pipe(sname)
    extra = dict(amo_noise=inputs()["amo_noise"]) if sname == "amo" else {}
    plain = call(pipe, **extra)
    ones = torch.full((B, H, W), 255, dtype=torch.uint8)
    assert torch.equal(call(pipe, **keep_kw(ones), strength=1.0, **extra), plain)
    assert torch.equal(call(pipe, **keep_kw(ones, keep_known=dict(mode="cover", grow=2)), **extra), plain)


def test_all_zeros_mask_returns_the_image_latents():
    pipe = make_pipe()
    zeros = torch.zeros(B, H, W, dtype=torch.uint8)
    for graph in (False, True):
        out = call(pipe.enable_hip_graph(graph), **keep_kw(zeros))
        assert same(out, inputs()["x0"])


def test_known_tokens_follow_the_noised_original_after_every_step():
    inp = inputs()
    pipe = make_pipe()
    seen = []
    out = call(pipe, **keep_kw(), callback_on_step_end=lambda p, i, t, kw: seen.append(kw["latents"].clone()) or {})
    assert len(seen) == N_STEPS and torch.equal(seen[-1], out) and pipe.num_timesteps == N_STEPS
    states = []
    want = python_loop(pipe, "euler_unfused", per_step=states)          # a callback: the unfused kernel
    assert torch.equal(out, want)
    tab = R.keep_sigma(pipe.scheduler._sigmas_host)
    known = (inp["mask"] == 0).cpu()
    assert known.any() and not known.all()
    for i in range(N_STEPS):
        assert torch.equal(seen[i], states[i]), i
        proper = R.scale_noise(inp["x0"].cpu(), float(tab[i]), inp["latents"].cpu())
        assert torch.equal(bits(seen[i].cpu())[known], bits(proper)[known]), i
    assert torch.equal(bits(out.cpu())[known], bits(inp["x0"].cpu())[known])                    # bit-equal to the original's
    assert not torch.equal(out.cpu()[~known], inp["x0"].cpu()[~known])
    assert torch.equal(call(pipe, **keep_kw()), out)                    # the fused form without the callback


def test_strength_runs_the_tail_of_the_grid_from_the_noised_original():
    inp = inputs()
    for sname in ("euler", "multistep"):
        pipe = make_pipe(sname)
        gen = lambda: torch.Generator(device="cuda").manual_seed(3)
        noise, _ = pipe.prepare_latents(B, 16, H, W, BF, torch.device("cuda"), gen())
        out = call(pipe, latents=False, generator=gen(), strength=0.5, **keep_kw())
        assert pipe.num_timesteps == 2 and pipe.scheduler.begin_index == 2
        sig = pipe.scheduler._sigmas_host
        start = R.scale_noise(inp["x0"].cpu(), float(sig[2]), noise.cpu()).cuda()
        c = inp["call"]
        want = R.loop(pipe, start, c["masked_image_latents"], c["prompt_embeds"], c["pooled_prompt_embeds"], GRID, inp["x0"], noise,
                      inp["mask"], sampler="fused" if sname == "euler" else sname)
        assert torch.equal(out, want), sname
        # strength alone: the same start, no blend
        out = call(pipe, latents=False, generator=gen(), strength=0.5, image_latents=inp["x0"])
        want = R.loop(pipe, start, c["masked_image_latents"], c["prompt_embeds"], c["pooled_prompt_embeds"], GRID, inp["x0"], noise,
                      None, sampler="fused" if sname == "euler" else sname)
        assert torch.equal(out, want) and pipe.num_timesteps == 2, sname
        # caller-given latents are both noise and start (the reference's quirk)
        out = call(pipe, strength=0.5, **keep_kw())
        assert torch.equal(out, python_loop(pipe, sname)) and pipe.num_timesteps == 2
        # and the next plain call starts at step 0 again
        assert torch.equal(call(pipe), call(make_pipe(sname)))
    with pytest.raises(ValueError, match="which is < 1 and not appropriate for this pipeline"):
        call(pipe, strength=0.0, **keep_kw())                           # int(4 - 0) = 4: no step left
    with pytest.raises(ValueError, match="need `image`"):
        call(pipe, strength=0.5)
    with pytest.raises(ValueError, match="needs `mask_image`"):
        call(pipe, keep_known=True, image_latents=inp["x0"])


def test_call_mixed_refuses_the_arguments():
    pipe = make_pipe()
    for kw in (dict(keep_known=True), dict(strength=0.5)):
        with pytest.raises(NotImplementedError, match="strength / keep_known"):
            pipe.call_mixed(sizes=[(256, 256), (384, 256)], latents=[torch.zeros(1, 256, 64), torch.zeros(1, 384, 64)],
                            masked_image_latents=[torch.zeros(1, 256, 320), torch.zeros(1, 384, 320)], prompt_embeds=torch.zeros(2, 64, 64),
                            pooled_prompt_embeds=torch.zeros(2, 128), output_type="latent", **kw)


# ----------------------------------------------------------------------------- end to end: image + mask + VAE
def test_end_to_end_the_extra_posterior_draw_comes_last(tmp_path):
    from tests.helpers import tiny_checkpoint as tc
    from tests.test_step_cache_gpu import T_TXT
    from textflux_amd.pipeline import FluxFillPipeline
    root = str(tmp_path / "pipe")
    tc.write_pipeline_dir(root, text=False)
    pipe = FluxFillPipeline.from_pretrained(root, text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None)
    pipe.set_progress_bar_config(disable=True)
    c = tc.TR_CFG
    g = torch.Generator().manual_seed(4)
    image = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros(B, H, W, dtype=torch.uint8)
    mask[:, 32:64, 32:96] = 255
    kw = dict(image=image, prompt_embeds=(torch.randn(B, T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF).cuda(),
              pooled_prompt_embeds=torch.randn(B, c.pooled_projection_dim, generator=g).to(BF).cuda(), height=H, width=W,
              num_inference_steps=2, guidance_scale=30.0, output_type="latent")
    gen = lambda: torch.Generator(device="cuda").manual_seed(11)
    drawn = []
    real = pipe._sample_and_pack

    def spy(moments, generator, dtype, dev, out=None, col0=0):
        res = real(moments, generator, dtype, dev, out=out, col0=col0)
        drawn.append(res[:, :, :64].clone())
        return res

    pipe._sample_and_pack = spy
    plain = pipe(mask_image=mask, generator=gen(), **kw).images
    assert len(drawn) == 1
    kept = pipe(mask_image=mask, generator=gen(), keep_known=True, **kw).images
    assert len(drawn) == 3 and torch.equal(drawn[1], drawn[0])          # the masked image's sample: the same draw as in the plain call
    x0 = drawn[2]
    assert not torch.equal(x0, drawn[0])                                # the unmasked image, from a later draw
    known = R.mask_pack(mask, 0, 0).cuda() == 0
    assert torch.equal(kept[known], x0[known]) and not torch.equal(kept, plain)
    ones = torch.full_like(mask, 255)
    assert torch.equal(pipe(mask_image=ones, generator=gen(), **kw).images,
                       pipe(mask_image=ones, generator=gen(), keep_known=True, strength=1.0, **kw).images)
    # strength < 1 from an image: two steps of four, from the noised x0, and a decoded image comes out
    out = pipe(mask_image=mask, generator=gen(), keep_known=dict(mode="cover", grow=1), strength=0.5,
               **dict(kw, num_inference_steps=4, output_type="pt")).images
    assert pipe.num_timesteps == 2 and out.shape == (B, 3, H, W) and torch.isfinite(out.float()).all()
