"""The first-block step cache on the GPU: the three passes alone against the same bf16 arithmetic in torch, and the pipeline switch
on the tiny model of tests/helpers/tiny_checkpoint.py (D = 256, 2 + 2 blocks, T = 64, 16 x 16 and 16 x 24 latent grids, B = 2,
6 steps): every step computed == the plain loop bit for bit, an explicit skip schedule == a reference the test assembles itself
from DitSession.run block ranges, threshold decisions == the decision function replayed on the reported metrics, graph == eager."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_oracle as fo
from tests.helpers import tiny_checkpoint as tc

BF = torch.bfloat16
T_TXT, N_STEPS, B = 64, 6, 2
GRIDS = {"16x16": (16, 16), "16x24": (16, 24)}
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
SENTINEL = 1234.0


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ----------------------------------------------------------------------------- the kernels alone
PAD_ROWS = 5      # rows in front of the view inside every sample: the origin is not the allocation's, the batch stride exceeds rows * D


class Passes:
    """hid as rows [PAD_ROWS, PAD_ROWS + rows) of a [B, PAD_ROWS + rows + 3, D] allocation, the cache's buffers, and the three entry points"""

    def __init__(self, rows, D, seed):
        from textflux_amd import _lib as L
        self.L, self.rows, self.D = L, rows, D
        self.full = torch.full((B, PAD_ROWS + rows + 3, D), SENTINEL, dtype=BF, device="cuda")
        self.hid = self.full[:, PAD_ROWS:PAD_ROWS + rows]
        self.hid.copy_(rnd((B, rows, D), seed).to(BF))
        self.x0 = (self.hid.float().cpu() + rnd((B, rows, D), seed + 1, 0.5)).to(BF).cuda()
        self.f_prev = ((self.hid.float() - self.x0.float()).cpu() + rnd((B, rows, D), seed + 2, 0.1)).to(BF).cuda()
        self.h1 = torch.full((B, rows, D), SENTINEL, dtype=BF, device="cuda")
        self.r = torch.full((B, rows, D), SENTINEL, dtype=BF, device="cuda")
        self.partials = torch.zeros(B * 512, dtype=torch.float32, device="cuda")
        self.metric = torch.full((B,), -1.0, dtype=torch.float32, device="cuda")
        self.desc = L.StepCache()
        for k in ("x0", "f_prev", "h1", "r", "partials", "metric"):
            setattr(self.desc, k, getattr(self, k).data_ptr())
        self.desc.ld, self.desc.bstride, self.desc.partials_bytes = D, rows * D, self.partials.numel() * 4

    def call(self, name):
        from textflux_amd import ops
        fn = getattr(self.L.lib(), "tfx_step_cache_" + name)
        self.L.check(fn(self.hid.data_ptr(), self.hid.stride(1), self.hid.stride(0), C.byref(self.desc), self.rows, B, self.D, ops._stream()), name)


def metric_bound(rows, D):
    """Relative bound of num and den, all terms non-negative: a term passes through at most L + log2(parts) fp32 additions, each
    with relative error 2^-24.  L, the longest sequential chain of the first kernel: a thread adds the 8 elements of each of its
    ceil(chunks / (parts * 256)) chunks in sequence, then the workgroup's tree has depth 8 (6 butterfly levels over the wave's 64 lanes,
    (w0 + w1) + (w2 + w3) over the 4 waves); the finishing kernel is a tree over the `parts` partial sums.  parts = min(256,
    ceil(chunks / 256)) as csrc/launch.h::step_cache_parts has it."""
    chunks = rows * D // 8
    parts = min(256, -(-chunks // 256))
    L = 8 * -(-chunks // (parts * 256)) + 8
    return (L + math.log2(parts)) * 2.0 ** -24, parts


@pytest.mark.parametrize("D", [256, 3072])
@pytest.mark.parametrize("rows", [1, 320, 777])
def test_passes_alone(rows, D):
    p = Passes(rows, D, seed=100 + rows + D)
    hid0, x00, fp0 = p.hid.clone(), p.x0.clone(), p.f_prev.clone()
    f_ref = (hid0.float() - x00.float()).to(BF)
    num = (f_ref.double() - fp0.double()).abs().sum(dim=(1, 2))
    den = fp0.double().abs().sum(dim=(1, 2))
    # ---- metric
    p.call("metric")
    assert torch.equal(p.x0, f_ref) and torch.equal(p.h1, hid0) and torch.equal(p.hid, hid0) and torch.equal(p.f_prev, fp0)
    got = p.metric.double()
    bound, parts = metric_bound(rows, D)
    rel = ((got - num / den).abs() / (num / den)).max().item()
    print(f"rows {rows} D {D}: {parts} partials per sample, metric {got.tolist()}, relative error {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound, (rel, bound)
    # ---- the same inputs give the same bits
    first = p.metric.clone()
    p.x0.copy_(x00)
    p.metric.fill_(-1.0)
    p.call("metric")
    assert torch.equal(p.metric, first) and torch.equal(p.x0, f_ref)
    # ---- a sample whose f_prev is zero reports +inf; its neighbour's bits do not change
    p.x0.copy_(x00)
    p.f_prev[0].zero_()
    p.call("metric")
    assert math.isinf(p.metric[0].item()) and p.metric[0].item() > 0 and p.metric[1].item() == first[1].item()
    p.f_prev.copy_(fp0)
    # ---- store: hid has moved on (the blocks behind block 0)
    hid1 = (hid0.float().cpu() + rnd((B, rows, D), 7, 0.3)).to(BF).cuda()
    p.hid.copy_(hid1)
    p.call("store")
    r_ref = (hid1.float() - hid0.float()).to(BF)
    assert torch.equal(p.r, r_ref) and torch.equal(p.f_prev, f_ref) and torch.equal(p.hid, hid1) and torch.equal(p.h1, hid0)
    # ---- apply on a fresh state behind block 0
    hid2 = (hid0.float().cpu() + rnd((B, rows, D), 8, 0.05)).to(BF).cuda()
    p.hid.copy_(hid2)
    p.call("apply")
    assert torch.equal(p.hid, (hid2.float() + r_ref.float()).to(BF)) and torch.equal(p.r, r_ref)
    # nothing outside the view was written
    assert (p.full[:, :PAD_ROWS] == SENTINEL).all() and (p.full[:, PAD_ROWS + rows:] == SENTINEL).all()


# ----------------------------------------------------------------------------- the pipeline
_sd = {}


def state_dict():
    if not _sd:
        _sd.update({k: v.to(BF) for k, v in fo.seeded_state_dict(tc.TR_CFG, 7).items()})
    return _sd


def make_pipe(sname="euler", fp8=False):
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler, StochasticRFOvershotDiscreteScheduler
    from textflux_amd.transformer import FluxTransformer2DModel

    class _VaeCfg:   # output_type "latent" with injected masked_image_latents: only the VAE's config is consulted
        class config:
            block_out_channels = (128, 256, 512, 512)
            latent_channels = 16
            scaling_factor, shift_factor = 0.3611, 0.1159

    c = tc.TR_CFG
    tr = FluxTransformer2DModel(in_channels=c.in_channels, out_channels=c.out_channels, num_layers=c.num_layers,
                                num_single_layers=c.num_single_layers, num_attention_heads=c.num_attention_heads,
                                joint_attention_dim=c.joint_attention_dim, pooled_projection_dim=c.pooled_projection_dim,
                                guidance_embeds=True).load_state_dict(state_dict(), device="cuda")
    if fp8:
        tr.enable_fp8()
    if sname == "euler":
        sch = FlowMatchEulerDiscreteScheduler(**SCHED)
    else:
        sch = StochasticRFOvershotDiscreteScheduler(**SCHED)
        sch.set_c(2.0)
        sch.set_overshot_func(lambda t, dt: t + dt)
    pipe = FluxFillPipeline(scheduler=sch, vae=_VaeCfg(), text_encoder=None, tokenizer=None, text_encoder_2=None, tokenizer_2=None,
                            transformer=tr)
    pipe.set_progress_bar_config(disable=True)
    return pipe


_inputs = {}


def inputs(grid, seed=5):
    """the call's tensors for a latent grid: drawn once, never modified"""
    if (grid, seed) not in _inputs:
        h2, w2 = GRIDS[grid]
        S, c = h2 * w2, tc.TR_CFG
        g = torch.Generator().manual_seed(seed)
        _inputs[(grid, seed)] = dict(
            latents=torch.randn(B, S, 64, generator=g).to(BF).cuda(),
            masked_image_latents=torch.cat([torch.randn(B, S, 64, generator=g), (torch.randn(B, S, 256, generator=g) > 0).float()], -1).to(BF).cuda(),
            prompt_embeds=(torch.randn(B, T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF).cuda(),
            pooled_prompt_embeds=torch.randn(B, c.pooled_projection_dim, generator=g).to(BF).cuda(),
            height=h2 * 16, width=w2 * 16, num_inference_steps=N_STEPS, guidance_scale=30.0, output_type="latent")
    return _inputs[(grid, seed)]


def amo_noise(grid):
    h2, w2 = GRIDS[grid]
    return [rnd((B, h2 * w2, 64), 50 + i) for i in range(N_STEPS)]


def call(pipe, grid, **kw):
    out = pipe(**inputs(grid), **kw).images
    assert out.shape == (B, GRIDS[grid][0] * GRIDS[grid][1], 64) and torch.isfinite(out.float()).all()
    return out


def skipped(pipe):
    return [r["skipped"] for r in pipe.step_cache_report]


@pytest.mark.parametrize("variant", ["euler_fused", "euler_unfused", "amo", "fp8", "lora"])
def test_all_computed_equals_the_plain_loop(variant):
    """threshold 0 never skips: phases 1 + 2 issue the launches of a whole step, so the latents are the plain loop's bit for bit --
    eager and as captured graphs -- and the report shows six computed steps with a metric per sample (step 0: +inf, no reference yet)."""
    grid = "16x24" if variant == "euler_unfused" else "16x16"
    pipe = make_pipe("amo" if variant == "amo" else "euler", fp8=variant == "fp8")
    pipe.fuse_euler_step = variant != "euler_unfused"
    if variant == "lora":           # a runtime (unmerged) adapter on double and single blocks: the block-range forward carries it
        from tests.test_lora_runtime_gpu import RUNTIME_TARGETS, synthetic_lora
        lora, _ = synthetic_lora(fo.seeded_state_dict(tc.TR_CFG, 7), RUNTIME_TARGETS, 3)
        pipe.load_lora_weights(dict(lora), adapter_name="a", runtime=True)
    kw = dict(amo_noise=amo_noise(grid)) if variant == "amo" else {}
    for graph in (False, True):
        pipe.enable_hip_graph(graph)
        pipe.disable_step_cache()
        plain = call(pipe, grid, **kw)
        pipe.enable_step_cache(0.0)
        cached = call(pipe, grid, **kw)
        assert torch.equal(cached, plain), (variant, graph)
        rep = pipe.step_cache_report
        assert len(rep) == N_STEPS and not any(skipped(pipe))
        assert all(len(r["metric"]) == B for r in rep) and all(math.isinf(m) for m in rep[0]["metric"])
        assert all(math.isfinite(m) and m > 0 for r in rep[1:] for m in r["metric"]), rep
    ses = pipe.transformer._session
    assert ses.cache is not None and sum(1 for k in ses.graphs if "step_cache" in k) == 3 and all(ses.graphs.values())


def reference_with_schedule(pipe, grid, skip):
    """The loop with `skip` assembled from block-range forwards (DitSession.run: first_block / last_block / flags) and torch bf16
    arithmetic for the residual and its re-use, inside helpers/plain_loop.py's loop: Euler update by the separate scheduler kernel.
    Call after a pipeline call at this geometry: the scheduler then holds the call's timesteps and coefficients."""
    from tests.helpers.plain_loop import plain_loop
    inp = inputs(grid)
    nblk = tc.TR_CFG.num_layers + tc.TR_CFG.num_single_layers
    assert len(pipe.scheduler.timesteps) == N_STEPS
    state = {}

    def forward(ses, mod_i, i):
        img = ses.hid[:, T_TXT:]
        ses.run(mod_i, 0, 0, flags=2)                         # embedders
        ses.run(mod_i, 0, 1, flags=3)                         # block 0
        if i in skip:
            img.copy_((img.float() + state["r"].float()).to(BF))
            return ses.run(mod_i, nblk, nblk, flags=1)        # norm_out + proj_out
        h1 = img.clone()
        v = ses.run(mod_i, 1, -1, flags=1)                    # blocks 1 ... n, norm_out + proj_out
        state["r"] = (img.float() - h1.float()).to(BF)
        return v

    return plain_loop(pipe, inp["latents"], inp["masked_image_latents"], inp["prompt_embeds"], inp["pooled_prompt_embeds"], GRIDS[grid],
                      forward=forward)


def test_explicit_schedule_equals_the_block_range_reference_and_resets_between_calls():
    grid, skip = "16x24", {2, 4, 5}
    pipe = make_pipe()
    plain = call(pipe, grid)
    ref = reference_with_schedule(pipe, grid, skip)
    assert torch.equal(reference_with_schedule(pipe, grid, set()), plain)        # the reference's own plumbing
    pipe.enable_step_cache(0.0, skip_steps=skip)
    eager = call(pipe, grid)
    assert skipped(pipe) == [i in skip for i in range(N_STEPS)]
    assert torch.equal(eager, ref)
    assert not torch.equal(eager, plain)
    print(f"skip {sorted(skip)}: latent MAE vs the plain loop {(eager.float() - plain.float()).abs().mean().item():.3e}")
    pipe.enable_hip_graph(True)
    graphed = call(pipe, grid)
    assert torch.equal(graphed, eager) and skipped(pipe) == [i in skip for i in range(N_STEPS)]
    # nothing leaks across calls: another schedule in between, then the same call again -- same session, same graphs, same bits
    pipe.enable_step_cache(0.0, skip_steps={1, 3})
    other = call(pipe, grid)
    assert not torch.equal(other, eager)
    pipe.enable_step_cache(0.0, skip_steps=skip)
    handles = dict(pipe.transformer._session.graphs)
    assert torch.equal(call(pipe, grid), eager) and torch.equal(call(pipe, grid), eager)
    assert dict(pipe.transformer._session.graphs) == handles
    # unfused Euler and a step callback (the eager loop with the latents as a tensor every step) take the same decisions
    pipe.enable_hip_graph(False)
    seen = []
    assert torch.equal(call(pipe, grid, callback_on_step_end=lambda p, i, t, kw: seen.append(kw["latents"].clone()) or {}), eager)
    assert len(seen) == N_STEPS and torch.equal(seen[-1], eager)
    pipe.fuse_euler_step = False
    assert torch.equal(call(pipe, grid), eager)
    pipe.disable_step_cache()
    assert torch.equal(call(pipe, grid), plain)


def test_threshold_decisions_follow_the_reported_metrics():
    from textflux_amd.step_cache import StepCacheConfig, replay
    grid = "16x16"
    pipe = make_pipe().enable_hip_graph(True)
    pipe.enable_step_cache(0.0)
    call(pipe, grid)
    worst = sorted(max(r["metric"]) for r in pipe.step_cache_report[1:])
    print("largest metric per step, threshold 0:", [max(r["metric"]) for r in pipe.step_cache_report])
    assert worst[0] < worst[1], worst                       # a threshold fits between the two smallest
    thr = 0.5 * (worst[0] + worst[1])
    pipe.enable_step_cache(thr)
    got = call(pipe, grid)
    rep = pipe.step_cache_report
    flags = skipped(pipe)
    print(f"threshold {thr:.4f}: skipped {flags}, largest metric per step {[max(r['metric']) for r in rep]}")
    assert any(flags) and not all(flags) and not flags[0]
    assert flags == replay(StepCacheConfig.make(thr), [r["metric"] for r in rep])
    pipe.enable_step_cache(0.0, skip_steps={i for i, s in enumerate(flags) if s})
    assert torch.equal(call(pipe, grid), got) and skipped(pipe) == flags
    pipe.enable_hip_graph(False)
    pipe.enable_step_cache(thr)
    assert torch.equal(call(pipe, grid), got) and skipped(pipe) == flags


def test_consecutive_cap():
    pipe = make_pipe()
    pipe.enable_step_cache(float("inf"), max_consecutive=2)
    call(pipe, "16x16")
    assert skipped(pipe) == [False, True, True, False, True, True]
    pipe.enable_step_cache(float("inf"))
    call(pipe, "16x16")
    assert skipped(pipe) == [False] + [True] * (N_STEPS - 1)


def test_call_mixed_refuses_the_cache():
    pipe = make_pipe()
    pipe.enable_step_cache(0.1)
    with pytest.raises(NotImplementedError, match="step cache"):
        pipe.call_mixed(sizes=[(256, 256), (384, 256)], latents=[torch.zeros(1, 256, 64), torch.zeros(1, 384, 64)],
                        masked_image_latents=[torch.zeros(1, 256, 320), torch.zeros(1, 384, 320)], prompt_embeds=torch.zeros(2, T_TXT, 64),
                        pooled_prompt_embeds=torch.zeros(2, 128), output_type="latent")
