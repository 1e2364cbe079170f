"""The second-order multistep sampler on the GPU: tfx_multistep_step against the numpy restatement of helpers/multistep_ref.py bit
for bit (shape edges, host and device step index, a NaN history at step 0, refusals), FlowMatchMultistepScheduler.step over the
15-step analytic run, and the pipeline on the tiny model of tests/helpers/tiny_checkpoint.py (16 x 16 latent grid, B = 2, 4 steps):
eager == captured graph == the same forwards issued from Python followed by ops.multistep_step_, with the step cache, a step
callback, the fp8 linears and a runtime LoRA adapter."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import multistep_ref as R

BF = torch.bfloat16
N_STEPS = 4
GRID = "16x16"


def bits(t):
    return t.contiguous().view(torch.int16)


def to_np(t):
    return t.float().cpu().numpy()


def from_np(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF)


def rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF).cuda()


COEF3 = R.coef_table(R.shifted_sigmas(3, 1.15))


# ----------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("device_step", [False, True], ids=["host_step", "step_ptr"])
@pytest.mark.parametrize("rows,C,ldxin", [(1, 8, 0), (257, 8, 0), (33, 64, 128), (0, 64, 0)],
                         ids=["one_chunk", "second_workgroup_tail", "xin_mirror_ld128", "no_rows"])
def test_kernel_equals_the_restatement(rows, C, ldxin, device_step):
    from textflux_amd import ops
    coef = torch.from_numpy(COEF3).cuda()
    x = rnd((rows, C), 1)
    hist = rnd((rows, C), 2)                                          # arbitrary finite bits: step 0 must not look at them
    xin = rnd((rows, ldxin), 3) if ldxin else None
    xin0 = xin.clone() if ldxin else None
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref_x, ref_h = to_np(x), None
    for s in range(3):
        v = rnd((rows, C), 10 + s, 0.7)
        ref_x, ref_h = R.step(ref_x, to_np(v), ref_h, COEF3, s)
        cursor.fill_(s)
        # the index that is NOT in use points at another row of the table
        got = ops.multistep_step_(v, x, coef, hist, step=(2 - s) if device_step else s, step_ptr=cursor if device_step else None, xin=xin)
        assert got is x
        assert torch.equal(bits(x), bits(from_np(ref_x).cuda())), (s, "state")
        assert torch.equal(bits(hist), bits(v)), (s, "history")
        if ldxin:
            assert torch.equal(bits(xin[:, :C]), bits(x)) and torch.equal(bits(xin[:, C:]), bits(xin0[:, C:])), (s, "xin")
    assert rows == 0 or not torch.equal(x, rnd((rows, C), 1))


def test_a_nan_history_is_not_read_at_step_0():
    """a fresh history buffer holds arbitrary bits; 0 * NaN would poison the state if step 0 loaded it"""
    from textflux_amd import ops
    coef = torch.from_numpy(COEF3).cuda()
    for step_ptr in (None, torch.zeros(1, dtype=torch.int32, device="cuda")):
        x, v = rnd((33, 64), 4), rnd((33, 64), 5)
        hist = torch.full((33, 64), float("nan"), dtype=BF, device="cuda")
        want, _ = R.step(to_np(x), to_np(v), None, COEF3, 0)
        ops.multistep_step_(v, x, coef, hist, step=0, step_ptr=step_ptr)
        assert torch.isfinite(x.float()).all()
        assert torch.equal(bits(x), bits(from_np(want).cuda())) and torch.equal(bits(hist), bits(v))
    # from step 1 on the history IS read: the same call at step 1 carries the NaN through
    x, v = rnd((33, 64), 4), rnd((33, 64), 5)
    ops.multistep_step_(v, x, coef, torch.full((33, 64), float("nan"), dtype=BF, device="cuda"), step=1)
    assert torch.isnan(x.float()).all()


def test_refusals():
    from textflux_amd import ops
    coef = torch.from_numpy(COEF3).cuda()
    x, v, hist = rnd((16, 64), 6), rnd((16, 64), 7), rnd((16, 64), 8)
    x0 = x.clone()
    with pytest.raises(RuntimeError, match="alias"):
        ops.multistep_step_(v, x, coef, v)
    with pytest.raises(RuntimeError, match="alias"):
        ops.multistep_step_(v, x, coef, x)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.multistep_step_(rnd((16, 12), 7), rnd((16, 12), 6), coef, rnd((16, 12), 8))
    with pytest.raises(RuntimeError, match="ldxin"):
        ops.multistep_step_(v, x, coef, hist, xin=rnd((16, 56), 9))
    with pytest.raises(RuntimeError, match="ldxin"):
        ops.multistep_step_(v, x, coef, hist, xin=rnd((16, 68), 9))                 # wide enough, but rows that are not 16-byte aligned
    with pytest.raises(ValueError, match="outside the coefficient table"):
        ops.multistep_step_(v, x, coef, hist, step=3)
    with pytest.raises(TypeError, match="bf16"):
        ops.multistep_step_(v.float(), x, coef, hist)
    with pytest.raises(TypeError, match="bf16"):
        ops.multistep_step_(v, x, coef, hist.float())
    assert torch.equal(x, x0)                                         # nothing was launched


# ----------------------------------------------------------------------------- scheduler.step
def test_scheduler_step_follows_the_restatements_trajectory():
    from textflux_amd.schedulers import FlowMatchMultistepScheduler
    n, s2 = 15, 0.25
    sch = FlowMatchMultistepScheduler(use_dynamic_shifting=True)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cuda", mu=1.15)
    sig = sch._sigmas_host.numpy()
    x1 = np.random.default_rng(0).standard_normal(4096)
    traj = []
    _, err = R.run(n, "multistep", s2=s2, mu=1.15, x1=x1, sigmas=sig, trajectory=traj)
    x = from_np(R.bf16_round(x1.astype(np.float32))).cuda().view(1, 64, 64)
    for i, t in enumerate(sch.timesteps):
        sigma = float(sig[i])
        v = (x.double() * (sigma - (1.0 - sigma) * s2) / ((1.0 - sigma) ** 2 * s2 + sigma ** 2)).float().to(BF)     # the model, in torch
        new = sch.step(v, t, x, return_dict=False)[0]
        assert new is not x and new.shape == x.shape and sch.step_index == i + 1
        assert torch.equal(bits(new.view(-1)), bits(from_np(traj[i]).cuda())), i
        x = new
    want = R.exact(R.bf16_round(x1.astype(np.float32)), 0.0, s2)
    got = float(np.linalg.norm(to_np(x).reshape(-1) - want) / np.linalg.norm(want))
    print(f"15 steps on the device: relative error {got:.3e} (restatement {err:.3e})")
    assert got == err
    # the history is the scheduler's: set_timesteps drops it, another shape replaces it
    assert sch._v_prev is not None and sch._v_prev.shape == (1, 64, 64)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / 2, 2), device="cuda", mu=1.15)
    assert sch._v_prev is None and sch.step_index is None
    y = rnd((2, 8, 16), 3)
    out = sch.step(rnd((2, 8, 16), 4), sch.timesteps[0], y)
    assert sch._v_prev.shape == (2, 8, 16) and out.prev_sample.shape == y.shape and torch.isfinite(out.prev_sample.float()).all()


# ----------------------------------------------------------------------------- the pipeline
def make_pipe(sname="multistep", fp8=False):
    from tests.test_step_cache_gpu import make_pipe as base
    from textflux_amd.schedulers import FlowMatchMultistepScheduler
    pipe = base("amo" if sname == "amo" else "euler", fp8=fp8)
    if sname == "multistep":
        pipe.scheduler = FlowMatchMultistepScheduler.from_config(pipe.scheduler.config)
    return pipe


def inputs():
    from tests.test_step_cache_gpu import inputs as base
    return dict(base(GRID), num_inference_steps=N_STEPS)


def call(pipe, **kw):
    out = pipe(**inputs(), **kw).images
    assert out.shape == (2, 256, 64) and torch.isfinite(out.float()).all()
    return out


def per_step(pipe):
    """(the latents after every step, the final result) of an eager call with a callback that returns the latents unchanged"""
    seen = []
    out = call(pipe, callback_on_step_end=lambda p, i, t, kw: seen.append(kw["latents"].clone()) or {"latents": kw["latents"]})
    assert len(seen) == N_STEPS and torch.equal(seen[-1], out)
    return seen, out


def python_issued_loop(pipe):
    """helpers/plain_loop.py's loop with the multistep update: one forward per step issued from Python, then ops.multistep_step_.
    Call after a pipeline call: the scheduler then holds the call's timesteps."""
    from tests.helpers.plain_loop import mod_table
    from tests.test_step_cache_gpu import GRIDS
    from textflux_amd import ops
    inp, tr, sch = inputs(), pipe.transformer, pipe.scheduler
    B, S, C = inp["latents"].shape
    T = inp["prompt_embeds"].shape[1]
    assert len(sch.timesteps) == N_STEPS
    ses = tr.session(B, S, T)
    ses.set_conditioning(inp["prompt_embeds"], torch.zeros(T, 3), pipe._prepare_latent_image_ids(B, *GRIDS[GRID], "cuda", BF))
    coef = sch.coef_table("cuda")
    mod = mod_table(pipe, sch.timesteps, B, inp["pooled_prompt_embeds"], inp["guidance_scale"])
    lat = inp["latents"].clone()
    hist = torch.full_like(lat, float("nan"))
    ops.scatter_cols_(lat, ses.xin, 0)
    ops.scatter_cols_(inp["masked_image_latents"], ses.xin, C)
    states = []
    for i in range(N_STEPS):
        ops.multistep_step_(ses.run(mod[i]), lat, coef, hist, step=i, xin=ses.xin)
        states.append(lat.clone())
    return states


@pytest.mark.parametrize("variant", ["bf16", "fp8", "lora"])
def test_eager_graph_and_the_python_issued_loop_agree(variant):
    pipe = make_pipe(fp8=variant == "fp8")
    if variant == "lora":
        from oracle import flux_oracle as fo
        from tests.helpers import tiny_checkpoint as tc
        from tests.test_lora_runtime_gpu import RUNTIME_TARGETS, synthetic_lora
        lora, _ = synthetic_lora(fo.seeded_state_dict(tc.TR_CFG, 7), RUNTIME_TARGETS, 3)
        pipe.load_lora_weights(dict(lora), adapter_name="a", runtime=True)
    eager = call(pipe.enable_hip_graph(False))
    want = python_issued_loop(pipe)
    seen, with_callback = per_step(pipe)
    for i in range(N_STEPS):
        assert torch.equal(seen[i], want[i]), (variant, i)
    assert torch.equal(eager, want[-1]) and torch.equal(with_callback, eager)
    ses = pipe.transformer._session
    assert not any(ses.graphs.values())
    graphed = call(pipe.enable_hip_graph(True))
    assert torch.equal(graphed, eager)
    assert ses.graphs.get(("multistep", False)) and torch.equal(call(pipe), eager)      # ONE graph, and it serves a second call


def test_step_cache_that_never_skips_is_the_plain_loop_and_a_skip_schedule_runs():
    pipe = make_pipe()
    plain = call(pipe)
    for graph in (False, True):
        pipe.enable_hip_graph(graph)
        pipe.enable_step_cache(0.0)
        assert torch.equal(call(pipe), plain), graph
        assert len(pipe.step_cache_report) == N_STEPS and not any(r["skipped"] for r in pipe.step_cache_report)
    pipe.enable_step_cache(0.0, skip_steps={2})
    graphed = call(pipe)
    assert [r["skipped"] for r in pipe.step_cache_report] == [False, False, True, False] and not torch.equal(graphed, plain)
    assert torch.equal(call(pipe.enable_hip_graph(False)), graphed)             # the cached tail ends in the same update
    pipe.disable_step_cache()
    assert torch.equal(call(pipe), plain)


def test_the_result_is_the_samplers_own():
    ms, ms_final = per_step(make_pipe())
    euler = make_pipe("euler")
    eu, eu_final = per_step(euler)                                    # a callback: the unfused Euler kernel
    assert torch.equal(call(euler), eu_final)                         # ... which the fused form equals
    from tests.test_step_cache_gpu import amo_noise
    amo_final = call(make_pipe("amo"), amo_noise=amo_noise(GRID)[:N_STEPS])
    for i in range(1, N_STEPS):
        assert not torch.equal(ms[i], eu[i]), i
    assert not torch.equal(ms_final, eu_final) and not torch.equal(ms_final, amo_final)
    d0 = (ms[0].float() - eu[0].float()).abs().max().item()      # step 0 is Euler's step up to its rounding points
    d = (ms_final.float() - eu_final.float()).abs().mean().item()
    print(f"step 0 differs from Euler's by at most {d0:.3e}; final latents: MAE {d:.3e} against Euler's")


def test_call_mixed_refuses_the_sampler():
    pipe = make_pipe()
    with pytest.raises(NotImplementedError, match="multistep sampler"):
        pipe.call_mixed(sizes=[(256, 256), (384, 256)], latents=[torch.zeros(1, 256, 64), torch.zeros(1, 384, 64)],
                        masked_image_latents=[torch.zeros(1, 256, 320), torch.zeros(1, 384, 320)], prompt_embeds=torch.zeros(2, 64, 64),
                        pooled_prompt_embeds=torch.zeros(2, 128), output_type="latent")
