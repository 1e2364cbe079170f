"""True CFG on the device (DESIGN.md section 4 "True CFG"): tfx_cfg_combine against the restatement that equals the reference bit for
bit (tests/test_true_cfg_cpu.py); tfx_dit_step_run_ex3 inside the pipeline against the same launches issued from Python, for every
unfused sampler and both blends, eager and captured; the pipeline against the reference's loop written with the literal torch
expression and scheduler.step; off is off; both halves of the doubled batch stay in step; one graph serves every scale.  Tiny
checkpoint (helpers/tiny_checkpoint.py), 128 x 128 (64 image tokens), B = 2 (sessions of 4)."""
import os

import pytest
import torch
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu

from tests.helpers import change_map_ref as CM
from tests.helpers import keep_known_ref as KK
from tests.helpers import true_cfg_ref as R

BF = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 2, 128, 128
GRID = (H // 16, W // 16)
S = GRID[0] * GRID[1]
G = 3.3                                                                     # tells the wrong variants apart (test_true_cfg_cpu.py)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ----------------------------------------------------------------------------- tfx_cfg_combine alone
_gold = {}


def gold():
    if not _gold:
        _gold.update(load_file(os.path.join(REPO, "tests", "golden", "g18_true_cfg.safetensors")))
    return _gold


_operands = {}


def operands(rows, C):
    """neg, pos [rows, C] on the host, drawn once; the first 12 rows of a 64-column pair are g18's, planted special values included"""
    if (rows, C) not in _operands:
        neg, pos = rnd((rows, C), 100 + rows, 0.5).to(BF), rnd((rows, C), 200 + rows, 0.5).to(BF)
        if C == 64 and rows >= 12:
            neg[:12], pos[:12] = gold()["neg"].view(12, 64), gold()["pos"].view(12, 64)
        _operands[(rows, C)] = (neg, pos)
    return _operands[(rows, C)]


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("g", R.SCALES)
@pytest.mark.parametrize("rows,C", [(1, 8), (37, 64), (513, 64)], ids=["one_chunk", "296_chunks", "4104_chunks"])
def test_combine_equals_the_restatement(rows, C, g, in_place):
    from textflux_amd import ops
    neg, pos = operands(rows, C)
    want = R.combine(neg, pos, g)
    if C == 64 and rows >= 12:                                              # the planted rows are the fixture's: the reference's own bits
        assert R.same(want[:12], gold()[f"g{R.SCALES.index(g)}_combined"].view(12, 64))
        # planted: inf - inf on four pairs and a NaN on either side give six NaNs, a finite neg under an infinite pos two infinities
        assert torch.isnan(want[:12]).sum() >= 6 and torch.isinf(want[:12]).sum() >= 2
    scale = torch.tensor([g], dtype=torch.float32, device="cuda")
    dn, dp = neg.cuda(), pos.cuda()
    guard = torch.full((rows + 2, C), 77.0, dtype=BF, device="cuda")       # a row in front of and behind a separate out
    out = dn if in_place else guard[1:rows + 1]
    got = ops.cfg_combine(dn, dp, scale, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert R.same(got, want), R.differing(got.cpu(), want)
    assert torch.equal(R.bits(dp.cpu()), R.bits(pos)) and (in_place or torch.equal(R.bits(dn.cpu()), R.bits(neg)))   # bits: the operands hold NaNs
    assert (guard[0] == 77.0).all() and (guard[-1] == 77.0).all()
    if not in_place:
        assert R.same(ops.cfg_combine(dn, dp, scale), want)                 # out=None: a new tensor
    if g == G:
        assert not R.same(got, R.combine_scale_in_bf16(neg, pos, g)) or rows == 1
        assert not R.same(got, R.combine_single_rounding(neg, pos, g)) or rows == 1


def test_combine_reads_the_scale_when_it_runs():
    from textflux_amd import ops
    neg, pos = operands(37, 64)
    scale = torch.tensor([1.5], dtype=torch.float32, device="cuda")
    dn, dp = neg.cuda(), pos.cuda()
    assert R.same(ops.cfg_combine(dn, dp, scale), R.combine(neg, pos, 1.5))
    scale.fill_(7.0)
    assert R.same(ops.cfg_combine(dn, dp, scale), R.combine(neg, pos, 7.0))


def test_combine_refusals_and_empty_launch_nothing():
    from textflux_amd import _lib as L
    from textflux_amd import ops
    lib = L.lib()
    neg, pos = (t.cuda() for t in operands(37, 64))
    scale = torch.tensor([G], dtype=torch.float32, device="cuda")
    out = torch.full((37, 64), 5.0, dtype=BF, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda n=neg.data_ptr(), p=pos.data_ptr(), o=out.data_ptr(), Cc=64, rows=37, s=scale.data_ptr(): lib.tfx_cfg_combine(n, p, o, Cc, rows, s, st)
    assert call(rows=0) == 0                                                # rows == 0 launches nothing
    for kw, msg in ((dict(Cc=12), b"multiple of 8"), (dict(Cc=0), b"multiple of 8"), (dict(rows=-1), b"negative row count"),
                    (dict(n=None), b"null pointer"), (dict(p=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(s=None), b"null pointer"),
                    (dict(o=out.data_ptr() + 2), b"16-byte aligned"), (dict(n=neg.data_ptr() + 8), b"16-byte aligned"),
                    (dict(o=pos.data_ptr()), b"must not overlap v_pos"), (dict(o=pos.data_ptr() + 16, rows=36), b"must not overlap v_pos"),
                    (dict(n=out.data_ptr() + 16, rows=36), b"v_neg itself or not overlap")):
        assert call(**kw) != 0 and msg in lib.tfx_last_error(), kw
    torch.cuda.synchronize()
    assert (out == 5.0).all() and all(torch.equal(R.bits(t.cpu()), R.bits(o)) for t, o in zip((neg, pos), operands(37, 64)))
    with pytest.raises(TypeError, match="bf16"):
        ops.cfg_combine(neg.float(), pos.float(), scale)
    with pytest.raises(TypeError, match="scale"):
        ops.cfg_combine(neg, pos, torch.ones(2, device="cuda"))
    with pytest.raises(ValueError, match="one shape"):
        ops.cfg_combine(neg, pos[:36], scale)
    with pytest.raises(ValueError, match="contiguous"):
        ops.cfg_combine(neg[:, :32], pos[:, :32], scale)
    empty = torch.empty(0, 64, dtype=BF, device="cuda")
    assert ops.cfg_combine(empty, empty.clone(), scale).shape == (0, 64)


# ----------------------------------------------------------------------------- the pipeline
def make_pipe(sname="euler", fp8=False):
    """the tiny pipeline of the known-region tests with an encode_prompt that is a fixed function of the strings (it has no text encoders)"""
    from tests.test_keep_known_gpu import make_pipe as base
    from tests.test_step_cache_gpu import T_TXT
    from tests.helpers import tiny_checkpoint as tc
    pipe = base(sname, fp8=fp8)
    c = tc.TR_CFG

    def row(p):
        g = torch.Generator().manual_seed(sum(p.encode()) % 100003)
        return (torch.randn(T_TXT, c.joint_attention_dim, generator=g) * 0.1).to(BF), torch.randn(c.pooled_projection_dim, generator=g).to(BF)

    def encode_prompt(prompt, prompt_2, device=None, num_images_per_prompt=1, prompt_embeds=None, pooled_prompt_embeds=None,
                      max_sequence_length=512, lora_scale=None):
        if prompt_embeds is None:
            ps = [prompt] if isinstance(prompt, str) else list(prompt)
            rows = [row(p) for p in ps]
            prompt_embeds, pooled_prompt_embeds = torch.stack([r[0] for r in rows]).cuda(), torch.stack([r[1] for r in rows]).cuda()
        return prompt_embeds, pooled_prompt_embeds, torch.zeros(prompt_embeds.shape[1], 3, device="cuda", dtype=BF)

    pipe.encode_prompt = encode_prompt
    pipe.encoded = lambda prompts: encode_prompt(prompts, None)[:2]
    return pipe


_inputs = {}
PROMPTS, NEGATIVE = ["a sign that says OPEN", "a shop front"], "blurry, smudged letters"


def inputs(n_steps=3):
    """the call's tensors: drawn once, never modified"""
    if n_steps not in _inputs:
        g = torch.Generator().manual_seed(11)
        mask_u8 = torch.zeros(B, H, W, dtype=torch.uint8)
        mask_u8[:, :, W // 2:] = 255
        mask_u8[1, 40:56, 8:40] = 255
        grey = (torch.arange(W) * 255 // (W - 1)).to(torch.uint8)[None, None, :].repeat(B, H, 1)
        grey[1] = torch.randint(0, 256, (H, W), generator=g).to(torch.uint8)
        _inputs[n_steps] = dict(
            call=dict(masked_image_latents=torch.cat([torch.randn(B, S, 64, generator=g), (torch.randn(B, S, 256, generator=g) > 0).float()], -1).to(BF).cuda(),
                      height=H, width=W, num_inference_steps=n_steps, guidance_scale=30.0, output_type="latent"),
            latents=torch.randn(B, S, 64, generator=g).to(BF).cuda(),
            x0=torch.randn(B, S, 64, generator=g).to(BF).cuda(),
            mask_u8=mask_u8, mask=KK.mask_pack(mask_u8, 0, 0).cuda(), grey=grey, hold=CM.pack(grey, 0, 0),
            amo_noise=[torch.randn(B, S, 64, generator=g) for _ in range(n_steps)])
    return _inputs[n_steps]


def call(pipe, n_steps=3, prompt=PROMPTS, **kw):
    inp = inputs(n_steps)
    kw.setdefault("latents", inp["latents"])
    out = pipe(prompt=prompt, **inp["call"], **kw).images
    assert out.shape == (B, S, 64) and torch.isfinite(out.float()).all()
    return out


def python_launches(pipe, sname, g=G, **kw):
    inp = inputs()
    (pe, pooled), (npe, npooled) = pipe.encoded(PROMPTS), pipe.encoded([NEGATIVE] * B)
    return R.launch_loop(pipe, inp["latents"], inp["call"]["masked_image_latents"], pe, pooled, npe, npooled, GRID, g,
                         sampler={"euler_unfused": "euler"}.get(sname, sname), amo_noise=inp["amo_noise"], **kw)


CASES = {"euler": ("euler", {}), "amo": ("amo", {}), "multistep": ("multistep", {}), "euler_keep_known": ("euler", dict(keep=True)),
         "multistep_change_map": ("multistep", dict(change=True))}


@pytest.mark.parametrize("case", list(CASES))
def test_step_run_ex3_equals_the_python_issued_launches(case):
    """eager, then the captured graph (one for all steps), against forward on 2B -> ops.cfg_combine -> the sampler's op -> the blend ->
    the copy into the second half of xin, issued from Python"""
    sname, blend = CASES[case]
    inp = inputs()
    pipe = make_pipe(sname)
    kw, loop_kw = dict(negative_prompt=NEGATIVE, true_cfg=G), {}
    if sname == "amo":
        kw["amo_noise"] = inp["amo_noise"]
    if blend.get("keep"):
        kw.update(keep_known=True, image_latents=inp["x0"], mask_image=inp["mask_u8"])
        loop_kw["keep"] = dict(x0=inp["x0"], noise=inp["latents"], mask=inp["mask"])
    if blend.get("change"):
        kw.update(change_map=dict(map=inp["grey"], last="keep"), image_latents=inp["x0"], mask_image=inp["mask_u8"])
        loop_kw["change"] = dict(x0=inp["x0"], noise=inp["latents"], hold=inp["hold"], last="keep")
    pipe.enable_hip_graph(False)
    eager = call(pipe, **kw)
    assert pipe.num_timesteps == 3
    ses = pipe.transformer._session
    assert (ses.B, ses.S) == (2 * B, S) and not any(ses.graphs.values())
    want = python_launches(pipe, sname, **loop_kw)
    assert torch.equal(eager, want)
    C = 64
    assert torch.equal(ses.xin[:B, :, :C], want) and torch.equal(ses.xin[B:, :, :C], want)               # both halves of xin hold the new latents
    plain_kw = {k: v for k, v in kw.items() if k not in ("negative_prompt", "true_cfg")}
    assert not torch.equal(call(make_pipe(sname), **plain_kw), want)                                      # the negative prompt matters
    pipe.enable_hip_graph(True)
    assert torch.equal(call(pipe, **kw), want)
    keys = [k for k, h in pipe.transformer._session.graphs.items() if h]
    assert len(keys) == 1 and keys[0][-1] == "cfg"                                                       # one graph, whatever the number of steps
    assert torch.equal(call(pipe, **kw), want) and [k for k, h in pipe.transformer._session.graphs.items() if h] == keys


@pytest.mark.parametrize("case", ["bf16", "fp8", "callback", "negative_embeds"])
def test_pipeline_equals_the_references_loop(case):
    """the reference's loop (pipeline_flux_with_cfg.py:778-812) on the engine's forward: torch.cat of the latents, the combine as the
    literal torch expression, scheduler.step"""
    inp = inputs()
    pipe = make_pipe("euler", fp8=case == "fp8")
    (pe, pooled), (npe, npooled) = pipe.encoded(PROMPTS), pipe.encoded([NEGATIVE] * B)
    replacement = rnd((B, S, 64), 77).to(BF).cuda()
    kw, on_step = dict(negative_prompt=NEGATIVE), None
    if case == "negative_embeds":                                           # embeds alone switch it on here
        kw = dict(negative_prompt_embeds=npe, negative_pooled_prompt_embeds=npooled)
    if case == "callback":
        seen = []

        def cb(p, i, t, tensors):
            seen.append((i, tuple(tensors["latents"].shape)))
            return {"latents": replacement} if i == 1 else {}

        kw["callback_on_step_end"] = cb
        on_step = lambda i, lat: replacement if i == 1 else None
    got = call(pipe, true_cfg=G, **kw)
    if case == "callback":
        assert seen == [(i, (B, S, 64)) for i in range(3)]                  # the callback sees the B-sample latents
    want = R.loop(pipe, inp["latents"], inp["call"]["masked_image_latents"], pe, pooled, npe, npooled, GRID, G, on_step=on_step)
    assert torch.equal(got, want)
    if case == "callback":
        assert not torch.equal(want, R.loop(pipe, inp["latents"], inp["call"]["masked_image_latents"], pe, pooled, npe, npooled, GRID, G))


def test_off_is_off():
    """true_cfg = 1 with a negative prompt, and true_cfg = 3 without one, are the call without the arguments: same latents, the fused
    Euler step, no session of 2B"""
    pipe = make_pipe("euler")
    made = []
    real = pipe.transformer.session
    pipe.transformer.session = lambda Bs, *a, **k: (made.append(Bs), real(Bs, *a, **k))[1]
    plain = call(pipe)
    off1 = call(pipe, negative_prompt=NEGATIVE, true_cfg=1.0)
    off2 = call(pipe, true_cfg=3.0)
    off3 = call(pipe, negative_prompt=NEGATIVE)
    assert torch.equal(off1, plain) and torch.equal(off2, plain) and torch.equal(off3, plain)
    assert made == [B] * 4 and pipe.transformer._session.B == B
    on = call(pipe, negative_prompt=NEGATIVE, true_cfg=1.5)
    assert made[-1] == 2 * B and not torch.equal(on, plain)


def test_both_halves_stay_in_step():
    """negative_prompt == prompt makes d zero everywhere: whatever the scale, four CFG steps are four plain unfused steps -- unless the
    two halves of xin drift apart.  With the GEMM and attention forms whose bits do not depend on the batch."""
    from textflux_amd import ops
    ops.set_option("gemm_splitk", 0)
    ops.set_option("attention_streamk", 0)
    try:
        plain_pipe = make_pipe("euler_unfused")
        plain = call(plain_pipe, n_steps=4)
        assert plain_pipe.transformer._session.B == B
        for g in (G, 30.0):
            pipe = make_pipe("euler")
            got = call(pipe, n_steps=4, negative_prompt=PROMPTS, true_cfg=g)
            ses = pipe.transformer._session
            assert ses.B == 2 * B and torch.equal(got, plain), g
            assert torch.equal(ses.xin[:B], ses.xin[B:])
    finally:
        ops.set_option("gemm_splitk", 2)
        ops.set_option("attention_streamk", 1)


def test_a_captured_graph_sees_a_new_scale():
    pipe = make_pipe("euler").enable_hip_graph(True)
    first = call(pipe, negative_prompt=NEGATIVE, true_cfg=2.0)
    ses = pipe.transformer._session
    handles = {k: h for k, h in ses.graphs.items() if h}
    assert len(handles) == 1 and list(handles)[0][-1] == "cfg"
    second = call(pipe, negative_prompt=NEGATIVE, true_cfg=5.0)
    assert pipe.transformer._session is ses and {k: h for k, h in ses.graphs.items() if h} == handles        # no new capture
    fresh = call(make_pipe("euler").enable_hip_graph(False), negative_prompt=NEGATIVE, true_cfg=5.0)
    assert torch.equal(second, fresh) and not torch.equal(second, first)
    assert torch.equal(call(pipe, negative_prompt=NEGATIVE, true_cfg=2.0), first)


def test_refusals_when_on():
    pipe = make_pipe("euler")
    pipe.enable_step_cache(0.1)
    with pytest.raises(NotImplementedError, match="step cache"):
        call(pipe, negative_prompt=NEGATIVE, true_cfg=2.0)
    pipe.disable_step_cache()

    class Foreign:
        config = pipe.scheduler.config
        order = 1

        def set_timesteps(self, num_inference_steps=None, device=None, sigmas=None, mu=None):
            pipe_sched.set_timesteps(num_inference_steps, device=device, sigmas=sigmas, mu=mu)
            self.timesteps, self.sigmas = pipe_sched.timesteps, pipe_sched.sigmas

    pipe_sched = pipe.scheduler
    pipe.scheduler = Foreign()
    with pytest.raises(NotImplementedError, match="engine's schedulers"):
        call(pipe, negative_prompt=NEGATIVE, true_cfg=2.0)
    pipe.scheduler = pipe_sched
    with pytest.raises(ValueError, match="Negative prompt batch size"):
        call(pipe, negative_prompt=["a", "b", "c"], true_cfg=2.0)
