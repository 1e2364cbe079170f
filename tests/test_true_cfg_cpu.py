"""True CFG (DESIGN.md section 4 "True CFG") without a GPU: the combine's restatement against the reference's own results
(golden/g18_true_cfg.safetensors, written by golden/make_true_cfg_goldens.py) and two wrong variants it must be told apart from; the
new arguments' checks and the on / off decision; the callers; the ABI; the launch plan of a CFG step (golden/true_cfg_launch_trace.txt)
and every refusal of tfx_dit_step_run_ex3.

Regenerate the launch-trace golden on purpose only:   python tests/test_true_cfg_cpu.py --write tests/golden/true_cfg_launch_trace.txt"""
import ctypes as C
import glob
import importlib
import inspect
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import pytest
import torch
from safetensors.torch import load_file

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests.helpers import true_cfg_ref as R
from tests.test_dit_launch_trace import CSRC, CXX, HAVE_HIP_HEADERS, HELPERS, ROCM, compare, parse

GOLD = os.path.join(REPO, "tests", "golden", "g18_true_cfg.safetensors")
TRACE_GOLDEN = os.path.join(REPO, "tests", "golden", "true_cfg_launch_trace.txt")
BF = torch.bfloat16
N = 5


@pytest.fixture(scope="module")
def gold():
    return load_file(GOLD)


# ---------------------------------------------------------------------------------------------- the arithmetic
def test_fixture_holds_the_planted_values(gold):
    neg, pos = gold["neg"].view(-1), gold["pos"].view(-1)
    assert gold["neg"].shape == gold["pos"].shape == (2, 6, 64) and gold["neg"].dtype == BF
    assert tuple(float(s) for s in gold["scales"]) == R.SCALES
    signs = {(bool(torch.signbit(neg[i])), bool(torch.signbit(pos[i]))) for i in range(4)}
    assert all(float(neg[i]) == 0 and float(pos[i]) == 0 for i in range(4)) and len(signs) == 4         # the four sign combinations of zero
    assert torch.isinf(neg[:16]).sum() == 4 and torch.isinf(pos[:16]).sum() == 4
    assert torch.isnan(neg[:16]).sum() == 1 and torch.isnan(pos[:16]).sum() == 1
    sub = 2.0 ** -130
    assert float(neg[12]) == sub and float(pos[13]) == sub and 0 < sub < 2.0 ** -126                     # bf16 subnormals


@pytest.mark.parametrize("k", range(4))
def test_restatement_equals_the_reference_bit_for_bit(gold, k):
    g = R.SCALES[k]
    want = gold[f"g{k}_combined"]
    got = R.combine(gold["neg"], gold["pos"], g)
    assert R.same(got, want), R.differing(got, want)
    assert torch.isnan(want).sum() >= 3                              # NaN operands and inf - inf reached the result
    for i in range(N):                                               # and the Euler step behind it, every step of g16's grid
        lat = R.euler_step(got, gold[f"s{i}_latents_in"], gold["sigmas"], i)
        assert R.same(lat, gold[f"g{k}_s{i}_latents"]), (i, R.differing(lat, gold[f"g{k}_s{i}_latents"]))


def test_the_wrong_variants_differ_at_3p3(gold):
    """what the test scale tells apart: g rounded to bf16 (3.3 -> 3.296875) and the three ops under one rounding"""
    want = gold["g1_combined"]
    assert R.SCALES[1] == 3.3
    for wrong in (R.combine_scale_in_bf16, R.combine_single_rounding):
        got = wrong(gold["neg"], gold["pos"], 3.3)
        assert not R.same(got, want) and R.differing(got, want) >= 8, wrong.__name__
    assert R.same(R.combine_scale_in_bf16(gold["neg"], gold["pos"], 1.5), gold["g0_combined"])          # 1.5 is a bf16: it cannot tell


def test_same_compares_nans_by_position():
    a = torch.tensor([1.0, float("nan"), -0.0], dtype=BF)
    assert R.same(a, a.clone()) and not R.same(a, torch.tensor([1.0, float("nan"), 0.0], dtype=BF))
    assert not R.same(a, torch.tensor([float("nan"), 1.0, -0.0], dtype=BF))


def test_the_doubled_batch_is_negative_then_positive(gold):
    """the reference's torch.cat on index rows; the pipeline hands its session and its modulation table the same order"""
    assert gold["cat_prompt_embeds"].view(-1).tolist() == [0, 1, 100, 101] == gold["cat_pooled"].view(-1).tolist()
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
    seen = {}

    class Stop(Exception):
        pass

    class Ses:
        xin = torch.zeros(4, 16, 384)

        def set_conditioning(self, pe, txt_ids, img_ids):
            seen["pe"] = pe

    class Tr:
        device = "cpu"
        out_channels = 64

        def session(self, B, S, T):
            seen["session"] = (B, S, T)
            return Ses()

    pipe = FluxFillPipeline.__new__(FluxFillPipeline)
    pipe.transformer, pipe.fuse_euler_step, pipe._step_cache = Tr(), True, None
    pipe.scheduler = FlowMatchEulerDiscreteScheduler(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256,
                                                     max_image_seq_len=4096, shift=3.0)
    pipe.scheduler.set_timesteps(sigmas=[1.0, 0.5], device="cpu", mu=0.6)

    def table(timesteps, B, pooled, guidance_scale, dsigma=None):
        seen.update(B=B, pooled=pooled, dsigma=dsigma)
        raise Stop

    pipe._modulation_table = table
    rows = lambda ids, w: torch.tensor(ids, dtype=torch.float32).view(-1, 1, 1).expand(-1, 3, w).to(BF) if w else None
    pe, neg_pe = rows([100, 101], 4), rows([0, 1], 4)
    pooled, neg_pooled = pe[:, 0], neg_pe[:, 0]
    with pytest.raises(Stop):
        pipe._engine_loop(torch.zeros(2, 16, 64), torch.zeros(2, 16, 320), pe, pooled, torch.zeros(3, 3), None, pipe.scheduler.timesteps, 30.0,
                          None, ["latents"], None, None, cfg=dict(scale=3.3, prompt_embeds=neg_pe, pooled=neg_pooled))
    assert seen["session"] == (4, 16, 3) and seen["B"] == 4 and seen["dsigma"] is None                   # 2B samples, Euler unfused
    assert seen["pe"][:, 0, 0].tolist() == gold["cat_prompt_embeds"].view(-1).tolist()
    assert seen["pooled"][:, 0].tolist() == gold["cat_pooled"].view(-1).tolist()
    seen.clear()
    with pytest.raises(Stop):                                        # off: today's session, the fused Euler table
        pipe._engine_loop(torch.zeros(2, 16, 64), torch.zeros(2, 16, 320), pe, pooled, torch.zeros(3, 3), None, pipe.scheduler.timesteps, 30.0,
                          None, ["latents"], None, None)
    assert seen["session"] == (2, 16, 3) and seen["B"] == 2 and seen["dsigma"] is not None and seen["pe"][:, 0, 0].tolist() == [100, 101]


# ---------------------------------------------------------------------------------------------- arguments
def test_check_inputs_raises_the_references_messages():
    from textflux_amd.pipeline import FluxFillPipeline
    pipe = FluxFillPipeline.__new__(FluxFillPipeline)
    pe, other = torch.zeros(1, 4, 8), torch.zeros(1, 5, 8)
    chk = lambda **kw: pipe.check_inputs(kw.pop("prompt", "p"), None, 64, 64, **kw)
    with pytest.raises(ValueError, match="Cannot forward both `negative_prompt`: bad and `negative_prompt_embeds`:"):
        chk(negative_prompt="bad", negative_prompt_embeds=pe, negative_pooled_prompt_embeds=pe)
    with pytest.raises(ValueError, match="Cannot forward both `negative_prompt_2`: bad2 and `negative_prompt_embeds`:"):
        chk(negative_prompt_2="bad2", negative_prompt_embeds=pe, negative_pooled_prompt_embeds=pe)
    with pytest.raises(ValueError, match="`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but got: "
                                         r"`prompt_embeds` torch.Size\(\[1, 4, 8\]\) != `negative_prompt_embeds` torch.Size\(\[1, 5, 8\]\)\."):
        chk(prompt=None, prompt_embeds=pe, pooled_prompt_embeds=pe, negative_prompt_embeds=other, negative_pooled_prompt_embeds=pe)
    with pytest.raises(ValueError, match="If `negative_prompt_embeds` are provided, `negative_pooled_prompt_embeds` also have to be passed. Make sure "
                                         "to generate `negative_pooled_prompt_embeds` from the same text encoder that was used to generate "
                                         "`negative_prompt_embeds`."):
        chk(negative_prompt_embeds=pe)
    chk(negative_prompt="bad", negative_prompt_2="bad2")                                                # the valid forms pass
    chk(negative_prompt_embeds=pe, negative_pooled_prompt_embeds=pe)
    chk(prompt=None, prompt_embeds=pe, pooled_prompt_embeds=pe, negative_prompt="bad")
    params = inspect.signature(FluxFillPipeline.__call__).parameters
    for name in ("negative_prompt", "negative_prompt_2", "negative_prompt_embeds", "negative_pooled_prompt_embeds"):
        assert params[name].default is None
    assert params["true_cfg"].default == 1.0
    assert not any("negative" in p or p == "true_cfg" for p in inspect.signature(FluxFillPipeline.call_mixed).parameters)
    with pytest.raises(ValueError, match="Cannot forward both `negative_prompt`"):                       # __call__ runs the checks first
        pipe.default_sample_size, pipe.vae_scale_factor, pipe._callback_tensor_inputs = 8, 8, ["latents"]
        pipe(prompt="p", negative_prompt="n", negative_prompt_embeds=pe, negative_pooled_prompt_embeds=pe, true_cfg=2.0)


def test_on_and_off_are_decided_as_specified():
    from textflux_amd.pipeline import _true_cfg_on
    pe = torch.zeros(1, 4, 8)
    assert _true_cfg_on(3.3, "bad", None) and _true_cfg_on(1.0001, "bad", None)
    assert _true_cfg_on(3.3, None, pe)                               # embeds alone: on here (the reference switches it off silently)
    assert _true_cfg_on(2.0, [""], None) and _true_cfg_on(2.0, "", None)                                 # an empty negative prompt is a prompt
    assert not _true_cfg_on(1.0, "bad", None) and not _true_cfg_on(0.5, "bad", pe) and not _true_cfg_on(3.3, None, None)


def test_the_step_cache_and_foreign_schedulers_are_refused_when_on():
    from textflux_amd.pipeline import FluxFillPipeline
    pipe = FluxFillPipeline.__new__(FluxFillPipeline)
    pipe.default_sample_size, pipe.vae_scale_factor, pipe._callback_tensor_inputs = 8, 8, ["latents"]
    pipe._step_cache = object()
    with pytest.raises(NotImplementedError, match="true CFG does not run with the step cache"):
        pipe(prompt="p", negative_prompt="n", true_cfg=2.0)
    src = inspect.getsource(FluxFillPipeline._call_body)
    assert "true CFG needs one of the engine's schedulers" in src and "halve the batch" in src
    from textflux_amd import step_loop
    assert list(inspect.signature(step_loop.denoise).parameters)[-3:] == ["cfg", "keep", "change"]
    src = open(os.path.join(REPO, "textflux_amd", "step_loop.py")).read()
    assert 'key += ("cfg",)' in src and "tfx_dit_step_run_ex3" in src and "tfx_dit_step_capture_ex3" in src


# ---------------------------------------------------------------------------------------------- callers
def test_run_items_hands_the_arguments_to_every_call_and_refuses_mixed_batches():
    from tests.test_batch_driver_cpu import StubPipe, _items, _loader
    from tests.test_per_line_cpu import ONE, TWO, PasteStub, _run
    from textflux_amd import batch_driver as bd

    class Seen(StubPipe):
        def __call__(self, *a, true_cfg="absent", negative_prompt="absent", **k):
            self.seen = getattr(self, "seen", []) + [(true_cfg, negative_prompt)]
            return super().__call__(*a, **k)

    items = _items()[:3]
    run = lambda pipe, **kw: bd.run_items(items, pipe, None, batch_size=2, device="cpu", loader=_loader, save=lambda i, im: None, **kw)
    pipe = Seen(0)
    assert sorted(run(pipe, true_cfg=3.3, negative_prompt="blurry")["done"]) == [0, 1, 2] and pipe.seen == [(3.3, "blurry")] * 2
    for kw in ({}, dict(true_cfg=3.3), dict(negative_prompt="blurry"), dict(true_cfg=1.0, negative_prompt="blurry")):    # off: today's calls
        pipe = Seen(0)
        run(pipe, **kw)
        assert pipe.seen == [("absent", "absent")] * 2, kw
    assert sorted(run(StubPipe(0), true_cfg=1.0, negative_prompt=None)["done"]) == [0, 1, 2]             # a pipeline that does not know them

    class SeenPaste(PasteStub):
        def __call__(self, height, width, image, mask_image, **kw):
            self.seen = getattr(self, "seen", []) + [(kw.get("true_cfg", "absent"), kw.get("negative_prompt", "absent"))]
            return super().__call__(height, width, image, mask_image, **kw)

    for its, pb, calls in ((ONE, dict(region=dict(min_side=256)), 1), (TWO, dict(per_line=True), 1), (ONE + TWO, dict(per_line=True), None)):
        pipe = SeenPaste()
        res, _ = _run(pipe, its, paste_back=pb, true_cfg=2.5, negative_prompt="smudged")
        assert res["all_done"] == list(range(len(its))) and len(pipe.pastes) >= len(its)
        assert pipe.seen and all(s == (2.5, "smudged") for s in pipe.seen) and (calls is None or len(pipe.seen) >= calls)
    with pytest.raises(NotImplementedError, match="true CFG.*mixed-geometry"):
        run(Seen(0), mixed_pad=0.1, true_cfg=2.0, negative_prompt="x")
    with pytest.raises(NotImplementedError, match="true CFG.*step_cache"):
        run(Seen(0), step_cache=dict(threshold=0.1), true_cfg=2.0, negative_prompt="x")
    with pytest.raises(ValueError, match="one string"):
        run(Seen(0), true_cfg=2.0, negative_prompt=["a", "b"])


def test_clis_parse_the_flags(monkeypatch):
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    importlib.import_module("run_eval_lora")
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    flags = ["--true_cfg", "3.3", "--negative_prompt", "blurry, smudged"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single), (re_.build_parser(), ["--json_path", "j"]),
                         (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.true_cfg, a.negative_prompt) == (1.0, None)
        a = parser.parse_args(base + flags)
        assert (a.true_cfg, a.negative_prompt) == (3.3, "blurry, smudged")
    parse_known = lambda extra: ri.known_region_from_args(ri.build_parser().parse_args(single + extra))
    assert parse_known([]) is None and parse_known(flags) == dict(true_cfg=3.3, negative_prompt="blurry, smudged")
    assert parse_known(flags + ["--strength", "0.6"]) == dict(true_cfg=3.3, negative_prompt="blurry, smudged", strength=0.6)
    for bad in (["--true_cfg", "3"], ["--negative_prompt", "x"], ["--true_cfg", "1.0", "--negative_prompt", "x"], ["--true_cfg", "0.5", "--negative_prompt", "x"]):
        with pytest.raises(SystemExit):
            parse_known(bad)
    seen = []
    monkeypatch.setattr(ri, "process_normal_mode", lambda *a, **k: seen.append(k.get("known", "absent")))
    monkeypatch.setattr(ri, "report_step_cache", lambda pipe: None)
    monkeypatch.setattr(rl, "load_flux_pipeline", lambda *a, **k: SimpleNamespace())
    for mod in (ri, rl):
        mod.main(single)
        mod.main(single + flags)
    assert seen == ["absent", dict(true_cfg=3.3, negative_prompt="blurry, smudged")] * 2
    src = open(os.path.join(REPO, "scripts", "run_eval.py")).read()
    assert 'known["true_cfg"], known["negative_prompt"] = a.true_cfg, a.negative_prompt' in src and "paste_back=paste_back, **known," in src
    for lora, w in ((False, "--weights_path"), (True, "--lora_weights_path")):
        common = ["--json_path", "j", "--original_images_dir", "o", w, "w", "--scheduler", ""]
        with pytest.raises(SystemExit, match="--true_cfg does not serve mixed-geometry"):
            re_.main(common + ["--mixed_pad", "0.1"] + flags, lora=lora)
        with pytest.raises(SystemExit, match="--true_cfg needs --negative_prompt"):
            re_.main(common + ["--true_cfg", "2"], lora=lora)
        with pytest.raises(SystemExit, match="--negative_prompt needs --true_cfg > 1"):
            re_.main(common + ["--negative_prompt", "x"], lora=lora)
        with pytest.raises(SystemExit, match="--true_cfg does not run with --step_cache"):
            re_.main(common + ["--step_cache", "0.1"] + flags, lora=lora)


# ---------------------------------------------------------------------------------------------- ABI and host checks
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


NEW = ("tfx_cfg_combine", "tfx_dit_step_run_ex3", "tfx_dit_step_capture_ex3")


def test_symbols_are_declared_bound_exported_and_the_abi_stamp_stays(lib, tmp_path):
    from textflux_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    for sym in NEW:
        assert sym + "(" in hdr and sym in L.SIGNATURES and hasattr(lib, sym)
    assert len(L.SIGNATURES["tfx_cfg_combine"][1]) == 7 and len(L.SIGNATURES["tfx_dit_step_run_ex3"][1]) == 5
    assert len(L.SIGNATURES["tfx_dit_step_capture_ex3"][1]) == 6
    assert L.ABI_VERSION == L.header_abi_version() == 11
    assert [f for f, _ in L.StepExtra._fields_] == ["v_prev", "keep_x0", "keep_noise", "keep_mask", "keep_sigma"]   # as they were
    assert [f for f, _ in L.StepChange._fields_] == ["hold", "cut"]
    L._check_abi(lib)
    assert [f for f, _ in L.StepCfg._fields_] == ["scale"]
    (tmp_path / "layout.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "textflux_hip.h"\nint main(void){'
                                       'printf("%zu %zu\\n", sizeof(tfx_step_cfg), offsetof(tfx_step_cfg, scale));return 0;}')
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    size, off = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    assert int(size) == C.sizeof(L.StepCfg) and int(off) == L.StepCfg.scale.offset


def test_cfg_combine_checks_its_arguments_before_it_launches(lib):
    a = [k << 20 for k in range(1, 6)]                               # never dereferenced: every call is refused, or launches nothing
    call = lambda neg=a[0], pos=a[1], out=a[2], Cc=64, rows=4, scale=a[3]: lib.tfx_cfg_combine(neg, pos, out, Cc, rows, scale, None)
    nbytes = 4 * 64 * 2
    for kw, msg in ((dict(Cc=12), b"multiple of 8"), (dict(Cc=0), b"multiple of 8"), (dict(Cc=-8), b"multiple of 8"),
                    (dict(rows=-1), b"negative row count"),
                    (dict(neg=None), b"null pointer"), (dict(pos=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(scale=None), b"null pointer"),
                    (dict(neg=a[0] + 8), b"16-byte aligned"), (dict(pos=a[1] + 2), b"16-byte aligned"), (dict(out=a[2] + 4), b"16-byte aligned"),
                    (dict(scale=a[3] + 2), b"4-byte aligned"),
                    (dict(out=a[1]), b"must not overlap v_pos"), (dict(out=a[1] + 16), b"must not overlap v_pos"),
                    (dict(out=a[1] - nbytes + 16), b"must not overlap v_pos"), (dict(neg=a[1], out=a[1]), b"must not overlap v_pos"),
                    (dict(out=a[0] + 16), b"v_neg itself or not overlap"), (dict(out=a[0] - 16), b"v_neg itself or not overlap"),
                    (dict(out=a[0] + nbytes - 16), b"v_neg itself or not overlap"),
                    (dict(scale=a[2]), b"scale must not lie in out"), (dict(scale=a[2] + nbytes - 4), b"scale must not lie in out"),
                    (dict(out=a[0], scale=a[0] + 4), b"scale must not lie in out")):
        assert call(**kw) != 0 and msg in lib.tfx_last_error(), kw
    assert call(rows=0) == 0 and call(rows=0, neg=None, pos=None, out=None, scale=None) == 0


def test_ops_wrapper_checks_before_it_launches():
    from textflux_amd import ops
    x = torch.zeros(4, 8, dtype=BF)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.cfg_combine(x, x.clone(), torch.ones(1))


def test_ex3_entry_points_refuse_without_a_device(lib):
    from tests.test_keep_known_cpu import step_desc
    from textflux_amd import _lib as L
    hold, out = [], C.c_void_p()
    base = 1 << 31
    ref = lambda o: C.byref(o) if o is not None else None
    cfg = lambda scale=base + (6 << 20): L.StepCfg(scale=scale)
    run = lambda sd, e, c, g: lib.tfx_dit_step_run_ex3(C.byref(sd), ref(e), ref(c), ref(g), None)
    cap = lambda sd, e, c, g: lib.tfx_dit_step_capture_ex3(C.byref(sd), ref(e), ref(c), ref(g), None, C.byref(out))
    for fn in (run, cap):
        assert fn(step_desc(L, hold), None, None, cfg()) != 0 and b"null tfx_step_extra" in lib.tfx_last_error()
        assert fn(step_desc(L, hold, 2), L.StepExtra(), None, cfg()) != 0 and b"sampler 2" in lib.tfx_last_error()
        sd = step_desc(L, hold)
        sd.dit.seq_len = 1 << 22
        assert fn(sd, L.StepExtra(), None, cfg()) != 0 and b"dit.seq_len" in lib.tfx_last_error()
        for B in (1, 3):
            sd = step_desc(L, hold)
            sd.dit.B = B
            assert fn(sd, L.StepExtra(), None, cfg()) != 0 and b"even dit.B" in lib.tfx_last_error()
        assert fn(step_desc(L, hold), L.StepExtra(), None, cfg(None)) != 0 and b"cfg->scale is null" in lib.tfx_last_error()
        sd = step_desc(L, hold)                                       # B = 2, S = 48: latents have 1 * 48 rows, out and xin 2 * 48
        for target in (sd.latents, sd.latents + 48 * 64 * 2 - 4, sd.dit.out + 2 * 48 * 64 * 2 - 4, sd.dit.xin + 2 * 48 * 384 * 2 - 4, sd.mod_cur,
                       sd.mod_cur + 4096 * 2 - 4, sd.step_ptr):
            assert fn(sd, L.StepExtra(), None, cfg(target)) != 0 and b"buffer the step writes" in lib.tfx_last_error(), target
        assert fn(sd, L.StepExtra(v_prev=base), None, cfg(base + 48 * 64 * 2 - 4)) != 0 and b"buffer the step writes" in lib.tfx_last_error()
        sd.phase = 1
        assert fn(sd, L.StepExtra(), None, cfg()) != 0 and b"needs a step cache" in lib.tfx_last_error()      # a phase without cache: as ever
    sd = step_desc(L, hold)
    assert lib.tfx_dit_step_capture_ex3(C.byref(sd), C.byref(L.StepExtra()), None, C.byref(cfg()), None, None) != 0
    assert b"null output handle" in lib.tfx_last_error()
    assert cap(sd, L.StepExtra(), None, cfg()) != 0 and b"NULL stream" in lib.tfx_last_error()            # a valid set gets as far as the capture
    assert cap(sd, L.StepExtra(), None, cfg(sd.latents + 48 * 64 * 2)) != 0 and b"NULL stream" in lib.tfx_last_error()   # behind the B * S rows
    assert cap(sd, L.StepExtra(), None, None) != 0 and b"NULL stream" in lib.tfx_last_error()             # no cfg: the _ex2 step


# ---------------------------------------------------------------------------------------------- the step's launch plan
def trace(csrc=CSRC, workdir=None):
    """what helpers/true_cfg_trace_driver.cpp prints: csrc's host code against the recording launch layer"""
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        exe = os.path.join(tmp, "true_cfg_trace")
        srcs = sorted(p for p in glob.glob(os.path.join(csrc, "*.cpp")) if os.path.basename(p) != "launch.cpp")
        srcs += [os.path.join(HELPERS, f) for f in ("launch_recorder.cpp", "step_cache_recorder.cpp", "change_map_recorder.cpp",
                                                    "true_cfg_recorder.cpp", "true_cfg_trace_driver.cpp")]
        cmd = [CXX, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", csrc, "-I",
               os.path.join(REPO, "include"), *srcs, "-Wl,--unresolved-symbols=ignore-all", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"trace binary ended with {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
        return r.stdout


def golden_part(text):
    """the scenarios the golden holds: all but the `null_*` ones, which are compared with each other"""
    out, keep = [], True
    for line in text.splitlines():
        if line.startswith("== "):
            keep = not line.startswith("== null_")
        if keep:
            out.append(line)
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    return trace(workdir=str(tmp_path_factory.mktemp("true_cfg_trace")))


def launches(lines):
    assert lines[-2:] == ["rc 0", "error "], lines[-2:]
    return lines[:-2]


def fields(line):
    return dict(f.split("=") for f in line.split()[1:])


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_launch_trace_matches_the_golden(traced):
    bad = compare(golden_part(traced), open(TRACE_GOLDEN).read())
    assert not bad, "\n".join(bad[:20])
    assert sum(1 for n in parse(traced) if n.startswith("cfg_")) == 10


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
@pytest.mark.parametrize("sampler", [0, 1, 3], ids=["euler", "amo", "multistep"])
def test_a_cfg_step_combines_between_proj_out_and_the_update_on_half_the_rows(traced, sampler):
    sc = parse(traced)
    B2, S, C_OUT, C_IN = 4, 256, 16, 64
    half = B2 // 2 * S
    for mode in ("plain", "keep", "change"):
        cfg = launches(sc[f"cfg_sampler{sampler}_{mode}"][0])
        null = launches(sc[f"null_ex3_sampler{sampler}_{mode}"][0])
        at = [i for i, l in enumerate(cfg) if l.startswith("cfg_combine ")]
        assert len(at) == 1
        i = at[0]
        assert cfg[:i] == null[:i]                                   # the forward on 2B is the forward: nothing in it knows about CFG
        assert cfg[i - 1].startswith("gemm_bf16 ") and "W=proj_out.w" in cfg[i - 1] and f"batch={B2}" in cfg[i - 1]
        f = fields(cfg[i])
        assert f == dict(v_neg="out", v_pos=f"out+{half * C_OUT * 2:#x}", out="out", C=str(C_OUT), rows=str(half), scale="cfg_scale")
        names = [l.split()[0] for l in cfg[i + 1:]]
        update = "multistep_step" if sampler == 3 else "sched_step"
        blend = {"plain": [], "keep": ["known_region_blend"], "change": ["change_map_blend"]}[mode]
        assert names == [update] + blend + ["copy_rows", "advance_step"]
        assert [l.split()[0] for l in null[i:]] == [update] + blend + ["advance_step"]
        up = cfg[i + 1]
        if sampler == 3:
            assert fields(up)["rows"] == str(half) and fields(up)["x"] == "latents" and fields(up)["xin"] == "xin"
            assert fields(null[i])["rows"] == str(2 * half)
        else:                                                        # sched_step amo v x xin ldxin C rows coef step_ptr step noise
            assert up.split()[1:8] == [str(sampler), "out", "latents", "xin", str(C_IN), str(C_OUT), str(half)]
            assert null[i].split()[1:8] == [str(sampler), "out", "latents", "xin", str(C_IN), str(C_OUT), str(2 * half)]
        if blend:
            b = fields(cfg[i + 2])
            assert (b["rows"], b["x"], b["xin"], b["ldxin"]) == (str(half), "latents", "xin", str(C_IN))
        # both halves of xin: the update and the blend mirror into the first, the copy fills the second
        assert cfg[-2] == f"copy_rows xin {C_IN} {S * C_IN} xin+{half * C_IN * 2:#x} {C_IN} {S * C_IN} {S} {C_OUT} {B2 // 2}"


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_a_null_cfg_is_the_ex2_step(traced):
    sc = parse(traced)
    n = 0
    for sampler in range(4):
        for mode in ("plain", "keep", "change"):
            a, b = sc[f"null_ex3_sampler{sampler}_{mode}"], sc[f"null_ex2_sampler{sampler}_{mode}"]
            assert a == b and len(launches(a[0])) >= 20 and not any("cfg_combine" in l for l in a[0])
            n += 1
    assert n == 12


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_ex3_refusals_launch_nothing(traced):
    sc = parse(traced)
    want = dict(fail_sampler_2="sampler 2", fail_seq_len="dit.seq_len", fail_phase_1="phase 1", fail_phase_2="phase 2", fail_phase_3="phase 3",
                fail_odd_B="even dit.B", fail_B_1="even dit.B", fail_null_scale="cfg->scale is null", fail_scale_misaligned="4-byte aligned",
                fail_scale_in_latents="buffer the step writes", fail_scale_in_out_second_half="buffer the step writes",
                fail_scale_in_xin="buffer the step writes", fail_scale_in_mod_cur="buffer the step writes",
                fail_scale_in_step_ptr="buffer the step writes", fail_scale_in_v_prev="buffer the step writes",
                fail_scale_in_hid="buffer the step writes", fail_keep_x0_in_latents="must not alias")
    for name, text in want.items():
        lines = sc[name][0]
        assert lines[0] == "rc 1" and text in lines[1] and len(lines) == 2, name                        # refused before anything is launched
    assert len([k for k in sc if k.startswith("fail_")]) == len(want)
    assert launches(sc["cfg_latents_half_then_keep_x0"][0])          # the loop state is B * S rows: what lies behind them is free


def test_the_step_loop_keys_its_graphs_with_cfg():
    from tests.test_keep_known_cpu import Bar, Recorder
    from textflux_amd.step_loop import run_steps
    seen = {}
    for key in ((False, False), (False, False, "cfg"), (False, False, "keep", "cfg")):
        rec, graphs = Recorder(), {}
        pipe = SimpleNamespace(_interrupt=False, scheduler=SimpleNamespace(_step_index=0))
        run_steps(rec, 4, pipe, Bar(), graphs, key, None, use_graph=True)
        seen[key] = (rec.ops, list(graphs))
    assert seen[(False, False)][0] == seen[(False, False, "cfg")][0] == seen[(False, False, "keep", "cfg")][0]
    assert seen[(False, False, "cfg")][1] == [(False, False, "cfg")] and seen[(False, False)][1] == [(False, False)]


def main():
    import argparse
    ap = argparse.ArgumentParser(description="launch trace of a true-CFG step of a csrc directory, compared with the golden")
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("--write", metavar="FILE", help="write the golden part of the trace to FILE instead of comparing it")
    a = ap.parse_args()
    got = golden_part(trace(os.path.abspath(a.csrc)))
    if a.write:
        with open(a.write, "w") as f:
            f.write(got)
        print(f"{a.write}: {len(got)} bytes, {len(parse(got))} scenarios")
        return 0
    bad = compare(got, open(TRACE_GOLDEN).read())
    print("\n".join(bad) if bad else f"launch trace equals {os.path.relpath(TRACE_GOLDEN, REPO)} ({len(parse(got))} scenarios)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
