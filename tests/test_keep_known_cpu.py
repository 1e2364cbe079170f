"""Known-region sampling without a GPU (DESIGN.md section 4 "Known-region sampling"): the torch-CPU restatement of
helpers/keep_known_ref.py and the engine schedulers' scale_noise / keep_sigma_table / coef_table against what the reference computes
(tests/golden/g16_keep_known.safetensors, written by tests/golden/make_keep_known_goldens.py), bit for bit; the step loop's control
flow, the new entry points' declarations and host checks, and the callers' arguments."""
import ctypes as C
import importlib
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from tests.helpers import keep_known_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SCHED = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
N = 5
STRENGTH_TEXT = "The value of strength should in [0.0, 1.0] but is {}"


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(REPO, "tests", "golden", "g16_keep_known.safetensors"))


def bits(t):
    return t.contiguous().view(torch.int16)


def scheduler_classes():
    from textflux_amd.schedulers import (FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler,
                                         StochasticRFOvershotDiscreteScheduler)
    return FlowMatchEulerDiscreteScheduler, StochasticRFOvershotDiscreteScheduler, FlowMatchMultistepScheduler


def make_scheduler(cls, gold, n=N):
    s = cls.from_config(SCHED)
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cpu", mu=float(gold["mu"]))
    return s


# ---------------------------------------------------------------------------------------------- the restatement == the reference
@pytest.mark.parametrize("begin", [0, 2])
def test_helper_equals_the_reference(gold, begin):
    x0, noise, sig = gold["x0"], gold["noise"], gold["sigmas"]
    assert x0.shape == (2, 6, 64) and sig.shape == (N + 1,) and sig.dtype == torch.float32
    tab = R.keep_sigma(sig, begin)
    assert tab.shape == (N - begin,) and tab[-1] == -1 and torch.equal(tab[:-1], sig[begin + 1:-1].to(BF).float())
    assert torch.equal(bits(R.scale_noise(x0, sig[begin], noise)), bits(gold[f"b{begin}_start"]))
    for i in range(N - begin):
        proper = R.scale_noise(x0, tab[i], noise)
        assert torch.equal(bits(proper), bits(gold[f"b{begin}_s{i}_proper"])), i
        for name in ("binary", "soft"):
            got = R.blend(gold[f"b{begin}_s{i}_latents"], x0, noise, gold[f"mask_{name}"], tab[i])
            assert torch.equal(bits(got), bits(gold[f"b{begin}_s{i}_blend_{name}"])), (i, name)
    # the last step hands x0 over untouched, signed zeros included -- which sigma = 0 would not: 0 * (-0) + 1 * (+0) = +0
    last = gold[f"b{begin}_s{N - begin - 1}_proper"]
    assert torch.equal(bits(last), bits(x0)) and (bits(x0).view(-1)[:4] == torch.tensor([0, -32768, 0, -32768], dtype=torch.int16)).all()
    assert not torch.equal(bits(R.scale_noise(x0, 0.0, noise)), bits(x0))
    assert set(gold["mask_soft"].float().unique().tolist()) == {0.0, 0.25, 0.5, 1.0}


def test_helper_get_timesteps_and_mask_pack_equal_the_reference(gold):
    rows = gold["get_timesteps"].tolist()
    assert len(rows) == 18
    for n, s100, t_start, steps in rows:
        assert R.get_timesteps(n, s100 / 100) == (t_start, steps), (n, s100)
    assert [r[3] for r in rows if r[0] == 30] == [0, 1, 9, 15, 18, 30]              # int(30 - 0.3) = 29: one step
    pix = gold["mask_pixels_u8"]
    assert pix.shape == (32, 48) and pix.dtype == torch.uint8
    got = R.mask_pack(pix[None], 0, 0)
    assert got.shape == (1, 6, 64) and torch.equal(bits(got), bits(gold["mask_packed"]))
    assert 0 < got.float().sum() < got.numel()


# ---------------------------------------------------------------------------------------------- the schedulers
@pytest.mark.parametrize("which", [0, 1, 2], ids=["euler", "amo", "multistep"])
def test_scheduler_scale_noise_and_keep_sigma_table_equal_the_reference(gold, which):
    cls = scheduler_classes()[which]
    x0, noise = gold["x0"], gold["noise"]
    sch = make_scheduler(cls, gold)
    if which != 1:           # the AMO class shifts without the f32 cast (its own grid, last ulp): the Euler grid is the fixture's
        assert torch.equal(sch.sigmas, gold["sigmas"]) and torch.equal(sch.timesteps, gold["timesteps"])
    sig = sch._sigmas_host
    # begin_index None: the timestep's own index
    for i in (0, 3):
        assert torch.equal(bits(sch.scale_noise(x0, sch.timesteps[i:i + 1], noise)), bits(R.scale_noise(x0, sig[i], noise)))
    for begin in (0, 2):
        sch = make_scheduler(cls, gold)
        sch.set_begin_index(begin)
        start = sch.scale_noise(x0, sch.timesteps[begin:begin + 1].repeat(2), noise)            # step_index None: sigmas[begin_index]
        assert torch.equal(bits(start), bits(R.scale_noise(x0, sig[begin], noise)))
        tab = sch.keep_sigma_table("cpu")
        assert tab.dtype == torch.float32 and torch.equal(tab, R.keep_sigma(sig, begin))
        for i in range(N - begin - 1):
            sch._step_index = begin + i + 1                                                      # as after step i of the loop
            got = sch.scale_noise(x0, torch.tensor([float(sch.timesteps[begin + i + 1])]), noise)
            assert torch.equal(bits(got), bits(R.scale_noise(x0, tab[i], noise))), i
            if which != 1:
                assert torch.equal(bits(got), bits(gold[f"b{begin}_s{i}_proper"])), i
        if which != 1:
            assert torch.equal(bits(start), bits(gold[f"b{begin}_start"]))


@pytest.mark.parametrize("which", [0, 1, 2], ids=["euler", "amo", "multistep"])
def test_pipeline_get_timesteps_equals_the_reference(gold, which):
    from textflux_amd.pipeline import FluxFillPipeline
    pipe = FluxFillPipeline.__new__(FluxFillPipeline)
    for n, s100, t_start, steps in gold["get_timesteps"].tolist():
        pipe.scheduler = make_scheduler(scheduler_classes()[which], gold, n)
        ts, got = pipe.get_timesteps(n, s100 / 100, "cpu")
        assert (pipe.scheduler.begin_index, got) == (t_start, steps) and len(ts) == steps
        assert torch.equal(ts, pipe.scheduler.timesteps[t_start:])


def test_coef_tables_start_at_begin_index(gold):
    euler_cls, amo_cls, ms_cls = scheduler_classes()
    sliced = np.linspace(1.0, 1 / N, N)[2:]
    # multistep: the first executed step is the history-free one -- the table of a scheduler set to the sliced grid
    ms, ref = make_scheduler(ms_cls, gold), ms_cls.from_config(SCHED)
    ref.set_timesteps(sigmas=sliced, device="cpu", mu=float(gold["mu"]))
    full = ms.coef_table("cpu").clone()
    ms.set_begin_index(2)
    got = ms.coef_table("cpu")
    assert got.shape == (N - 2, 2) and torch.equal(got.view(torch.int32), ref.coef_table("cpu").view(torch.int32))
    assert got[0, 1] == 0 and not torch.equal(got[0], full[2]) and torch.equal(got[1:], full[3:])
    eu = make_scheduler(euler_cls, gold)
    full = eu.coef_table("cpu").clone()
    eu.set_begin_index(2)
    assert torch.equal(eu.coef_table("cpu"), full[2:])
    amo = make_scheduler(amo_cls, gold)
    amo.set_c(2.0), amo.set_overshot_func(lambda t, dt: t + dt)
    full = amo.coef_table("cpu").clone()
    amo.set_begin_index(2)
    assert torch.equal(amo.coef_table("cpu"), full[2:])
    for s in (ms, eu, amo):                                            # set_timesteps clears the begin index and the tables with it
        s.set_timesteps(sigmas=np.linspace(1.0, 1 / N, N), device="cpu", mu=float(gold["mu"]))
        assert s.begin_index is None and s.coef_table("cpu").shape[0] == N and s.keep_sigma_table("cpu").shape == (N,)


# ---------------------------------------------------------------------------------------------- the step loop's control flow
class Recorder:
    """run_steps' device operations as a list of what was asked for"""

    def __init__(self, refuse=False):
        self.ops, self.refuse, self.n = [], refuse, 0

    def feed_noise(self, i):
        self.ops.append(("noise", i))

    def run(self, ph):
        self.ops.append(("run", ph))

    def replay(self, h):
        self.ops.append(("replay", h[1]))

    def capture(self, ph):
        from textflux_amd.step_loop import CaptureRefused
        self.ops.append(("capture", ph))
        if self.refuse:
            raise CaptureRefused("no")
        self.n += 1
        return ("graph", ph, self.n)

    def destroy(self, h):
        self.ops.append(("destroy", h[1]))

    def metric(self):
        self.ops.append(("metric",))
        return [1.0]

    def save(self):
        self.ops.append(("save",))
        return None

    def restore(self, s):
        self.ops.append(("restore",))


class Bar:
    def update(self):
        pass


@pytest.mark.parametrize("cache", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_run_steps_issues_the_same_sequence_with_and_without_keep(graph, cache):
    """the blend rides inside the step (tfx_dit_step_run_ex): the loop's control flow does not know it, only the graph key does"""
    from textflux_amd.step_cache import Decider, StepCacheConfig
    from textflux_amd.step_loop import run_steps
    seen = {}
    for key in ((False, True), (False, True, "keep")):
        rec, graphs = Recorder(), {}
        pipe = SimpleNamespace(_interrupt=False, scheduler=SimpleNamespace(_step_index=2))
        decider = Decider(StepCacheConfig.make(0.0, {2}, None)) if cache else None
        run_steps(rec, 4, pipe, Bar(), graphs, key, decider, use_graph=graph)
        assert pipe.scheduler._step_index == 6                         # counts on from the begin index
        seen[key] = (rec.ops, sorted(graphs, key=str))
    plain, keep = seen[(False, True)], seen[(False, True, "keep")]
    assert plain[0] == keep[0] and len(plain[0]) >= 8
    assert all("keep" in k for k in keep[1]) and not any("keep" in k for k in plain[1])
    assert len(keep[1]) == (0 if not graph else 3 if cache else 1)


# ---------------------------------------------------------------------------------------------- ABI and host checks
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


NEW = ("tfx_known_region_blend", "tfx_keep_mask_pack", "tfx_dit_step_run_ex", "tfx_dit_step_capture_ex")


def test_symbols_are_declared_bound_exported_and_the_abi_stamp_stays(lib, tmp_path):
    from textflux_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    for sym in NEW:
        assert sym + "(" in hdr and sym in L.SIGNATURES and hasattr(lib, sym)
    assert len(L.SIGNATURES["tfx_known_region_blend"][1]) == 13 and len(L.SIGNATURES["tfx_keep_mask_pack"][1]) == 9
    assert L.ABI_VERSION == L.header_abi_version() == 11
    assert [f for f, _ in L.StepDesc._fields_][-2:] == ["cache", "phase"]
    L._check_abi(lib)
    # tfx_step_extra as gcc lays it out == the ctypes mirror (the method of test_capi_symbols.py)
    fields = [f for f, _ in L.StepExtra._fields_]
    assert fields == ["v_prev", "keep_x0", "keep_noise", "keep_mask", "keep_sigma"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "textflux_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(tfx_step_extra));']
    lines += [f'printf("{f} %zu\\n", offsetof(tfx_step_extra, {f}));' for f in fields] + ["return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.StepExtra)
    for f in fields:
        assert int(got[f]) == getattr(L.StepExtra, f).offset, f


def test_known_region_blend_checks_its_arguments_before_it_launches(lib):
    a = [k << 20 for k in range(1, 8)]                                # never dereferenced: every call is refused, or launches nothing
    call = lambda x=a[0], ldx=64, x0=a[1], noise=a[2], mask=a[3], Cc=64, rows=4, sig=a[4], xin=None, ldxin=0: lib.tfx_known_region_blend(
        x, ldx, x0, noise, mask, Cc, rows, sig, None, 0, xin, ldxin, None)
    for kw, msg in ((dict(Cc=12), b"multiple of 8"), (dict(Cc=0), b"multiple of 8"), (dict(Cc=-8), b"multiple of 8"),
                    (dict(rows=-1), b"negative row count"),
                    (dict(ldx=56), b"ldx"), (dict(ldx=68), b"ldx"), (dict(xin=a[5], ldxin=56), b"ldxin"), (dict(xin=a[5], ldxin=68), b"ldxin"),
                    (dict(x=None), b"null pointer"), (dict(x0=None), b"null pointer"), (dict(noise=None), b"null pointer"),
                    (dict(mask=None), b"null pointer"), (dict(sig=None), b"null pointer"),
                    (dict(x=a[0] + 8), b"16-byte aligned"), (dict(x0=a[1] + 2), b"16-byte aligned"), (dict(noise=a[2] + 4), b"16-byte aligned"),
                    (dict(mask=a[3] + 8), b"16-byte aligned"), (dict(xin=a[5] + 8, ldxin=64), b"16-byte aligned"),
                    (dict(x0=a[0]), b"alias"), (dict(noise=a[0]), b"alias"), (dict(mask=a[0]), b"alias"),
                    (dict(x0=a[0] + 64), b"alias"), (dict(mask=a[0] - 16), b"alias"),                       # partial overlaps
                    (dict(ldx=384, noise=a[0] + 3 * 384 * 2), b"alias")):                                   # inside a pitched x's last row
        assert call(**kw) != 0 and msg in lib.tfx_last_error(), kw
    assert call(rows=0) == 0 and call(rows=0, x=None, x0=None, noise=None, mask=None, sig=None) == 0


def test_keep_mask_pack_checks_its_arguments_before_it_launches(lib):
    call = lambda m=1 << 20, o=2 << 20, B=1, H=32, W=48, Cc=64, mode=0, grow=0: lib.tfx_keep_mask_pack(m, o, B, H, W, Cc, mode, grow, None)
    for kw, msg in ((dict(H=24), b"multiples of 16"), (dict(W=40), b"multiples of 16"), (dict(Cc=12), b"multiple of 8"),
                    (dict(mode=2), b"mode must be"), (dict(mode=-1), b"mode must be"), (dict(mode=0, grow=1), b"grow must be 0"),
                    (dict(mode=1, grow=9), b"outside 0..8"), (dict(mode=1, grow=-1), b"outside 0..8"),
                    (dict(m=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(m=(1 << 20) + 4), b"aligned"),
                    (dict(o=(2 << 20) + 8), b"aligned")):
        assert call(**kw) != 0 and msg in lib.tfx_last_error(), kw
    assert call(B=0) == 0 and call(H=0, m=None, o=None) == 0


def step_desc(L, keep, sampler=0):
    """a descriptor over fake addresses that passes the step's host checks (nothing is launched by the calls below)"""
    sd = L.StepDesc()
    a = iter(range(1 << 24, 1 << 30, 1 << 24))
    sd.mod_table, sd.mod_cur, sd.step_ptr, sd.latents, sd.coef = (next(a) for _ in range(5))
    sd.dit.mod, sd.dit.out, sd.dit.xin = sd.mod_cur, next(a), next(a)
    sd.dit.B, sd.dit.S, sd.dit.in_channels, sd.dit.out_channels = 2, 48, 384, 64
    sd.mod_step_elems, sd.sampler = 4096, sampler
    if sampler == 2:
        sd.dit.euler_gate, sd.latents, sd.coef = sd.mod_cur, None, None
    keep.append(sd)
    return sd


def test_ex_entry_points_refuse_null_and_partial_keep_sets_without_a_device(lib):
    from textflux_amd import _lib as L
    hold, out = [], C.c_void_p()
    base = 1 << 31
    full = dict(keep_x0=base, keep_noise=base + (1 << 20), keep_mask=base + (2 << 20), keep_sigma=base + (3 << 20))
    run = lambda sd, ex: lib.tfx_dit_step_run_ex(C.byref(sd), C.byref(ex) if ex is not None else None, None)
    cap = lambda sd, ex: lib.tfx_dit_step_capture_ex(C.byref(sd), C.byref(ex) if ex is not None else None, None, C.byref(out))
    for fn in (run, cap):
        assert fn(step_desc(L, hold), None) != 0 and b"null tfx_step_extra" in lib.tfx_last_error()
        for missing in full:                                           # every partial set, one and three members
            ex = L.StepExtra(**{k: v for k, v in full.items() if k != missing})
            assert fn(step_desc(L, hold), ex) != 0 and b"all set or all NULL" in lib.tfx_last_error(), missing
            ex = L.StepExtra(**{missing: full[missing]})
            assert fn(step_desc(L, hold), ex) != 0 and b"all set or all NULL" in lib.tfx_last_error(), missing
        for sampler in (0, 2):
            sd = step_desc(L, hold, sampler)
            sd.dit.seq_len = 1 << 22                                   # mixed-geometry batches
            want = b"dit.seq_len"
            assert fn(sd, L.StepExtra(**full)) != 0 and want in lib.tfx_last_error()
        sd = step_desc(L, hold)
        for field in full:
            for target in (sd.latents, sd.dit.out, sd.dit.xin, sd.latents + 64, sd.dit.xin + 2 * 48 * 384 * 2 - 16):
                ex = L.StepExtra(**dict(full, **{field: target}))
                assert fn(sd, ex) != 0 and b"must not alias" in lib.tfx_last_error(), (field, target)
        ex = L.StepExtra(v_prev=full["keep_x0"], **full)
        assert fn(sd, ex) != 0 and b"must not alias" in lib.tfx_last_error()
        # v_prev carries the multistep entry points' checks over
        sd = step_desc(L, hold, 2)
        assert fn(sd, L.StepExtra(v_prev=base)) != 0 and b"sampler must be 0" in lib.tfx_last_error()
        sd = step_desc(L, hold)
        assert fn(sd, L.StepExtra(v_prev=sd.latents)) != 0 and b"alias" in lib.tfx_last_error()
        sd = step_desc(L, hold)
        sd.latents = None
        assert fn(sd, L.StepExtra(**full)) != 0 and b"null pointer" in lib.tfx_last_error()
        assert lib.tfx_dit_step_run_ex(None, C.byref(L.StepExtra()), None) != 0 and b"null descriptor" in lib.tfx_last_error()
    sd = step_desc(L, hold)
    assert lib.tfx_dit_step_capture_ex(C.byref(sd), C.byref(L.StepExtra(**full)), None, None) != 0 and b"null output handle" in lib.tfx_last_error()
    assert cap(sd, L.StepExtra(**full)) != 0 and b"NULL stream" in lib.tfx_last_error()     # a valid set gets as far as the capture
    assert cap(sd, L.StepExtra()) != 0 and b"NULL stream" in lib.tfx_last_error()           # all NULL is the plain step


def test_ops_wrappers_check_before_they_launch():
    from textflux_amd import ops
    x = torch.zeros(4, 8, dtype=BF)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.known_region_blend(x, x.clone(), x.clone(), x.clone(), torch.zeros(3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.keep_mask_pack(torch.zeros(1, 16, 16, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------- callers
def test_strength_value_errors_are_the_references():
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd import batch_driver as bd
    pipe = FluxFillPipeline.__new__(FluxFillPipeline)                 # refused on the first line, before any component is used
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError) as e:
            pipe(prompt="x", strength=bad)
        assert str(e.value) == STRENGTH_TEXT.format(bad)
        with pytest.raises(ValueError) as e:
            bd.run_items([], object(), None, strength=bad, device="cpu")
        assert str(e.value) == STRENGTH_TEXT.format(bad)
    want = ("After adjusting the num_inference_steps by strength parameter: 0.01, the number of pipelinesteps is 0 which is < 1 and not "
            "appropriate for this pipeline.")
    src = open(os.path.join(REPO, "textflux_amd", "pipeline.py")).read()
    assert 'f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline"' in src
    assert 'f"steps is {num_inference_steps} which is < 1 and not appropriate for this pipeline."' in src
    strength, num_inference_steps = 0.01, 0
    assert (f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline"
            f"steps is {num_inference_steps} which is < 1 and not appropriate for this pipeline.") == want


def test_keep_known_argument_forms():
    from textflux_amd.pipeline import _keep_known_cfg
    assert _keep_known_cfg(None) is None and _keep_known_cfg(False) is None
    assert _keep_known_cfg(True) == ("nearest", 0) and _keep_known_cfg({}) == ("nearest", 0)
    assert _keep_known_cfg(dict(mode="cover", grow=3)) == ("cover", 3) and _keep_known_cfg(dict(mode="cover")) == ("cover", 0)
    for bad in (dict(mode="nearest", grow=1), dict(mode="cover", grow=9), dict(mode="cover", grow=-1), dict(mode="bilinear"), dict(radius=2)):
        with pytest.raises(ValueError, match="keep_known"):
            _keep_known_cfg(bad)


def test_mixed_geometry_batches_refuse_the_arguments():
    from tests.test_batch_driver_cpu import StubPipe, _items, _loader
    from textflux_amd.batch_driver import run_items
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
    for kw in (dict(keep_known=True), dict(strength=0.6), dict(keep_known=dict(mode="cover", grow=1), strength=0.5)):
        with pytest.raises(NotImplementedError, match="known-region sampling"):
            run_items(_items()[:2], StubPipe(0), None, mixed_pad=0.1, device="cpu", loader=_loader, **kw)
        real = FluxFillPipeline.__new__(FluxFillPipeline)             # call_mixed refuses on its first lines
        real.scheduler, real.transformer, real._step_cache, real.fuse_euler_step = FlowMatchEulerDiscreteScheduler(**SCHED), None, None, True
        with pytest.raises(NotImplementedError, match="call_mixed: strength / keep_known"):
            real.call_mixed(sizes=[(256, 256)], latents=[torch.zeros(1, 256, 64)], masked_image_latents=[torch.zeros(1, 256, 320)],
                            prompt_embeds=torch.zeros(1, 64, 64), pooled_prompt_embeds=torch.zeros(1, 128), output_type="latent", **kw)


def test_run_items_hands_the_arguments_to_every_call_and_only_when_given():
    from tests.test_batch_driver_cpu import StubPipe, _items, _loader
    from textflux_amd import batch_driver as bd

    class Known(StubPipe):
        def __call__(self, *a, keep_known="absent", strength="absent", **k):
            self.seen = getattr(self, "seen", []) + [(keep_known, strength)]
            return super().__call__(*a, **k)

    items = _items()[:3]
    run = lambda pipe, **kw: bd.run_items(items, pipe, None, batch_size=2, device="cpu", loader=_loader, save=lambda i, im: None, **kw)
    pipe = Known(0)
    res = run(pipe, keep_known=dict(mode="cover", grow=2), strength=0.6)
    assert sorted(res["done"]) == [0, 1, 2] and len(pipe.seen) == 2
    assert all(s == (dict(mode="cover", grow=2), 0.6) for s in pipe.seen)
    pipe = Known(0)
    run(pipe, keep_known=True)
    assert all(s == (True, "absent") for s in pipe.seen)
    pipe = Known(0)
    run(pipe)                                                          # the defaults: the call carries neither key
    assert all(s == ("absent", "absent") for s in pipe.seen)
    assert sorted(run(StubPipe(0))["done"]) == [0, 1, 2]               # a pipeline that knows neither argument still runs
    assert sorted(run(StubPipe(0), strength=1.0, keep_known=None)["done"]) == [0, 1, 2]


def test_clis_carry_the_flags(monkeypatch):
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    flags = ["--strength", "0.6", "--keep_known", "--keep_known_mode", "cover", "--keep_known_grow", "2"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single), (re_.build_parser(), ["--json_path", "j"]),
                         (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.strength, a.keep_known, a.keep_known_mode, a.keep_known_grow) == (1.0, False, "nearest", 0)
        a = parser.parse_args(base + flags)
        assert (a.strength, a.keep_known, a.keep_known_mode, a.keep_known_grow) == (0.6, True, "cover", 2)
    assert ri.known_region_from_args(ri.build_parser().parse_args(single)) is None
    assert ri.known_region_from_args(ri.build_parser().parse_args(single + flags)) == dict(keep_known=dict(mode="cover", grow=2), strength=0.6)
    assert ri.known_region_from_args(ri.build_parser().parse_args(single + ["--keep_known"])) == dict(keep_known=dict(mode="nearest", grow=0))
    for bad in (["--keep_known_grow", "1"], ["--keep_known_mode", "cover"], ["--strength", "1.5"], ["--keep_known", "--keep_known_grow", "1"],
                ["--keep_known", "--keep_known_mode", "cover", "--keep_known_grow", "9"]):
        with pytest.raises(SystemExit):
            ri.known_region_from_args(ri.build_parser().parse_args(single + bad))
    # main -> process_normal_mode: the keyword appears only when a flag was given
    seen = []
    monkeypatch.setattr(ri, "process_normal_mode", lambda *a, **k: seen.append(k.get("known", "absent")))
    monkeypatch.setattr(ri, "report_step_cache", lambda pipe: None)
    monkeypatch.setattr(rl, "load_flux_pipeline", lambda *a, **k: SimpleNamespace())
    for mod in (ri, rl):
        mod.main(single)
        mod.main(single + flags)
    both = dict(keep_known=dict(mode="cover", grow=2), strength=0.6)
    assert seen == ["absent", both, "absent", both]
    # run_inference -> the pipeline call
    calls = []

    class Pipe:
        def __call__(self, **kw):
            calls.append(kw)
            from PIL import Image
            return SimpleNamespace(images=[Image.new("RGB", (kw["width"], kw["height"]))])

    real_generator = torch.Generator
    monkeypatch.setattr(ri.torch, "Generator", lambda device=None: real_generator())
    from PIL import Image
    img = Image.new("RGB", (64, 64))
    ri.run_inference(img, img, ["AB"], num_steps=2, pipe=Pipe())
    ri.run_inference(img, img, ["AB"], num_steps=2, pipe=Pipe(), known=both)
    assert "strength" not in calls[0] and "keep_known" not in calls[0]
    assert calls[1]["strength"] == 0.6 and calls[1]["keep_known"] == dict(mode="cover", grow=2)
    # the eval scripts: refused with --mixed_pad before anything is loaded
    for lora, w in ((False, "--weights_path"), (True, "--lora_weights_path")):
        for f in (["--keep_known"], ["--strength", "0.6"]):
            with pytest.raises(SystemExit, match="--keep_known / --strength do not serve"):
                re_.main(["--json_path", "j", "--original_images_dir", "o", w, "w", "--scheduler", "", "--mixed_pad", "0.1"] + f, lora=lora)


# ---------------------------------------------------------------------------------------------- cover mode, on the restatement
def test_cover_mode_properties():
    g = torch.Generator().manual_seed(5)
    H, W = 64, 96
    m = ((torch.rand(2, H, W, generator=g) < 0.003) * 255).to(torch.uint8)
    m[0, 17, 33] = 127                                                 # below the threshold everywhere it matters
    nearest, cover0 = R.mask_pack(m, 0, 0), R.mask_pack(m, 1, 0)
    assert cover0.shape == (2, 24, 64) and ((cover0 >= nearest).all())                               # grow 0 cover contains nearest
    assert cover0.float().sum() > nearest.float().sum()
    prev = cover0
    for grow in (1, 2, 8):
        cur = R.mask_pack(m, 1, grow)
        assert (cur >= prev).all()
        prev = cur
    z = torch.zeros(1, H, W, dtype=torch.uint8)
    for mode, grow in ((0, 0), (1, 0), (1, 3), (1, 8)):
        assert R.mask_pack(z, mode, grow).float().abs().sum() == 0                                    # all zero stays zero
    z127 = torch.full((1, H, W), 127, dtype=torch.uint8)
    assert R.mask_pack(z127, 1, 8).float().abs().sum() == 0
    # one masked pixel away from the borders marks exactly its (2 grow + 1)^2 latent pixels
    for grow in (0, 1, 2):
        one = torch.zeros(1, H, W, dtype=torch.uint8)
        one[0, 8 * 4 + 3, 8 * 5 + 6] = 128                             # latent pixel (4, 5), off the sampling lattice
        got = R.mask_pack(one, 1, grow)
        lat = torch.zeros(H // 8, W // 8)
        for t in range(got.shape[1]):
            ty, tx = divmod(t, W // 16)
            for p in range(4):
                assert (got[0, t, p::4] == got[0, t, p]).all()         # the same for every latent channel
                lat[2 * ty + p // 2, 2 * tx + p % 2] = float(got[0, t, p])
        want = torch.zeros_like(lat)
        want[4 - grow:4 + grow + 1, 5 - grow:5 + grow + 1] = 1
        assert torch.equal(lat, want) and int(lat.sum()) == (2 * grow + 1) ** 2
        assert R.mask_pack(one, 0, 0).float().sum() == 0               # which nearest does not see at all
    # at a border the window is clipped
    corner = torch.zeros(1, H, W, dtype=torch.uint8)
    corner[0, 0, 0] = 255
    assert R.mask_pack(corner, 1, 1).float().sum() == 4 * 16 and R.mask_pack(corner, 0, 0).float().sum() == 16
