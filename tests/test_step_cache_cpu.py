"""The first-block step cache without a GPU: the launch plan of the three phases of tfx_dit_step_run, every refusal of the step
path, the new symbols, and the host decision.

Launch plan: as tests/test_dit_launch_trace.py does for the forward, the host code of csrc/ is compiled with the plain C++ compiler
and linked against the recording launch layer (helpers/launch_recorder.cpp, plus helpers/step_cache_recorder.cpp for the four
launchers the cache adds) and helpers/step_cache_trace_driver.cpp, which runs a 2 + 2-block model through tfx_dit_step_run as a whole
step and as phases 1 / 2 / 3 -- joint and separate text launches, bf16 and fp8 linears, sampler 0 / 1 / 2.  The output is pinned by
golden/step_cache_launch_trace.txt, and the properties that make "every step computed == the plain loop" hold by construction are
asserted on it.  Regenerate the golden on purpose only:   python tests/test_step_cache_cpu.py --write tests/golden/step_cache_launch_trace.txt"""
import ctypes as C
import glob
import math
import os
import subprocess
import sys
import tempfile

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.test_dit_launch_trace import CSRC, CXX, HAVE_HIP_HEADERS, HELPERS, REPO, ROCM, compare, parse

GOLDEN = os.path.join(REPO, "tests", "golden", "step_cache_launch_trace.txt")
CONFIGS = ("bf16_joint", "bf16_separate", "fp8")
CACHE_LAUNCHERS = ("step_cache_save", "step_cache_metric", "step_cache_store", "step_cache_apply")
BLOCK_LAUNCHERS = ("joint_attention", "rmsnorm_rope", "quantize_rows_fp8", "ln_modulate_split", "ln_modulate_fp8", "gemm_fp8",
                   "gemm_bf16_lora")


def trace(workdir=None):
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        exe = os.path.join(tmp, "step_cache_trace")
        srcs = sorted(p for p in glob.glob(os.path.join(CSRC, "*.cpp")) if os.path.basename(p) != "launch.cpp")
        srcs += [os.path.join(HELPERS, f) for f in ("launch_recorder.cpp", "step_cache_recorder.cpp", "step_cache_trace_driver.cpp")]
        cmd = [CXX, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I",
               os.path.join(REPO, "include"), *srcs, "-Wl,--unresolved-symbols=ignore-all", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"trace binary ended with {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
        return r.stdout


@pytest.fixture(scope="module")
def scenarios(tmp_path_factory):
    """{scenario: every line between its header and the next, in order (probe lines included)}"""
    text = trace(workdir=str(tmp_path_factory.mktemp("step_cache_trace")))
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        else:
            cur.append(line)
    return text, out


def launches(lines):
    """a scenario's lines without its return code / error text; asserts that it ran"""
    assert lines[-2:] == ["rc 0", "error "], lines[-2:]
    return lines[:-2]


def name_of(line):
    return line.split(" ", 1)[0]


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_trace_matches_the_golden(scenarios):
    text, sc = scenarios
    want = open(GOLDEN).read()
    assert list(parse(text)) == list(parse(want))
    bad = compare(text, want)
    assert not bad, "\n".join(bad[:20])
    assert sum(1 for lines in sc.values() if lines[-2] == "rc 0") == 3 * 3 * 4 + 1


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("sampler", (0, 1, 2))
def test_head_plus_computed_tail_is_the_whole_step(scenarios, cfg, sampler):
    """Phase 1 + phase 2 without the cache's own launchers == the whole step, line by line (probes included): the same kernels with
    the same arguments in the same order, which is what makes a run that computes every step bit-equal to the plain loop."""
    _, sc = scenarios
    base = f"{cfg}_sampler{sampler}"
    whole = launches(sc[base + "_whole"])
    head, tail = launches(sc[base + "_phase1"]), launches(sc[base + "_phase2"])
    assert [l for l in head + tail if name_of(l) not in CACHE_LAUNCHERS] == whole
    assert len(whole) > 30 and not any(name_of(l) in CACHE_LAUNCHERS for l in whole)
    # the head: select_step first, x0 taken between the embedders and block 0, the metric last
    names = [name_of(l) for l in head if not l.startswith("probe ")]
    assert names[0] == "select_step" and names[-1] == "step_cache_metric" and names.count("step_cache_save") == 1
    k = names.index("step_cache_save")
    assert names[:k] == ["select_step", "gemm_bf16", "copy_rows"]                   # x_embedder, ctx0 copy
    assert names[k + 1:-1].count("joint_attention") == 1                            # exactly block 0 behind it
    assert [n for n in names if n in CACHE_LAUNCHERS] == ["step_cache_save", "step_cache_metric"]
    # the computed tail: the store pass after the sampler update, the cursor advance last
    names = [name_of(l) for l in tail if not l.startswith("probe ")]
    assert [n for n in names if n in CACHE_LAUNCHERS] == ["step_cache_store"]
    assert names[-2:] == ["step_cache_store", "advance_step"] and names.count("joint_attention") == 3
    assert (names[-3] == "sched_step") == (sampler != 2)


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("sampler", (0, 1, 2))
def test_cached_tail_holds_no_block(scenarios, cfg, sampler):
    _, sc = scenarios
    base = f"{cfg}_sampler{sampler}"
    tail3 = launches(sc[base + "_phase3"])
    names = [name_of(l) for l in tail3]
    assert not any(n in BLOCK_LAUNCHERS or n == "probe" for n in names), names
    want = ["step_cache_apply", "ln_modulate", "gemm_bf16"] + (["sched_step"] if sampler != 2 else []) + ["advance_step"]
    assert names == want
    # norm_out / proj_out, the sampler update and the advance are the whole step's own last launches
    assert tail3[1:] == launches(sc[base + "_whole"])[-(len(want) - 1):]


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_phase_0_ignores_the_cache_and_the_views_are_the_image_rows(scenarios):
    _, sc = scenarios
    assert sc["whole_with_cache"] == sc["bf16_joint_sampler2_whole"]
    for cfg, T in (("bf16_joint", 256), ("bf16_separate", 100)):
        line = next(l for l in sc[f"{cfg}_sampler0_phase1"] if l.startswith("step_cache_metric"))
        D, S = 256, 256
        off = f"+{T * D * 2:#x}"
        assert f" hid=hid{off} ldh={D} hbs={(S + T) * D} x0=x0 f_prev=f_prev h1=h1 r=r ld={D} bs={S * D} " in line and line.endswith(f"rows={S} batch=2 D={D}")


REFUSALS = {
    "fail_phase_without_cache": "phase 1 needs a step cache",
    "fail_phase_4": "phase must be 0 (whole step), 1 (head), 2 (computed tail) or 3 (cached tail)",
    "fail_phase_negative": "phase must be 0",
    "fail_seq_len": "cannot serve a mixed-geometry batch (dit.seq_len)",
    "fail_first_block": "needs the whole forward",
    "fail_last_block": "needs the whole forward",
    "fail_flags_1": "needs the whole forward",
    "fail_flags_2_phase_0": "needs the whole forward",
    "fail_one_block": "needs at least 2 blocks (n_double + n_single = 1)",
    "fail_null_x0": "null pointer in tfx_step_cache",
    "fail_null_metric": "null pointer in tfx_step_cache",
    "fail_partials_small": "partials_bytes 8 is too small",
    "fail_cache_ld": "row pitches must be >= D",
}


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_step_check_refuses(scenarios, name):
    _, sc = scenarios
    lines = sc[name]
    assert lines[0] == "rc 1" and len(lines) == 2, lines           # refused before anything is launched
    assert lines[1].startswith("error tfx_dit_step") and REFUSALS[name] in lines[1], lines[1]


# ---------------------------------------------------------------------------------------------- symbols
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


def test_abi_11_and_the_descriptor_fields():
    from textflux_amd import _lib as L
    assert L.ABI_VERSION == L.header_abi_version() == 11
    names = [f for f, _ in L.StepDesc._fields_]
    assert names[-2:] == ["cache", "phase"]
    sd = L.StepDesc()
    assert not sd.cache and sd.phase == 0                          # a value-initialised descriptor is a whole step without a cache
    assert [f for f, _ in L.StepCache._fields_] == ["x0", "f_prev", "h1", "r", "ld", "bstride", "partials", "partials_bytes", "metric"]


@pytest.mark.parametrize("sym", ("tfx_step_cache_metric", "tfx_step_cache_store", "tfx_step_cache_apply"))
def test_kernel_entry_points_check_their_arguments(lib, sym):
    from textflux_amd import _lib as L
    fn = getattr(lib, sym)
    sc = L.StepCache()
    buf = 1 << 20                                                   # never dereferenced: every call below is refused on the host
    assert fn(None, 256, 0, C.byref(sc), 1, 1, 256, None) != 0 and b"null pointer" in lib.tfx_last_error()
    assert fn(buf, 256, 0, None, 1, 1, 256, None) != 0 and b"null pointer" in lib.tfx_last_error()
    assert fn(buf, 256, 0, C.byref(sc), 1, 1, 256, None) != 0 and b"null pointer in tfx_step_cache" in lib.tfx_last_error()
    for k in ("x0", "f_prev", "h1", "r", "partials", "metric"):
        setattr(sc, k, buf)
    sc.ld, sc.bstride, sc.partials_bytes = 256, 256 * 4, 4096
    for k in ("x0", "f_prev", "h1", "r", "partials", "metric"):    # each pointer on its own
        setattr(sc, k, None)
        assert fn(buf, 256, 1024, C.byref(sc), 4, 2, 256, None) != 0 and b"null pointer in tfx_step_cache" in lib.tfx_last_error(), k
        setattr(sc, k, buf)
    assert fn(buf, 256, 1024, C.byref(sc), 4, 2, 252, None) != 0 and b"multiple of 8" in lib.tfx_last_error()
    for rows, batch, D in ((0, 2, 256), (4, 0, 256), (4, 2, 0), (-1, 2, 256)):
        assert fn(buf, 256, 1024, C.byref(sc), rows, batch, D, None) != 0 and b"must be positive" in lib.tfx_last_error()
    assert fn(buf, 128, 1024, C.byref(sc), 4, 2, 256, None) != 0 and b"row pitches" in lib.tfx_last_error()
    assert fn(buf, 256, 1020, C.byref(sc), 4, 2, 256, None) != 0 and b"multiple of 8" in lib.tfx_last_error()
    assert fn(buf, 256, 512, C.byref(sc), 4, 2, 256, None) != 0 and b"batch stride smaller" in lib.tfx_last_error()
    assert fn(buf + 8, 256, 1024, C.byref(sc), 4, 2, 256, None) != 0 and b"16-byte aligned" in lib.tfx_last_error()
    sc.partials_bytes = 8
    assert fn(buf, 256, 1024, C.byref(sc), 4, 2, 256, None) != 0 and b"partials_bytes" in lib.tfx_last_error()


# ---------------------------------------------------------------------------------------------- the host decision
def test_config_has_no_default_threshold_and_checks_its_values():
    from textflux_amd.step_cache import StepCacheConfig
    with pytest.raises(ValueError, match="no default threshold"):
        StepCacheConfig.make(None)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            StepCacheConfig.make(bad)
    with pytest.raises(ValueError):
        StepCacheConfig.make(0.1, max_consecutive=0)
    c = StepCacheConfig.make(0.25, skip_steps=[4, 2, 2], max_consecutive=3)
    assert c.threshold == 0.25 and c.skip_steps == frozenset({2, 4}) and c.max_consecutive == 3


def test_decision_function():
    from textflux_amd.step_cache import Decider, StepCacheConfig, decide, replay
    inf = float("inf")
    always = StepCacheConfig.make(inf)
    # step 0 is always computed, and nothing is skipped before a computed step exists in this call
    assert not decide(always, 0, [0.0], True, 0)
    assert not decide(always, 3, [0.0], False, 0)
    assert decide(always, 1, [0.0], True, 0)
    # the threshold is strict and the LARGEST metric of the batch decides
    c = StepCacheConfig.make(0.1)
    assert decide(c, 1, [0.05, 0.0999], True, 0)
    assert not decide(c, 1, [0.05, 0.1], True, 0)
    assert not decide(c, 1, [0.2, 0.01], True, 0) and not decide(c, 1, [0.01, 0.2], True, 0)
    # threshold 0 never skips; +inf (a zero reference residual) and NaN never pass, not even threshold inf
    assert not decide(StepCacheConfig.make(0), 1, [0.0, 0.0], True, 0)
    assert not decide(always, 1, [0.0, inf], True, 0) and not decide(always, 1, [math.nan, 0.0], True, 0)
    assert not decide(c, 1, [inf], True, 0)
    # an explicit schedule skips whatever the metric says -- but never step 0, never without a computed step, never a forced step
    s = StepCacheConfig.make(0, skip_steps={0, 2, 4, 5})
    assert replay(s, [[inf]] * 7) == [False, False, True, False, True, True, False]
    assert not decide(s, 2, [0.0], False, 0)
    assert not decide(StepCacheConfig.make(inf, skip_steps={2}, force_compute={2}), 2, [0.0], True, 0)
    # max_consecutive caps runs of threshold skips: computed / skip / skip / computed ...
    assert replay(StepCacheConfig.make(inf, max_consecutive=2), [[0.0, 0.0]] * 8) == [False, True, True, False, True, True, False, True]
    assert replay(StepCacheConfig.make(inf, max_consecutive=1), [[0.0]] * 5) == [False, True, False, True, False]
    assert replay(always, [[0.0]] * 4) == [False, True, True, True]
    # a mixed trajectory, and the report the pipeline publishes
    d = Decider(StepCacheConfig.make(0.1, max_consecutive=2))
    rows = [[inf, inf], [0.3, 0.01], [0.05, 0.02], [0.01, 0.01], [0.01, 0.01], [0.5, 0.01], [0.09, 0.09]]
    assert [d.step(i, m) for i, m in enumerate(rows)] == [False, False, True, True, False, False, True]
    assert [r["skipped"] for r in d.report] == [False, False, True, True, False, False, True] and d.report[1]["metric"] == [0.3, 0.01]


def test_pipeline_switches_without_a_gpu():
    """enable / disable store the settings; call_mixed refuses before it touches anything"""
    from textflux_amd.pipeline import FluxFillPipeline
    pipe = FluxFillPipeline.__new__(FluxFillPipeline)
    pipe._step_cache = None
    with pytest.raises(ValueError, match="no default threshold"):
        pipe.enable_step_cache(None)
    assert pipe.enable_step_cache(0.2, skip_steps={3}, max_consecutive=2) is pipe
    assert pipe._step_cache.threshold == 0.2 and pipe._step_cache.skip_steps == frozenset({3}) and pipe._step_cache.max_consecutive == 2
    pipe.scheduler = pipe.transformer = None
    with pytest.raises(NotImplementedError, match="step cache"):
        pipe.call_mixed(prompt="x", sizes=[(256, 256)])
    assert pipe.disable_step_cache() is pipe and pipe._step_cache is None


def test_run_items_passes_the_settings_and_counts_the_steps():
    """run_items(step_cache=dict): switched on for the run and off afterwards (also when the run raises), steps counted from the
    pipeline's reports; refused with mixed_pad and for a pipeline without the switch.  The CLIs carry the two flags."""
    import importlib
    from textflux_amd import batch_driver as bd
    from tests.test_batch_driver_cpu import StubPipe, _items, _loader

    class CachedStub(StubPipe):
        def __init__(self):
            super().__init__(0)
            self.cfg, self.log, self.step_cache_report = None, [], None

        def enable_step_cache(self, threshold, skip_steps=None, max_consecutive=None):
            self.cfg = (threshold, skip_steps, max_consecutive)
            self.log.append(("on", self.cfg))

        def disable_step_cache(self):
            self.cfg = None
            self.log.append(("off",))

        def __call__(self, **kw):
            assert self.cfg == (0.25, None, 2)
            self.step_cache_report = [dict(metric=[0.0], skipped=i in (2, 3)) for i in range(kw["num_inference_steps"])]
            return super().__call__(**kw)

    pipe = CachedStub()
    res = bd.run_items(_items()[:3], pipe, None, batch_size=8, num_inference_steps=5, device="cpu", loader=_loader, save=lambda i, im: None,
                       step_cache=dict(threshold=0.25, max_consecutive=2))
    assert res["all_done"] == [0, 1, 2] and len(pipe.calls) == 2
    assert (res["steps_skipped"], res["steps_total"]) == (4, 10) and pipe.log == [("on", (0.25, None, 2)), ("off",)] and pipe.cfg is None
    plain = bd.run_items(_items()[:3], StubPipe(0), None, batch_size=8, device="cpu", loader=_loader, save=lambda i, im: None)
    assert "steps_total" not in plain
    with pytest.raises(NotImplementedError, match="mixed"):
        bd.run_items(_items()[:3], CachedStub(), None, device="cpu", loader=_loader, mixed_pad=0.1, step_cache=dict(threshold=0.1))
    with pytest.raises(ValueError, match="enable_step_cache"):
        bd.run_items(_items()[:3], StubPipe(0), None, device="cpu", loader=_loader, step_cache=dict(threshold=0.1))
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    sys.path.insert(0, REPO)
    for mod, argv in (("run_eval", ["--json_path", "a", "--original_images_dir", "o", "--weights_path", "w"]),
                      ("run_inference_lora", ["--image", "i", "--mask", "m", "--words", "w"])):
        ap = importlib.import_module(mod).build_parser()
        a = ap.parse_args(argv)
        assert a.step_cache is None and a.step_cache_max_consecutive is None           # off unless asked for: no default threshold
        a = ap.parse_args(argv + ["--step_cache", "0.2", "--step_cache_max_consecutive", "3"])
        assert a.step_cache == 0.2 and a.step_cache_max_consecutive == 3


def main():
    import argparse
    ap = argparse.ArgumentParser(description="launch trace of the step cache's phases, compared with the golden")
    ap.add_argument("--write", metavar="FILE", help="write the trace to FILE instead of comparing it")
    a = ap.parse_args()
    got = trace()
    if a.write:
        with open(a.write, "w") as f:
            f.write(got)
        print(f"{a.write}: {len(got)} bytes, {len(parse(got))} scenarios")
        return 0
    bad = compare(got, open(GOLDEN).read())
    print("\n".join(bad) if bad else f"launch trace equals {os.path.relpath(GOLDEN, REPO)} ({len(parse(got))} scenarios)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
