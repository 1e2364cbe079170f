"""Mixed-geometry batches, the host side (no GPU): the batch plan with a padding cap, the per-sample sigma schedules, and the
launch plan of a forward whose descriptor carries seq_len / rope_bstride -- recorded like tests/test_dit_launch_trace.py records the
uniform forward, with a recorder and a driver of its own (helpers/mixed_launch_recorder.cpp, helpers/mixed_trace_driver.cpp) and
its own golden, so that the uniform path's files stay untouched."""
import glob
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.test_dit_launch_trace import compare, parse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "textflux_amd", "csrc")
HELPERS = os.path.join(REPO, "tests", "helpers")
GOLDEN = os.path.join(REPO, "tests", "golden", "mixed_launch_trace.txt")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HAVE_HIP_HEADERS = os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h"))

SCENARIOS = """mixed_bf16_joint mixed_bf16_separate_no_rope_cs mixed_fp8 rope_bstride_alone mixed_step_sampler_2
mixed_fail_rope_bstride_0 mixed_fail_rope_bstride_negative mixed_step_fail_sampler_0 mixed_step_fail_sampler_1""".split()


# ----------------------------------------------------------------------------- plan_batches
def _works(sizes):
    from textflux_amd.batch_driver import Work
    return [Work(i, None, None, f"p{i}", {}, s) for i, s in enumerate(sizes)]


MIXED_LIST = [(576, 512), (1024, 1024), (576, 512), (512, 672), (1024, 1024), (640, 512), (576, 512), (512, 576), (1024, 672),
              (512, 672), (672, 1024), (1024, 1024), (576, 544), (512, 512), (640, 512), (1024, 992)]


def test_plan_batches_cap_0_is_todays_plan():
    from textflux_amd.batch_driver import plan_batches
    works = _works(MIXED_LIST)
    # today's plan, restated: geometries in order of first appearance, items in list order, chunks of batch_size
    want = []
    for size in dict.fromkeys(MIXED_LIST):
        idx = [i for i, s in enumerate(MIXED_LIST) if s == size]
        want += [(size, idx[k:k + 2]) for k in range(0, len(idx), 2)]
    for plan in (plan_batches(works, 2), plan_batches(works, 2, 0.0), plan_batches(works, 2, max_pad_fraction=0.0, text_tokens=64)):
        assert [(b.size, [w.index for w in b.items]) for b in plan] == want
        assert not any(b.mixed for b in plan)


@pytest.mark.parametrize("cap", [0.02, 0.1, 0.3])
@pytest.mark.parametrize("batch_size", [3, 8])
def test_plan_batches_with_a_padding_cap(cap, batch_size):
    from textflux_amd.batch_driver import image_tokens, pad_fraction, plan_batches
    works = _works(MIXED_LIST)
    plan = plan_batches(works, batch_size, cap)
    again = plan_batches(list(works), batch_size, cap)
    assert [(b.size, b.mixed, [w.index for w in b.items]) for b in plan] == [(b.size, b.mixed, [w.index for w in b.items]) for b in again]
    assert sorted(w.index for b in plan for w in b.items) == list(range(len(works)))          # every item exactly once
    order = [w.index for b in plan for w in b.items]
    assert order == sorted(range(len(works)), key=lambda i: image_tokens(MIXED_LIST[i]))     # sorted by token count, stable
    for b in plan:
        sizes = [w.size for w in b.items]
        assert 1 <= len(sizes) <= batch_size
        assert b.mixed == (len(set(sizes)) > 1)
        assert pad_fraction(sizes) <= cap, (sizes, pad_fraction(sizes))
        assert image_tokens(b.size) == max(image_tokens(s) for s in sizes)
    # greedy: a batch was closed only because it was full or the next item would have broken the cap
    for b, nxt in zip(plan, plan[1:]):
        sizes = [w.size for w in b.items]
        assert len(sizes) == batch_size or pad_fraction(sizes + [nxt.items[0].size]) > cap
    if cap >= 0.1:
        assert any(b.mixed for b in plan) and len(plan) < len(plan_batches(works, batch_size))


def test_pad_fraction_is_the_share_of_padded_rows():
    from textflux_amd.batch_driver import pad_fraction
    assert pad_fraction([(576, 512), (576, 512)]) == 0.0                   # one geometry: the uniform path, nothing is padded
    # 512 + 1152 = 1664 and 512 + 1024 = 1536 rows in a launch of N = 1792 (1664 rounded up to a multiple of 256)
    assert pad_fraction([(576, 512), (512, 512)]) == pytest.approx(1 - (1664 + 1536) / (2 * 1792))
    assert pad_fraction([(64, 64), (96, 64)], text_tokens=16) == pytest.approx(1 - (32 + 40) / (2 * 256))
    from textflux_amd.batch_driver import plan_batches
    with pytest.raises(ValueError):
        plan_batches([], 2, 1.0)


def test_run_items_refuses_mixed_pad_up_front_where_call_mixed_cannot_serve_it():
    """Before anything is prepared or encoded: a pipeline without call_mixed, and the AMO sampler (its coefficients are per step)."""
    from textflux_amd.batch_driver import run_items
    from textflux_amd.schedulers import StochasticRFOvershotDiscreteScheduler

    class Pipe:
        scheduler = StochasticRFOvershotDiscreteScheduler()

        def encode_prompt(self, *a, **k):
            raise AssertionError("reached the encoder")

        def call_mixed(self, *a, **k):
            raise AssertionError("reached call_mixed")

    with pytest.raises(NotImplementedError, match="Euler sampler"):
        run_items([dict(image="a", mask="b", text="c")], Pipe(), None, mixed_pad=0.1, device="cpu")
    with pytest.raises(ValueError, match="call_mixed"):
        run_items([], object(), None, mixed_pad=0.1, device="cpu")


# ----------------------------------------------------------------------------- per-sample sigma schedules
def test_per_sample_sigma_tables_are_each_samples_own_schedule():
    from textflux_amd.pipeline import calculate_shift, per_sample_schedules
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
    kw = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
    lens, n = [1152, 4096, 256, 1152, 2688], 7
    tabs = per_sample_schedules(FlowMatchEulerDiscreteScheduler(**kw), lens, n)
    assert tabs["timesteps"].shape == (5, n) and tabs["sigmas"].shape == (5, n + 1) and tabs["dsigma"].shape == (5, n)
    for b, S in enumerate(lens):
        fresh = FlowMatchEulerDiscreteScheduler(**kw)
        mu = calculate_shift(S, 256, 4096, 0.5, 1.15)
        fresh.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cpu", mu=mu)
        assert torch.equal(tabs["timesteps"][b], fresh.timesteps.float())
        assert torch.equal(tabs["sigmas"][b], fresh.sigmas.float())
        assert torch.equal(tabs["dsigma"][b], fresh.coef_table("cpu", torch.bfloat16)[:n])
    assert torch.equal(tabs["sigmas"][0], tabs["sigmas"][3]) and not torch.equal(tabs["sigmas"][0], tabs["sigmas"][1])
    # custom sigmas pass through
    custom = [1.0, 0.7, 0.2]
    t2 = per_sample_schedules(FlowMatchEulerDiscreteScheduler(**kw), [256, 4096], 3, sigmas=custom)
    fresh = FlowMatchEulerDiscreteScheduler(**kw)
    fresh.set_timesteps(sigmas=custom, device="cpu", mu=calculate_shift(4096, 256, 4096, 0.5, 1.15))
    assert torch.equal(t2["sigmas"][1], fresh.sigmas.float())


# ----------------------------------------------------------------------------- launch trace
def trace(workdir=None):
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        exe = os.path.join(tmp, "mixed_trace")
        srcs = sorted(p for p in glob.glob(os.path.join(CSRC, "*.cpp")) if os.path.basename(p) != "launch.cpp")
        srcs += [os.path.join(HELPERS, "mixed_launch_recorder.cpp"), os.path.join(HELPERS, "mixed_trace_driver.cpp")]
        cmd = [CXX, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I",
               os.path.join(REPO, "include"), *srcs, "-Wl,--unresolved-symbols=ignore-all", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"trace binary ended with {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
        return r.stdout


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_mixed_launch_trace_matches_its_golden(tmp_path):
    got = trace(workdir=str(tmp_path))
    want = open(GOLDEN).read()
    assert list(parse(want)) == SCENARIOS and list(parse(got)) == SCENARIOS
    bad = compare(got, want)
    assert not bad, "\n".join(bad[:20])
    sc = {n: lines for n, (lines, _) in parse(got).items()}
    # one whole mixed forward: every attention launch carries the lengths, every fused projection the table stride
    full = sc["mixed_bf16_joint"]
    attn = [l for l in full if l.startswith("joint_attention")]
    assert len(attn) == 4 and all(" seq_len=seq_len" in l for l in attn) and full[-2:] == ["rc 0", "error "]
    qkn = [l for l in full if " rope_cs=" in l]
    assert len(qkn) == 4 and all(" rope_bs=512 " in l for l in qkn)
    assert not any(l.startswith("rmsnorm_rope") for l in full)
    sep = sc["mixed_bf16_separate_no_rope_cs"]
    tabs = [l for l in sep if l.startswith("rmsnorm_rope_tab ")]
    assert len(tabs) == 3 and all(l.split()[-2] == str(356 * 128) for l in tabs) and not any(l.startswith("rmsnorm_rope ") for l in sep)
    assert all(" seq_len=seq_len" in l for l in sc["mixed_fp8"] if l.startswith("joint_attention"))
    assert not any("seq_len" in l for l in sc["rope_bstride_alone"]) and any(" rope_bs=512 " in l for l in sc["rope_bstride_alone"])
    assert sc["mixed_step_sampler_2"][0].startswith("select_step") and sc["mixed_step_sampler_2"][-2:] == ["rc 0", "error "]
    # the refusals: return code and text
    for name, text in (("mixed_fail_rope_bstride_0", "needs rope_bstride > 0"), ("mixed_fail_rope_bstride_negative", "must not be negative"),
                       ("mixed_step_fail_sampler_0", "needs sampler 2"), ("mixed_step_fail_sampler_1", "needs sampler 2")):
        assert sc[name][0] == "rc 1" and text in sc[name][1] and len(sc[name]) == 2, (name, sc[name])


# ----------------------------------------------------------------------------- emitted ISA of the per-sample-length attention kernels
@pytest.mark.skipif(not (os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) or shutil.which("hipcc")), reason="hipcc not available")
def test_seq_len_attention_kernels_have_no_mfma_result_hazard_and_no_spill(tmp_path):
    """attn_w4v_kernel<0> / <4> read their scores from inline asm like attn_w4_kernel does (tests/test_isa_hazards.py): the same
    static check of the wait states behind MFMA results on their emitted ISA, and no scratch (a spill would also fail the launch)."""
    import re
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_mfma_hazard as ck
    out = tmp_path / "attention_w4.s"
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                        "--cuda-device-only", "-S", "-mllvm", "-amdgpu-mfma-vgpr-form", "-o", str(out), os.path.join(CSRC, "attention_w4.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    ks = [k for k in ck.check_all(asm) if "attn_w4v_kernel" in k[0]]
    assert len(ks) == 2, [k[0] for k in ks]
    for name, n, n_mfma, rep in ks:
        assert n_mfma > 250 and n > 3000, name
        assert rep == [], (name, rep[:5])
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", asm[asm.index(".amdhsa_kernel " + name):]).group(1)) == 0, name
