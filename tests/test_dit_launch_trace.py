"""The launch plan of tfx_dit_forward / tfx_dit_step_run, pinned without a GPU.

Everything the forward reaches goes through the internal launch API (csrc/launch.h), so the host code of csrc/ (every .cpp except
launch.cpp) is compiled with the plain C++ compiler and linked against a recording stand-in for that API
(helpers/launch_recorder.cpp) and a driver (helpers/dit_trace_driver.cpp) that runs the public entry points over fake device
addresses.  The output -- which kernels, in which order, with which arguments, for bf16 joint / separate, fp8, runtime LoRA, block
ranges, the step path and every refusal -- is compared with golden/dit_launch_trace.txt:

  * launch lines, return codes and error texts: equal as a sequence, byte for byte;
  * `probe` lines (the questions the forward asks the launch layer: gemm_rowsplit_ok / gemm_qkn_ok / gemm_fp8_qkn_ok with their
    full arguments): as a set per scenario.  The code may ask fewer questions than the golden holds, never a new one -- a probe with
    other arguments (say, without the workspace attached) would get another answer from the real launch layer.

Point it at another checkout:   python tests/test_dit_launch_trace.py --csrc OTHER/textflux_amd/csrc [--write FILE]
The golden is regenerated on purpose only ("The forward's structure and its launch trace")."""
import argparse
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "textflux_amd", "csrc")
HELPERS = os.path.join(REPO, "tests", "helpers")
GOLDEN = os.path.join(REPO, "tests", "golden", "dit_launch_trace.txt")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HAVE_HIP_HEADERS = os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h"))

SCENARIOS = """
bf16_joint bf16_joint_qkn_refused bf16_joint_no_rope_cs bf16_joint_ln_joint_0 bf16_group_streams_0
bf16_separate_T100 bf16_separate_T100_qkn_refused bf16_separate_T100_no_rope_cs bf16_separate_T256_rowsplit_refused bf16_separate_T0
fp8_H2 fp8_H2_qkn_refused fp8_H2_fuse_qkn_0 fp8_H1_bf16_fallback fp8_linears_without_w8 fp8_T0
lora_joint_img_D384 lora_joint_both_D384 lora_separate_D384 lora_separate_no_rope_cs lora_planes_joint_D256 lora_planes_separate_D256
lora_single_D512 lora_single_planes_D256 lora_desc_proj_out lora_desc_proj_out_euler_gate
lora_fail_null_t_xn lora_fail_null_t_y lora_fail_null_scale lora_fail_fp8_quantised_by_ln lora_fail_fp8_quantise_pass
lora_fail_fp8_without_w8 lora_fail_partner_ldw lora_fail_partner_rank lora_fail_nseg_5 lora_fail_rank_0 lora_fail_x_embedder
lora_fail_planes_in_y
flags_1_skip_embed flags_2_skip_tail flags_3 blocks_0_1 blocks_1_3 blocks_3_4_separate blocks_first_negative_last_beyond euler_gate
step_sampler_0 step_sampler_1 step_sampler_2 step_fail_null_desc step_fail_null_mod_table step_fail_null_mod_cur
step_fail_null_step_ptr step_fail_mod_not_mod_cur step_fail_sampler_3 step_fail_sampler_negative step_fail_sampler_2_null_gate
step_fail_sampler_2_gate_outside step_fail_gate_without_sampler_2 step_fail_null_latents step_fail_null_coef
step_fail_amo_null_noise step_fail_null_out step_fail_forward_refuses
fail_D_not_128H fail_B_0 fail_S_0 fail_T_negative fail_fp8_null_q8 fail_fp8_null_q8_scale fail_null_desc fail_null_xin fail_null_mod
fail_null_hid fail_null_xn fail_null_y fail_null_out fail_null_cos_tab fail_null_sin_tab fail_null_dbl fail_null_sgl fail_null_ctx0
""".split()


def trace(csrc=CSRC, workdir=None):
    """Builds the trace binary from the host sources of `csrc` and returns what it prints."""
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        exe = os.path.join(tmp, "dit_trace")
        srcs = sorted(p for p in glob.glob(os.path.join(csrc, "*.cpp")) if os.path.basename(p) != "launch.cpp")
        srcs += [os.path.join(HELPERS, "launch_recorder.cpp"), os.path.join(HELPERS, "dit_trace_driver.cpp")]
        include = os.path.normpath(os.path.join(csrc, "..", "..", "include"))
        # what the host sources reference beyond the recorder (the other launchers, the HIP runtime) stays unresolved: the
        # forward must not reach it, and a call through such a symbol ends the run
        cmd = [CXX, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", csrc, "-I", include,
               *srcs, "-Wl,--unresolved-symbols=ignore-all", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"trace binary ended with {r.returncode}: a launcher the recorder does not define?\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
        return r.stdout


def parse(text):
    """{scenario: (launch / rc / error lines in order, set of probe lines)}, scenarios in order of appearance"""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("== "):
            cur = line[3:]
            assert cur not in out, f"scenario {cur} twice"
            out[cur] = ([], set())
        elif line.startswith("probe "):
            out[cur][1].add(line)
        else:
            out[cur][0].append(line)
    return out


def compare(got_text, want_text):
    """list of differences (empty = the launch plan is the golden's)"""
    got, want = parse(got_text), parse(want_text)
    bad = []
    if list(got) != list(want):
        bad.append(f"scenario lists differ: {sorted(set(got) ^ set(want))}")
    for name in want:
        if name not in got:
            continue
        (gl, gp), (wl, wp) = got[name], want[name]
        if gl != wl:
            i = next((i for i, (a, b) in enumerate(zip(gl, wl)) if a != b), min(len(gl), len(wl)))
            bad.append(f"{name}: line {i} of {len(gl)} (golden {len(wl)}):\n  got    {gl[i] if i < len(gl) else '<end>'}\n  golden {wl[i] if i < len(wl) else '<end>'}")
        for p in sorted(gp - wp):
            bad.append(f"{name}: a probe the golden does not hold:\n  {p}")
    return bad


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_dit_launch_trace_matches_the_golden(tmp_path):
    got = trace(workdir=str(tmp_path))
    want = open(GOLDEN).read()
    assert list(parse(want)) == SCENARIOS             # no scenario drops out of the golden ...
    assert list(parse(got)) == SCENARIOS              # ... or out of the driver
    bad = compare(got, want)
    assert not bad, "\n".join(bad[:20])
    ran = [n for n, (lines, _) in parse(got).items() if "rc 0" in lines and len(lines) >= 4]
    assert len(ran) == 37, ran                        # the forwards really ran: not a file of refusals


def test_compare_refuses_a_changed_launch_and_a_new_probe():
    """the comparison itself: order matters for launches, probes may only disappear"""
    want = "== a\nprobe gemm_qkn_ok M=1 workspace=ws\nprobe gemm_qkn_ok M=2 workspace=ws\ngemm_bf16 M=1\nln_modulate x\nrc 0\nerror \n"
    assert compare(want, want) == []
    assert compare(want.replace("probe gemm_qkn_ok M=2 workspace=ws\n", ""), want) == []            # one question fewer
    assert compare(want.replace("M=2 workspace=ws", "M=2"), want)                                   # the question changed
    assert compare(want.replace("gemm_bf16 M=1\nln_modulate x\n", "ln_modulate x\ngemm_bf16 M=1\n"), want)   # order
    assert compare(want.replace("rc 0", "rc 1"), want) and compare(want.replace("error ", "error x"), want)
    assert compare(want.replace("== a", "== b"), want) and compare(want + "== b\nrc 0\nerror \n", want)


def main():
    ap = argparse.ArgumentParser(description="launch trace of the DiT forward of a csrc directory, compared with the golden")
    ap.add_argument("--csrc", default=CSRC, help="directory with capi.cpp and the other host sources (default: this checkout)")
    ap.add_argument("--write", metavar="FILE", help="write the trace to FILE instead of comparing it")
    a = ap.parse_args()
    got = trace(os.path.abspath(a.csrc))
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
