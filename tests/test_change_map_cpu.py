"""Change-map sampling without a GPU (DESIGN.md section 4 "Change-map sampling"): the restatement of helpers/change_map_ref.py and
schedulers.change_cut_table against what the reference computes (tests/golden/g17_change_map.safetensors, written by
tests/golden/make_change_map_goldens.py), bit for bit; the new entry points' declarations and host checks; the step's launch plan
on the recording launch layer; the callers' arguments."""
import ctypes as C
import glob
import importlib
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from tests.helpers import change_map_ref as R
from tests.helpers import keep_known_ref as K
from tests.test_dit_launch_trace import CSRC, CXX, HAVE_HIP_HEADERS, HELPERS, ROCM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
N = 5
RUNS = (("1", 1), ("3", 3), ("5", 5), ("30", 30), ("4s50", 2))          # the recorded n; "4s50": 4 steps after strength 0.5 run 2
ISSUE_N = (1, 2, 3, 4, 5, 7, 28, 30, 50, 100, 255, 256, 257, 300, 1000)


@pytest.fixture(scope="module")
def gold():
    return load_file(os.path.join(REPO, "tests", "golden", "g17_change_map.safetensors"))


def bits(t):
    return t.contiguous().view(torch.int16)


def as_original_mask(hold, C=64):
    """what the reference's preprocess -> prepare_mask_latents make of its mask bytes: bf16(q / 255), repeated over the channels"""
    return (hold.float() / 255).to(BF).repeat(1, 1, C // 4)


# ---------------------------------------------------------------------------------------------- the restatement == the reference
def test_pack_restatement_equals_the_references_mask_latents(gold):
    cmap = gold["map_u8"]
    assert cmap.shape == (32, 48) and cmap.dtype == torch.uint8
    hold = R.pack(cmap[None], 0, 0)
    assert hold.shape == (1, 6, 4) and hold.dtype == torch.uint8
    assert torch.equal(bits(as_original_mask(hold)), bits(gold["map_original_mask"]))
    assert len(hold.unique()) > 2                                                      # a grey map, not a binary one
    # the lone pixels: nearest sees the one on the lattice and not the ones off it; cover sees them all
    lat = lambda h: torch.stack([h[0, t, p] for ty in range(2) for py in range(2) for tx in range(3) for px in range(2)
                                 for t, p in [(ty * 3 + tx, py * 2 + px)]]).view(4, 6)
    near, cov = lat(hold), lat(R.pack(cmap[None], 1, 0))
    assert near[3, 5] == 255 and cmap[24, 40] == 0 and cmap[24, 41] > 0                # on the lattice: held to the end
    assert near[3, 0] == 255 - cmap[24, 0] and cov[3, 0] == 0 and cmap[25, 1] == 255   # off it: only cover frees the token
    assert near[0, 2] == 255 - cmap[0, 16] and cov[0, 2] == 0 and cmap[7, 23] == 255
    assert (cov <= near).all()                                                         # cover never holds longer than nearest
    q = gold["bytes_hold_u8"]
    hold256 = R.pack((255 - q)[None], 0, 0)
    assert sorted(hold256.flatten().tolist()) == list(range(256))
    assert torch.equal(bits(as_original_mask(hold256, 4)), bits(gold["bytes_original_mask4"]))


@pytest.mark.parametrize("name,n", RUNS)
def test_cut_tables_equal_the_references_masks_for_every_byte(gold, name, n):
    from textflux_amd.schedulers import change_cut_table
    hold256 = R.pack((255 - gold["bytes_hold_u8"])[None], 0, 0)[0]                    # [64, 4], every byte once
    masks = gold[f"bytes_masks_n{name}"]
    assert masks.shape == (n, 64, 4)
    for table in (change_cut_table(n, "keep"), R.cut_table(n, "keep")):
        assert table.dtype == torch.int32 and table.shape == (n,)
        for i in range(n):
            assert torch.equal(hold256.to(torch.int32) > int(table[i]), masks[i].bool()), (n, i)
    # ... and on the recorded grey map
    hold = R.pack(gold["map_u8"][None], 0, 0)
    m = gold[f"map_masks_n{name}"]
    assert m.shape == (n, 6, 64)
    cut = change_cut_table(n, "keep")
    for i in range(n):
        assert torch.equal(R.hold_mask(hold, cut[i])[0].bool(), m[i].bool()), (n, i)
    assert 0 < m.float().sum() < m.numel() or n == 1


def test_cut_table_values_order_and_last():
    from textflux_amd.schedulers import change_cut_table
    for n in ISSUE_N:
        keep, free = change_cut_table(n), change_cut_table(n, "free")
        assert torch.equal(keep, R.cut_table(n, "keep")) and torch.equal(free, R.cut_table(n, "free")), n
        assert (keep[1:] >= keep[:-1]).all() and keep[0] == 0 and int(free[-1]) == 255 and torch.equal(free[:-1], keep[:-1])
        assert (int(keep[-1]) == 255) == (n >= 300), n                                 # from n = 300 on the last entries reach 255
    assert change_cut_table(30).tolist()[:4] + change_cut_table(30).tolist()[-3:] == [0, 8, 17, 25, 229, 238, 246]
    assert change_cut_table(3).tolist() == [0, 85, 170]                                # byte 85 is NOT held at step 1: a bf16 tie
    assert change_cut_table(1).tolist() == [0] and change_cut_table(1, "free").tolist() == [255]
    for bad in (0, -1):
        with pytest.raises(ValueError):
            change_cut_table(bad)
    with pytest.raises(ValueError, match="last"):
        change_cut_table(3, "loose")


@pytest.mark.parametrize("begin", [0, 2])
def test_loop_restatement_equals_the_reference(gold, begin):
    x0, noise, hold, sig = gold["x0"], gold["noise"], gold["loop_hold_u8"], gold["sigmas"]
    n = N - begin
    assert x0.shape == (2, 6, 64) and hold.shape == (2, 6, 4) and sig.shape == (N + 1,)
    assert torch.equal(bits(as_original_mask(hold)), bits(gold["loop_original_mask"]))
    tab, cut = R.keep_sigma(sig, begin), R.cut_table(n, "free")
    lats = [gold[f"b{begin}_s{i}_latents"] for i in range(n)]
    outs = R.run_blends(lats, x0, noise, hold, sig, begin, "free")
    changed = 0
    for i in range(n):
        assert torch.equal(bits(R.scale_noise(x0, tab[i], noise)), bits(gold[f"b{begin}_s{i}_image_latent"])), i
        assert torch.equal(bits(outs[i]), bits(gold[f"b{begin}_s{i}_out"])), i
        changed += int((bits(outs[i]) != bits(lats[i])).sum())
    assert changed > 0
    assert torch.equal(bits(outs[-1]), bits(lats[-1]))                                  # the reference's last step leaves the latents alone
    # the planted signed zeros: all sixteen combinations of held, latent sign, x0 sign, noise sign are in columns 0..15 of token 0
    z = lambda t: bits(t)[0, 0, :16].tolist()
    assert set(z(x0)) == set(z(noise)) == set(z(lats[0])) == {0, -32768}
    assert len({(c & 2 > 0, z(lats[0])[c], z(x0)[c], z(noise)[c]) for c in range(16)}) == 16
    assert -32768 in z(outs[0]) and 0 in z(outs[0])
    # the ties: at n = 3 (begin 2) step 1 holds byte 86 and not 85; at n = 5 step 1 holds 52 and not 51
    k1 = R.hold_mask(hold, cut[1]) if n > 1 else None
    if n == 3:
        assert k1[0, 1, :4].tolist() == [0, 1, 0, 1] and hold[0, 1].tolist() == [85, 86, 84, 170]
    if n == 5:
        assert k1[0, 2, :4].tolist() == [1, 1, 0, 1] and hold[0, 2].tolist() == [171, 169, 51, 52]
    # last="keep": the held pixels end as x0's own bits, the others keep the model's
    keep_out = R.run_blends(lats, x0, noise, hold, sig, begin, "keep")
    for i in range(n - 1):
        assert torch.equal(bits(keep_out[i]), bits(outs[i]))
    k = R.hold_mask(hold, R.cut_table(n, "keep")[-1]).bool()
    nz = (x0.float() != 0) & (lats[-1].float() != 0)
    assert torch.equal(bits(keep_out[-1])[k & nz], bits(x0)[k & nz]) and torch.equal(bits(keep_out[-1])[~k & nz], bits(lats[-1])[~k & nz])
    assert k.any() and (~k).any()


@pytest.mark.parametrize("begin", [0, 2])
def test_a_binary_map_is_the_known_region_blend(gold, begin):
    """With a map of 0 / 255 the restated loop (last="keep") equals the keep_known restatement with mask = map >= 128.  No exception
    for signed zeros arises: hold is 255 or 0 and every cut entry lies in [0, 254] here, so k = 1 - mask exactly; both formulas then
    form the same two products, p (1 - m) and x m, and IEEE addition commutes (a -0 meeting a +0 gives +0 in either order).  The two
    differ only where cut reaches 255 (last="free", or n >= 300), where change-map sampling does not write at all."""
    x0, noise, sig = gold["x0"], gold["noise"], gold["sigmas"]
    n = N - begin
    g = torch.Generator().manual_seed(11)
    free = torch.rand(2, 6, 4, generator=g) < 0.5                                      # per latent pixel: free to change
    hold = torch.where(free, 0, 255).to(torch.uint8)
    mask = free.to(BF).repeat(1, 1, 16)                                                # keep_known's mask: 1 = the model's
    lats = [gold[f"b{begin}_s{i}_latents"] for i in range(n)]
    got = R.run_blends(lats, x0, noise, hold, sig, begin, "keep")
    tab = K.keep_sigma(sig, begin)
    assert int(R.cut_table(n, "keep").max()) < 255
    for i in range(n):
        assert torch.equal(bits(got[i]), bits(K.blend(lats[i], x0, noise, mask, tab[i]))), i
    last_free = R.run_blends(lats, x0, noise, hold, sig, begin, "free")[-1]
    assert not torch.equal(bits(last_free), bits(got[-1])) and torch.equal(bits(last_free), bits(lats[-1]))


def test_cover_restatement_properties():
    g = torch.Generator().manual_seed(5)
    H, W = 64, 96
    m = torch.randint(0, 256, (2, H, W), generator=g).to(torch.uint8)
    near, prev = R.pack(m, 0, 0), R.pack(m, 1, 0)
    assert prev.shape == (2, 24, 4) and (prev <= near).all() and (prev < near).any()
    for grow in (1, 2, 8):
        cur = R.pack(m, 1, grow)
        assert (cur <= prev).all()
        prev = cur
    assert (prev == 255 - m.amax(dim=(1, 2))[:, None, None]).all()                     # grow 8 on an 8 x 12 latent grid sees everything
    one = torch.zeros(1, H, W, dtype=torch.uint8)
    one[0, 8 * 4 + 3, 8 * 5 + 6] = 77                                                  # latent pixel (4, 5), off the lattice
    assert int((R.pack(one, 0, 0) != 255).sum()) == 0
    for grow in (0, 1, 2):
        got = R.pack(one, 1, grow)
        assert int((got == 255 - 77).sum()) == (2 * grow + 1) ** 2 and int((got == 255).sum()) == got.numel() - (2 * grow + 1) ** 2
    corner = torch.zeros(1, H, W, dtype=torch.uint8)
    corner[0, H - 1, W - 1] = 255
    assert int((R.pack(corner, 1, 1) == 0).sum()) == 4 and int((R.pack(corner, 0, 0) == 0).sum()) == 0


# ---------------------------------------------------------------------------------------------- ABI and host checks
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


NEW = ("tfx_change_map_blend", "tfx_change_map_pack", "tfx_dit_step_run_ex2", "tfx_dit_step_capture_ex2")


def test_symbols_are_declared_bound_exported_and_the_abi_stamp_stays(lib, tmp_path):
    from textflux_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    for sym in NEW:
        assert sym + "(" in hdr and sym in L.SIGNATURES and hasattr(lib, sym)
    assert len(L.SIGNATURES["tfx_change_map_blend"][1]) == 14 and len(L.SIGNATURES["tfx_change_map_pack"][1]) == 8
    assert L.ABI_VERSION == L.header_abi_version() == 11
    assert [f for f, _ in L.StepExtra._fields_] == ["v_prev", "keep_x0", "keep_noise", "keep_mask", "keep_sigma"]   # as it was
    L._check_abi(lib)
    fields = [f for f, _ in L.StepChange._fields_]
    assert fields == ["hold", "cut"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "textflux_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(tfx_step_change));']
    lines += [f'printf("{f} %zu\\n", offsetof(tfx_step_change, {f}));' for f in fields] + ["return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.StepChange)
    for f in fields:
        assert int(got[f]) == getattr(L.StepChange, f).offset, f


def test_change_map_blend_checks_its_arguments_before_it_launches(lib):
    a = [k << 20 for k in range(1, 9)]                                # never dereferenced: every call is refused, or launches nothing
    call = lambda x=a[0], ldx=64, x0=a[1], noise=a[2], hold=a[3], cut=a[6], Cc=64, rows=4, sig=a[4], xin=None, ldxin=0: \
        lib.tfx_change_map_blend(x, ldx, x0, noise, hold, cut, Cc, rows, sig, None, 0, xin, ldxin, None)
    for kw, msg in ((dict(Cc=12), b"multiple of 8"), (dict(Cc=0), b"multiple of 8"), (dict(Cc=-8), b"multiple of 8"),
                    (dict(rows=-1), b"negative row count"),
                    (dict(ldx=56), b"ldx"), (dict(ldx=68), b"ldx"), (dict(xin=a[5], ldxin=56), b"ldxin"), (dict(xin=a[5], ldxin=68), b"ldxin"),
                    (dict(x=None), b"null pointer"), (dict(x0=None), b"null pointer"), (dict(noise=None), b"null pointer"),
                    (dict(hold=None), b"null pointer"), (dict(cut=None), b"null pointer"), (dict(sig=None), b"null pointer"),
                    (dict(x=a[0] + 8), b"16-byte aligned"), (dict(x0=a[1] + 2), b"16-byte aligned"), (dict(noise=a[2] + 4), b"16-byte aligned"),
                    (dict(xin=a[5] + 8, ldxin=64), b"16-byte aligned"),
                    (dict(hold=a[3] + 2), b"4-byte aligned"), (dict(hold=a[3] + 1), b"4-byte aligned"), (dict(cut=a[6] + 2), b"4-byte aligned"),
                    (dict(x0=a[0]), b"alias"), (dict(noise=a[0]), b"alias"), (dict(x0=a[0] + 64), b"alias"),
                    (dict(hold=a[0]), b"hold must not alias"), (dict(hold=a[0] + 4 * 64 * 2 - 4), b"hold must not alias"),
                    (dict(hold=a[0] - 12), b"hold must not alias"),                                         # its last word on x's first
                    (dict(xin=a[5], ldxin=384, hold=a[5] + 3 * 384 * 2 + 124), b"hold must not alias"),     # inside a pitched xin's last row
                    (dict(ldx=384, noise=a[0] + 3 * 384 * 2), b"alias")):
        assert call(**kw) != 0 and msg in lib.tfx_last_error(), kw
    assert call(rows=0) == 0 and call(rows=0, x=None, x0=None, noise=None, hold=None, cut=None, sig=None) == 0


def test_change_map_pack_checks_its_arguments_before_it_launches(lib):
    call = lambda m=1 << 20, o=2 << 20, B=1, H=32, W=48, mode=0, grow=0: lib.tfx_change_map_pack(m, o, B, H, W, mode, grow, None)
    for kw, msg in ((dict(H=24), b"multiples of 16"), (dict(W=40), b"multiples of 16"), (dict(B=-1), b"B >= 0"),
                    (dict(mode=2), b"mode must be"), (dict(mode=-1), b"mode must be"), (dict(mode=0, grow=1), b"grow must be 0"),
                    (dict(mode=1, grow=9), b"outside 0..8"), (dict(mode=1, grow=-1), b"outside 0..8"),
                    (dict(m=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(m=(1 << 20) + 4), b"aligned"),
                    (dict(o=(2 << 20) + 2), b"aligned")):
        assert call(**kw) != 0 and msg in lib.tfx_last_error(), kw
    assert call(B=0) == 0 and call(H=0, m=None, o=None) == 0


def test_ops_wrappers_check_before_they_launch():
    from textflux_amd import ops
    x = torch.zeros(4, 8, dtype=BF)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.change_map_blend(x, x.clone(), x.clone(), torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), torch.zeros(3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.change_map_pack(torch.zeros(1, 16, 16, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------- the step's launch plan
@pytest.fixture(scope="module")
def scenarios(tmp_path_factory):
    """{scenario: its lines}: csrc's host code against the recording launch layer, driven by helpers/change_map_trace_driver.cpp"""
    with tempfile.TemporaryDirectory(dir=str(tmp_path_factory.mktemp("change_map_trace"))) as tmp:
        exe = os.path.join(tmp, "change_map_trace")
        srcs = sorted(p for p in glob.glob(os.path.join(CSRC, "*.cpp")) if os.path.basename(p) != "launch.cpp")
        srcs += [os.path.join(HELPERS, f) for f in ("launch_recorder.cpp", "step_cache_recorder.cpp", "change_map_recorder.cpp",
                                                    "change_map_trace_driver.cpp")]
        cmd = [CXX, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I",
               os.path.join(REPO, "include"), *srcs, "-Wl,--unresolved-symbols=ignore-all", "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"trace binary ended with {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
    out, cur = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        else:
            cur.append(line)
    return out


def launches(lines):
    assert lines[-2:] == ["rc 0", "error "], lines[-2:]
    return lines[:-2]


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
@pytest.mark.parametrize("sampler", [0, 1, 2, 3], ids=["euler", "amo", "fused", "multistep"])
def test_a_change_map_step_issues_a_keep_known_step_with_the_blend_replaced(scenarios, sampler):
    for phase in (0, 1, 2, 3):
        plain, keep, change = (launches(scenarios[f"{m}_sampler{sampler}_phase{phase}"]) for m in ("plain", "keep", "change"))
        if phase == 1:                                                                 # the head never reaches the sampler update
            assert plain == keep == change and not any("blend" in l for l in plain)
            continue
        assert len(keep) == len(change) == len(plain) + 1
        at = [i for i, l in enumerate(keep) if l.startswith("known_region_blend ")]
        assert len(at) == 1 and not any("blend" in l for l in plain)
        i = at[0]
        assert keep[:i] == change[:i] == plain[:i] and keep[i + 1:] == change[i + 1:] == plain[i:]          # nothing else moved
        assert change[i].startswith("change_map_blend ") and sum("blend" in l for l in change) == 1
        kf, cf = (dict(f.split("=") for f in l.split()[1:]) for l in (keep[i], change[i]))
        assert kf.pop("mask") == "keep_mask" and (cf.pop("hold"), cf.pop("cut")) == ("hold", "cut") and kf == cf
        assert cf["step_ptr"] == "step_ptr" and cf["sigma"] == "keep_sigma"
        assert (cf["x"], cf["ldx"], cf["xin"]) == (("xin", "64", "0") if sampler == 2 else ("latents", "16", "xin"))
        # behind the sampler update, in front of the step cache's store pass and the cursor advance
        rest = [l.split()[0] for l in change[i + 1:]]
        assert rest == (["step_cache_store", "advance_step"] if phase == 2 else ["advance_step"])
        before = change[i - 1].split()[0]
        assert before == {0: "sched_step", 1: "sched_step", 3: "multistep_step"}.get(sampler, before) and (sampler != 2 or "gemm" in before)


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
def test_ex2_refusals_and_the_null_change(scenarios):
    assert launches(scenarios["ex2_null_change"]) == launches(scenarios["keep_sampler0_phase0"])
    want = dict(fail_keep_mask_set="keep_mask must be NULL", fail_no_x0="keep_x0, keep_noise and keep_sigma must be set",
                fail_no_noise="keep_x0, keep_noise and keep_sigma must be set", fail_no_sigma="keep_x0, keep_noise and keep_sigma must be set",
                fail_no_hold="hold and change->cut must both be set", fail_no_cut="hold and change->cut must both be set",
                fail_seq_len="dit.seq_len", fail_hold_in_xin="must not alias", fail_hold_in_latents="must not alias",
                fail_cut_in_out="must not alias", fail_x0_in_v_prev="must not alias")
    for name, text in want.items():
        lines = scenarios[name]
        assert lines[0] == "rc 1" and text in lines[1] and len(lines) == 2, name       # refused before anything is launched
    assert len([k for k in scenarios if k.startswith("fail_")]) == len(want)


@pytest.mark.skipif(not CXX, reason="no C++ compiler")
@pytest.mark.skipif(not HAVE_HIP_HEADERS, reason="no ROCm headers")
@pytest.mark.parametrize("sampler", [0, 1, 2, 3], ids=["euler", "amo", "fused", "multistep"])
def test_every_entry_point_issues_the_same_step(scenarios, sampler):
    """tfx_dit_step_run(s), tfx_dit_step_run_ex(s, {}) and tfx_dit_step_run_ex2(s, {}, NULL) are one step, and so are
    tfx_dit_step_run_multistep(s, v) and the two with v_prev = v: the step loop drives every sampler through _ex2 alone"""
    first = "multistep" if sampler == 3 else "run"
    for phase in (0, 1, 2, 3):
        one, ex, ex2 = (launches(scenarios[f"entry_{e}_sampler{sampler}_phase{phase}"]) for e in (first, "ex", "ex2"))
        assert one == ex == ex2 and len(one) >= 3 and not any("blend" in l for l in one)
        assert one == launches(scenarios[f"plain_sampler{sampler}_phase{phase}"])
        update = [l.split()[0] for l in one if l.split()[0] in ("sched_step", "multistep_step")]
        assert update == ([] if phase == 1 or sampler == 2 else ["multistep_step" if sampler == 3 else "sched_step"])


def test_ex2_entry_points_refuse_without_a_device(lib):
    from tests.test_keep_known_cpu import step_desc
    from textflux_amd import _lib as L
    hold, out = [], C.c_void_p()
    base = 1 << 31
    ex = lambda **kw: L.StepExtra(**dict(dict(keep_x0=base, keep_noise=base + (1 << 20), keep_sigma=base + (3 << 20)), **kw))
    ch = lambda **kw: L.StepChange(**dict(dict(hold=base + (4 << 20), cut=base + (5 << 20)), **kw))
    ref = lambda o: C.byref(o) if o is not None else None
    run = lambda sd, e, c: lib.tfx_dit_step_run_ex2(C.byref(sd), ref(e), ref(c), None)
    cap = lambda sd, e, c: lib.tfx_dit_step_capture_ex2(C.byref(sd), ref(e), ref(c), None, C.byref(out))
    for fn in (run, cap):
        assert fn(step_desc(L, hold), None, ch()) != 0 and b"null tfx_step_extra" in lib.tfx_last_error()
        assert fn(step_desc(L, hold), None, None) != 0 and b"null tfx_step_extra" in lib.tfx_last_error()
        assert fn(step_desc(L, hold), ex(keep_mask=base + (2 << 20)), ch()) != 0 and b"keep_mask must be NULL" in lib.tfx_last_error()
        for missing in ("keep_x0", "keep_noise", "keep_sigma"):
            assert fn(step_desc(L, hold), ex(**{missing: None}), ch()) != 0 and b"must be set" in lib.tfx_last_error(), missing
        for missing in ("hold", "cut"):
            assert fn(step_desc(L, hold), ex(), ch(**{missing: None})) != 0 and b"must both be set" in lib.tfx_last_error(), missing
        for sampler in (0, 2):
            sd = step_desc(L, hold, sampler)
            sd.dit.seq_len = 1 << 22
            assert fn(sd, ex(), ch()) != 0 and b"dit.seq_len" in lib.tfx_last_error()
        sd = step_desc(L, hold)
        for target in (sd.latents, sd.dit.out, sd.dit.xin, sd.latents + 64, sd.dit.xin + 2 * 48 * 384 * 2 - 4):
            for field in ("hold", "cut"):
                assert fn(sd, ex(), ch(**{field: target})) != 0 and b"must not alias" in lib.tfx_last_error(), (field, target)
            assert fn(sd, ex(keep_x0=target), ch()) != 0 and b"must not alias" in lib.tfx_last_error()
        assert fn(sd, ex(v_prev=base + (4 << 20) + 8), ch()) != 0 and b"must not alias" in lib.tfx_last_error()      # hold inside v_prev
        sd = step_desc(L, hold, 2)
        assert fn(sd, ex(v_prev=base + (6 << 20)), ch()) != 0 and b"sampler must be 0" in lib.tfx_last_error()
    sd = step_desc(L, hold)
    assert lib.tfx_dit_step_capture_ex2(C.byref(sd), C.byref(ex()), C.byref(ch()), None, None) != 0 and b"null output handle" in lib.tfx_last_error()
    assert cap(sd, ex(), ch()) != 0 and b"NULL stream" in lib.tfx_last_error()          # a valid set gets as far as the capture
    assert cap(sd, L.StepExtra(), None) != 0 and b"NULL stream" in lib.tfx_last_error()  # no change: the _ex step


# ---------------------------------------------------------------------------------------------- the step loop's control flow
@pytest.mark.parametrize("cache", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_run_steps_issues_the_same_sequence_and_keys_its_graphs(graph, cache):
    from tests.test_keep_known_cpu import Bar, Recorder
    from textflux_amd.step_cache import Decider, StepCacheConfig
    from textflux_amd.step_loop import run_steps
    seen = {}
    for key in ((False, True), (False, True, "keep"), (False, True, "change")):
        rec, graphs = Recorder(), {}
        pipe = SimpleNamespace(_interrupt=False, scheduler=SimpleNamespace(_step_index=2))
        decider = Decider(StepCacheConfig.make(0.0, {2}, None)) if cache else None
        run_steps(rec, 4, pipe, Bar(), graphs, key, decider, use_graph=graph)
        seen[key] = (rec.ops, sorted(graphs, key=str))
    plain, keep, change = seen[(False, True)], seen[(False, True, "keep")], seen[(False, True, "change")]
    assert plain[0] == keep[0] == change[0] and len(plain[0]) >= 8
    assert all("change" in k for k in change[1]) and not any("change" in k for k in plain[1] + keep[1])
    assert len(change[1]) == (0 if not graph else 3 if cache else 1)                    # one graph per phase whatever the number of steps


def test_denoise_carries_the_change_dict_next_to_keep():
    src = open(os.path.join(REPO, "textflux_amd", "step_loop.py")).read()
    assert 'key += ("change",)' in src and "tfx_dit_step_run_ex2" in src and "tfx_dit_step_capture_ex2" in src
    from textflux_amd import step_loop
    import inspect
    assert list(inspect.signature(step_loop.denoise).parameters)[-2:] == ["keep", "change"]


# ---------------------------------------------------------------------------------------------- callers
def test_change_map_argument_forms():
    from textflux_amd.pipeline import _change_map_cfg
    from textflux_amd.paste_back import DILATE, FEATHER
    assert _change_map_cfg(None) is None and _change_map_cfg(False) is None
    base = dict(map=None, dilate=DILATE, feather=FEATHER, mode="nearest", grow=0, last="keep")
    assert _change_map_cfg(True) == _change_map_cfg({}) == base
    assert _change_map_cfg(dict(dilate=3, feather=2, mode="cover", grow=3, last="free")) == dict(map=None, dilate=3, feather=2, mode="cover",
                                                                                                  grow=3, last="free")
    arr = np.zeros((32, 48), np.uint8)
    assert _change_map_cfg(arr)["map"] is arr and _change_map_cfg(dict(map=arr, last="free"))["map"] is arr
    t = torch.zeros(1, 32, 48, dtype=torch.uint8)
    assert _change_map_cfg(t)["map"] is t
    for bad, match in ((dict(radius=2), r"unknown keys \['radius'\]"), (dict(mode="nearest", grow=1), "grow"), (dict(mode="cover", grow=9), "grow"),
                       (dict(mode="bilinear"), "mode"), (dict(last="loose"), "last"), (dict(dilate=-1), "dilate"),
                       (dict(map=arr, dilate=3), "explicit map"), (dict(map=arr, feather=3), "explicit map")):
        with pytest.raises(ValueError, match="change_map.*" + match):
            _change_map_cfg(bad)


def test_change_map_excludes_keep_known_and_mixed_batches():
    from tests.test_batch_driver_cpu import StubPipe, _items, _loader
    from textflux_amd.batch_driver import run_items
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.schedulers import FlowMatchEulerDiscreteScheduler
    pipe = FluxFillPipeline.__new__(FluxFillPipeline)                 # refused on the first lines, before any component is used
    for kk in (True, dict(mode="cover", grow=1)):
        with pytest.raises(ValueError, match="change_map and keep_known exclude each other"):
            pipe(prompt="x", change_map=True, keep_known=kk)
        with pytest.raises(ValueError, match="change_map and keep_known exclude each other"):
            run_items(_items()[:2], StubPipe(0), None, device="cpu", loader=_loader, change_map=dict(dilate=2), keep_known=kk)
    with pytest.raises(ValueError, match="change_map: unknown keys"):
        pipe(prompt="x", change_map=dict(radius=1))
    sched = dict(use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift=3.0)
    for cm in (True, dict(dilate=2, feather=1), np.zeros((256, 256), np.uint8)):
        with pytest.raises(NotImplementedError, match="change_map"):
            run_items(_items()[:2], StubPipe(0), None, mixed_pad=0.1, device="cpu", loader=_loader, change_map=cm)
        real = FluxFillPipeline.__new__(FluxFillPipeline)
        real.scheduler, real.transformer, real._step_cache, real.fuse_euler_step = FlowMatchEulerDiscreteScheduler(**sched), None, None, True
        with pytest.raises(NotImplementedError, match="call_mixed: change_map"):
            real.call_mixed(sizes=[(256, 256)], latents=[torch.zeros(1, 256, 64)], masked_image_latents=[torch.zeros(1, 256, 320)],
                            prompt_embeds=torch.zeros(1, 64, 64), pooled_prompt_embeds=torch.zeros(1, 128), output_type="latent", change_map=cm)


def test_run_items_hands_change_map_to_every_call_and_only_when_given():
    from tests.test_batch_driver_cpu import StubPipe, _items, _loader
    from textflux_amd import batch_driver as bd

    class Seen(StubPipe):
        def __call__(self, *a, change_map="absent", **k):
            self.seen = getattr(self, "seen", []) + [change_map]
            return super().__call__(*a, **k)

    items = _items()[:3]
    run = lambda pipe, **kw: bd.run_items(items, pipe, None, batch_size=2, device="cpu", loader=_loader, save=lambda i, im: None, **kw)
    pipe = Seen(0)
    cm = dict(dilate=5, feather=2, mode="cover", grow=1, last="free")
    res = run(pipe, change_map=cm)
    assert sorted(res["done"]) == [0, 1, 2] and pipe.seen == [cm, cm]
    pipe = Seen(0)
    run(pipe)
    assert pipe.seen == ["absent", "absent"]
    assert sorted(run(StubPipe(0), change_map=None)["done"]) == [0, 1, 2]              # a pipeline that does not know the argument still runs


def test_clis_carry_the_flags(monkeypatch):
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    flags = ["--change_map", "--change_dilate", "6", "--change_feather", "3", "--change_mode", "cover", "--change_grow", "2", "--change_last", "free"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single), (re_.build_parser(), ["--json_path", "j"]),
                         (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.change_map, a.change_dilate, a.change_feather, a.change_mode, a.change_grow, a.change_last) == (False, None, None, "nearest", 0, "keep")
        a = parser.parse_args(base + flags)
        assert (a.change_map, a.change_dilate, a.change_feather, a.change_mode, a.change_grow, a.change_last) == (True, 6, 3, "cover", 2, "free")
    full = dict(dilate=6, feather=3, mode="cover", grow=2, last="free")
    parse = lambda extra: ri.known_region_from_args(ri.build_parser().parse_args(single + extra))
    assert parse([]) is None and parse(flags) == dict(change_map=full)
    assert parse(["--change_map"]) == dict(change_map=dict(mode="nearest", grow=0, last="keep"))      # dilate / feather: the pipeline's defaults
    assert parse(["--change_map", "--strength", "0.6"]) == dict(change_map=dict(mode="nearest", grow=0, last="keep"), strength=0.6)
    for bad in (["--change_dilate", "3"], ["--change_last", "free"], ["--change_map", "--keep_known"], ["--change_map", "--change_grow", "1"],
                ["--change_map", "--change_mode", "cover", "--change_grow", "9"], ["--change_map", "--change_feather", "-1"]):
        with pytest.raises(SystemExit):
            parse(bad)
    # main -> process_normal_mode -> run_inference -> the pipeline call
    seen = []
    monkeypatch.setattr(ri, "process_normal_mode", lambda *a, **k: seen.append(k.get("known", "absent")))
    monkeypatch.setattr(ri, "report_step_cache", lambda pipe: None)
    monkeypatch.setattr(rl, "load_flux_pipeline", lambda *a, **k: SimpleNamespace())
    for mod in (ri, rl):
        mod.main(single)
        mod.main(single + flags)
    assert seen == ["absent", dict(change_map=full), "absent", dict(change_map=full)]
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
    ri.run_inference(img, img, ["AB"], num_steps=2, pipe=Pipe(), known=dict(change_map=full))
    assert "change_map" not in calls[0] and calls[1]["change_map"] == full
    # the eval scripts: the flags become run_items' change_map; refused with --mixed_pad / --keep_known before anything is loaded
    src = open(os.path.join(REPO, "scripts", "run_eval.py")).read()
    assert 'known["change_map"] = dict(mode=a.change_mode' in src and "paste_back=paste_back, **known," in src
    for lora, w in ((False, "--weights_path"), (True, "--lora_weights_path")):
        common = ["--json_path", "j", "--original_images_dir", "o", w, "w", "--scheduler", ""]
        with pytest.raises(SystemExit, match="--change_map does not serve mixed-geometry"):
            re_.main(common + ["--mixed_pad", "0.1", "--change_map"], lora=lora)
        with pytest.raises(SystemExit, match="exclude each other"):
            re_.main(common + ["--change_map", "--keep_known"], lora=lora)
        with pytest.raises(SystemExit, match="need --change_map"):
            re_.main(common + ["--change_feather", "2"], lora=lora)


def test_the_derived_map_of_a_per_line_paste_back_item_comes_from_each_lines_own_mask():
    """The derived form is computed inside the pipeline call from that call's mask_image, so per_line + paste_back need no further
    work: every line's call is handed the dict (no explicit map) next to that line's own mask, and the alpha of that mask -- the map
    the call then makes, restated on the CPU -- covers that line only."""
    from tests.helpers import paste_back_ref as ref
    from tests.test_per_line_cpu import PasteStub, _run
    # two lines of different sizes, so that their masks differ on the canvases too
    two = [dict(image=("scene", 900, 700, None), mask=("mask", 900, 700, [(300, 200, 400, 230), (320, 320, 380, 340)]), text="UPPER\nLOWER")]

    class Seen(PasteStub):
        def __call__(self, height, width, image, mask_image, change_map="absent", **kw):
            self.maps = getattr(self, "maps", []) + [(change_map, [np.array(m.convert("L")) for m in mask_image])]
            return super().__call__(height, width, image, mask_image, **kw)

    cm = dict(dilate=3, feather=2)
    pipe = Seen()
    res, _ = _run(pipe, two, paste_back=dict(per_line=True), change_map=cm)
    assert res["all_done"] == [0] and not res["failed"] and len(pipe.pastes) == 2
    assert all(got == cm and "map" not in got for got, _ in pipe.maps)                 # every call: the dict, no explicit map
    masks = [m for _, ms in pipe.maps for m in ms]
    assert len(masks) == 2 and masks[0].shape == masks[1].shape
    alphas = [ref.alpha_mask(m, 3, 2) for m in masks]
    assert not np.array_equal(masks[0], masks[1])
    for m, a in zip(masks, alphas):
        assert a.shape == m.shape and (a[m >= 128] > 0).all() and a.max() == 255 and 0 < int((a > 0).sum()) < a.size // 4
        assert len(np.unique(a)) > 2                                                   # a graded halo, not a binary map
    # without the keyword the calls stay as they were
    plain = Seen()
    _run(plain, two, paste_back=dict(per_line=True))
    assert plain.maps[0][0] == "absent"
