"""Seamless paste without a GPU (DESIGN.md section 4 "Seamless paste"): the properties of the arithmetic on its numpy restatement
(tests/helpers/seamless_ref.py), and the package's plumbing: the configuration, what the per-line composer and the batch driver hand to
a pipeline, the CLIs' flags, and the C entry points' declarations and refusals (none of which touches a device)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from tests.helpers import seamless_ref as sref
from textflux_amd import batch_driver as bd
from textflux_amd import paste_back as pb
from textflux_amd import per_line as pl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 17), (2, 3), (37, 53), (5, 130))
SMOOTHS = (0, 1, 2, 5)


def _masks(rng, h, w):
    """known, free bool [h, w]: a free blob in the middle, a band of `neither` pixels, the rest known (tiny shapes: random)."""
    if h * w < 64:
        free = rng.random((h, w)) < 0.4
        known = ~free & (rng.random((h, w)) < 0.7)
        return known, free
    y, x = np.mgrid[:h, :w]
    free = ((y - h / 2) / (h / 3)) ** 2 + ((x - w / 2) / (w / 3)) ** 2 < 1
    neither = ~free & (x < w // 8)
    return ~free & ~neither, free


# ---------------------------------------------------------------------------------------------- the arithmetic, on the restatement
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("smooth", SMOOTHS)
def test_a_constant_difference_is_reproduced_exactly(hw, smooth):
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    known, free = _masks(rng, *hw)
    if not known.any():
        known[0, 0], free[0, 0] = True, False
    for k in (-255, -7, 0, 1, 255):
        d = np.where(known[..., None], k, rng.integers(-255, 256, hw + (3,)))        # off the known set d is never read
        assert (sref.membrane(d, known, free, smooth) == 64 * k).all()


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("smooth", SMOOTHS)
def test_min_max_principle_and_known_pixels_keep_their_values(hw, smooth):
    rng = np.random.default_rng(hw[0] * 77 + hw[1] + smooth)
    known, free = _masks(rng, *hw)
    d = rng.integers(-255, 256, hw + (3,))
    v = sref.membrane(d, known, free, smooth)
    assert v.shape == hw + (3,)
    assert (v[known] == 64 * d[known]).all()
    if known.any():
        for c in range(3):
            lo, hi = 64 * d[..., c][known].min(), 64 * d[..., c][known].max()
            assert lo <= v[..., c].min() and v[..., c].max() <= hi
    else:
        assert (v == 0).all()


@pytest.mark.parametrize("hw", SHAPES)
def test_nothing_known_gives_zero_and_todays_overlay(hw):
    rng = np.random.default_rng(5)
    none = np.zeros(hw, bool)
    assert (sref.membrane(rng.integers(-255, 256, hw + (2,)), none, ~none, 3) == 0).all()
    o, r, e = (rng.integers(0, 256, (1,) + hw + (3,), dtype=np.uint8) for _ in range(3))
    a = rng.integers(1, 256, (1,) + hw, dtype=np.uint8)                                # alpha > 0 everywhere: no known pixel
    assert np.array_equal(sref.seamless_overlay(o, r, e, a), ref.overlay(o, e, a))
    a0 = rng.integers(0, 256, (1,) + hw, dtype=np.uint8)                               # or nothing covered
    assert np.array_equal(sref.seamless_overlay(o, r, e, a0, covered=np.zeros_like(a0)), ref.overlay(o, e, a0))


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("smooth", SMOOTHS)
def test_max_shift_zero_is_the_overlay_and_alpha_zero_the_original(hw, smooth):
    rng = np.random.default_rng(hw[1] + smooth)
    o, r, e = (rng.integers(0, 256, (2,) + hw + (3,), dtype=np.uint8) for _ in range(3))
    known, free = _masks(rng, *hw)
    a = np.where(free, rng.integers(1, 256, hw), 0).astype(np.uint8)[None].repeat(2, 0)
    lut = rng.integers(0, 256, (2, 3, 256), dtype=np.uint8)
    assert np.array_equal(sref.seamless_overlay(o, r, e, a, smooth=smooth, max_shift=0), ref.overlay(o, e, a))
    assert np.array_equal(sref.seamless_overlay(o, r, e, a, lut=lut, smooth=smooth, max_shift=0), plref.overlay_lut(o, e, a, lut))
    assert np.array_equal(sref.seamless_overlay(o, r, e, np.zeros_like(a), lut=lut, smooth=smooth), o)
    got = sref.seamless_overlay(o, r, e, a, lut=lut, smooth=smooth)
    assert np.array_equal(got[a == 0], o[a == 0])                                      # bytes outside alpha's support


def test_the_membrane_moves_the_edit_onto_the_scene():
    """edit = scene - 9 everywhere: the corrected edit is the scene, so the paste returns the scene, where a plain paste leaves -9."""
    rng = np.random.default_rng(3)
    hw = (37, 53)
    scene = rng.integers(40, 216, (1,) + hw + (3,), dtype=np.uint8)
    _, free = _masks(rng, *hw)
    a = np.where(free, 255, 0).astype(np.uint8)[None]
    edit = scene - 9
    assert np.array_equal(sref.seamless_overlay(scene, scene, edit, a), scene)
    assert np.array_equal(sref.seamless_overlay(scene, scene, edit, a, max_shift=4)[0][free], (scene - 5)[0][free])
    assert np.array_equal(ref.overlay(scene, edit, a)[0][free], edit[0][free])


@pytest.mark.parametrize("smooth", (0, 8))
def test_seam_residual_on_a_ramp_plus_noise_ellipse(smooth):
    """A 96 x 301 window, an elliptical support, d = a ramp plus N(0, 1.5) noise: on the support's pixels 4-adjacent to the known area
    the mean |d - correction| is at most half the mean |d| there (the step a plain paste leaves to the feather).  The floor is the
    noise of d itself, so the factor of two leaves room for the seed without letting a broken push pass."""
    h, w = 96, 301
    rng = np.random.default_rng(11)
    y, x = np.mgrid[:h, :w]
    free = ((y - h / 2) / (h * 0.4)) ** 2 + ((x - w / 2) / (w * 0.45)) ** 2 < 1
    known = ~free
    d = np.floor(np.linspace(-17, 17, w)[None, :] + rng.normal(0, 1.5, (h, w)) + 0.5).astype(np.int64)[..., None]
    v = sref.membrane(d, known, free, smooth)
    pk = np.pad(known, 1)
    edge = free & (pk[:-2, 1:-1] | pk[2:, 1:-1] | pk[1:-1, :-2] | pk[1:-1, 2:])
    assert edge.sum() > 400
    residual = np.abs(d[edge] - v[edge] / 64).mean()
    step = np.abs(d[edge]).mean()
    print(f"smooth {smooth}: residual {residual:.3f}, plain step {step:.3f}, ratio {residual / step:.3f}")
    assert 7 < step < 10 and residual <= 0.5 * step


# ---------------------------------------------------------------------------------------------- configuration
def test_cfgs_accept_validate_and_refuse():
    assert pb.seamless_cfg(True) == dict(smooth=8, max_shift=32) == dict(smooth=pb.SEAMLESS_SMOOTH, max_shift=pb.SEAMLESS_MAX_SHIFT)
    assert pb.seamless_cfg(dict(smooth=0)) == dict(smooth=0, max_shift=32)
    assert pb.seamless_cfg(dict(max_shift=255, smooth=None)) == dict(smooth=8, max_shift=255)
    for bad, match in ((dict(sweeps=3), r"unknown keys \['sweeps'\]"), (dict(smooth=-1), "smooth"), (dict(smooth=256), "smooth"),
                       (dict(max_shift=-1), "max_shift"), (dict(max_shift=256), "max_shift"), (7, "True or a dict")):
        with pytest.raises(ValueError, match="seamless: .*" + match):
            pb.seamless_cfg(bad)
        with pytest.raises(ValueError, match="paste_back: .*seamless"):
            bd._paste_back_cfg(dict(seamless=bad))
    assert bd._paste_back_cfg(dict(seamless=True)) == dict(dilate=16, feather=4, region=None, seamless=dict(smooth=8, max_shift=32))
    assert bd._paste_back_cfg(dict(per_line=True, seamless=dict(smooth=3), curve=True))["seamless"] == dict(smooth=3, max_shift=32)
    assert bd._paste_back_cfg(dict(seamless=None)) == bd._paste_back_cfg(dict(seamless=False)) == bd._paste_back_cfg({}) == \
        dict(dilate=16, feather=4, region=None)
    with pytest.raises(ValueError, match="unknown keys"):
        bd._paste_back_cfg(dict(seemless=True))


# ---------------------------------------------------------------------------------------------- what a pipeline is handed
class Recorder:
    """A pipeline stand-in whose paste returns the window unchanged and records its keyword arguments."""

    def __init__(self):
        self.pastes = []

    def paste_back(self, original, edited, mask, dilate=None, feather=None, **kw):
        self.pastes.append(kw)
        return np.array(original)


class Older:
    """A pipeline whose paste_back predates every optional key."""

    def __init__(self):
        self.n = 0

    def paste_back(self, original, edited, mask, dilate=None, feather=None):
        self.n += 1
        return np.array(original)


def _works():
    rng = np.random.default_rng(1)
    scene = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    mask = np.zeros((40, 60, 3), np.uint8)
    mask[10:14, 8:30] = 255
    mask[26:30, 20:50] = 255
    regs = (pb.Region(0, 0, 40, 24, 40, 24), pb.Region(10, 16, 60, 40, 50, 24))
    works = [bd.Work(0, None, None, "", {}, (r.tw, r.th), orig_scene=scene, orig_mask=mask, region=r, parent=0, line=k) for k, r in enumerate(regs)]
    crops = [np.zeros((r.th, r.tw, 3), np.uint8) for r in regs]
    return scene, works, crops


@pytest.mark.parametrize("seamless", (True, dict(smooth=2, max_shift=9)))
@pytest.mark.parametrize("color_match", (None, True))
def test_compose_lines_and_the_driver_pass_the_key_exactly_when_configured(seamless, color_match):
    scene, works, crops = _works()
    base = dict(per_line=True, dilate=2, feather=1)
    if color_match:
        base["color_match"] = color_match
    cfg0, cfg1 = bd._paste_back_cfg(base), bd._paste_back_cfg(dict(base, seamless=seamless))
    p0, p1 = Recorder(), Recorder()
    pl.compose_lines(p0, works, crops, cfg0)
    out = pl.compose_lines(p1, works, crops, cfg1)
    assert np.array_equal(np.array(out), scene) and len(p0.pastes) == len(p1.pastes) == 2
    for w, k0, k1 in zip(works, p0.pastes, p1.pastes):
        assert "seamless" not in k0 and ("color_ref" in k0) == bool(color_match)
        assert set(k1) == set(k0) | {"seamless", "color_ref"}
        r = w.region
        assert k1["seamless"] == pb.seamless_cfg(seamless) and np.array_equal(k1["color_ref"], scene[r.y0:r.y1, r.x0:r.x1])
        assert k1.get("color_match") == k0.get("color_match")
    # the single-region path of the driver
    q0, q1 = Recorder(), Recorder()
    bd._paste_into_original(q0, works[0], crops[0], cfg0)
    bd._paste_into_original(q1, works[0], crops[0], cfg1)
    assert "seamless" not in q0.pastes[0] and q1.pastes[0] == dict(q0.pastes[0], seamless=pb.seamless_cfg(seamless))
    # a pipeline that predates the key serves everything without it, and fails loudly (no silent plain paste) with it
    old = Older()
    if not color_match:
        pl.compose_lines(old, works, crops, cfg0)
        bd._paste_into_original(old, works[0], crops[0], cfg0)
        assert old.n == 3
    with pytest.raises(TypeError):
        pl.compose_lines(old, works, crops, cfg1)


def test_paste_refuses_before_it_launches_and_keeps_the_old_rule_without_the_key():
    from textflux_amd import ops
    from textflux_amd.pipeline import FluxFillPipeline
    import inspect
    assert inspect.signature(pb.paste).parameters["seamless"].default is None
    assert inspect.signature(FluxFillPipeline.paste_back).parameters["seamless"].default is None
    img, m = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="color_ref needs color_match"):
        pb.paste(img, img, m, color_ref=img)
    with pytest.raises(ValueError, match="seamless: unknown keys"):
        pb.paste(img, img, m, seamless=dict(sweeps=1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.seamless_overlay(img, img, img, m)                                         # no CPU fallback
    with pytest.raises(RuntimeError, match="ROCm device"):
        pb.paste(img, img, m, seamless=True, color_ref=img)                            # allowed now: it gets as far as the device check


def test_ops_wrapper_checks_before_it_launches(monkeypatch):
    from textflux_amd import ops
    monkeypatch.setattr(ops, "_chk_dev", lambda *a: None)
    img, m = torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8)
    lut = torch.zeros(2, 3, 256, dtype=torch.uint8)
    for bad in (dict(orig=img.float()), dict(ref=img[:1]), dict(edit=img[:, :2]), dict(alpha=m[:1]), dict(alpha=m.float()), dict(covered=m[:, :2]),
                dict(lut=lut[:1]), dict(lut=lut[:, :2]), dict(smooth=-1), dict(smooth=256), dict(max_shift=-1), dict(max_shift=256),
                dict(out=img[:1]), dict(orig=img.permute(0, 2, 1, 3)), dict(orig=torch.zeros(2, 4, 4, 5, dtype=torch.uint8))):
        kw = dict(dict(orig=img, ref=img, edit=img, alpha=m), **bad)
        with pytest.raises(ValueError, match="seamless_overlay"):
            ops.seamless_overlay(**kw)


# ---------------------------------------------------------------------------------------------- the CLIs
def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.paste_seamless, a.paste_seamless_smooth, a.paste_seamless_max_shift) == (False, None, None)
        a = parser.parse_args(base + ["--paste_back", "--paste_seamless", "--paste_seamless_smooth", "3", "--paste_seamless_max_shift", "20"])
        assert (a.paste_seamless, a.paste_seamless_smooth, a.paste_seamless_max_shift) == (True, 3, 20)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(["--paste_back"]) == dict(dilate=16, feather=4, region=None)          # without the new flags: the dict it was
    assert parse(["--paste_back", "--paste_seamless"]) == dict(dilate=16, feather=4, region=None, seamless=True)
    assert parse(["--paste_back", "--paste_seamless_smooth", "3"])["seamless"] == dict(smooth=3)
    assert parse(["--paste_back", "--paste_per_line", "--paste_curve", "--paste_seamless_max_shift", "20"])["seamless"] == dict(max_shift=20)
    assert bd._paste_back_cfg(parse(["--paste_back", "--paste_seamless_smooth", "3"]))["seamless"] == dict(smooth=3, max_shift=32)
    for flag in (["--paste_seamless"], ["--paste_seamless_smooth", "3"], ["--paste_seamless_max_shift", "20"]):
        with pytest.raises(SystemExit, match="needs --paste_back"):
            parse(flag)
        with pytest.raises(SystemExit, match="needs --paste_back"):
            re_.main(["--json_path", "j", "--original_images_dir", "o", "--weights_path", "w"] + flag)
        with pytest.raises(SystemExit, match="needs --paste_back"):
            re_.main(["--json_path", "j", "--original_images_dir", "o", "--lora_weights_path", "l"] + flag, lora=True)


# ---------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


def test_symbols_are_declared_bound_exported_and_the_abi_version_stays(lib):
    from textflux_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    for sym in ("tfx_seamless_workspace_bytes", "tfx_seamless_overlay_u8"):
        assert sym in L.SIGNATURES and hasattr(lib, sym)
    assert "int64_t tfx_seamless_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C);" in hdr
    assert "int tfx_seamless_overlay_u8(const void* orig, const void* ref, const void* edit, const void* alpha, const void* covered" in hdr
    assert len(L.SIGNATURES["tfx_seamless_overlay_u8"][1]) == 16 and L.SIGNATURES["tfx_seamless_workspace_bytes"][0] is L.c_int64
    assert L.ABI_VERSION == 11 == L.header_abi_version() and hdr.count("without a new") >= 6
    for phrase in ("(2 s + n) // (2 n)", "9 c[i, j] + 3 c[i, j2] + 3 c[i2, j] + c[i2, j2] + 8) >> 4", "(N + S + E + W + 2) >> 2", "(v + 32) >> 6"):
        assert phrase in hdr, phrase


def test_workspace_bytes_is_host_arithmetic(lib):
    f = lib.tfx_seamless_workspace_bytes
    for B, H, W, C in ((1, 1, 1, 1), (2, 37, 53, 3), (1, 256, 1024, 3), (3, 5, 130, 4), (1, 1536, 2048, 3)):
        n = f(B, H, W, C)
        level0 = B * H * W * (4 * C + 1)                                               # two i16 value buffers and the flags
        assert level0 <= n <= level0 + B * H * W * (2 * C + 1) + 16 * 3 * 34           # the coarser levels hold fewer pixels than level 0 (+ a few for odd sides), plus alignment
    assert f(1, 64, 64, 3) < f(2, 64, 64, 3) and f(1, 64, 64, 3) < f(1, 64, 65, 3) and f(1, 64, 64, 3) < f(1, 64, 64, 4)
    for bad, msg in (((0, 4, 4, 3), b"at least 1"), ((1, 0, 4, 3), b"at least 1"), ((1, 4, 4, 5), b"1..4 channels"), ((1, 4, 4, 0), b"1..4 channels"),
                     ((65536, 4, 4, 3), b"65535")):
        assert f(*bad) == -1 and msg in lib.tfx_last_error()


def test_entry_point_checks_its_arguments(lib):
    need = lib.tfx_seamless_workspace_bytes(2, 8, 8, 3)
    p = [k << 20 for k in range(1, 9)]               # orig, ref, edit, alpha, covered, lut, out, workspace: never dereferenced, every call is refused

    def call(ptrs=p, ws=need, dims=(2, 8, 8, 3), smooth=8, max_shift=32):
        return lib.tfx_seamless_overlay_u8(*ptrs[:8], ws, *dims, smooth, max_shift, None)
    for k in (0, 1, 2, 3, 6, 7):                                                       # covered and lut alone may be NULL
        assert call(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_seamless_overlay_u8: null pointer" in lib.tfx_last_error()
    assert call(ws=need - 1) != 0 and b"workspace" in lib.tfx_last_error() and str(need).encode() in lib.tfx_last_error()
    assert call(ws=0) != 0 and b"workspace" in lib.tfx_last_error()
    for c in (0, 5):
        assert call(dims=(2, 8, 8, c)) != 0 and b"1..4 channels" in lib.tfx_last_error()
    for k in range(3):
        dims = [2, 8, 8, 3]
        dims[k] = 0
        assert call(dims=tuple(dims)) != 0 and b"at least 1" in lib.tfx_last_error()
    assert call(dims=(65536, 8, 8, 3), ws=1 << 40) != 0 and b"65535" in lib.tfx_last_error()
    for s in (-1, 256):
        assert call(smooth=s) != 0 and b"smooth" in lib.tfx_last_error()
        assert call(max_shift=s) != 0 and b"max_shift" in lib.tfx_last_error()
    for k in (1, 2, 3, 4, 5, 7):                                                       # out may be orig, and nothing else
        ptrs = list(p)
        ptrs[6] = p[k]
        assert call(ptrs) != 0 and b"alias orig only" in lib.tfx_last_error()
    assert call(p[:7] + [p[7] + 8]) != 0 and b"16-byte aligned" in lib.tfx_last_error()
    assert b"seamless_overlay_u8" in lib.tfx_last_error()
