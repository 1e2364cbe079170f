"""Grain spectrum match without a GPU (DESIGN.md section 4 "Grain spectrum"): the model behind the estimator, the estimator on noise
synthesised by the numpy restatement (tests/helpers/grain_spectrum_ref.py), the closed loop, the package's host arithmetic against the
restatement's, and the plumbing: the configuration, the CLIs' flags, the wrappers' refusals and the C entry points' declarations and
refusals (none of which touches a device)."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import grain_ref as gref
from tests.helpers import grain_spectrum_ref as sref
from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from textflux_amd import batch_driver as bd
from textflux_amd import paste_back as pb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = 1.4826 / math.sqrt(164)                         # grey levels per histogram bin
SIDE, SIGMA = 256, 4.0
FULL = dict(ring=24, max_sigma=6.0, strength=1.0, min_pixels=256, seed=0)


# ---------------------------------------------------------------------------------------------- the model
def test_q_model_rises_strictly_from_one_and_has_the_stated_values():
    q = [pb.grain_q_model(s) for s in range(65)]
    assert all(b > a for a, b in zip(q, q[1:]))
    for s, want in ((0, 1.000), (16, 1.079), (32, 1.216), (64, 1.926)):
        assert abs(q[s] - want) < 1e-3 and abs(sref.q_model(s) - want) < 1e-3, (s, q[s])
    assert q[0] == 1.0 and max(abs(q[s] - sref.q_model(s)) for s in range(65)) < 1e-12


def test_white_grain_has_unit_levels_and_the_package_agrees_with_the_restatement():
    assert pb.grain_shape_levels(0, 0) == (1.0, 1.0) == sref.levels(0, 0)
    for s, lam in ((16, 0), (64, 128), (0, 256), (23, 101)):
        assert np.allclose(pb.grain_shape_levels(s, lam), sref.levels(s, lam), rtol=1e-13, atol=0)
    assert abs(sref.variance(0, 1) - 164) < 1e-9 and abs(sref.variance(0, 2) - 164) < 1e-9
    w, t = pb.grain_shape_levels(64, 128)             # the weakest grain: the largest gain a level of 64 can ask for stays below 2^18
    assert 64 / t / gref.SIGMA0 * 65536 < 2 ** 18 and w < t < 1


def test_the_restatements_channels_are_noise_fields():
    assert np.array_equal(sref.noise_channels(9, 13, [0, 1, 2], (2 ** 32 - 3, 5), 7), gref.noise_field(9, 13, 3, (2 ** 32 - 3, 5), 7))
    assert np.array_equal(sref.noise_channels(4, 5, [255], (1, 2), 3)[:, :, 0], gref.noise_field(4, 5, 256, (1, 2), 3)[:, :, 255])


# ---------------------------------------------------------------------------------------------- synthesis and the estimator
@pytest.fixture(scope="module")
def synthesised():
    """(s, lam) -> the step-1 and step-2 histograms of a flat 256 x 256 image with shaped grain of TRUE deviation 4 (origin (17, 5),
    seed 7, alpha 255), and its measured deviation: computed once."""
    flat, full = np.full((1, SIDE, SIDE, 3), 128, np.uint8), np.full((1, SIDE, SIDE), 255, np.uint8)
    out = {}
    for s, lam in ((0, 0), (16, 0), (32, 0), (64, 0), (0, 128), (0, 256), (32, 128)):
        gain = math.floor(SIGMA / sref.levels(s, lam)[1] / gref.SIGMA0 * 65536 + 0.5)
        img = sref.grain_shaped(flat, full, np.full((1, 3), gain), (s, lam), (17, 5), 7)
        out[(s, lam)] = (sref.highpass_hist_step(img, full, 255, 255, 1), sref.highpass_hist_step(img, full, 255, 255, 2),
                         (img.astype(np.float64) - 128).std(axis=(0, 1, 2)))
    return out


def test_shaped_grain_has_the_true_deviation_and_reads_as_its_white_equivalent(synthesised):
    """t and w of the model against the synthesis: the bytes' deviation is sigma (plus 1 / 12 of rounding variance) and the step-1
    estimator reads sigma w / t, within the estimator's own tolerance of test_grain_cpu.py (one bin and 3 %)."""
    for (s, lam), (h1, _, std) in synthesised.items():
        w, t = sref.levels(s, lam)
        read = pb.noise_sigma(h1[:, :3])
        print(f"(s, lam) = ({s}, {lam}): deviation {std}, step-1 level {read.ravel()} for {SIGMA * w / t:.3f}")
        assert (np.abs(std / math.sqrt(SIGMA ** 2 + 1 / 12) - 1) < 0.02).all()
        assert (np.abs(read - SIGMA * w / t) <= BIN + 0.03 * SIGMA).all()


@pytest.mark.parametrize("s,within", [(0, 1), (16, 4), (32, 2), (64, 5)])
def test_the_blur_is_recovered(synthesised, s, within):
    """Measured on these windows (256 x 256, sigma 4, lam 0): s = 0 / 16 / 32 / 64 come back as 0 / 13 / 31 / 60 (q = 1.000 / 1.061 /
    1.207 / 1.824 for the model's 1 / 1.079 / 1.216 / 1.926): the medians are whole bins, about 3 % of q each at this level, and the
    rounding to bytes adds white noise, which pulls the large-s end down.  The bounds are those distances plus one step."""
    h1, h2, _ = synthesised[(s, 0)]
    got = pb.grain_shape(h1, h2, True)
    print(f"s {s}: recovered (s, lam) = {got.ravel()}")
    assert np.array_equal(got, sref.grain_shape(h1, h2))                 # the package's host arithmetic is the restatement's
    assert abs(int(got[0, 0]) - s) <= within and got[0, 1] == 0
    capped = pb.grain_shape(h1, h2, dict(spectrum=dict(max_blur=8)))
    assert capped[0, 0] == min(int(got[0, 0]), 8) and np.array_equal(capped, sref.grain_shape(h1, h2, dict(spectrum=dict(max_blur=8))))


@pytest.mark.parametrize("lam,within", [(0, 1), (128, 3), (256, 1)])
def test_the_channel_share_is_recovered(synthesised, lam, within):
    """Measured on these windows (256 x 256, sigma 4, s 0): lam = 0 / 128 / 256 come back as 0 / 126 / 256.  The bounds are those
    distances plus one step."""
    h1, h2, _ = synthesised[(0, lam)]
    got = pb.grain_shape(h1, h2, True)
    print(f"lam {lam}: recovered (s, lam) = {got.ravel()}")
    assert np.array_equal(got, sref.grain_shape(h1, h2))
    assert abs(int(got[0, 1]) - lam) <= within and got[0, 0] == 0
    assert pb.grain_shape(h1, h2, dict(spectrum=dict(luma=False)))[0, 1] == 0
    assert pb.grain_shape(h1[:, [0, 3]], h2[:, [0, 3]], True)[0, 1] == 0  # one channel: nothing to share


def _hist_at(bins, n=4000):
    h = np.zeros((1, len(bins), 1024), np.int64)
    for c, b in enumerate(bins):
        h[0, c, b] = n
    return h


def test_grain_shape_thresholds_and_ties():
    white, soft = _hist_at((20, 20, 10, 30)), _hist_at((30, 30, 15, 45))
    assert np.array_equal(pb.grain_shape(white, white, True), [[0, 0]])                    # q = 1; rho = (30^2 - 900) / 1600 = 0: independent channels
    assert pb.grain_shape(white, soft, True)[0, 0] == int(np.argmin([abs(sref.q_model(s) - 30 / 20) for s in range(65)])) > 32
    assert pb.grain_shape(soft, white, True)[0, 0] == 0                                    # q < 1
    assert pb.grain_shape(_hist_at((0, 0, 0, 0)), soft, True).tolist() == [[0, 0]]          # M1 = 0, and a zero denominator
    few = _hist_at((20, 20, 10, 30), 255)
    assert pb.grain_shape(few, _hist_at((30, 30, 15, 45), 255), True)[0, 0] == 0            # fewer than min_pixels C counts
    assert pb.grain_shape(few, _hist_at((30, 30, 15, 45), 255), dict(min_pixels=255))[0, 0] > 32
    assert pb.grain_shape(_hist_at((20, 20, 10, 50)), white, True)[0, 1] == 256             # fully shared: M_S = sum M_c
    assert pb.grain_shape(_hist_at((20, 20, 10, 1023)), white, True)[0, 1] == 256           # rho is clamped
    assert pb.grain_shape(_hist_at((20, 20, 10, 10)), white, True)[0, 1] == 0
    for h1, h2 in ((white, soft), (_hist_at((30, 20, 25, 60)), _hist_at((33, 22, 30, 70)))):
        assert np.array_equal(pb.grain_shape(h1, h2, True), sref.grain_shape(h1, h2))
    both = pb.grain_shape(np.concatenate([white, soft]), np.concatenate([soft, white]), True)
    assert both.dtype == np.int32 and both.shape == (2, 2) and both[0, 0] > 32 and both[1, 0] == 0
    with pytest.raises(ValueError, match="grain_shape"):
        pb.grain_shape(white, soft[:, :3], True)


def test_gains_divide_by_the_white_equivalent_and_hold_the_true_deviation():
    hs, he = _hist_at((40, 40, 40, 70), 1000), _hist_at((10, 10, 10, 17), 1000)
    add = BIN * math.sqrt(1500)                                                            # 4.48 grey levels, as test_grain_cpu.py
    white = pb.grain_shaped_gains(hs, he, [[0, 0]], True)
    assert np.array_equal(white, pb.grain_gains(hs[:, :3], he[:, :3], True)) and white.dtype == np.int32
    for s, lam in ((16, 0), (0, 128), (32, 128), (64, 128)):
        w, t = sref.levels(s, lam)
        level = min(add / w, 6.0 / t)
        got = pb.grain_shaped_gains(hs, he, [[s, lam]], True)
        assert (got == math.floor(level / gref.SIGMA0 * 65536 + 0.5)).all() and np.array_equal(got, sref.grain_shaped_gains(hs, he, [[s, lam]]))
    assert 4.48 / sref.levels(64, 128)[0] > 6.0 / sref.levels(64, 128)[1] > 4.48 / sref.levels(16, 0)[0]                   # ... of which this one was held at max_sigma
    top = pb.grain_shaped_gains(_hist_at((1023,) * 4, 1000), _hist_at((0,) * 4, 1000), [[64, 128]], dict(max_sigma=64, strength=4))
    assert (top == math.floor(64 / sref.levels(64, 128)[1] / gref.SIGMA0 * 65536 + 0.5)).all() and (65536 < top).all() and (top <= 2 ** 18).all()
    assert (pb.grain_shaped_gains(he, hs, [[16, 64]], True) == 0).all()                    # nothing is denoised


# ---------------------------------------------------------------------------------------------- closure
@pytest.mark.parametrize("shape,sigma_e", [((32, 128), 0), ((16, 0), 2), ((0, 0), 0)])
def test_closure_the_interior_ends_at_the_scenes_step_1_level(shape, sigma_e):
    """test_grain_cpu.py's closure with a scene whose noise is shaped: after the match the step-1 level of the interior meets the
    scene's within the same tolerance, two bins and 3 %."""
    h, w = 96, 192
    full = np.full((1, h, w), 255, np.uint8)
    colour = lambda rgb: np.broadcast_to(np.array(rgb, np.uint8), (1, h, w, 3)).copy()
    gain = math.floor(SIGMA / sref.levels(*shape)[1] / gref.SIGMA0 * 65536 + 0.5)
    scene = sref.grain_shaped(colour((120, 128, 140)), full, np.full((1, 3), gain), shape, (31, 9), 3)
    edit = colour((124, 126, 133))
    if sigma_e:
        edit = gref.grain(edit, full, np.full((1, 3), math.floor(sigma_e / gref.SIGMA0 * 65536 + 0.5)), (31, 9), 11)
    alpha = np.zeros((1, h, w), np.uint8)
    alpha[0, h // 4: h - h // 4, w // 4: w - w // 4] = 255
    ring = plref.ring_mask(alpha, 12)
    pasted = ref.overlay(scene, edit, alpha)
    cfg = dict(seed=5, spectrum=True)
    out, gains, got = sref.match(pasted, scene, alpha, ring, cfg, (31, 9))
    level = lambda img, sel: pb.noise_sigma(sref.highpass_hist_step(img, sel)[:, :3])
    s_scene, s_before, s_after = level(scene, ring), level(pasted, alpha), level(out, alpha)
    print(f"shape {shape} -> {got.ravel()}, scene {s_scene.ravel()}, interior before {s_before.ravel()}, after {s_after.ravel()}, gains {gains.ravel()}")
    h1, h2 = sref.highpass_hist_step(scene, ring), sref.highpass_hist_step(scene, ring, 255, 255, 2)
    assert np.array_equal(got, pb.grain_shape(h1, h2, cfg)) and np.array_equal(gains, pb.grain_shaped_gains(h1, sref.highpass_hist_step(pasted, alpha), got, cfg))
    assert (gains > 0).all()
    assert (np.abs(s_after - s_scene) <= 2 * BIN + 0.03 * s_scene).all()
    assert (s_before < s_scene - 2 * BIN).all()                          # ... which it did not before
    assert np.array_equal(out[alpha == 0], scene[alpha == 0])
    flat = sref.match(pasted, scene, alpha, ring, dict(seed=5, spectrum=dict(max_blur=0, luma=False)), (31, 9))
    assert np.array_equal(flat[0], gref.match(pasted, scene, alpha, ring, dict(seed=5), (31, 9))[0]) and not flat[2].any()


# ---------------------------------------------------------------------------------------------- the restatement's exact properties
def test_restatement_properties():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (2, 9, 13), dtype=np.uint8)
    alpha[0, :3] = 0
    gains = np.array([[65536, 20000, 0], [1, 300, 65536]])
    assert np.array_equal(sref.grain_shaped(img, alpha, gains, (0, 0), (17, 5), 9), gref.grain(img, alpha, gains, (17, 5), 9))
    out = sref.grain_shaped(img, alpha, gains * 4, (23, 101), (17, 5), 9)
    assert np.array_equal(out[alpha == 0], img[alpha == 0]) and np.array_equal(out[0, :, :, 2], img[0, :, :, 2]) and not np.array_equal(out, img)
    whole = sref.grain_shaped(img[:1], alpha[:1], gains[:1], (64, 128), (100, 50), 2)
    part = sref.grain_shaped(img[:1, 2:7, 3:9], alpha[:1, 2:7, 3:9], gains[:1], (64, 128), (103, 52), 2)
    assert np.array_equal(whole[:, 2:7, 3:9], part)                      # the window's border included
    f = sref.shaped_field(6, 7, 3, 0, 256, (5, 5), 1)
    assert np.array_equal(f[:, :, 0], f[:, :, 1]) and np.array_equal(f[:, :, 0], 2 ** 24 * gref.noise_field(6, 7, 256, (5, 5), 1)[:, :, 255])
    h = sref.highpass_hist_step(img, alpha, 1, 255, 1)
    assert np.array_equal(h[:, :3], gref.highpass_hist(img, alpha, 1, 255)) and np.array_equal(h.sum(-1), np.broadcast_to((alpha >= 1).sum(axis=(1, 2))[:, None], (2, 4)))
    grey = np.repeat(img[:, :, :, :1], 3, axis=3)                        # equal channels: the sum's residual is three times each
    hg = sref.highpass_hist_step(grey, alpha, 0, 255, 2)
    r = np.repeat(np.arange(1024), hg[0, 0])
    assert np.array_equal(np.bincount(np.minimum(3 * r, 1023), minlength=1024), hg[0, 3])


# ---------------------------------------------------------------------------------------------- configuration and the CLIs
def test_cfg_carries_spectrum_only_when_given():
    assert pb.grain_cfg(True) == FULL and "spectrum" not in pb.grain_cfg(dict(seed=3)) and pb.grain_cfg(dict(spectrum=None)) == FULL
    assert pb.grain_cfg(dict(spectrum=False)) == FULL
    assert pb.grain_cfg(dict(spectrum=True)) == dict(FULL, spectrum=dict(max_blur=64, luma=True))
    assert pb.grain_cfg(dict(spectrum=True))["spectrum"] == dict(max_blur=64, luma=True)
    given = pb.grain_cfg(dict(seed=4, spectrum=dict(max_blur=0, luma=False)))
    assert given == dict(FULL, seed=4, spectrum=dict(max_blur=0, luma=False)) and pb.grain_cfg(given) == given
    assert pb.grain_cfg(dict(spectrum=dict(max_blur=None)))["spectrum"] == dict(max_blur=64, luma=True)
    for bad in (dict(max_blur=-1), dict(max_blur=65), dict(max_blur=1.5), dict(max_blur=True), dict(luma=1), dict(luma="yes"), dict(blur=3), 7, "on"):
        with pytest.raises(ValueError, match="grain: .*spectrum"):
            pb.grain_cfg(dict(spectrum=bad))
        with pytest.raises(ValueError, match="paste_back: grain: .*spectrum"):
            bd._paste_back_cfg(dict(grain=dict(spectrum=bad)))
    assert bd._paste_back_cfg(dict(grain=True)) == dict(dilate=16, feather=4, region=None, grain=FULL)
    assert bd._paste_back_cfg(dict(grain=dict(spectrum=True)))["grain"] == dict(FULL, spectrum=dict(max_blur=64, luma=True))


def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.paste_grain_spectrum, a.paste_grain_max_blur) == (False, None)
        a = parser.parse_args(base + ["--paste_back", "--paste_grain_spectrum", "--paste_grain_max_blur", "0"])
        assert (a.paste_grain_spectrum, a.paste_grain_max_blur) == (True, 0)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(["--paste_back", "--paste_grain"]) == dict(dilate=16, feather=4, region=None, grain=True)     # without the new flags: as it was
    assert parse(["--paste_back", "--paste_grain_spectrum"])["grain"] == dict(spectrum=True)
    assert parse(["--paste_back", "--paste_grain", "--paste_grain_seed", "2", "--paste_grain_spectrum"])["grain"] == dict(seed=2, spectrum=True)
    assert parse(["--paste_back", "--paste_grain_max_blur", "0"])["grain"] == dict(spectrum=dict(max_blur=0))
    assert bd._paste_back_cfg(parse(["--paste_back", "--paste_grain_max_blur", "24"]))["grain"] == dict(FULL, spectrum=dict(max_blur=24, luma=True))
    with pytest.raises(ValueError, match="paste_back: grain: .*spectrum"):
        bd._paste_back_cfg(parse(["--paste_back", "--paste_grain_max_blur", "65"]))
    for flag in (["--paste_grain_spectrum"], ["--paste_grain_max_blur", "0"]):
        with pytest.raises(SystemExit, match="needs --paste_back"):
            parse(flag)
        with pytest.raises(SystemExit, match="needs --paste_back"):
            re_.main(["--json_path", "j", "--original_images_dir", "o", "--weights_path", "w"] + flag)
        with pytest.raises(SystemExit, match="needs --paste_back"):
            re_.main(["--json_path", "j", "--original_images_dir", "o", "--lora_weights_path", "l"] + flag, lora=True)


# ---------------------------------------------------------------------------------------------- the wrappers
def test_ops_wrappers_check_before_they_launch(monkeypatch):
    from textflux_amd import ops
    img, m = torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8)
    g = np.zeros((2, 3), np.int32)
    for call in (lambda: ops.highpass_hist_step(img, m, step=2), lambda: ops.grain_shaped(img, m, g, (0, 0)),
                 lambda: pb.paste(img, img, m, grain=dict(spectrum=True))):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()                                                                   # no CPU fallback
    with pytest.raises(ValueError, match="grain: .*spectrum"):
        pb.paste(img, img, m, grain=dict(spectrum=dict(max_blur=99)))
    monkeypatch.setattr(ops, "_chk_dev", lambda *a: None)
    monkeypatch.setattr(ops.L, "lib", lambda: pytest.fail("a refused call reached the library"))
    for bad in (dict(img=img.float()), dict(sel=m.float()), dict(sel=m[:1]), dict(img=img.permute(0, 2, 1, 3)),
                dict(img=torch.zeros(2, 4, 4, 5, dtype=torch.uint8)), dict(img=img[0]), dict(lo=-1), dict(hi=256), dict(step=0), dict(step=9),
                dict(step=1.5), dict(out=torch.zeros(2, 3, 1024, dtype=torch.int32)), dict(out=torch.zeros(2, 4, 1024, dtype=torch.int64))):
        with pytest.raises(ValueError, match="highpass_hist_step: "):
            ops.highpass_hist_step(**dict(dict(img=img, sel=m), **bad))
    for bad in (dict(img=img.float()), dict(alpha=m.float()), dict(alpha=m[:1]), dict(img=torch.zeros(2, 4, 4, 5, dtype=torch.uint8)),
                dict(gain=g[:1]), dict(gain=g.astype(np.float32)), dict(gain=g - 1), dict(gain=g + 2 ** 18 + 1),
                dict(gain=torch.full((2, 3), 2 ** 18 + 1)), dict(shape=(65, 0)), dict(shape=(0, 257)), dict(shape=(-1, 0)), dict(shape=(0, -1)),
                dict(shape=(0.5, 1.0)), dict(shape=(1, 2, 3)), dict(shape=np.zeros((3, 2), int)), dict(shape=torch.tensor([[0, 0], [64, 300]])),
                dict(origin=(1, 2, 3)), dict(origin=(0.5, 1.0)), dict(out=img[:1]), dict(out=img.float())):
        with pytest.raises(ValueError, match="grain_shaped: "):
            ops.grain_shaped(**dict(dict(img=img, alpha=m, gain=g, shape=(0, 0)), **bad))
    assert ops.GRAIN_MAX_GAIN == 2 ** 18 and ops.GRAIN_MAX_BLUR == 64


# ---------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


def test_symbols_are_declared_bound_exported_and_the_abi_version_stays(lib):
    from textflux_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    for sym in ("tfx_highpass_hist_step_u8", "tfx_grain_shaped_u8"):
        assert sym in L.SIGNATURES and hasattr(lib, sym)
    assert "int tfx_highpass_hist_step_u8(const void* img, const void* sel, int32_t lo, int32_t hi, int32_t step, void* out, int32_t B," in hdr
    assert "int tfx_grain_shaped_u8(const void* img, const void* alpha, const int32_t* gain, const int32_t* shape, const int32_t* origin, uint32_t seed," in hdr
    assert len(L.SIGNATURES["tfx_highpass_hist_step_u8"][1]) == 11 and len(L.SIGNATURES["tfx_grain_shaped_u8"][1]) == 12
    assert L.ABI_VERSION == 11 == L.header_abi_version() and hdr.count("without a new") >= 8
    for phrase in ("m(x, y, c) = (256 - lam) n(x, y, c) + lam nL(x, y)", "k = [s, 256 - 2 s, s]",
                   "d = floor((f gain[b][c] alpha + 255 * 2^39) / (255 * 2^40))", "out[b][C][min(|sum_c r_c|, 1023)] += 1"):
        assert phrase in hdr, phrase


def test_entry_points_check_their_arguments(lib):
    p = [k << 20 for k in range(1, 8)]               # never dereferenced: every call is refused

    def hist(ptrs=p, step=1, dims=(2, 8, 8, 3)):
        return lib.tfx_highpass_hist_step_u8(ptrs[0], ptrs[1], 255, 255, step, ptrs[2], *dims, None)

    def grain(ptrs=p, dims=(2, 8, 8, 3)):
        return lib.tfx_grain_shaped_u8(ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], 7, ptrs[5], *dims, None)
    for k in range(3):
        assert hist(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_highpass_hist_step_u8: null pointer" in lib.tfx_last_error()
    for k in (0, 1, 2, 3, 5):                                                          # origin alone may be NULL
        assert grain(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_grain_shaped_u8: null pointer" in lib.tfx_last_error()
    for step in (0, 9, -1):
        assert hist(step=step) != 0 and b"highpass_hist_step_u8: step must be in 1..8" in lib.tfx_last_error()
    for call, name in ((hist, b"highpass_hist_step_u8"), (grain, b"grain_shaped_u8")):
        for c in (0, 5):
            assert call(dims=(2, 8, 8, c)) != 0 and b"1..4 channels" in lib.tfx_last_error() and name in lib.tfx_last_error()
        for k in range(3):
            dims = [2, 8, 8, 3]
            dims[k] = 0
            assert call(dims=tuple(dims)) != 0 and b"at least 1" in lib.tfx_last_error()
        assert call(dims=(65536, 8, 8, 3)) != 0 and b"65535" in lib.tfx_last_error()
    assert hist(dims=(1, 65536, 65536, 1)) != 0 and b"32-bit" in lib.tfx_last_error()
    assert hist([p[0], p[1], p[2] + 2]) != 0 and b"4-byte aligned" in lib.tfx_last_error()
    for k in (0, 1):
        assert hist([p[0], p[1], p[k]]) != 0 and b"alias" in lib.tfx_last_error()
    for k in (1, 2, 3, 4):                                                             # out may be img, and nothing else
        ptrs = list(p)
        ptrs[5] = p[k]
        assert grain(ptrs) != 0 and b"alias img only" in lib.tfx_last_error()
    for k in (2, 3, 4):
        ptrs = list(p)
        ptrs[k] += 2
        assert grain(ptrs) != 0 and b"4-byte aligned" in lib.tfx_last_error()
