"""Grain match without a GPU (DESIGN.md section 4 "Grain match"): the statistics of the hashed grain, of the estimator and of the whole
step on the numpy restatement (tests/helpers/grain_ref.py), the package's host arithmetic against it, and the plumbing: the
configuration, what the pipeline, the per-line composer and the batch driver hand on, the CLIs' flags, and the C entry points'
declarations and refusals (none of which touches a device)."""
import importlib
import inspect
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests.helpers import grain_ref as gref
from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from textflux_amd import batch_driver as bd
from textflux_amd import paste_back as pb
from textflux_amd import per_line as pl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = 1.4826 / math.sqrt(164)                         # grey levels per histogram bin
SIGMAS = (1, 2, 3, 5, 8)


def _gain(sigma):
    return math.floor(sigma / gref.SIGMA0 * 65536 + 0.5)


def _noisy(shape_hw, colour, sigma, origin, seed):
    """A flat colour plus the restatement's grain of standard deviation sigma: u8 [1, H, W, 3]."""
    h, w = shape_hw
    flat = np.broadcast_to(np.array(colour, np.uint8), (1, h, w, 3)).copy()
    return gref.grain(flat, np.full((1, h, w), 255, np.uint8), np.full((1, 3), _gain(sigma)), origin, seed)


# ---------------------------------------------------------------------------------------------- the noise and its synthesis
def test_the_hash_is_centred_has_the_stated_deviation_and_is_scene_anchored():
    n = gref.noise_field(256, 256, 3, (0, 0), 1)
    print(f"n: mean {n.mean():.4f}, std {n.std():.3f}, range [{n.min()}, {n.max()}]")
    assert abs(gref.SIGMA0 - 147.8005) < 1e-4 and n.min() >= -510 and n.max() <= 510
    assert abs(n.mean()) < 0.5 and abs(n.std() / 147.80 - 1) < 0.01
    big, small = gref.noise_field(30, 40, 3, (100, 50), 1), gref.noise_field(8, 10, 3, (110, 60), 1)
    assert np.array_equal(big[10:18, 10:20], small)                     # the same scene pixels, whatever window holds them
    assert not np.array_equal(small, gref.noise_field(8, 10, 3, (110, 60), 2)) and not np.array_equal(small, gref.noise_field(8, 10, 3, (111, 60), 1))
    assert not np.array_equal(small[:, :, 0], small[:, :, 1])
    # coordinates wrap in 32 bits
    assert np.array_equal(gref.noise_field(4, 6, 3, (2 ** 32 - 2, 2 ** 32 - 1), 5)[1:, 2:], gref.noise_field(3, 4, 3, (0, 0), 5))


@pytest.fixture(scope="module")
def synthesised():
    """sigma -> the flat 128 image with grain of that sigma (origin (17, 5), seed 7, alpha 255): computed once, never modified."""
    img, alpha = np.full((1, 128, 128, 3), 128, np.uint8), np.full((1, 128, 128), 255, np.uint8)
    out = {s: gref.grain(img, alpha, np.full((1, 3), _gain(s)), (17, 5), 7) for s in SIGMAS}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("sigma", SIGMAS)
def test_synthesised_grain_has_the_requested_deviation(synthesised, sigma):
    """The rounding to a byte adds 1 / 12 of variance; the standard error of a deviation over 128 x 128 samples is 0.55 %."""
    d = synthesised[sigma].astype(np.float64) - 128
    for c in range(3):
        ratio = d[0, :, :, c].std() / math.sqrt(sigma ** 2 + 1 / 12)
        print(f"sigma {sigma} channel {c}: ratio {ratio:.4f}")
        assert abs(ratio - 1) < 0.02


@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_estimator_recovers_it(synthesised, sigma):
    hist = gref.highpass_hist(synthesised[sigma], np.full((1, 128, 128), 255, np.uint8))
    assert (hist.sum(-1) == 128 * 128).all()
    est = pb.noise_sigma(hist)
    print(f"sigma {sigma}: estimate {est.ravel()}")
    assert np.array_equal(est, gref.noise_sigma(hist))                  # the package's host arithmetic is the restatement's
    assert (np.abs(est - sigma) <= BIN + 0.03 * sigma).all()


def test_noise_sigma_is_the_lower_median_bin():
    h = np.zeros((1, 4, 1024), np.int64)
    h[0, 0, 3], h[0, 0, 7] = 2, 2                     # n = 4: the second of four
    h[0, 1, 3], h[0, 1, 7] = 2, 3                     # n = 5: the third of five
    h[0, 2, 1023] = 9                                 # everything saturated
    want = BIN * np.array([[3, 7, 1023, 0]])          # and an empty histogram
    assert np.allclose(pb.noise_sigma(h), want, rtol=0, atol=1e-12) and np.array_equal(pb.noise_sigma(h), gref.noise_sigma(h))
    assert np.array_equal(pb.noise_sigma(torch.from_numpy(h).to(torch.int32)), pb.noise_sigma(h))
    with pytest.raises(ValueError, match="1024"):
        pb.noise_sigma(h[:, :, :100])


def test_edges_below_half_of_the_pixels_do_not_move_the_estimate(synthesised):
    img = synthesised[3].copy()
    img[0, 30:34, :, :] = 255                         # strokes: outliers of the residual
    img[0, :, 60:63, :] = 0
    alpha = np.full((1, 128, 128), 255, np.uint8)
    clean, marked = gref.noise_sigma(gref.highpass_hist(synthesised[3], alpha)), gref.noise_sigma(gref.highpass_hist(img, alpha))
    assert (np.abs(marked - clean) <= 3 * BIN).all() and gref.highpass_hist(img, alpha)[0, :, 1023].min() > 0


# ---------------------------------------------------------------------------------------------- closure: estimate, add, estimate again
def _closure(sigma_s, sigma_e, hw):
    h, w = hw
    scene = _noisy(hw, (120, 128, 140), sigma_s, (31, 9), 3) if sigma_s else np.broadcast_to(np.array((120, 128, 140), np.uint8), (1, h, w, 3)).copy()
    edit = _noisy(hw, (124, 126, 133), sigma_e, (31, 9), 11) if sigma_e else np.broadcast_to(np.array((124, 126, 133), np.uint8), (1, h, w, 3)).copy()
    alpha = np.zeros((1, h, w), np.uint8)
    alpha[0, h // 4: h - h // 4, w // 4: w - w // 4] = 255
    ring = plref.ring_mask(alpha, 12)
    pasted = ref.overlay(scene, edit, alpha)
    out, gains = gref.match(pasted, scene, alpha, ring, dict(seed=5), (31, 9))
    return scene, alpha, ring, pasted, out, gains


@pytest.mark.parametrize("sigma_s,sigma_e,hw", [(4, 0, (96, 160)), (4, 2, (96, 160)), (6, 3, (64, 256)), (2, 0, (48, 96))])
def test_closure_the_interior_ends_at_the_scenes_level(sigma_s, sigma_e, hw):
    scene, alpha, ring, pasted, out, gains = _closure(sigma_s, sigma_e, hw)
    s_scene = pb.noise_sigma(gref.highpass_hist(scene, ring))
    s_before, s_after = pb.noise_sigma(gref.highpass_hist(pasted, alpha)), pb.noise_sigma(gref.highpass_hist(out, alpha))
    print(f"scene {s_scene.ravel()}, interior before {s_before.ravel()}, after {s_after.ravel()}, gains {gains.ravel()}")
    assert (gains > 0).all() and np.array_equal(gains, pb.grain_gains(gref.highpass_hist(scene, ring), gref.highpass_hist(pasted, alpha), dict(seed=5)))
    assert (np.abs(s_after - s_scene) <= 2 * BIN + 0.03 * s_scene).all()
    assert (s_before < s_scene - 2 * BIN).all()                          # ... which it did not before
    assert np.array_equal(out[alpha == 0], scene[alpha == 0])            # where alpha is 0 the bytes are the scene's


def test_closure_an_edit_that_is_noisier_is_left_alone():
    scene, alpha, ring, pasted, out, gains = _closure(3, 5, (96, 160))
    assert (gains == 0).all() and np.array_equal(out, pasted) and np.array_equal(out[alpha == 0], scene[alpha == 0])


# ---------------------------------------------------------------------------------------------- the restatement's exact properties
def test_grain_properties_alpha_zero_gain_zero_clamps():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (2, 9, 13), dtype=np.uint8)
    alpha[0, :3] = 0
    gains = np.array([[65536, 20000, 0], [1, 300, 65536]])
    out = gref.grain(img, alpha, gains, (17, 5), 9)
    assert np.array_equal(out[alpha == 0], img[alpha == 0]) and np.array_equal(out[0, :, :, 2], img[0, :, :, 2]) and not np.array_equal(out, img)
    assert np.array_equal(gref.grain(img, alpha, np.zeros((2, 3), int), (17, 5), 9), img)
    full = np.full((2, 9, 13), 255, np.uint8)
    d = gref.grain(np.full_like(img, 128), full, gains, None, 9).astype(int) - 128
    n = gref.noise_field(9, 13, 3, (0, 0), 9)
    assert np.array_equal(d[0, :, :, 0], np.clip(n[:, :, 0], -128, 127))   # gain 1.0, alpha 255: d = n exactly
    lo, hi = gref.grain(np.zeros_like(img), full, gains, None, 9), gref.grain(np.full_like(img, 255), full, gains, None, 9)
    assert lo.min() == 0 and hi.max() == 255 and (lo[0, :, :, 0] == np.clip(n[:, :, 0], 0, 255)).all() and (hi[0, :, :, 0] == np.clip(255 + n[:, :, 0], 0, 255)).all()
    # per-sample origins: sample 1 at another place is the single-sample call there
    both = gref.grain(img, alpha, gains, np.array([[17, 5], [400, 300]]), 9)
    assert np.array_equal(both[1:], gref.grain(img[1:], alpha[1:], gains[1:], (400, 300), 9)) and np.array_equal(both[:1], out[:1])


def test_highpass_hist_properties():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (2, 7, 11, 3), dtype=np.uint8)
    sel = rng.integers(0, 256, (2, 7, 11), dtype=np.uint8)
    sel[0, 2:5, 3:9] = 255
    h = gref.highpass_hist(img, sel, 255, 255)
    assert np.array_equal(h.sum(-1), np.broadcast_to((sel == 255).sum(axis=(1, 2))[:, None], (2, 3)))
    assert np.array_equal(gref.highpass_hist(img, sel, 1, 255).sum(-1)[:, 0], (sel >= 1).sum(axis=(1, 2)))
    assert gref.highpass_hist(img, np.zeros_like(sel), 255, 255).sum() == 0
    flat = gref.highpass_hist(np.full_like(img, 77), sel, 0, 255)
    assert (flat[:, :, 0] == 77).all() and flat[:, :, 1:].sum() == 0    # a constant image has no residual, the borders included
    y, x = np.mgrid[:7, :11]
    board = np.where((y + x) % 2 == 0, 255, 0).astype(np.uint8)[None, :, :, None].repeat(3, axis=3)
    hb = gref.highpass_hist(board, np.full((1, 7, 11), 255, np.uint8))
    assert (hb[0, :, 1023] == 7 * 11).all()           # |16 p - blur| = 8 * 255 inside and at least 6 * 255 on the replicated border: all saturated
    one = gref.highpass_hist(img[:1, :1, :1], np.full((1, 1, 1), 255, np.uint8))
    assert (one[0, :, 0] == 1).all()                  # a single pixel is its own neighbourhood


# ---------------------------------------------------------------------------------------------- gains and configuration
def _hist_at(bin_, n, c=3):
    h = np.zeros((1, c, 1024), np.int64)
    h[:, :, bin_] = n
    return h


def test_grain_gains_thresholds_and_clamp():
    hs, he = _hist_at(40, 1000), _hist_at(10, 1000)   # sigma 4.63 against 1.16
    ss, se, add = pb.grain_levels(hs, he, True)
    assert np.allclose(ss, 40 * BIN) and np.allclose(se, 10 * BIN) and np.allclose(add, BIN * math.sqrt(1500))
    g = pb.grain_gains(hs, he, True)
    assert g.dtype == np.int32 and g.shape == (1, 3) and (g == math.floor(BIN * math.sqrt(1500) / gref.SIGMA0 * 65536 + 0.5)).all()
    assert np.array_equal(g, gref.grain_gains(hs, he))
    assert (pb.grain_gains(hs, he, dict(strength=0.5)) == math.floor(0.5 * BIN * math.sqrt(1500) / gref.SIGMA0 * 65536 + 0.5)).all()
    assert (pb.grain_gains(hs, he, dict(max_sigma=2.0)) == _gain(2.0)).all()                        # clamped
    assert (pb.grain_gains(_hist_at(1023, 1000), _hist_at(0, 1000), True) == _gain(6.0)).all()     # ... by default at 6
    assert (pb.grain_gains(_hist_at(1023, 1000), _hist_at(0, 1000), dict(max_sigma=64, strength=4)) == _gain(64.0)).all()
    assert _gain(64.0) <= 65536
    for cfg in (dict(strength=0), dict(max_sigma=0)):
        assert (pb.grain_gains(hs, he, cfg) == 0).all()
    assert (pb.grain_gains(_hist_at(40, 255), he, True) == 0).all() and (pb.grain_gains(hs, _hist_at(10, 255), True) == 0).all()
    assert (pb.grain_gains(_hist_at(40, 255), _hist_at(10, 255), dict(min_pixels=255)) > 0).all()
    assert (pb.grain_gains(he, hs, True) == 0).all() and (pb.grain_gains(hs, hs, True) == 0).all()   # nothing is denoised
    mixed_s, mixed_e = np.concatenate([hs, he]), np.concatenate([he, hs])
    assert np.array_equal(pb.grain_gains(mixed_s, mixed_e, True), np.concatenate([g, np.zeros_like(g)]))
    with pytest.raises(ValueError, match="agree"):
        pb.grain_levels(hs, he[:, :2], True)


def test_cfgs_accept_validate_and_refuse():
    full = dict(ring=24, max_sigma=6.0, strength=1.0, min_pixels=256, seed=0)
    assert pb.grain_cfg(True) == full == dict(ring=pb.RING, max_sigma=pb.GRAIN_MAX_SIGMA, strength=pb.GRAIN_STRENGTH, min_pixels=pb.MIN_PIXELS, seed=0)
    assert pb.grain_cfg(dict(ring=8, seed=None)) == dict(full, ring=8) and pb.grain_cfg(dict(max_sigma=64, strength=4, seed=2 ** 32 - 1))["seed"] == 2 ** 32 - 1
    assert abs(pb.GRAIN_K - 0.11577) < 1e-5 and abs(pb.GRAIN_K - BIN) < 1e-15
    for bad, match in ((dict(sigma=3), r"unknown keys \['sigma'\]"), (dict(ring=0), "ring"), (dict(ring=256), "ring"), (dict(max_sigma=-0.1), "max_sigma"),
                       (dict(max_sigma=64.5), "max_sigma"), (dict(max_sigma=float("nan")), "max_sigma"), (dict(strength=-1), "strength"),
                       (dict(strength=4.5), "strength"), (dict(min_pixels=0), "min_pixels"), (dict(seed=-1), "seed"), (dict(seed=2 ** 32), "seed"),
                       (7, "True or a dict")):
        with pytest.raises(ValueError, match="grain: .*" + match):
            pb.grain_cfg(bad)
        with pytest.raises(ValueError, match="paste_back: .*grain"):
            bd._paste_back_cfg(dict(grain=bad))
    assert bd._paste_back_cfg(dict(grain=True)) == dict(dilate=16, feather=4, region=None, grain=full)
    assert bd._paste_back_cfg(dict(per_line=True, grain=dict(seed=3), curve=True, seamless=True))["grain"] == dict(full, seed=3)
    assert bd._paste_back_cfg(dict(grain=None)) == bd._paste_back_cfg(dict(grain=False)) == bd._paste_back_cfg({}) == dict(dilate=16, feather=4, region=None)
    with pytest.raises(ValueError, match="unknown keys"):
        bd._paste_back_cfg(dict(grains=True))


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


@pytest.mark.parametrize("grain", (True, dict(max_sigma=3.0, seed=4)))
@pytest.mark.parametrize("others", ({}, dict(color_match=True), dict(seamless=True)))
def test_compose_lines_and_the_driver_pass_the_key_exactly_when_configured(grain, others):
    scene, works, crops = _works()
    base = dict(per_line=True, dilate=2, feather=1, **others)
    cfg0, cfg1 = bd._paste_back_cfg(base), bd._paste_back_cfg(dict(base, grain=grain))
    p0, p1 = Recorder(), Recorder()
    pl.compose_lines(p0, works, crops, cfg0)
    out = pl.compose_lines(p1, works, crops, cfg1)
    assert np.array_equal(np.array(out), scene) and len(p0.pastes) == len(p1.pastes) == 2
    for w, k0, k1 in zip(works, p0.pastes, p1.pastes):
        assert "grain" not in k0 and "origin" not in k0 and ("color_ref" in k0) == bool(others)
        assert set(k1) == set(k0) | {"grain", "origin", "color_ref"}
        r = w.region
        assert k1["grain"] == pb.grain_cfg(grain) and k1["origin"] == (r.x0, r.y0) and np.array_equal(k1["color_ref"], scene[r.y0:r.y1, r.x0:r.x1])
        assert all(k1[k] is k0[k] or k1[k] == k0[k] for k in k0 if k != "color_ref")
    # the single-region path of the driver: the region's own place in the scene, and no colour reference (the window is the original)
    q0, q1 = Recorder(), Recorder()
    bd._paste_into_original(q0, works[1], crops[1], cfg0)
    bd._paste_into_original(q1, works[1], crops[1], cfg1)
    assert "grain" not in q0.pastes[0] and "origin" not in q0.pastes[0]
    assert q1.pastes[0] == dict(q0.pastes[0], grain=pb.grain_cfg(grain), origin=(10, 16))
    # a pipeline that predates the key serves everything without it, and fails loudly (no silent plain paste) with it
    old = Older()
    if not others:
        pl.compose_lines(old, works, crops, cfg0)
        bd._paste_into_original(old, works[0], crops[0], cfg0)
        assert old.n == 3
    with pytest.raises(TypeError):
        pl.compose_lines(old, works, crops, cfg1)
    with pytest.raises(TypeError):
        bd._paste_into_original(old, works[0], crops[0], cfg1)


def test_the_pipeline_method_hands_grain_and_origin_on_only_with_the_key(monkeypatch):
    from textflux_amd.pipeline import FluxFillPipeline
    assert inspect.signature(pb.paste).parameters["grain"].default is None
    assert inspect.signature(FluxFillPipeline.paste_back).parameters["grain"].default is None
    calls = []
    monkeypatch.setattr(pb, "paste", lambda original, edited, mask, dilate, feather, **kw: (calls.append(kw), original)[1])
    me = types.SimpleNamespace(_execution_device="cpu")
    img, m = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)
    FluxFillPipeline.paste_back(me, img, img, m)
    FluxFillPipeline.paste_back(me, img, img, m, seamless=True)
    FluxFillPipeline.paste_back(me, img, img, m, grain=dict(seed=2), origin=(7, 9))
    FluxFillPipeline.paste_back(me, img, img, m, grain=True, color_ref=img)
    assert calls[0] == {} and calls[1] == dict(seamless=True)
    assert calls[2] == dict(grain=dict(seed=2), origin=(7, 9))
    assert set(calls[3]) == {"grain", "origin", "color_match", "color_ref"} and calls[3]["color_match"] is None and calls[3]["origin"] == (0, 0)
    assert torch.equal(calls[3]["color_ref"], torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


def test_paste_refuses_before_it_launches_and_keeps_the_old_rule_without_the_key():
    from textflux_amd import ops
    img, m = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="color_ref needs color_match"):
        pb.paste(img, img, m, color_ref=img)
    with pytest.raises(ValueError, match="grain: unknown keys"):
        pb.paste(img, img, m, grain=dict(sigma=1))
    for call in (lambda: ops.highpass_hist(img, m), lambda: ops.grain(img, m, np.zeros((1, 3), np.int32)),
                 lambda: pb.paste(img, img, m, grain=True, color_ref=img)):          # allowed now: it gets as far as the device check
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()                                                                   # no CPU fallback


def test_ops_wrappers_check_before_they_launch(monkeypatch):
    from textflux_amd import ops
    monkeypatch.setattr(ops, "_chk_dev", lambda *a: None)
    monkeypatch.setattr(ops.L, "lib", lambda: pytest.fail("a refused call reached the library"))
    img, m = torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8)
    g = np.zeros((2, 3), np.int32)
    for bad in (dict(img=img.float()), dict(sel=m.float()), dict(sel=m[:1]), dict(sel=m[:, :2]), dict(img=img.permute(0, 2, 1, 3)),
                dict(img=torch.zeros(2, 4, 4, 5, dtype=torch.uint8)), dict(img=img[0]), dict(lo=-1), dict(hi=256),
                dict(out=torch.zeros(2, 3, 1024, dtype=torch.int64)), dict(out=torch.zeros(2, 3, 512, dtype=torch.int32))):
        with pytest.raises(ValueError, match="highpass_hist"):
            ops.highpass_hist(**dict(dict(img=img, sel=m), **bad))
    for bad in (dict(img=img.float()), dict(alpha=m.float()), dict(alpha=m[:1]), dict(img=torch.zeros(2, 4, 4, 5, dtype=torch.uint8)),
                dict(img=img.permute(0, 2, 1, 3)), dict(gain=g[:1]), dict(gain=g[:, :2]), dict(gain=g.astype(np.float32)), dict(gain=g - 1),
                dict(gain=g + 65537), dict(gain=torch.full((2, 3), 65537)), dict(origin=(1, 2, 3)), dict(origin=(0.5, 1.0)),
                dict(origin=np.zeros((3, 2), int)), dict(out=img[:1]), dict(out=img.float())):
        with pytest.raises(ValueError, match="grain"):
            ops.grain(**dict(dict(img=img, alpha=m, gain=g), **bad))
    assert ops.HIGHPASS_BINS == 1024 and abs(ops.GRAIN_SIGMA0 - gref.SIGMA0) < 1e-12


# ---------------------------------------------------------------------------------------------- the CLIs
def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    flags = lambda a: (a.paste_grain, a.paste_grain_max_sigma, a.paste_grain_strength, a.paste_grain_seed)
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        assert flags(parser.parse_args(base)) == (False, None, None, None)
        a = parser.parse_args(base + ["--paste_back", "--paste_grain", "--paste_grain_max_sigma", "3.5", "--paste_grain_strength", "0.5", "--paste_grain_seed", "9"])
        assert flags(a) == (True, 3.5, 0.5, 9)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(["--paste_back"]) == dict(dilate=16, feather=4, region=None)          # without the new flags: the dict it was
    assert parse(["--paste_back", "--paste_grain"]) == dict(dilate=16, feather=4, region=None, grain=True)
    assert parse(["--paste_back", "--paste_grain_max_sigma", "3"])["grain"] == dict(max_sigma=3.0)
    assert parse(["--paste_back", "--paste_grain_seed", "0"])["grain"] == dict(seed=0)
    assert parse(["--paste_back", "--paste_per_line", "--paste_curve", "--paste_seamless", "--paste_grain_strength", "2"])["grain"] == dict(strength=2.0)
    assert bd._paste_back_cfg(parse(["--paste_back", "--paste_grain_seed", "5"]))["grain"] == dict(ring=24, max_sigma=6.0, strength=1.0, min_pixels=256, seed=5)
    for flag in (["--paste_grain"], ["--paste_grain_max_sigma", "3"], ["--paste_grain_strength", "0"], ["--paste_grain_seed", "0"]):
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
    for sym in ("tfx_highpass_hist_u8", "tfx_grain_u8"):
        assert sym in L.SIGNATURES and hasattr(lib, sym)
    assert "int tfx_highpass_hist_u8(const void* img, const void* sel, int32_t lo, int32_t hi, void* out, int32_t B, int32_t H, int32_t W, int32_t C," in hdr
    assert "int tfx_grain_u8(const void* img, const void* alpha, const int32_t* gain, const int32_t* origin, uint32_t seed, void* out, int32_t B," in hdr
    assert len(L.SIGNATURES["tfx_highpass_hist_u8"][1]) == 10 and len(L.SIGNATURES["tfx_grain_u8"][1]) == 11
    assert L.ABI_VERSION == 11 == L.header_abi_version() and hdr.count("without a new") >= 7
    for phrase in ("h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16", "x * 0x9E3779B1 + y * 0x85EBCA77 + c * 0xC2B2AE3D",
                   "floor((n gain[b][c] alpha + 255 * 32768) / (255 * 65536))", "out[b][c][min(v, 1023)] += 1"):
        assert phrase in hdr, phrase


def test_entry_points_check_their_arguments(lib):
    p = [k << 20 for k in range(1, 7)]               # never dereferenced: every call is refused

    def hist(ptrs=p, dims=(2, 8, 8, 3)):
        return lib.tfx_highpass_hist_u8(ptrs[0], ptrs[1], 255, 255, ptrs[2], *dims, None)

    def grain(ptrs=p, dims=(2, 8, 8, 3)):
        return lib.tfx_grain_u8(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 7, ptrs[4], *dims, None)
    for k in range(3):
        assert hist(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_highpass_hist_u8: null pointer" in lib.tfx_last_error()
    for k in (0, 1, 2, 4):                                                             # origin alone may be NULL
        assert grain(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_grain_u8: null pointer" in lib.tfx_last_error()
    for call, name in ((hist, b"highpass_hist_u8"), (grain, b"grain_u8")):
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
    for k in (1, 2, 3):                                                                # out may be img, and nothing else
        ptrs = list(p)
        ptrs[4] = p[k]
        assert grain(ptrs) != 0 and b"alias img only" in lib.tfx_last_error()
    assert grain([p[0], p[1], p[2] + 2, p[3], p[4]]) != 0 and b"4-byte aligned" in lib.tfx_last_error()
