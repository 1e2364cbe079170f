"""Grain spectrum match on the GPU (DESIGN.md section 4 "Grain spectrum"): ops.highpass_hist_step and ops.grain_shaped (imageops.hip:
highpass_hist_kernel, grain_shaped_kernel) and paste_back.paste(grain=dict(spectrum=...)) against the numpy restatement in
tests/helpers/grain_spectrum_ref.py, bit for bit (integer arithmetic only; the host arithmetic is float64 on exact integers)."""
import itertools
import math

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from tests.helpers import grain_ref as gref
from tests.helpers import grain_spectrum_ref as sref
from tests.helpers import paste_back_ref as ref
from tests.helpers import rectify_ref as rref

pytestmark = pytest.mark.gpu
# a single pixel (every neighbour is a clamp, the tile is all halo); a few pixels, narrower than a step of 4; an odd width in two
# samples with partial tiles in both directions; four channels over several tiles (64 x 16) each way; one channel in one long row
SHAPES = ((1, 1, 1, 1), (1, 3, 5, 3), (2, 17, 33, 3), (1, 70, 131, 4), (1, 9, 300, 1))
STEPS = (1, 2, 4)
KINDS = ((0, 0), (64, 0), (0, 256), (23, 101))
ORIGINS = ((0, 0), (-3, -70), (2 ** 32 - 2, 2 ** 32 - 5))      # the second and third cross the wrap inside the larger windows


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def _dev(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays)


# ---------------------------------------------------------------------------------------------- ops.highpass_hist_step
@pytest.mark.parametrize("shape", SHAPES)
def test_highpass_hist_step_is_the_restatement_exactly(ops, shape):
    rng = np.random.default_rng(sum(shape))
    b, h, w, c = shape
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    sel = rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    pick = rng.random((b, h, w))
    sel[pick < 0.3], sel[pick > 0.6] = 0, 255
    idev, sdev = _dev(img, sel)
    out = torch.full((b, c + 1, 1024), 7, dtype=torch.int32, device="cuda")      # stale contents: the call zeroes it itself
    for step, (lo, hi) in itertools.product(STEPS, ((255, 255), (1, 255), (0, 255))):
        want = sref.highpass_hist_step(img, sel, lo, hi, step)
        got = ops.highpass_hist_step(idev, sdev, lo, hi, step)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (step, lo, hi)
        n = ((sel >= lo) & (sel <= hi)).sum(axis=(1, 2))
        assert np.array_equal(want.sum(-1), np.broadcast_to(n[:, None], (b, c + 1)))
        again = ops.highpass_hist_step(idev, sdev, lo, hi, step, out=out)
        assert again.data_ptr() == out.data_ptr() and torch.equal(out, got)
        if step == 1:
            assert torch.equal(got[:, :c], ops.highpass_hist(idev, sdev, lo, hi))
    assert int(ops.highpass_hist_step(idev, torch.zeros_like(sdev), 255, 255, 2).abs().sum()) == 0      # nothing selected: all zeros
    flat = ops.highpass_hist_step(torch.full_like(idev, 77), sdev, 0, 255, 4)
    assert (flat[:, :, 0] == h * w).all() and int(flat[:, :, 1:].sum()) == 0     # a constant image has no residual, the borders included


# ---------------------------------------------------------------------------------------------- ops.grain_shaped
@pytest.mark.parametrize("shape", SHAPES)
def test_grain_shaped_is_the_restatement_exactly(ops, shape):
    rng = np.random.default_rng(200 + sum(shape))
    b, h, w, c = shape
    imgs = dict(random=rng.integers(0, 256, shape, dtype=np.uint8), zeros=np.zeros(shape, np.uint8), ones=np.full(shape, 255, np.uint8))
    alpha = rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    pick = rng.random((b, h, w))
    alpha[pick < 0.2], alpha[pick > 0.7] = 0, 255
    alpha.flat[0] = 255
    full = np.full((b, h, w), 255, np.uint8)
    gains = dict(mixed=rng.choice(np.array([0, 1, 2661, 65536, 2 ** 18], np.int32), (b, c)), top=np.full((b, c), 2 ** 18, np.int32),
                 one=np.full((b, c), 65536, np.int32), zero=np.zeros((b, c), np.int32))
    gains["mixed"].flat[0] = 2 ** 18
    for kind, origin in itertools.product(KINDS, ORIGINS):
        for iname, aname, gname in (("random", "random", "mixed"), ("zeros", "full", "top"), ("ones", "full", "top"), ("random", "full", "zero")):
            if iname != "random" and origin != ORIGINS[1]:
                continue                                                          # the constant images are about the clamp: one origin
            img, a, gain = imgs[iname], (alpha if aname == "random" else full), gains[gname]
            idev, adev = _dev(img, a)
            want = sref.grain_shaped(img, a, gain, kind, origin, 7)
            got = ops.grain_shaped(idev, adev, gain, kind, origin, 7)
            assert np.array_equal(got.cpu().numpy(), want), (kind, origin, iname, aname, gname)
            assert np.array_equal(idev.cpu().numpy(), img)                        # out of place: the input is untouched
            assert np.array_equal(want[a == 0], img[a == 0])                      # alpha 0 leaves the byte
            if gname == "zero":
                assert np.array_equal(want, img)                                  # gain 0 copies
            if origin == ORIGINS[1] and iname == "random":                        # in place, everything as tensors
                work = idev.clone()
                same = ops.grain_shaped(work, adev, torch.from_numpy(gain).cuda(), torch.tensor([list(kind)] * b).cuda(),
                                        torch.tensor([list(origin)] * b), 7, out=work)
                assert same.data_ptr() == work.data_ptr() and np.array_equal(work.cpu().numpy(), want)
        if kind == (0, 0):                                                        # white: ops.grain, bit for bit
            idev, adev = _dev(imgs["random"], alpha)
            assert torch.equal(ops.grain_shaped(idev, adev, gains["one"], kind, origin, 7), ops.grain(idev, adev, gains["one"], origin, 7))
    if h * w > 64:                                                                # the clamp was at work in what was compared above
        lo = sref.grain_shaped(imgs["zeros"], full, gains["top"], (23, 101), ORIGINS[1], 7)
        hi = sref.grain_shaped(imgs["ones"], full, gains["top"], (23, 101), ORIGINS[1], 7)
        assert lo.min() == 0 and lo.max() > 100 and hi.max() == 255 and hi.min() < 155
    # per-sample shapes and origins; no origin is origin (0, 0)
    idev, adev = _dev(imgs["random"], alpha)
    per_o, per_s = np.array([[40 * s - 1, 9 + s] for s in range(b)]), np.array([[64 - 30 * s, 256 * s] for s in range(b)])
    assert np.array_equal(ops.grain_shaped(idev, adev, gains["one"], per_s, per_o, 3).cpu().numpy(),
                          sref.grain_shaped(imgs["random"], alpha, gains["one"], per_s, per_o, 3))
    assert torch.equal(ops.grain_shaped(idev, adev, gains["mixed"], (23, 101)), ops.grain_shaped(idev, adev, gains["mixed"], (23, 101), (0, 0), 0))


def test_the_grain_of_a_scene_pixel_does_not_depend_on_the_window(ops):
    """A 40 x 56 window cut from a 96 x 128 scene: its bytes, border rows and columns included, are the whole-scene call's."""
    rng = np.random.default_rng(8)
    scene = rng.integers(60, 200, (1, 96, 128, 3), dtype=np.uint8)
    alpha = rng.integers(1, 256, (1, 96, 128), dtype=np.uint8)
    gains = np.array([[120000, 9000, 2 ** 18]], np.int32)
    whole = ops.grain_shaped(*_dev(scene, alpha), gains, (64, 128), (1030, 2020), 4)
    part = ops.grain_shaped(*_dev(scene[:, 21:61, 37:93], alpha[:, 21:61, 37:93]), gains, (64, 128), (1030 + 37, 2020 + 21), 4)
    assert part.shape == (1, 40, 56, 3) and torch.equal(whole[:, 21:61, 37:93], part)
    assert not torch.equal(part.cpu(), torch.from_numpy(scene[:, 21:61, 37:93]))


def test_both_kernels_beyond_one_grid_step(ops):
    """More pixels than the histogram's 256 workgroups cover in one step, and more tiles than the grain's 2048 workgroups: both go
    round their loops."""
    rng = np.random.default_rng(6)
    shape = (1, 300, 301, 3)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    sel = np.where(rng.random(shape[:3]) < 0.5, 255, 0).astype(np.uint8)
    assert np.array_equal(ops.highpass_hist_step(*_dev(img, sel), 255, 255, 2).cpu().numpy(), sref.highpass_hist_step(img, sel, 255, 255, 2))
    shape = (1, 16 * 2048 + 5, 3, 2)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    alpha = rng.integers(0, 256, shape[:3], dtype=np.uint8)
    gains = np.array([[2 ** 18, 30000]], np.int32)
    assert np.array_equal(ops.grain_shaped(*_dev(img, alpha), gains, (40, 200), (17, -5), 11).cpu().numpy(),
                          sref.grain_shaped(img, alpha, gains, (40, 200), (17, -5), 11))


# ---------------------------------------------------------------------------------------------- paste(grain=dict(spectrum=...))
D, R = 8, 2
HW = (96, 160)
GRAIN = dict(ring=12, seed=3, min_pixels=64)


def _soft_scene(hw, origin, sigma=4.0, shape=(32, 160)):
    """A colour ramp plus the restatement's shaped grain of true deviation sigma: a photo whose noise is soft and mostly luma."""
    h, w = hw
    ramp = np.linspace(70, 170, w)[None, None, :, None] + np.array([0.0, 8.0, -12.0])
    flat = np.broadcast_to(np.floor(ramp + 0.5), (1, h, w, 3)).astype(np.uint8)
    gain = np.full((1, 3), math.floor(sigma / sref.levels(*shape)[1] / gref.SIGMA0 * 65536 + 0.5))
    return flat, sref.grain_shaped(flat, np.full((1, h, w), 255, np.uint8), gain, shape, origin, 21)


@pytest.mark.parametrize("seamless", [None, dict(smooth=3, max_shift=12)])
def test_paste_of_a_plain_line_is_the_restatement(ops, seamless):
    """test_grain_gpu.py's plain-line case with a scene whose noise is shaped."""
    from textflux_amd import paste_back as pb
    clean, orig = _soft_scene(HW, (40, 30))
    edit = ref.resize(np.clip(clean.astype(np.int64) + 6, 0, 255).astype(np.uint8), (80, 132))
    grey = np.zeros((1,) + HW, np.uint8)
    grey[0, 36:60, 50:110] = 255
    sm = None if seamless is None else pb.seamless_cfg(seamless)
    kw = {} if seamless is None else dict(seamless=seamless)
    od, ed, gd = _dev(orig, edit, grey)
    cfg = dict(GRAIN, spectrum=True)
    want, gains, shape = sref.paste(orig, edit, grey, D, R, cfg, (40, 30), seamless=sm)
    print(f"seamless {seamless is not None}: shape {shape.ravel()}, gains {gains.ravel()}")
    assert (gains > 0).all() and shape[0, 0] > 8 and shape[0, 1] > 64           # the scene's softness and shared part were seen
    got = pb.paste(od, ed, gd, D, R, grain=cfg, origin=(40, 30), **kw).cpu().numpy()
    assert np.array_equal(got, want)
    outside = ref.dilate(grey, D + 3 * R) == 0
    plain = pb.paste(od, ed, gd, D, R, **kw).cpu().numpy()
    white = pb.paste(od, ed, gd, D, R, grain=GRAIN, origin=(40, 30), **kw).cpu().numpy()
    assert outside.any() and np.array_equal(got[outside], orig[outside]) and np.array_equal(got[outside], plain[outside])
    assert not np.array_equal(got, plain) and not np.array_equal(got, white)    # the key does something, and something else than white grain
    off = pb.paste(od, ed, gd, D, R, grain=dict(GRAIN, spectrum=dict(max_blur=0, luma=False)), origin=(40, 30), **kw).cpu().numpy()
    assert np.array_equal(off, white)                                           # no blur, no sharing: grain=... without the sub-key
    assert np.array_equal(off, gref.paste(orig, edit, grey, D, R, GRAIN, (40, 30), seamless=sm)[0])
    assert np.array_equal(od.cpu().numpy(), orig)                               # the inputs are untouched


def _drawn(length, thickness, deg, centre, size):
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    pts = [np.array(centre) + su * u * length / 2 + sv * v * thickness / 2 for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    im = Image.new("L", size, 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in pts], fill=255)
    return np.array(im)


def test_paste_of_a_rectified_line_is_the_restatement(ops):
    """test_grain_gpu.py's rectified case: a window at the image's corner, so part of the ring has no coverage and is left out."""
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    slant = _drawn(140, 20, 25, (80, 60), (240, 160))
    rect = rc.select_rect(rc.mask_points(slant), D, R, pad=0.0, min_side=96)
    x0, y0, x1, y1 = rc.rect_window(rect, (240, 160))
    back = rc.matrices(rect, (x0, y0))[1]
    orig = _soft_scene((y1 - y0, x1 - x0), (x0, y0))[1]
    edit = np.full((1, rect.rh - 9, rect.rw + 14, 3), 131, np.uint8)
    grey = slant[None, y0:y1, x0:x1]
    warped = rref.warp_affine(ref.resize(edit, (rect.rh, rect.rw)), back, orig.shape[1:3], coverage=True)
    cfg = dict(ring=24, min_pixels=64, seed=9, spectrum=dict(max_blur=48))
    want, gains, shape = sref.paste(orig, edit, grey, D, R, cfg, (x0, y0), warped=warped)
    print(f"shape {shape.ravel()}, gains {gains.ravel()}")
    assert (gains > 0).all() and 0 < shape[0, 0] <= 48
    od, ed, gd = _dev(orig, edit, grey)
    got = pb.paste(od, ed, gd, D, R, rect=rect, origin=(x0, y0), grain=cfg).cpu().numpy()
    assert np.array_equal(got, want)
    outside = ref.dilate(grey, D + 3 * R) == 0
    plain = pb.paste(od, ed, gd, D, R, rect=rect, origin=(x0, y0)).cpu().numpy()
    assert outside.any() and np.array_equal(got[outside], orig[outside]) and not np.array_equal(got, plain)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_carry_a_message_and_launch_nothing(ops):
    img = torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device="cuda")
    m = torch.full((2, 4, 6), 9, dtype=torch.uint8, device="cuda")
    g = np.zeros((2, 3), np.int32)
    for bad in (dict(img=img.float()), dict(sel=m[:1]), dict(step=0), dict(step=9), dict(img=img[:, :, ::2])):
        with pytest.raises(ValueError, match="highpass_hist_step: "):
            ops.highpass_hist_step(**dict(dict(img=img, sel=m), **bad))
    for bad in (dict(alpha=m[:, :2]), dict(gain=g + 2 ** 18 + 1), dict(gain=g - 1), dict(shape=(65, 0)), dict(shape=(0, 257)), dict(out=img[:1])):
        with pytest.raises(ValueError, match="grain_shaped: "):
            ops.grain_shaped(**dict(dict(img=img, alpha=m, gain=g, shape=(0, 0)), **bad))
    one = torch.zeros(2, 4, 6, 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="alias img only"):
        ops.grain_shaped(one, m, np.full((2, 1), 2 ** 18, np.int32), (64, 256), out=m.view(2, 4, 6, 1))      # out aliasing alpha: the library's
    torch.cuda.synchronize()
    assert int(m.min()) == int(m.max()) == 9                                                               # ... before anything was written
