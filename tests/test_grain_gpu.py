"""Grain match on the GPU (DESIGN.md section 4 "Grain match"): ops.highpass_hist and ops.grain (imageops.hip: highpass_hist_kernel,
grain_u8_kernel) and paste_back.paste(grain=...) against the numpy restatement in tests/helpers/grain_ref.py, bit for bit (integer
arithmetic only; the host arithmetic is float64 on exact integers)."""
import itertools
import math

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from tests.helpers import grain_ref as gref
from tests.helpers import paste_back_ref as ref
from tests.helpers import rectify_ref as rref

pytestmark = pytest.mark.gpu
# a single pixel; a few pixels in two samples; widths that are no multiple of 4 or 64 with several workgroups; one channel in three
# samples; four channels in one long row.  LARGE: more pixels than the histogram's 256 workgroups and more bytes than the grain's 4096
# cover in one step, so both kernels go round their grid-stride loops.
SHAPES = ((1, 1, 1, 3), (2, 3, 5, 3), (1, 35, 67, 3), (3, 16, 130, 1), (1, 5, 259, 4))
LARGE = (1, 600, 601, 3)
RANGES = ((255, 255), (1, 255), (0, 0))
ORIGINS = ((0, 0), (17, 5), (2 ** 30 - 3, 2 ** 30 - 7))


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def _dev(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays)


def _images(rng, shape):
    b, h, w, c = shape
    y, x = np.mgrid[:h, :w]
    board = np.where((y + x) % 2 == 0, 255, 0).astype(np.uint8)[None, :, :, None]
    return dict(random=rng.integers(0, 256, shape, dtype=np.uint8), zeros=np.zeros(shape, np.uint8), ones=np.full(shape, 255, np.uint8),
                board=np.ascontiguousarray(np.broadcast_to(board, shape)))


def _sels(rng, shape):
    """all selected / none selected under (255, 255), and random bytes with 0 and 255 frequent enough for every range to select some."""
    b, h, w, _ = shape
    r = rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    pick = rng.random((b, h, w))
    r[pick < 0.3], r[pick > 0.7] = 0, 255
    return dict(all=np.full((b, h, w), 255, np.uint8), none=np.zeros((b, h, w), np.uint8), random=r)


# ---------------------------------------------------------------------------------------------- ops.highpass_hist
@pytest.mark.parametrize("shape", SHAPES)
def test_highpass_hist_is_the_restatement_exactly(ops, shape):
    rng = np.random.default_rng(sum(shape))
    b, h, w, c = shape
    out = torch.full((b, c, 1024), 7, dtype=torch.int32, device="cuda")          # stale contents: the call zeroes it itself
    for (iname, img), (sname, sel) in itertools.product(_images(rng, shape).items(), _sels(rng, shape).items()):
        idev, sdev = _dev(img, sel)
        for lo, hi in RANGES:
            want = gref.highpass_hist(img, sel, lo, hi)
            got = ops.highpass_hist(idev, sdev, lo, hi)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (iname, sname, lo, hi)
            n = ((sel >= lo) & (sel <= hi)).sum(axis=(1, 2))
            assert np.array_equal(got.sum(-1).cpu().numpy(), np.broadcast_to(n[:, None], (b, c)))
            again = ops.highpass_hist(idev, sdev, lo, hi, out=out)                # a second call into the same buffer
            assert again.data_ptr() == out.data_ptr() and torch.equal(out, got)
            if iname == "board" and sname == "all" and (lo, hi) == (255, 255):
                assert (want[:, :, 1023] == h * w).all() or h * w == 1           # the checkerboard saturates the last bin
            if sname == "none" and (lo, hi) != (0, 0):
                assert int(got.abs().sum()) == 0                                  # nothing selected: all zeros


def test_both_kernels_on_a_window_beyond_one_grid_step(ops):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, LARGE, dtype=np.uint8)
    sel = np.where(rng.random(LARGE[:3]) < 0.5, 255, 0).astype(np.uint8)
    alpha = rng.integers(0, 256, LARGE[:3], dtype=np.uint8)
    idev, sdev, adev = _dev(img, sel, alpha)
    assert np.array_equal(ops.highpass_hist(idev, sdev).cpu().numpy(), gref.highpass_hist(img, sel))
    gains = np.array([[65536, 3000, 0]], np.int32)
    assert np.array_equal(ops.grain(idev, adev, gains, (17, 5), 11).cpu().numpy(), gref.grain(img, alpha, gains, (17, 5), 11))


# ---------------------------------------------------------------------------------------------- ops.grain
@pytest.mark.parametrize("shape", SHAPES)
def test_grain_is_the_restatement_exactly(ops, shape):
    rng = np.random.default_rng(100 + sum(shape))
    b, h, w, c = shape
    imgs = _images(rng, shape)
    alphas = dict(random=rng.integers(0, 256, (b, h, w), dtype=np.uint8), zero=np.zeros((b, h, w), np.uint8), full=np.full((b, h, w), 255, np.uint8))
    gains = dict(zero=np.zeros((b, c), np.int32), middle=np.full((b, c), 2661, np.int32), one=np.full((b, c), 65536, np.int32),
                 mixed=rng.choice(np.array([0, 1, 2661, 40000, 65536], np.int32), (b, c)))
    for iname in ("random", "zeros", "ones"):
        img = imgs[iname]
        idev = _dev(img)[0]
        for (aname, alpha), (gname, gain), origin in itertools.product(alphas.items(), gains.items(), ORIGINS):
            if iname != "random" and origin != ORIGINS[1]:
                continue                                                          # the constant images are about the clamp: one origin
            adev = _dev(alpha)[0]
            want = gref.grain(img, alpha, gain, origin, 7)
            got = ops.grain(idev, adev, gain, origin, 7)
            assert np.array_equal(got.cpu().numpy(), want), (iname, aname, gname, origin)
            assert np.array_equal(idev.cpu().numpy(), img)                        # out of place: the input is untouched
            assert np.array_equal(want[alpha == 0], img[alpha == 0])
            if gname == "zero" or aname == "zero":
                assert np.array_equal(want, img)
            if origin == ORIGINS[1]:                                              # in place
                work = idev.clone()
                same = ops.grain(work, adev, torch.from_numpy(gain).cuda(), torch.tensor([list(origin)] * b), 7, out=work)
                assert same.data_ptr() == work.data_ptr() and np.array_equal(work.cpu().numpy(), want)
    full = alphas["full"]
    if h * w > 64:
        lo, hi = gref.grain(imgs["zeros"], full, gains["one"], ORIGINS[1], 7), gref.grain(imgs["ones"], full, gains["one"], ORIGINS[1], 7)
        assert lo.min() == 0 and lo.max() > 100 and hi.max() == 255 and hi.min() < 155      # the clamp was at work in what was compared above
        assert not np.array_equal(gref.grain(imgs["random"], full, gains["middle"], (0, 0), 7), gref.grain(imgs["random"], full, gains["middle"], (0, 0), 8))
    # no origin is origin (0, 0); a seed is taken modulo 2^32; per-sample origins
    idev, adev = _dev(imgs["random"], alphas["random"])
    assert torch.equal(ops.grain(idev, adev, gains["mixed"]), ops.grain(idev, adev, gains["mixed"], (0, 0), 0))
    assert torch.equal(ops.grain(idev, adev, gains["one"], None, 2 ** 32 + 5), ops.grain(idev, adev, gains["one"], None, 5))
    per = np.array([[40 * s, 9 + s] for s in range(b)])
    assert np.array_equal(ops.grain(idev, adev, gains["one"], per, 3).cpu().numpy(), gref.grain(imgs["random"], alphas["random"], gains["one"], per, 3))


def test_the_grain_of_a_scene_pixel_does_not_depend_on_the_window(ops):
    rng = np.random.default_rng(8)
    scene = rng.integers(60, 200, (1, 70, 90, 3), dtype=np.uint8)
    alpha = rng.integers(1, 256, (1, 70, 90), dtype=np.uint8)
    gains = np.array([[30000, 9000, 65536]], np.int32)
    big = ops.grain(*_dev(scene[:, 20:50, 30:70], alpha[:, 20:50, 30:70]), gains, (1030, 2020), 4)
    small = ops.grain(*_dev(scene[:, 30:38, 40:50], alpha[:, 30:38, 40:50]), gains, (1040, 2030), 4)
    assert torch.equal(big[:, 10:18, 10:20], small) and not torch.equal(small.cpu(), torch.from_numpy(scene[:, 30:38, 40:50]))


# ---------------------------------------------------------------------------------------------- paste(grain=...)
D, R = 8, 2
HW = (96, 160)
GRAIN = dict(ring=12, seed=3, min_pixels=64)


def _noisy_scene(hw, origin, sigma=4.0):
    """A colour ramp plus the restatement's grain of standard deviation sigma: a photo with sensor noise."""
    h, w = hw
    ramp = np.linspace(70, 170, w)[None, None, :, None] + np.array([0.0, 8.0, -12.0])
    flat = np.broadcast_to(np.floor(ramp + 0.5), (1, h, w, 3)).astype(np.uint8)
    gain = np.full((1, 3), math.floor(sigma / gref.SIGMA0 * 65536 + 0.5))
    return flat, gref.grain(flat, np.full((1, h, w), 255, np.uint8), gain, origin, 21)


@pytest.fixture(scope="module")
def plain_case():
    """orig (noisy), edit (the clean ramp, slightly off in colour, at another size), grey, and cref: the ORIGINAL region, another noisy image."""
    clean, orig = _noisy_scene(HW, (40, 30))
    cref = _noisy_scene(HW, (40, 30), 5.0)[1]
    edit = ref.resize(np.clip(clean.astype(np.int64) + 6, 0, 255).astype(np.uint8), (80, 132))
    grey = np.zeros((1,) + HW, np.uint8)
    grey[0, 36:60, 50:110] = 255
    for a in (orig, cref, edit, grey):
        a.setflags(write=False)
    return orig, cref, edit, grey


@pytest.mark.parametrize("seamless", [None, dict(smooth=3, max_shift=12)])
@pytest.mark.parametrize("color", [None, dict(ring=20, min_pixels=16)])
def test_paste_of_a_plain_line_is_the_restatement(ops, plain_case, color, seamless):
    from textflux_amd import paste_back as pb
    orig, cref, edit, grey = plain_case
    cm = None if color is None else pb.color_match_cfg(color)
    sm = None if seamless is None else pb.seamless_cfg(seamless)
    od, ed, gd, cd = _dev(orig, edit, grey, cref)
    kw = dict({} if color is None else dict(color_match=color), **({} if seamless is None else dict(seamless=seamless)))
    outside = ref.dilate(grey, D + 3 * R) == 0
    for color_ref, cr_dev in ((None, None), (cref, cd)):
        want, gains = gref.paste(orig, edit, grey, D, R, GRAIN, (40, 30), seamless=sm, color_match=cm, color_ref=color_ref)
        print(f"color {color is not None}, seamless {seamless is not None}, color_ref {color_ref is not None}: gains {gains.ravel()}")
        assert (gains > 0).all()
        got = pb.paste(od, ed, gd, D, R, grain=GRAIN, origin=(40, 30), color_ref=cr_dev, **kw).cpu().numpy()
        assert np.array_equal(got, want)
        plain_kw = dict(kw, color_ref=cr_dev) if (color is not None or seamless is not None) else kw       # without any key color_ref is refused, as before
        plain = pb.paste(od, ed, gd, D, R, **plain_kw).cpu().numpy()
        assert outside.any() and np.array_equal(got[outside], plain[outside]) and np.array_equal(got[outside], orig[outside])
        assert not np.array_equal(got, plain)                                    # the key does something
        still = pb.paste(od, ed, gd, D, R, grain=dict(GRAIN, strength=0), origin=(40, 30), color_ref=cr_dev, **kw).cpu().numpy()
        assert np.array_equal(still, plain)                                      # strength 0: the call without the key, everywhere
        assert np.array_equal(od.cpu().numpy(), orig)                            # the inputs are untouched
    moved = pb.paste(od, ed, gd, D, R, grain=GRAIN, origin=(41, 30), **kw).cpu().numpy()
    assert not np.array_equal(moved, pb.paste(od, ed, gd, D, R, grain=GRAIN, origin=(40, 30), **kw).cpu().numpy())     # scene-anchored


def _drawn(length, thickness, deg, centre, size):
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    pts = [np.array(centre) + su * u * length / 2 + sv * v * thickness / 2 for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    im = Image.new("L", size, 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in pts], fill=255)
    return np.array(im)


@pytest.mark.parametrize("seamless", [None, dict(smooth=4)])
def test_paste_of_a_rectified_line_is_the_restatement(ops, seamless):
    """A window at the image's corner: the rectangle sticks out of it, so part of the ring has no coverage and is left out."""
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    slant = _drawn(140, 20, 25, (80, 60), (240, 160))
    rect = rc.select_rect(rc.mask_points(slant), D, R, pad=0.0, min_side=96)
    x0, y0, x1, y1 = rc.rect_window(rect, (240, 160))
    back = rc.matrices(rect, (x0, y0))[1]
    orig = _noisy_scene((y1 - y0, x1 - x0), (x0, y0))[1]
    edit = np.full((1, rect.rh - 9, rect.rw + 14, 3), 131, np.uint8)
    grey = slant[None, y0:y1, x0:x1]
    warped = rref.warp_affine(ref.resize(edit, (rect.rh, rect.rw)), back, orig.shape[1:3], coverage=True)
    cfg = dict(ring=24, min_pixels=64, seed=9)
    sm = None if seamless is None else pb.seamless_cfg(seamless)
    want, gains = gref.paste(orig, edit, grey, D, R, cfg, (x0, y0), seamless=sm, warped=warped)
    assert (gains > 0).all()
    uncut = gref.paste(orig, edit, grey, D, R, cfg, (x0, y0), seamless=sm, warped=(warped[0], None))[0]
    od, ed, gd = _dev(orig, edit, grey)
    kw = {} if seamless is None else dict(seamless=seamless)
    got = pb.paste(od, ed, gd, D, R, rect=rect, origin=(x0, y0), grain=cfg, **kw).cpu().numpy()
    assert np.array_equal(got, want)
    assert not np.array_equal(want, uncut)                                       # leaving the coverage out of the ring would show
    outside = ref.dilate(grey, D + 3 * R) == 0
    plain = pb.paste(od, ed, gd, D, R, rect=rect, origin=(x0, y0), **kw).cpu().numpy()
    assert outside.any() and np.array_equal(got[outside], orig[outside]) and not np.array_equal(got, plain)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_carry_a_message_and_launch_nothing(ops):
    img = torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device="cuda")
    m = torch.zeros(2, 4, 6, dtype=torch.uint8, device="cuda")
    g = np.zeros((2, 3), np.int32)
    five = torch.zeros(2, 4, 6, 5, dtype=torch.uint8, device="cuda")
    for bad in (dict(img=img.float()), dict(sel=m.int()), dict(sel=m[:1]), dict(img=five), dict(img=img[:, :, ::2])):
        with pytest.raises(ValueError, match="highpass_hist: "):
            ops.highpass_hist(**dict(dict(img=img, sel=m), **bad))
    for bad in (dict(img=img.float()), dict(alpha=m.int()), dict(alpha=m[:, :2]), dict(img=five, gain=np.zeros((2, 5), np.int32)), dict(gain=g - 1),
                dict(gain=g + 65537), dict(gain=torch.full((2, 3), 70000, device="cuda")), dict(out=img[:1])):
        with pytest.raises(ValueError, match="grain: "):
            ops.grain(**dict(dict(img=img, alpha=m, gain=g), **bad))
    one = torch.zeros(2, 4, 6, 1, dtype=torch.uint8, device="cuda")
    a1 = torch.full((2, 4, 6), 9, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="alias img only"):
        ops.grain(one, a1, np.full((2, 1), 65536, np.int32), out=a1.view(2, 4, 6, 1))      # out aliasing alpha: refused by the library
    torch.cuda.synchronize()
    assert int(a1.min()) == int(a1.max()) == 9                                             # ... before anything was written
    store = torch.zeros(2, 1, 1024, dtype=torch.int32, device="cuda")                      # an image that starts at the histogram's first byte
    inside = store.view(torch.uint8).view(-1)[:48].view(2, 4, 6, 1)
    with pytest.raises(RuntimeError, match="alias neither img nor sel"):
        ops.highpass_hist(inside, a1, out=store)
