"""Seamless paste on the GPU (DESIGN.md section 4 "Seamless paste"): ops.seamless_overlay (imageops.hip: the seam_* kernels) and
paste_back.paste(seamless=...) against the numpy restatement in tests/helpers/seamless_ref.py, bit for bit (integer arithmetic only),
and batch_driver.run_items(per_line=True, seamless=...) end to end on the tiny synthetic checkpoint of the e2e tests."""
import itertools
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from tests.helpers import paste_back_ref as ref
from tests.helpers import rectify_ref as rref
from tests.helpers import seamless_ref as sref

pytestmark = pytest.mark.gpu
# 1 x 1 and 1 x 17 (the whole pyramid inside the one-workgroup kernel; one row); 37 x 53 (odd sides at every level, several workgroups,
# one per-level pull and push around that kernel) and 64 x 64 (the same with even sides); 96 x 301 (three per-level launches on either
# side, a width that is no multiple of the workgroup)
SHAPES = ((1, 1), (1, 17), (37, 53), (64, 64), (96, 301))
SMOOTHS = (0, 1, 2, 5)                                # both parities of the ping-pong


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def _case(h, w, c, seed, b=2):
    """orig, ref, edit u8 [b, h, w, c]; alpha, covered u8 [b, h, w]; lut u8 [b, c, 256].  Every sample has another support: an ellipse
    with a feathered rim, then an off-centre box that touches two window edges; covered drops a band and some scattered pixels."""
    rng = np.random.default_rng(seed)
    orig, rf, edit = (rng.integers(0, 256, (b, h, w, c), dtype=np.uint8) for _ in range(3))
    y, x = np.mgrid[:h, :w]
    alpha = np.zeros((b, h, w), np.uint8)
    for s in range(b):
        if h * w < 64:
            alpha[s] = np.where(rng.random((h, w)) < 0.45, rng.integers(1, 256, (h, w)), 0)
        elif s % 2 == 0:
            rr = ((y - h / 2) / (h / 3)) ** 2 + ((x - w / 2) / (w / 3)) ** 2
            alpha[s] = np.clip((1.2 - rr) * 600, 0, 255)
        else:
            alpha[s, h // 2:, : 2 * w // 3] = rng.integers(1, 256, (h - h // 2, 2 * w // 3))
    covered = np.where(rng.random((b, h, w)) < 0.9, 255, 0).astype(np.uint8)
    covered[:, :, : w // 5] = 0
    lut = np.clip(np.arange(256)[None, None] + rng.integers(-20, 21, (b, c, 256)), 0, 255).astype(np.uint8)
    return orig, rf, edit, alpha, covered, lut


def _dev(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _check(ops, orig, rf, edit, alpha, covered, lut, smooth, max_shift=32):
    want = sref.seamless_overlay(orig, rf, edit, alpha, covered, lut, smooth, max_shift)
    od, rd, ed, ad, cd, ld = _dev(orig, rf, edit, alpha, covered, lut)
    got = ops.seamless_overlay(od, od if rf is orig else rd, ed, ad, covered=cd, lut=ld, smooth=smooth, max_shift=max_shift)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(od.cpu(), torch.from_numpy(orig))                            # the inputs are untouched
    return want


@pytest.mark.parametrize("c", [3, 1, 4])
@pytest.mark.parametrize("hw", SHAPES)
def test_kernels_are_the_restatement_exactly(ops, hw, c):
    orig, rf, edit, alpha, covered, lut = _case(*hw, c, 1000 * hw[0] + 10 * hw[1] + c)
    seen = set()
    for smooth, with_cov, with_lut, own_ref in itertools.product(SMOOTHS, (False, True), (False, True), (False, True)):
        want = _check(ops, orig, rf if own_ref else orig, edit, alpha, covered if with_cov else None, lut if with_lut else None, smooth)
        seen.add(want.tobytes())
    if hw[0] * hw[1] > 64:
        assert len(seen) == 32                        # every axis changes the result: none of them is ignored
        assert not np.array_equal(sref.seamless_overlay(orig[:1], rf[:1], edit[:1], alpha[:1]), sref.seamless_overlay(orig[1:], rf[1:], edit[1:], alpha[1:]))


def test_one_large_window(ops):
    """256 x 1024, the per-line strip: five levels of per-level launches on either side of the one-workgroup kernel."""
    orig, rf, edit, alpha, covered, lut = _case(256, 1024, 3, 7)
    _check(ops, orig, rf, edit, alpha, covered, lut, 5)


def test_out_may_be_orig(ops):
    orig, rf, edit, alpha, covered, lut = _case(37, 53, 3, 21)
    want = sref.seamless_overlay(orig, orig, edit, alpha, covered, lut, 3, 32)
    od, ed, ad, cd, ld = _dev(orig, edit, alpha, covered, lut)
    same = ops.seamless_overlay(od, od, ed, ad, covered=cd, lut=ld, smooth=3, out=od)      # ref is orig as well
    assert same.data_ptr() == od.data_ptr() and torch.equal(od.cpu(), torch.from_numpy(want))
    for bad in (ed, ad):
        with pytest.raises((RuntimeError, ValueError)):
            ops.seamless_overlay(od, od, ed, ad, out=bad)


@pytest.mark.parametrize("hw", [(37, 53), (96, 301)])
def test_degenerate_supports(ops, hw):
    orig, rf, edit, alpha, covered, lut = _case(*hw, 3, 33)
    od, ed, ld = _dev(orig, edit, lut)
    # everything known: alpha == 0 everywhere gives the original bytes
    zero = np.zeros_like(alpha)
    assert np.array_equal(_check(ops, orig, rf, edit, zero, None, lut, 2), orig)
    # nothing known: alpha > 0 everywhere (or nothing covered) gives today's overlay
    full = np.maximum(alpha, 1)
    want = _check(ops, orig, rf, edit, full, None, lut, 2)
    assert torch.equal(ops.overlay_lut(od, ed, _dev(full)[0], ld).cpu(), torch.from_numpy(want))
    want = _check(ops, orig, rf, edit, alpha, np.zeros_like(covered), None, 2)
    assert torch.equal(ops.overlay(od, ed, _dev(alpha)[0]).cpu(), torch.from_numpy(want))
    # a support that touches all four window edges: a cross through the middle, known corners
    h, w = hw
    cross = np.zeros_like(alpha)
    cross[:, h // 3: 2 * h // 3, :] = 200
    cross[:, :, w // 3: 2 * w // 3] = 255
    for smooth in SMOOTHS:
        want = _check(ops, orig, rf, edit, cross, None, None, smooth)
    assert not np.array_equal(want, ref.overlay(orig, edit, cross)) and np.array_equal(want[cross == 0], orig[cross == 0])


@pytest.mark.parametrize("hw", [(37, 53), (64, 64)])
def test_max_shift_zero_is_the_overlay_bit_for_bit(ops, hw):
    orig, rf, edit, alpha, covered, lut = _case(*hw, 3, 5)
    od, rd, ed, ad, cd, ld = _dev(orig, rf, edit, alpha, covered, lut)
    for smooth in (0, 3):
        assert torch.equal(ops.seamless_overlay(od, rd, ed, ad, covered=cd, lut=ld, smooth=smooth, max_shift=0), ops.overlay_lut(od, ed, ad, ld))
        assert torch.equal(ops.seamless_overlay(od, rd, ed, ad, smooth=smooth, max_shift=0), ops.overlay(od, ed, ad))


def test_a_constant_drift_is_removed(ops):
    """edit = scene - 9: the seamless paste returns the scene, the plain paste keeps the step."""
    rng = np.random.default_rng(3)
    scene = rng.integers(40, 216, (1, 96, 131, 3), dtype=np.uint8)
    edit = scene - 9
    grey = np.zeros((1, 96, 131), np.uint8)
    grey[0, 40:56, 50:90] = 255
    alpha = ref.alpha_mask(grey, 8, 2)
    sd, ed, ad = _dev(scene, edit, alpha)
    assert torch.equal(ops.seamless_overlay(sd, sd, ed, ad), sd) and not torch.equal(ops.overlay(sd, ed, ad), sd)


# ---------------------------------------------------------------------------------------------- paste(seamless=...)
D, R = 8, 2
REGION = dict(pad=0.0, min_side=96)


@pytest.mark.parametrize("color", [None, dict(ring=20, min_pixels=16)])
@pytest.mark.parametrize("seamless", [True, dict(smooth=3, max_shift=12)])
def test_paste_of_a_plain_line_is_the_restatement(ops, seamless, color):
    from textflux_amd import paste_back as pb
    rng = np.random.default_rng(9)
    orig = rng.integers(40, 216, (1, 96, 131, 3), dtype=np.uint8)
    cref = np.clip(orig.astype(np.int64) + rng.integers(-6, 7, orig.shape), 0, 255).astype(np.uint8)      # the ORIGINAL region: another image
    ramp = np.linspace(-14, 14, 131)[None, None, :, None]
    edit_full = np.clip(np.floor(0.9 * cref + 12 + ramp + 0.5), 0, 255).astype(np.uint8)
    edit = ref.resize(edit_full, (80, 110))                                      # another size: resampled back first
    grey = np.zeros((1, 96, 131), np.uint8)
    grey[0, 40:56, 50:90] = 255
    cm = None if color is None else pb.color_match_cfg(color)
    sm = pb.seamless_cfg(seamless)
    od, ed, gd, cd = _dev(orig, edit, grey, cref)
    for color_ref, cr_dev in ((None, None), (cref, cd)):
        want = sref.paste(orig, edit, grey, D, R, seamless=sm, color_match=cm, color_ref=color_ref)
        kw = {} if color is None else dict(color_match=color)
        got = pb.paste(od, ed, gd, D, R, seamless=seamless, color_ref=cr_dev, **kw).cpu().numpy()
        assert np.array_equal(got, want)
        outside = ref.dilate(grey, D + 3 * R) == 0
        assert (got[outside] == orig[outside]).all() and (got[~outside] != orig[~outside]).any()
        plain = pb.paste(od, ed, gd, D, R, **(dict(kw, color_ref=cr_dev) if color is not None else {})).cpu().numpy()
        assert not np.array_equal(got, plain)                                    # the key does something


def _drawn(length, thickness, deg, centre, size):
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    pts = [np.array(centre) + su * u * length / 2 + sv * v * thickness / 2 for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    im = Image.new("L", size, 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in pts], fill=255)
    return np.array(im)


@pytest.mark.parametrize("color", [None, dict(ring=40, min_pixels=16)])
def test_paste_of_a_rectified_line_is_the_restatement(ops, color):
    """A window at the image's corner: the rectangle sticks out of it, so part of the window has no coverage and is not known."""
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    rng = np.random.default_rng(5)
    slant = _drawn(140, 20, 25, (80, 60), (240, 160))
    rect = rc.select_rect(rc.mask_points(slant), D, R, **REGION)
    x0, y0, x1, y1 = rc.rect_window(rect, (240, 160))
    back = rc.matrices(rect, (x0, y0))[1]
    orig = rng.integers(40, 216, (1, y1 - y0, x1 - x0, 3), dtype=np.uint8)
    edit = rng.integers(0, 256, (1, rect.rh - 9, rect.rw + 14, 3), dtype=np.uint8)
    grey = slant[None, y0:y1, x0:x1]
    cm = None if color is None else pb.color_match_cfg(color)
    warped = rref.warp_affine(ref.resize(edit, (rect.rh, rect.rw)), back, orig.shape[1:3], coverage=True)
    alpha = ref.alpha_mask(grey, D, R)
    assert ((alpha == 0) & (warped[1] == 0)).any() and ((alpha == 0) & (warped[1] != 0)).any()       # both kinds of alpha == 0 pixels
    want = sref.paste(orig, edit, grey, D, R, seamless=dict(smooth=4), color_match=cm, warped=warped)
    if color is None:                                                            # ... and leaving the coverage out would show
        assert not np.array_equal(want, sref.seamless_overlay(orig, orig, warped[0], alpha, None, None, 4, 32))
    od, ed, gd = _dev(orig, edit, grey)
    got = pb.paste(od, ed, gd, D, R, rect=rect, origin=(x0, y0), seamless=dict(smooth=4), **({} if color is None else dict(color_match=color)))
    assert np.array_equal(got.cpu().numpy(), want)
    outside = ref.dilate(grey, D + 3 * R) == 0
    assert outside.any() and (want[outside] == orig[outside]).all()


# ---------------------------------------------------------------------------------------------- end to end, through run_items
@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_seamless"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def test_end_to_end_two_lines(pipe):
    from textflux_amd import batch_driver, glyph
    from textflux_amd import paste_back as pb
    from textflux_amd import per_line as pl
    scene, mask, words = glyph.synthetic_case(384, 256, multiline=True)
    item = dict(image=scene, mask=mask, text="\n".join(words))
    sc = np.array(scene)
    lines = pl.split_lines(mask, words)
    assert len(lines) == 2
    grown = np.zeros(sc.shape[:2], bool)
    for _, _, lm in lines:
        grown |= ref.dilate(np.where(lm[:, :, 0] >= 128, 255, 0).astype(np.uint8), D + 3 * R) > 0
    outs = {}
    for name, sm in (("plain", None), ("seamless", dict(smooth=4))):
        saved, pastes = {}, []
        real = pipe.paste_back
        pipe.paste_back = lambda o_, e, m, **k: (pastes.append(dict(k, original=np.array(o_), edited=np.array(e), mask=np.array(m))), real(o_, e, m, **k))[1]
        try:
            cfg = dict(per_line=True, dilate=D, feather=R, region=REGION, **({} if sm is None else dict(seamless=sm)))
            res = batch_driver.run_items([item], pipe, None, batch_size=2, num_inference_steps=2, guidance_scale=30.0, seed=42,
                                         loader=lambda x: x, save=lambda i, im: saved.__setitem__(i, np.array(im)), paste_back=cfg)
        finally:
            del pipe.paste_back
        assert res["all_done"] == [0] and not res["failed"] and len(pastes) == 2
        assert all(("seamless" in k) == (sm is not None) and ("color_ref" in k) == (sm is not None) for k in pastes)
        out = outs[name] = saved[0]
        assert out.shape == sc.shape and (out[~grown] == sc[~grown]).all()        # bytes outside the grown masks are the original's
        # the restated composition of what the pipeline was handed, line by line
        want = sc.copy()
        works = pl.prepare_lines(0, item, lambda x: x, False, None, batch_driver._paste_back_cfg(cfg))
        for w, k in zip(works, pastes):
            reg = w.region
            assert np.array_equal(k["original"], want[reg.y0:reg.y1, reg.x0:reg.x1])
            if sm is None:                                                       # without the key: the plain paste, as before
                pasted = ref.paste(k["original"][None], k["edited"][None], k["mask"][None], D, R)
            else:
                assert k["seamless"] == pb.seamless_cfg(sm) and np.array_equal(k["color_ref"], sc[reg.y0:reg.y1, reg.x0:reg.x1])
                pasted = sref.paste(k["original"][None], k["edited"][None], k["mask"][None], D, R, seamless=k["seamless"], color_ref=k["color_ref"][None])
            want[reg.y0:reg.y1, reg.x0:reg.x1] = pasted[0]
        assert np.array_equal(out, want)
    assert not np.array_equal(outs["plain"], outs["seamless"])
