"""Rectified per-line edits without a GPU: the frame of a slanted line against drawn rectangles, the oriented rectangle, the numpy
restatement of the device warp against known answers, the batch driver around a stub pipeline whose warp IS the restatement, the
refusals, the CLI flags and the new C entry point (exported, bound, refusing bad arguments on the host)."""
import importlib
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from tests.helpers import rectify_ref as rref
from textflux_amd import batch_driver as bd
from textflux_amd import glyph
from textflux_amd import paste_back as pb
from textflux_amd import per_line as pl
from textflux_amd import rectify as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 1 << 16


def drawn(length, thickness, deg, centre=(256, 256), size=(512, 512)):
    """uint8 [H, W] mask: a length x thickness rectangle around `centre` whose long side points along (cos deg, sin deg), y down."""
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    pts = [np.array(centre) + su * u * length / 2 + sv * v * thickness / 2 for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    im = Image.new("L", size, 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in pts], fill=255)
    return np.array(im)


# ---------------------------------------------------------------------------------------------- the frame and the rule
@pytest.mark.parametrize("deg", [30, -20, 0])
def test_line_frame_known_answers(deg):
    cx, cy, length, thickness, theta = rc.line_frame(rc.mask_points(drawn(300, 40, deg)))
    assert abs(theta - deg) <= 1.0
    assert abs(cx - 256) <= 2 and abs(cy - 256) <= 2 and abs(length - 300) <= 2 and abs(thickness - 40) <= 2


def test_which_lines_are_rectified():
    frame = lambda *a: rc.line_frame(rc.mask_points(drawn(*a)))
    assert rc.is_rectified(frame(300, 40, 30)) and rc.is_rectified(frame(300, 40, -20)) and rc.is_rectified(frame(300, 40, 25))
    for deg in (0, 3, 60):
        assert not rc.is_rectified(frame(300, 40, deg)), deg
    assert not rc.is_rectified(frame(100, 90, 25))                               # a blob: the aspect rule
    assert rc.is_rectified(frame(300, 40, 3), min_angle=2.0) and rc.is_rectified(frame(300, 40, 60), max_angle=70.0)
    assert rc.is_rectified(frame(100, 90, 25), min_aspect=1.0)
    cfg = bd._paste_back_cfg(dict(per_line=True, rectify=True))
    assert rc.plan(drawn(300, 40, 30), cfg) is not None and rc.plan(drawn(300, 40, 3), cfg) is None
    assert rc.plan(drawn(300, 40, 30), bd._paste_back_cfg(dict(per_line=True))) is None             # the key absent: nobody is rectified
    assert rc.plan(np.zeros((64, 64), np.uint8), cfg) is None                    # the empty mask is left to the region rule's refusal


@pytest.mark.parametrize("deg,pad", [(30, 0.5), (-20, 0.5), (45, 0.0), (25, 0.0), (-40, 0.1)])
def test_select_rect_contains_the_grown_mask(deg, pad):
    d, r, min_side = 16, 4, 96
    m = drawn(300, 40, deg)
    rect = rc.select_rect(rc.mask_points(m), d, r, pad=pad, min_side=min_side)
    assert isinstance(rect.rw, int) and isinstance(rect.rh, int) and rect.rw >= min_side and rect.rh >= min_side
    grown = ref.dilate(m, pb.halo(d, r))                                         # the square window of the paste, in the scene's axes
    ys, xs = np.nonzero(grown)
    c, s = math.cos(math.radians(rect.theta)), math.sin(math.radians(rect.theta))
    u, v = (xs - rect.cx) * c + (ys - rect.cy) * s, -(xs - rect.cx) * s + (ys - rect.cy) * c
    assert np.abs(u).max() <= rect.rw / 2 and np.abs(v).max() <= rect.rh / 2
    # ... and through the matrices: every one of those pixels is covered by the warp back into the whole scene
    _, back = rc.matrices(rect)
    X, Y = back[0] * xs + back[1] * ys + back[2], back[3] * xs + back[4] * ys + back[5]
    assert ((X >> 16) >= 0).all() and ((X >> 16) < rect.rw).all() and ((Y >> 16) >= 0).all() and ((Y >> 16) < rect.rh).all()


def test_select_rect_sizes_are_select_regions():
    """The editing size is the one select_region gives an axis-aligned line of the same extents (in an image large enough that nothing is
    shifted), below and above max_side."""
    for length, thickness, deg, kw in ((300, 40, 30, {}), (300, 40, -20, dict(max_side=512)), (700, 60, 25, {}), (120, 30, 10, {})):
        pts = rc.mask_points(drawn(length, thickness, deg, centre=(600, 600), size=(1200, 1200)))
        rect = rc.select_rect(pts, 16, 4, **kw)
        _, _, fl, ft, _ = rc.line_frame(pts)
        L, T = math.ceil(fl + 1 - 1e-6), math.ceil(ft + 1 - 1e-6)                # the pixels' own extent: a half-open box counts n, not n - 1
        flat = np.zeros((4000, 4000), np.uint8)
        flat[2000:2000 + T, 1500:1500 + L] = 255
        reg = pb.select_region(flat, 16, 4, **kw)
        assert (rect.rw, rect.rh, rect.tw, rect.th) == (reg.x1 - reg.x0, reg.y1 - reg.y0, reg.tw, reg.th)
    assert rc.select_rect(pts, 16, 4, max_side=200).tw == 200


def test_matrices_map_the_centre_pixel_onto_itself_and_invert_each_other():
    rect = rc.select_rect(rc.mask_points(drawn(300, 40, 25)), 16, 4, pad=0.0, min_side=96)
    x0, y0, x1, y1 = rc.rect_window(rect, (512, 512))
    assert 0 <= x0 < x1 <= 512 and 0 <= y0 < y1 <= 512
    fwd, back = rc.matrices(rect, (x0, y0))
    assert fwd.dtype == back.dtype == np.int64 and fwd.shape == back.shape == (6,)
    ic, jc = rect.rw // 2, rect.rh // 2
    X, Y = fwd[0] * ic + fwd[1] * jc + fwd[2], fwd[3] * ic + fwd[4] * jc + fwd[5]
    assert X % Q == 0 and Y % Q == 0                                             # exactly on a scene pixel ...
    px, py = X // Q - x0, Y // Q - y0
    assert (back[0] * px + back[1] * py + back[2], back[3] * px + back[4] * py + back[5]) == (ic * Q, jc * Q)      # ... which maps back exactly
    for i, j in ((0, 0), (rect.rw - 1, 0), (0, rect.rh - 1), (rect.rw - 1, rect.rh - 1)):          # the corners: to within a 20th of a pixel
        X, Y = (fwd[0] * i + fwd[1] * j + fwd[2]) / Q - x0, (fwd[3] * i + fwd[4] * j + fwd[5]) / Q - y0
        assert abs((back[0] * X + back[1] * Y + back[2]) / Q - i) < 0.05 and abs((back[3] * X + back[4] * Y + back[5]) / Q - j) < 0.05


# ---------------------------------------------------------------------------------------------- the restatement
def test_tap_table():
    t = rc.catmull_rom_taps()
    assert t.dtype == np.int16 and t.shape == (256, 4) and (t.astype(np.int64).sum(axis=1) == 1 << 14).all()
    assert t[0].tolist() == [0, 1 << 14, 0, 0] and t[128].tolist() == [-1024, 9216, 9216, -1024]   # t = 0: the pixel; t = 1/2: (-1, 9, 9, -1) / 16
    assert (t[1:][:, ::-1] == t[:0:-1]).all() or np.abs(t[1:][:, ::-1].astype(int) - t[:0:-1]).max() <= 1         # symmetric up to the rounding fix
    assert t is not rref.TAPS and (t == rref.TAPS).all()


def test_restatement_identity_and_quarter_turn():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    ident = np.array([Q, 0, 0, 0, Q, 0], np.int64)
    out, cov = rref.warp_affine(x, ident, (9, 13), coverage=True)
    assert (out == x).all() and (cov == 255).all()
    turn = np.array([0, -Q, 12 * Q, Q, 0, 0], np.int64)                          # destination (i, j) reads source (W - 1 - j, i)
    out = rref.warp_affine(x, turn, (13, 9))
    assert (out == np.rot90(x, axes=(1, 2))).all()
    # a shift by a whole pixel replicates the edge and reports it uncovered; per-sample matrices reach their own sample
    per = np.stack([ident, np.array([Q, 0, -Q, 0, Q, 0], np.int64)])
    out, cov = rref.warp_affine(x, per, (9, 13), coverage=True)
    assert (out[0] == x[0]).all() and (out[1][:, 1:] == x[1][:, :-1]).all() and (out[1][:, 0] == x[1][:, 0]).all()
    assert (cov[0] == 255).all() and (cov[1][:, 0] == 0).all() and (cov[1][:, 1:] == 255).all()
    flat = np.full((1, 7, 5, 1), 201, np.uint8)                                  # rows sum to one: a constant stays that constant anywhere
    assert (rref.warp_affine(flat, np.array([51234, -40000, -3 * Q + 77, 40000, 51234, 12345], np.int64), (20, 20)) == 201).all()


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("case", ["border", "thin"])
def test_the_three_restatements_agree_on_an_affine_map(case, c):
    """tests/test_rectify_gpu.py's identity of the three entry points, over the three numpy restatements: it keeps them honest."""
    from tests.helpers import curve_ref as cref
    from tests.helpers import perspective_ref as pref
    from tests.test_rectify_gpu import CASES, affine_three_ways
    (H, W), (h, w), ms = CASES[case]
    x = np.random.default_rng(H * W + c).integers(0, 256, (2, H, W, c), dtype=np.uint8)
    want, want_cov = rref.warp_affine(x, np.stack(ms), (h, w), coverage=True)
    if case == "border":
        assert (want_cov == 0).mean() > 0.3 and (want_cov == 255).any()
    restated = {"warp_affine": rref.warp_affine, "warp_perspective": pref.warp_perspective, "warp_grid": cref.warp_grid}
    for way, args in affine_three_ways(ms, (h, w)).items():
        got, cov = restated[way.split(",")[0]](x, *args, (h, w), coverage=True)
        assert np.array_equal(got, want) and np.array_equal(cov, want_cov), way


# ---------------------------------------------------------------------------------------------- the batch driver around a stub
T, J, P = 6, 8, 4
SCENE_WH, FLAT_BOX, SLANT = (512, 384), (60, 40, 220, 70), (180, 28, 25, (330, 250))       # the slanted line: length, thickness, degrees, centre
D, R = 8, 2
REGION = dict(pad=0.0, min_side=96)


def _scene():
    return np.random.default_rng(11).integers(0, 256, (SCENE_WH[1], SCENE_WH[0], 3), dtype=np.uint8)


def _line_masks():
    flat = np.zeros((SCENE_WH[1], SCENE_WH[0]), np.uint8)
    x0, y0, x1, y1 = FLAT_BOX
    flat[y0:y1, x0:x1] = 255
    return flat, drawn(SLANT[0], SLANT[1], SLANT[2], centre=SLANT[3], size=SCENE_WH)


def _loader(kind):
    if kind == "scene":
        return Image.fromarray(_scene())
    flat, slant = _line_masks()
    return Image.fromarray(flat | slant)


ITEMS = [dict(image="scene", mask="mask", text="LEVEL\nSLANT")]


class Stub:
    """A pipeline whose result is its input canvas inverted (so that what is pasted shows where it came from), whose warp is the
    restatement and whose paste is the restated paste; it records what it is handed."""

    def __init__(self):
        self.calls, self.encodes, self.pastes, self.warps, self.text_encoder_2 = [], [], [], [], object()

    def encode_prompt(self, prompt, prompt_2, device=None, max_sequence_length=512, **kw):
        n = 1 if isinstance(prompt_2, str) else len(prompt_2)
        self.encodes.append(prompt_2)
        return torch.zeros(n, T, J), torch.zeros(n, P), torch.zeros(T, 3)

    def __call__(self, height, width, image, mask_image, **kw):
        self.calls.append((width, height, [np.array(im) for im in image], [np.array(im) for im in mask_image]))
        return SimpleNamespace(images=[Image.fromarray(255 - np.array(im)) for im in image])

    def paste_back(self, original, edited, mask, dilate=None, feather=None, **kw):
        self.pastes.append(dict(original=np.array(original), edited=np.array(edited), mask=np.array(mask), dilate=dilate, feather=feather, **kw))
        o, e, g = np.array(original)[None], np.array(edited)[None], np.array(mask)[None]
        if "rect" in kw:
            rect = kw["rect"]
            return rref.paste_rect(o, e, g, dilate, feather, rc.matrices(rect, kw["origin"])[1], rect.rw, rect.rh,
                                   color_match=kw.get("color_match"), color_ref=None if kw.get("color_ref") is None else kw["color_ref"][None])
        if "color_match" in kw:
            return plref.paste(o, e, g, dilate, feather, color_ref=kw["color_ref"][None], **kw["color_match"])[0]
        return ref.paste(o, e, g, dilate, feather)


class WarpStub(Stub):
    def warp_affine(self, image, m, out_size, coverage=False):
        self.warps.append((np.array(image), np.array(m), tuple(out_size)))
        return rref.warp_affine(image, m, out_size, coverage=coverage)


def _run(pipe, items=ITEMS, **kw):
    saved = {}
    res = bd.run_items(items, pipe, None, batch_size=4, num_inference_steps=2, device="cpu", loader=_loader,
                       save=lambda i, im: saved.__setitem__(i, np.array(im)), **kw)
    return res, saved


def _same_work(a, b):
    for f in ("index", "prompt", "meta", "size", "name", "region", "parent", "line", "rect"):
        assert getattr(a, f) == getattr(b, f), f
    for f in ("image", "mask", "orig_scene", "orig_mask"):
        assert np.array_equal(np.array(getattr(a, f)), np.array(getattr(b, f))), f


def test_two_lines_one_level_one_slanted():
    scene = _scene()
    flat, slant = _line_masks()
    base = dict(per_line=True, dilate=D, feather=R, region=REGION)
    plain, rect_ = Stub(), WarpStub()
    r0, s0 = _run(plain, paste_back=base)
    r1, s1 = _run(rect_, paste_back=dict(base, rectify=True))
    assert r0["all_done"] == r1["all_done"] == [0] and not r1["failed"]
    assert len(plain.pastes) == len(rect_.pastes) == 2 and plain.warps == [] and len(rect_.warps) == 2     # the scene and the mask of ONE line
    # ---- the level line: its Work, its pipeline call and its paste are those of the run without the key
    cfg0, cfg1 = bd._paste_back_cfg(base), bd._paste_back_cfg(dict(base, rectify=True))
    w0 = pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg0)
    w1 = pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg1, warp=rect_.warp_affine)
    _same_work(w0[0], w1[0])
    assert w0[0].rect is None and w0[1].rect is None and w1[0].rect is None and w1[1].rect is not None
    call = lambda p, w: next(c for c in p.calls if (c[0], c[1]) == w.size)
    for k in (2, 3):
        assert np.array_equal(call(plain, w0[0])[k][0], call(rect_, w1[0])[k][0])
    assert set(plain.pastes[0]) == set(rect_.pastes[0]) == {"original", "edited", "mask", "dilate", "feather"}     # nothing new was passed
    for k in plain.pastes[0]:
        assert np.array_equal(plain.pastes[0][k], rect_.pastes[0][k]), k
    # ---- the slanted line: the oriented rectangle, the restated warp as the pipeline's input, rect and origin at the paste
    rect = rc.select_rect(rc.mask_points(slant), D, R, **REGION)
    assert w1[1].rect == rect and abs(rect.theta - SLANT[2]) <= 1.0 and (rect.tw, rect.th) == (rect.rw, rect.rh)
    x0, y0, x1, y1 = rc.rect_window(rect, SCENE_WH)
    assert w1[1].region == pb.Region(x0, y0, x1, y1, rect.tw, rect.th)
    fwd, back = rc.matrices(rect, (x0, y0))
    for (img, m, size), src in zip(rect_.warps[-2:], (scene, np.repeat(slant[:, :, None], 3, 2))):
        assert np.array_equal(img, src) and (m == rc.matrices(rect)[0]).all() and size == (rect.rh, rect.rw)
    up_scene = rref.warp_affine(scene, fwd, (rect.rh, rect.rw))[0]
    up_mask = np.where(rref.warp_affine(np.repeat(slant[:, :, None], 3, 2), fwd, (rect.rh, rect.rw))[0] >= 128, 255, 0).astype(np.uint8)
    want = bd.prepare_plain(0, Image.fromarray(up_scene), Image.fromarray(up_mask), ["SLANT"])        # the usual preparation, of the upright crop
    assert want.size == w1[1].size != w0[1].size
    got = call(rect_, w1[1])
    assert np.array_equal(got[2][0], np.array(want.image)) and np.array_equal(got[3][0], np.array(want.mask))
    # the upright mask is a level bar: every row of the crop that holds mask pixels spans the line's length
    rows = np.flatnonzero(up_mask[:, :, 0].any(axis=1))
    assert abs(len(rows) - SLANT[1]) <= 3 and abs(int(up_mask[rows[len(rows) // 2], :, 0].sum()) // 255 - SLANT[0]) <= 3
    p = rect_.pastes[1]
    assert p["rect"] == rect and tuple(p["origin"]) == (x0, y0) and "color_match" not in p
    assert np.array_equal(p["mask"], slant[y0:y1, x0:x1]) and (p["dilate"], p["feather"]) == (D, R)
    # ---- the pasted scene is the restated composition, line by line onto the running result
    out = scene.copy()
    reg = pb.select_region(flat, D, R, **REGION)
    assert np.array_equal(rect_.pastes[0]["original"], out[reg.y0:reg.y1, reg.x0:reg.x1])
    out[reg.y0:reg.y1, reg.x0:reg.x1] = ref.paste(out[None, reg.y0:reg.y1, reg.x0:reg.x1], rect_.pastes[0]["edited"][None],
                                                  flat[None, reg.y0:reg.y1, reg.x0:reg.x1], D, R)[0]
    assert np.array_equal(p["original"], out[y0:y1, x0:x1])                      # the CURRENT pixels of the window
    edited = 255 - got[2][0]
    edited = edited[glyph.crop_box(w1[1].size, w1[1].meta)[1]:]
    assert np.array_equal(p["edited"], edited)
    out[y0:y1, x0:x1] = rref.paste_rect(out[None, y0:y1, x0:x1], edited[None], slant[None, y0:y1, x0:x1], D, R, back, rect.rw, rect.rh)[0]
    assert np.array_equal(s1[0], out)
    # ---- every byte outside each line's mask grown by dilate + 3 feather is the original's; inside, both lines changed; and the slanted
    # line's inverted pixels came back to where they were cut: on the mask's core the result is about 255 - scene
    grown = (ref.dilate(flat, D + 3 * R) > 0) | (ref.dilate(slant, D + 3 * R) > 0)
    assert (s1[0][~grown] == scene[~grown]).all() and (s0[0][~grown] == scene[~grown]).all()
    core = slant >= 128
    assert (s1[0][flat >= 128] != scene[flat >= 128]).any() and (s1[0][core] != scene[core]).any()
    assert (s1[0] != s0[0]).any()
    # random scene pixels are uncorrelated, so the round trip through two bicubic warps is judged on a smooth scene instead


def test_round_trip_of_a_smooth_scene_comes_back_in_place():
    """Forward and back through the two matrices puts every pixel back where it was cut: on a smooth image the difference is a few
    levels of resampling blur, while a misplaced warp (a transposed matrix, a wrong origin) misses by tens of levels."""
    yy, xx = np.mgrid[0:SCENE_WH[1], 0:SCENE_WH[0]]
    scene = np.stack([128 + 100 * np.sin(xx / 23.0) * np.cos(yy / 17.0), 128 + 100 * np.sin((xx + yy) / 29.0), 2 * xx % 256 * 0 + yy / 2], axis=2)
    scene = np.clip(scene, 0, 255).astype(np.uint8)
    _, slant = _line_masks()
    rect = rc.select_rect(rc.mask_points(slant), D, R, **REGION)
    x0, y0, x1, y1 = rc.rect_window(rect, SCENE_WH)
    fwd, back = rc.matrices(rect, (x0, y0))
    up = rref.warp_affine(scene, fwd, (rect.rh, rect.rw))
    again, cov = rref.warp_affine(up, back, (y1 - y0, x1 - x0), coverage=True)
    on = (cov[0] == 255) & (ref.dilate(slant, D + 3 * R)[y0:y1, x0:x1] > 0)
    assert on.sum() > SLANT[0] * SLANT[1]
    diff = np.abs(again[0].astype(int) - scene[y0:y1, x0:x1].astype(int))[on]
    assert diff.max() <= 6 and diff.mean() < 1.0
    assert (cov[0][ref.dilate(slant, pb.halo(D, R))[y0:y1, x0:x1] > 0] == 255).all()                 # alpha's support is covered


def test_color_match_gets_the_original_window_as_its_reference():
    scene = _scene()
    _, slant = _line_masks()
    pipe = WarpStub()
    res, saved = _run(pipe, paste_back=dict(per_line=True, dilate=D, feather=R, region=REGION, rectify=True, color_match=dict(ring=40, min_pixels=16)))
    assert res["all_done"] == [0]
    p = pipe.pastes[1]
    rect = p["rect"]
    x0, y0, x1, y1 = rc.rect_window(rect, SCENE_WH)
    assert p["color_match"] == pb.color_match_cfg(dict(ring=40, min_pixels=16)) and np.array_equal(p["color_ref"], scene[y0:y1, x0:x1])
    assert "rect" not in pipe.pastes[0] and pipe.pastes[0]["color_match"] == p["color_match"]
    grown = (ref.dilate(_line_masks()[0], D + 3 * R) > 0) | (ref.dilate(slant, D + 3 * R) > 0)
    assert (saved[0][~grown] == scene[~grown]).all()


# ---------------------------------------------------------------------------------------------- refusals and CLIs
def test_refusals_come_before_anything_is_encoded_or_run():
    pipe = WarpStub()
    for bad, match in ((dict(rectify=True), "rectify needs per_line"), (dict(per_line=False, rectify=True), "rectify needs per_line"),
                       (dict(per_line=True, rectify=dict(angle=3)), r"unknown keys \['rectify.angle'\]"),
                       (dict(per_line=True, rectify=dict(min_angle=30, max_angle=20)), "min_angle"),
                       (dict(per_line=True, rectify=dict(max_angle=120)), "max_angle"),
                       (dict(per_line=True, rectify=dict(min_aspect=0.5)), "min_aspect"), (dict(per_line=True, rectify=7), "rectify")):
        with pytest.raises(ValueError, match="paste_back: .*" + match):
            _run(pipe, paste_back=bad)
    old = Stub()                                                                 # a pipeline that predates warp_affine
    with pytest.raises(ValueError, match="warp_affine"):
        _run(old, paste_back=dict(per_line=True, rectify=True))
    with pytest.raises(ValueError, match="warp_affine"):
        pl.edit_scene(old, _loader("scene"), _loader("mask"), ["LEVEL", "SLANT"], bd._paste_back_cfg(dict(per_line=True, rectify=True)))
    for p in (pipe, old):
        assert p.encodes == [] and p.calls == [] and p.pastes == [] and p.warps == []
    # ... while that pipeline still serves the same item without the key, and the key changes nothing else in the cfg
    assert _run(old, paste_back=dict(per_line=True, region=REGION))[0]["all_done"] == [0]
    cfg = bd._paste_back_cfg(dict(per_line=True, rectify=dict(max_angle=30)))
    assert cfg == dict(dilate=16, feather=4, region={}, per_line=True, rectify=dict(min_angle=5.0, max_angle=30.0, min_aspect=1.5))
    assert bd._paste_back_cfg(dict(per_line=True, rectify=None)) == bd._paste_back_cfg(dict(per_line=True, rectify=False)) == \
        dict(dilate=16, feather=4, region={}, per_line=True)
    assert bd.Work(3, None, None, "p", {}, (64, 64)).rect is None


def test_run_inference_takes_the_same_path():
    sys.path.insert(0, REPO)
    ri = importlib.import_module("run_inference")

    class Pipe(WarpStub):
        _execution_device = "cpu"

        def __call__(self, height, width, image, mask_image, prompt=None, prompt_2=None, generator=None, **kw):
            return Stub.__call__(self, height, width, image, mask_image)
    saved = ri.scheduler_name
    ri.scheduler_name = ""
    cfg = dict(per_line=True, dilate=D, feather=R, region=REGION, rectify=True)
    try:
        pipe = Pipe()
        out = ri.run_inference(_loader("scene"), _loader("mask"), ["LEVEL", "SLANT"], num_steps=2, pipe=pipe, paste_back=cfg)
    finally:
        ri.scheduler_name = saved
    _, want = _run(WarpStub(), paste_back=cfg)
    assert np.array_equal(np.array(out), want[0]) and len(pipe.warps) == 2 and "rect" in pipe.pastes[1] and "rect" not in pipe.pastes[0]


def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    on = ["--paste_back", "--paste_per_line"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.paste_rectify, a.paste_rectify_min_angle, a.paste_rectify_max_angle) == (False, None, None)
        a = parser.parse_args(base + on + ["--paste_rectify", "--paste_rectify_min_angle", "7.5", "--paste_rectify_max_angle", "30"])
        assert (a.paste_rectify, a.paste_rectify_min_angle, a.paste_rectify_max_angle) == (True, 7.5, 30.0)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(on) == dict(dilate=16, feather=4, region=None, per_line=True)    # without the new flags: the dict it was
    assert parse(on + ["--paste_rectify"])["rectify"] is True
    assert parse(on + ["--paste_rectify_max_angle", "30"])["rectify"] == dict(max_angle=30.0)
    got = bd._paste_back_cfg(parse(on + ["--paste_rectify", "--paste_rectify_min_angle", "7.5"]))["rectify"]
    assert got == dict(min_angle=7.5, max_angle=45.0, min_aspect=1.5)
    for flag in (["--paste_rectify"], ["--paste_rectify_min_angle", "7"], ["--paste_rectify_max_angle", "30"]):
        for have in ([], ["--paste_back"]):
            with pytest.raises(SystemExit, match="needs --paste_back --paste_per_line"):
                parse(have + flag)
            with pytest.raises(SystemExit, match="needs --paste_back --paste_per_line"):
                re_.main(["--json_path", "j", "--original_images_dir", "o", "--weights_path", "w"] + have + flag)
            with pytest.raises(SystemExit, match="needs --paste_back --paste_per_line"):
                re_.main(["--json_path", "j", "--original_images_dir", "o", "--lora_weights_path", "l"] + have + flag, lora=True)


# ---------------------------------------------------------------------------------------------- the C entry point
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


def test_symbol_is_declared_bound_exported_and_the_abi_version_stays(lib):
    from textflux_amd import _lib as L
    assert "tfx_warp_affine_u8" in L.SIGNATURES and hasattr(lib, "tfx_warp_affine_u8")
    assert L.ABI_VERSION == 11 == L.header_abi_version()
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    assert "int tfx_warp_affine_u8(const void* in, void* out, void* coverage" in hdr and hdr.count("without a new") >= 3


def test_entry_point_checks_its_arguments(lib):
    p = [k << 20 for k in range(1, 6)]                                           # in, out, coverage, m, taps: never dereferenced, every call is refused
    call = lambda ptrs=p, dims=(2, 8, 8, 3, 4, 4): lib.tfx_warp_affine_u8(ptrs[0], ptrs[1], ptrs[2], *dims, ptrs[3], ptrs[4], None)
    for k in (0, 1, 3, 4):                                                       # coverage alone may be NULL
        assert call(p[:k] + [None] + p[k + 1:]) != 0 and b"null pointer" in lib.tfx_last_error()
    for k in range(6):
        if k != 3:
            dims = [2, 8, 8, 3, 4, 4]
            dims[k] = 0
            assert call(dims=tuple(dims)) != 0 and b"at least 1" in lib.tfx_last_error()
    for c in (0, 5):
        assert call(dims=(2, 8, 8, c, 4, 4)) != 0 and b"1..4 channels" in lib.tfx_last_error()
    assert call(dims=(65536, 8, 8, 3, 4, 4)) != 0 and b"65535" in lib.tfx_last_error()
    assert call(dims=(2, 8, 8, 3, 600000, 4)) != 0 and b"out_h" in lib.tfx_last_error()
    assert call([p[0], p[0], p[2], p[3], p[4]]) != 0 and b"different buffers" in lib.tfx_last_error()
    assert call([p[0], p[1], p[1], p[3], p[4]]) != 0 and b"different buffers" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2], p[3] + 4, p[4]]) != 0 and b"8-byte aligned" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2], p[3], p[4] + 2]) != 0 and b"8-byte aligned" in lib.tfx_last_error()


def test_ops_wrapper_checks_before_it_launches():
    import inspect
    from textflux_amd import ops
    from textflux_amd.pipeline import FluxFillPipeline
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.warp_affine_u8(img, np.array([Q, 0, 0, 0, Q, 0], np.int64), (4, 4))   # no CPU fallback
    assert hasattr(FluxFillPipeline, "warp_affine")
    for f in (FluxFillPipeline.paste_back, pb.paste):
        sig = inspect.signature(f).parameters
        assert sig["rect"].default is None and tuple(sig["origin"].default) == (0, 0)
