"""Perspective per-line edits without a GPU: the numpy restatement of the device warp against known answers and against the affine
restatement, the quad of a drawn region, the ordering, the rule, the upright crop's two guarantees, the precision of the integer
matrices, the batch driver around a stub pipeline whose warps ARE the restatements, the refusals, the CLI flags and the new C entry point
(exported, bound, refusing bad arguments on the host)."""
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
from tests.helpers import perspective_ref as pref
from tests.helpers import per_line_ref as plref
from tests.helpers import rectify_ref as rref
from textflux_amd import batch_driver as bd
from textflux_amd import glyph
from textflux_amd import paste_back as pb
from textflux_amd import per_line as pl
from textflux_amd import perspective as ps
from textflux_amd import rectify as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 1 << 16
IDENT = np.array([1 << 30, 0, 0, 0, 1 << 30, 0, 0, 0, 1 << 30], np.int64)

# drawn quads (TL, TR, BR, BL): a 2:1 taper, a 2.8:1 taper, a 1.5:1 taper tilted by some 25 degrees, a level rectangle
TAPER2 = [(100, 100), (400, 140), (400, 220), (100, 260)]
TAPER28 = [(100, 100), (380, 150), (380, 207), (100, 260)]
TILTED = [(60, 200), (300, 90), (320, 130), (80, 300)]
LEVEL = [(50, 50), (350, 50), (350, 120), (50, 120)]
VERTICAL = [(260, 40), (260, 300), (200, 330), (200, 60)]                        # a tapering vertical line: its midline is exactly vertical, read downward


def raster(quad, size=(512, 400)):
    return glyph.fill_polygon(size[1], size[0], quad)[:, :, 0]


def drawn(length, thickness, deg, centre=(256, 256), size=(512, 512)):
    """uint8 [H, W] mask: a length x thickness rectangle around `centre` whose long side points along (cos deg, sin deg), y down."""
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    pts = [np.array(centre) + su * u * length / 2 + sv * v * thickness / 2 for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    im = Image.new("L", size, 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in pts], fill=255)
    return np.array(im)


# ---------------------------------------------------------------------------------------------- the restatement
def test_embedded_affine_matrix_is_the_affine_restatement():
    x = np.random.default_rng(1).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    c, s = math.cos(math.radians(17)), math.sin(math.radians(17))
    a0 = np.array([round(c * Q), round(-s * Q), round(20.3 * Q), round(s * Q), round(c * Q), round(-9.1 * Q)], np.int64)
    a1 = np.array([round(1.3 * c * Q), round(1.3 * s * Q), round(-7.7 * Q), round(-1.3 * s * Q), round(1.3 * c * Q), round(11.2 * Q)], np.int64)
    aff = np.stack([a0, a1])
    want, want_cov = rref.warp_affine(x, aff, (29, 41), coverage=True)
    got, cov = pref.warp_perspective(x, pref.embed(aff), (29, 41), coverage=True)
    assert (want_cov == 0).any() and (want_cov == 255).any()                     # both kinds of pixel are compared
    assert np.array_equal(got, want) and np.array_equal(cov, want_cov)


def test_restatement_identity_horizon_and_floor():
    x = np.random.default_rng(3).integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    out, cov = pref.warp_perspective(x, IDENT, (9, 13), coverage=True)
    assert (out == x).all() and (cov == 255).all()
    # D = 2^30 (6 - i): columns 0..5 are in front of the horizon, column 6 is on it, 7.. are behind it
    m = IDENT.copy()
    m[6], m[8] = -(1 << 30), 6 << 30
    out, cov = pref.warp_perspective(x, m, (9, 13), coverage=True)
    assert (out[:, :, 6:] == 0).all() and (cov[:, :, 6:] == 0).all() and (cov[:, :, :6] == 255).all()
    assert (out[:, 0, 0] == x[:, 0, 0]).all() and (out[:, 6, 0] == x[:, 1, 0]).all()          # column 0 reads (0, j / 6); column 5 reads (5, j)
    assert (out[:, :, 5] == x[:, :, 5]).all()
    # floor, not truncation: Nx = -1, D = 3 is PX = floor(-256 / 3) = -86 (truncation: -85), so xi = -1 and fx = 170
    D, PX, PY = pref.positions(np.array([0, 0, -1, 0, 0, 7, 0, 0, 3], np.int64), (1, 1))
    assert (int(D[0, 0]), int(PX[0, 0]), int(PY[0, 0])) == (3, -86, 597) and (int(PX[0, 0]) >> 8, int(PX[0, 0]) & 255) == (-1, 170)
    # per-sample matrices reach their own sample
    shift = IDENT.copy()
    shift[2] = -(1 << 30)
    out, cov = pref.warp_perspective(x, np.stack([IDENT, shift]), (9, 13), coverage=True)
    assert (out[0] == x[0]).all() and (out[1][:, 1:] == x[1][:, :-1]).all() and (cov[1][:, 0] == 0).all() and (cov[1][:, 1:] == 255).all()


def test_a_constant_survives_forward_and_back():
    quad = ps.select_quad(rc.mask_points(raster(TAPER2)), 8, 2, pad=0.0, min_side=96)
    x0, y0, x1, y1 = ps.quad_window(quad, (512, 400))
    fwd, back = ps.matrices(quad, (x0, y0))
    src = np.full((1, 400, 512, 1), 137, np.uint8)
    up = pref.warp_perspective(src, ps.matrices(quad)[0], (quad.rh, quad.rw))
    again, cov = pref.warp_perspective(up, back, (y1 - y0, x1 - x0), coverage=True)
    assert (up == 137).all() and (again == 137).all() and 0 < (cov == 255).sum() < cov.size


# ---------------------------------------------------------------------------------------------- the quad of a region
def _inside(q, pts, eps=1e-6):
    e = np.roll(q, -1, axis=0) - q
    d = pts[:, None, :] - q[None]
    c = e[None, :, 0] * d[:, :, 1] - e[None, :, 1] * d[:, :, 0]
    return (c >= -eps).all() or (c <= eps).all()


@pytest.mark.parametrize("quad", [TAPER2, TAPER28, TILTED, LEVEL], ids=["taper2", "taper28", "tilted", "level"])
def test_hull_quad_recovers_a_drawn_quad_and_encloses_the_region(quad):
    pts = rc.mask_points(raster(quad))
    hq = ps.hull_quad(pts)
    assert hq is not None and hq.shape == (4, 2) and hq.dtype == np.float64
    assert _inside(hq, pts.astype(np.float64))                                   # every region pixel lies inside
    got = ps.order_quad(hq)
    err = np.abs(got - np.array(quad, np.float64)).max()
    print(f"corner error {err:.3f} px")
    assert err <= 1.0                                                            # the raster moves an edge by up to half a pixel on either side
    from scipy.spatial import ConvexHull
    assert abs(ps._area(got) / ConvexHull(pts).volume - 1.0) < 0.01


def test_hull_quad_of_degenerate_regions_is_none():
    assert ps.hull_quad(np.zeros((0, 2), np.int64)) is None
    assert ps.hull_quad(np.array([[3, 4], [9, 4], [20, 4]])) is None             # collinear
    assert ps.hull_quad(np.array([[0, 0], [10, 0], [5, 8]])) is None             # a triangle: three hull vertices


def test_order_quad_under_all_eight_corner_orders():
    for quad in (TAPER2, TILTED, VERTICAL):
        q = np.array(quad, np.float64)
        orders = [np.roll(q[::step], k, axis=0) for step in (1, -1) for k in range(4)]
        assert len(orders) == 8
        for o in orders:
            assert np.array_equal(ps.order_quad(o), q)
    tl, tr, br, bl = ps.order_quad(TILTED)
    assert ps._cross(tr - tl, br - tr) > 0                                       # clockwise on screen (y down)
    assert np.hypot(*(tr - tl)) + np.hypot(*(br - bl)) > np.hypot(*(br - tr)) + np.hypot(*(bl - tl))
    assert ((tr + br) / 2 - (tl + bl) / 2)[0] > 0


def test_which_lines_take_the_perspective_path():
    quad_of = lambda m: ps.order_quad(ps.hull_quad(rc.mask_points(m)))
    for q in (TAPER2, TAPER28, TILTED):
        assert ps.is_perspective(quad_of(raster(q)))
    assert not ps.is_perspective(quad_of(raster(LEVEL)))                         # fit = 1: today's path
    assert not ps.is_perspective(quad_of(drawn(300, 40, 25)))                    # fit = 1 at any angle: rectify's ground
    assert not ps.is_perspective(quad_of(raster(VERTICAL)))                      # vertical text: today's path
    assert not ps.is_perspective(None)
    assert not ps.is_perspective(np.array([(0, 0), (100, 0), (30, 10), (0, 50)], np.float64))         # not convex
    assert not ps.is_perspective(np.array([(0, 0), (100, 20), (100, 26), (0, 50)], np.float64))       # a side under 8 px
    blob = np.array([(0, 0), (60, 8), (60, 42), (0, 50)], np.float64)             # 60.5 long, 42 thick in the mean: the aspect rule alone
    assert not ps.is_perspective(blob) and ps.is_perspective(blob, ps.perspective_cfg(dict(min_aspect=1.0)))
    t2 = quad_of(raster(TAPER2))
    assert not ps.is_perspective(t2, ps.perspective_cfg(dict(max_fit=0.7))) and not ps.is_perspective(t2, ps.perspective_cfg(dict(max_taper=1.5)))
    assert ps.is_perspective(quad_of(drawn(300, 40, 25)), ps.perspective_cfg(dict(max_fit=1.0)))
    cfg = bd._paste_back_cfg(dict(per_line=True, perspective=True))
    assert isinstance(ps.plan(raster(TAPER2), cfg), ps.Quad) and ps.plan(raster(LEVEL), cfg) is None
    assert ps.plan(raster(TAPER2), bd._paste_back_cfg(dict(per_line=True))) is None                  # the key absent: nobody takes the path
    assert ps.plan(np.zeros((64, 64), np.uint8), cfg) is None


@pytest.mark.parametrize("quad,pad", [(TAPER2, 0.5), (TAPER2, 0.0), (TAPER28, 0.5), (TILTED, 0.5), (TILTED, 0.0)],
                         ids=["taper2-pad", "taper2", "taper28-pad", "tilted-pad", "tilted"])
def test_select_quad_keeps_its_two_guarantees(quad, pad):
    d, r, min_side, max_taper = 16, 4, 96, 4.0
    m = raster(quad)
    sq = ps.select_quad(rc.mask_points(m), d, r, pad=pad, min_side=min_side, max_taper=max_taper)
    assert isinstance(sq, ps.Quad) and sq.rw >= min_side and sq.rh >= min_side and all(isinstance(v, int) for v in sq[1:])
    assert np.abs(np.array(sq.corners) - np.array(quad, np.float64)).max() <= 1.0
    top, right, bottom, left = ps._sides(np.array(sq.corners))
    assert (sq.iw, sq.ih) == (math.ceil(max(top, bottom) + 1 - 1e-6), math.ceil(max(left, right) + 1 - 1e-6))
    assert min(sq.ox, sq.rw - sq.ox - sq.iw, sq.oy, sq.rh - sq.oy - sq.ih) >= pb.halo(d, r)
    # (a) D, normalised to 1 at the crop's centre pixel, stays at or above 1 / max_taper at the four corner pixels -- in the integer matrix too
    fwd = ps.matrices(sq)[0]
    Dc = fwd[6] * (sq.rw // 2) + fwd[7] * (sq.rh // 2) + fwd[8]
    assert Dc == 1 << 30
    for i, j in ((0, 0), (sq.rw - 1, 0), (0, sq.rh - 1), (sq.rw - 1, sq.rh - 1)):
        assert (fwd[6] * i + fwd[7] * j + fwd[8]) / Dc >= 1.0 / max_taper - 1e-6
    # (b) the warp back into the WHOLE scene covers every pixel with alpha > 0, through the integer matrices
    alpha = ref.alpha_mask(m[None], d, r)[0]
    back = ps.matrices(sq, (0, 0))[1]
    D, PX, PY = pref.positions(back, m.shape)
    cov = (D > 0) & ((PX >> 8) >= 0) & ((PX >> 8) < sq.rw) & ((PY >> 8) >= 0) & ((PY >> 8) < sq.rh)
    assert (alpha > 0).sum() > 0 and cov[alpha > 0].all()
    x0, y0, x1, y1 = ps.quad_window(sq, (m.shape[1], m.shape[0]))
    ys, xs = np.nonzero(alpha)
    assert x0 <= xs.min() and xs.max() < x1 and y0 <= ys.min() and ys.max() < y1  # ... and the window holds them
    # the sizes shrink under max_side as select_rect's do
    small = ps.select_quad(rc.mask_points(m), d, r, pad=pad, min_side=min_side, max_side=200, max_taper=max_taper)
    longer = max(small.rw, small.rh)
    assert (small.tw, small.th) == (max(32, small.rw * 200 // longer), max(32, small.rh * 200 // longer)) and (sq.tw, sq.th) == (sq.rw, sq.rh)


def test_select_quad_refuses_a_quad_no_padding_serves():
    steep = [(100, 100), (380, 170), (380, 190), (100, 260)]                     # 8:1: the crop would run into the horizon at any padding
    assert ps.select_quad(rc.mask_points(raster(steep)), 16, 4, pad=0.5, min_side=96) is None
    assert ps.select_quad(rc.mask_points(raster(TAPER28)), 16, 4, pad=0.5, min_side=96, max_taper=1.5) is None
    assert ps.select_quad(np.array([[0, 0], [10, 0], [5, 8]]), 16, 4) is None    # no quad at all


@pytest.mark.parametrize("quad", [TAPER2, TAPER28, TILTED], ids=["taper2", "taper28", "tilted"])
def test_matrices_compose_to_the_identity_within_a_256th_of_a_pixel(quad):
    sq = ps.select_quad(rc.mask_points(raster(quad)), 16, 4, pad=0.5, min_side=96)
    x0, y0, x1, y1 = ps.quad_window(sq, (512, 400))
    fwd, back = ps.matrices(sq, (x0, y0))
    assert fwd.dtype == back.dtype == np.int64 and fwd.shape == back.shape == (9,)
    assert (fwd == ps.matrices(sq)[0]).all()                                     # the origin moves the backward matrix only
    i, j = np.meshgrid(np.arange(sq.rw, dtype=np.float64), np.arange(sq.rh, dtype=np.float64))
    f, b = fwd.astype(np.float64), back.astype(np.float64)
    D = f[6] * i + f[7] * j + f[8]
    x, y = (f[0] * i + f[1] * j + f[2]) / D - x0, (f[3] * i + f[4] * j + f[5]) / D - y0
    Db = b[6] * x + b[7] * y + b[8]
    err = max(np.abs((b[0] * x + b[1] * y + b[2]) / Db - i).max(), np.abs((b[3] * x + b[4] * y + b[5]) / Db - j).max())
    print(f"round trip error {err:.2e} px, largest |Nx| 2^{math.log2(np.abs(f[0] * i + f[1] * j + f[2]).max()):.1f}")
    assert err <= 1.0 / 256 and (Db > 0).all()
    # the inner rectangle's corners land on the quad's corners
    for (u, v), (cx, cy) in zip(ps._inner(sq.ox, sq.oy, sq.iw, sq.ih), sq.corners):
        d = f[6] * u + f[7] * v + f[8]
        assert abs((f[0] * u + f[1] * v + f[2]) / d - cx) < 1e-3 and abs((f[3] * u + f[4] * v + f[5]) / d - cy) < 1e-3
    # and the magnitude contract of the kernel holds with room to spare
    assert np.abs(f[0] * i + f[1] * j + f[2]).max() < 2.0 ** 44 and D.max() < 2.0 ** 33


# ---------------------------------------------------------------------------------------------- the batch driver around a stub
T, J, P = 6, 8, 4
SCENE_WH, FLAT_BOX, SLANT = (640, 480), (40, 30, 200, 60), (180, 28, 25, (150, 340))
TRAP = [(360, 80), (600, 110), (600, 170), (360, 220)]                           # the third line: a 2.3:1 taper
D, R = 8, 2
REGION = dict(pad=0.0, min_side=96)


def _scene():
    return np.random.default_rng(11).integers(0, 256, (SCENE_WH[1], SCENE_WH[0], 3), dtype=np.uint8)


def _line_masks():
    flat = np.zeros((SCENE_WH[1], SCENE_WH[0]), np.uint8)
    x0, y0, x1, y1 = FLAT_BOX
    flat[y0:y1, x0:x1] = 255
    return flat, drawn(SLANT[0], SLANT[1], SLANT[2], centre=SLANT[3], size=SCENE_WH), raster(TRAP, SCENE_WH)


def _loader(kind):
    if kind == "scene":
        return Image.fromarray(_scene())
    flat, slant, trap = _line_masks()
    return Image.fromarray(flat | slant | trap)


ITEMS = [dict(image="scene", mask="mask", text="LEVEL\nTRAPEZOID\nSLANT")]       # in the split order: top to bottom


class Stub:
    """A pipeline whose result is its input canvas inverted, whose warps are the restatements and whose paste is the restated paste; it
    records what it is handed.  Without warp_perspective: a pipeline that predates it."""

    def __init__(self):
        self.calls, self.encodes, self.pastes, self.warps, self.quad_warps, self.text_encoder_2 = [], [], [], [], [], object()

    def encode_prompt(self, prompt, prompt_2, device=None, max_sequence_length=512, **kw):
        n = 1 if isinstance(prompt_2, str) else len(prompt_2)
        self.encodes.append(prompt_2)
        return torch.zeros(n, T, J), torch.zeros(n, P), torch.zeros(T, 3)

    def __call__(self, height, width, image, mask_image, **kw):
        self.calls.append((width, height, [np.array(im) for im in image], [np.array(im) for im in mask_image]))
        return SimpleNamespace(images=[Image.fromarray(255 - np.array(im)) for im in image])

    def warp_affine(self, image, m, out_size, coverage=False):
        self.warps.append((np.array(image), np.array(m), tuple(out_size)))
        return rref.warp_affine(image, m, out_size, coverage=coverage)

    def paste_back(self, original, edited, mask, dilate=None, feather=None, **kw):
        self.pastes.append(dict(original=np.array(original), edited=np.array(edited), mask=np.array(mask), dilate=dilate, feather=feather, **kw))
        o, e, g = np.array(original)[None], np.array(edited)[None], np.array(mask)[None]
        cm = dict(color_match=kw.get("color_match"), color_ref=None if kw.get("color_ref") is None else kw["color_ref"][None])
        if isinstance(kw.get("rect"), ps.Quad):
            return pref.paste_quad(o, e, g, dilate, feather, ps.matrices(kw["rect"], kw["origin"])[1], kw["rect"].rw, kw["rect"].rh, **cm)
        if "rect" in kw:
            return rref.paste_rect(o, e, g, dilate, feather, rc.matrices(kw["rect"], kw["origin"])[1], kw["rect"].rw, kw["rect"].rh, **cm)
        if "color_match" in kw:
            return plref.paste(o, e, g, dilate, feather, color_ref=kw["color_ref"][None], **kw["color_match"])[0]
        return ref.paste(o, e, g, dilate, feather)


class QuadStub(Stub):
    def warp_perspective(self, image, m, out_size, coverage=False):
        self.quad_warps.append((np.array(image), np.array(m), tuple(out_size)))
        return pref.warp_perspective(image, m, out_size, coverage=coverage)


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


@pytest.fixture(scope="module")
def both_keys():
    pipe = QuadStub()
    res, saved = _run(pipe, paste_back=dict(per_line=True, dilate=D, feather=R, region=REGION, rectify=True, perspective=True))
    return pipe, res, saved


def test_three_lines_take_the_plain_the_rect_and_the_quad_path(both_keys):
    pipe, res, saved = both_keys
    scene = _scene()
    flat, slant, trap = _line_masks()
    assert res["all_done"] == [0] and not res["failed"] and len(pipe.pastes) == 3
    assert len(pipe.warps) == 2 and len(pipe.quad_warps) == 2                    # the scene and the mask of ONE line each
    level, quad_, rect_ = pipe.pastes
    assert "rect" not in level and isinstance(quad_["rect"], ps.Quad) and isinstance(rect_["rect"], rc.Rect)
    # ---- the trapezoid: the Quad of its mask, the restated warp as the pipeline's input, rect and origin at the paste
    quad = ps.select_quad(rc.mask_points(trap), D, R, **REGION)
    assert quad_["rect"] == quad and np.abs(np.array(quad.corners) - np.array(TRAP, np.float64)).max() <= 1.0
    x0, y0, x1, y1 = ps.quad_window(quad, SCENE_WH)
    assert tuple(quad_["origin"]) == (x0, y0) and np.array_equal(quad_["mask"], trap[y0:y1, x0:x1]) and (quad_["dilate"], quad_["feather"]) == (D, R)
    fwd, back = ps.matrices(quad, (x0, y0))
    for (img, m, size), src in zip(pipe.quad_warps, (scene, np.repeat(trap[:, :, None], 3, 2))):
        assert np.array_equal(img, src) and (m == fwd).all() and size == (quad.rh, quad.rw)
    up_scene = pref.warp_perspective(scene, fwd, (quad.rh, quad.rw))[0]
    up_mask = np.where(pref.warp_perspective(np.repeat(trap[:, :, None], 3, 2), fwd, (quad.rh, quad.rw))[0] >= 128, 255, 0).astype(np.uint8)
    want = bd.prepare_plain(0, Image.fromarray(up_scene), Image.fromarray(up_mask), ["TRAPEZOID"])   # the usual preparation, of the upright crop
    got = next(c for c in pipe.calls if (c[0], c[1]) == want.size and np.array_equal(c[2][0], np.array(want.image)))
    assert np.array_equal(got[3][0], np.array(want.mask))
    # the upright mask is a level bar that fills the inner rectangle: the taper is gone
    bar = up_mask[:, :, 0] > 0
    cols = np.flatnonzero(bar.any(axis=0))
    heights = bar[:, cols[5:-5]].sum(axis=0)
    assert abs(int(heights.max()) - quad.ih) <= 3 and heights.max() - heights.min() <= 3 and abs(len(cols) - quad.iw) <= 3
    assert abs(int(cols[0]) - quad.ox) <= 2 and abs(int(np.flatnonzero(bar.any(axis=1))[0]) - quad.oy) <= 2
    # ---- the pasted scene is the restated composition, line by line onto the running result, in the split order
    out = scene.copy()
    reg = pb.select_region(flat, D, R, **REGION)
    out[reg.y0:reg.y1, reg.x0:reg.x1] = ref.paste(out[None, reg.y0:reg.y1, reg.x0:reg.x1], level["edited"][None],
                                                  flat[None, reg.y0:reg.y1, reg.x0:reg.x1], D, R)[0]
    assert np.array_equal(quad_["original"], out[y0:y1, x0:x1])                  # the CURRENT pixels of the window
    edited = (255 - got[2][0])[glyph.crop_box(want.size, want.meta)[1]:]
    assert np.array_equal(quad_["edited"], edited)
    out[y0:y1, x0:x1] = pref.paste_quad(out[None, y0:y1, x0:x1], edited[None], trap[None, y0:y1, x0:x1], D, R, back, quad.rw, quad.rh)[0]
    rect = rc.select_rect(rc.mask_points(slant), D, R, **REGION)
    assert rect_["rect"] == rect
    a0, b0, a1, b1 = rc.rect_window(rect, SCENE_WH)
    out[b0:b1, a0:a1] = rref.paste_rect(out[None, b0:b1, a0:a1], rect_["edited"][None], slant[None, b0:b1, a0:a1], D, R,
                                        rc.matrices(rect, (a0, b0))[1], rect.rw, rect.rh)[0]
    assert np.array_equal(saved[0], out)
    # ---- every byte outside each line's mask grown by dilate + 3 feather is the original's; inside, all three lines changed
    grown = np.zeros_like(flat, bool)
    for m in (flat, slant, trap):
        assert not (grown & (ref.dilate(m, D + 3 * R) > 0)).any()
        grown |= ref.dilate(m, D + 3 * R) > 0
    assert (saved[0][~grown] == scene[~grown]).all()
    for m in (flat, slant, trap):
        assert (saved[0][m >= 128] != scene[m >= 128]).any()


def test_lines_that_do_not_qualify_are_prepared_as_without_the_key(both_keys):
    pipe = QuadStub()
    base = dict(per_line=True, dilate=D, feather=R, region=REGION, rectify=True)
    cfg0, cfg1 = bd._paste_back_cfg(base), bd._paste_back_cfg(dict(base, perspective=True))
    w0 = pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg0, warp=pipe.warp_affine)
    w1 = pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg1, warp=pipe.warp_affine, warp_quad=pipe.warp_perspective)
    assert [type(w.rect).__name__ for w in w0] == ["NoneType", "NoneType", "Rect"]
    assert [type(w.rect).__name__ for w in w1] == ["NoneType", "Quad", "Rect"]
    _same_work(w0[0], w1[0]), _same_work(w0[2], w1[2])
    assert w0[1].size != w1[1].size or not np.array_equal(np.array(w0[1].image), np.array(w1[1].image))
    # the key set but no perspective warp at hand: nobody takes the path
    w2 = pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg1, warp=pipe.warp_affine)
    for a, b in zip(w0, w2):
        _same_work(a, b)
    # and in the whole run the level and the slanted line got the pastes of a run without the key
    without = QuadStub()
    _run(without, paste_back=base)
    assert without.quad_warps == [] and "rect" not in without.pastes[1]
    for k in (0, 2):
        assert set(without.pastes[k]) == set(both_keys[0].pastes[k])
        for f in ("edited", "mask", "dilate", "feather"):
            assert np.array_equal(without.pastes[k][f], both_keys[0].pastes[k][f]), (k, f)


def test_color_match_gets_the_original_window_as_its_reference():
    scene = _scene()
    pipe = QuadStub()
    res, saved = _run(pipe, paste_back=dict(per_line=True, dilate=D, feather=R, region=REGION, perspective=True, color_match=dict(ring=40, min_pixels=16)))
    assert res["all_done"] == [0] and pipe.warps == []                           # rectify is not set: the slanted line stays plain
    p = pipe.pastes[1]
    x0, y0, x1, y1 = ps.quad_window(p["rect"], SCENE_WH)
    assert p["color_match"] == pb.color_match_cfg(dict(ring=40, min_pixels=16)) and np.array_equal(p["color_ref"], scene[y0:y1, x0:x1])
    assert "rect" not in pipe.pastes[0] and "rect" not in pipe.pastes[2]
    grown = sum((ref.dilate(m, D + 3 * R) > 0) for m in _line_masks()) > 0
    assert (saved[0][~grown] == scene[~grown]).all()


# ---------------------------------------------------------------------------------------------- refusals and CLIs
def test_refusals_come_before_anything_is_encoded_or_run():
    pipe = QuadStub()
    for bad, match in ((dict(perspective=True), "perspective needs per_line"), (dict(per_line=False, perspective=True), "perspective needs per_line"),
                       (dict(per_line=True, perspective=dict(taper=3)), r"unknown keys \['perspective.taper'\]"),
                       (dict(per_line=True, perspective=dict(max_fit=1.5)), "max_fit"), (dict(per_line=True, perspective=dict(max_taper=0.5)), "max_taper"),
                       (dict(per_line=True, perspective=dict(min_aspect=0.5)), "min_aspect"),
                       (dict(per_line=True, perspective=dict(max_angle=120)), "max_angle"), (dict(per_line=True, perspective=7), "perspective")):
        with pytest.raises(ValueError, match="paste_back: .*" + match):
            _run(pipe, paste_back=bad)
    with pytest.raises(ValueError, match="unknown keys"):
        ps.perspective_cfg(dict(fit=1))
    old = Stub()                                                                 # a pipeline that predates warp_perspective
    with pytest.raises(ValueError, match="warp_perspective"):
        _run(old, paste_back=dict(per_line=True, perspective=True))
    with pytest.raises(ValueError, match="warp_perspective"):
        pl.edit_scene(old, _loader("scene"), _loader("mask"), ["A", "B", "C"], bd._paste_back_cfg(dict(per_line=True, perspective=True)))
    for p in (pipe, old):
        assert p.encodes == [] and p.calls == [] and p.pastes == [] and p.warps == [] and p.quad_warps == []
    # ... while that pipeline still serves the same item without the key, and the key changes nothing else in the cfg
    assert _run(old, paste_back=dict(per_line=True, region=REGION, rectify=True))[0]["all_done"] == [0]
    cfg = bd._paste_back_cfg(dict(per_line=True, perspective=dict(max_taper=3)))
    assert cfg == dict(dilate=16, feather=4, region={}, per_line=True, perspective=dict(max_fit=0.9, max_taper=3.0, min_aspect=1.5, max_angle=45.0))
    assert bd._paste_back_cfg(dict(per_line=True, perspective=None)) == bd._paste_back_cfg(dict(per_line=True, perspective=False)) == \
        dict(dilate=16, feather=4, region={}, per_line=True)


def test_run_inference_takes_the_same_path(both_keys):
    sys.path.insert(0, REPO)
    ri = importlib.import_module("run_inference")

    class Pipe(QuadStub):
        _execution_device = "cpu"

        def __call__(self, height, width, image, mask_image, prompt=None, prompt_2=None, generator=None, **kw):
            return Stub.__call__(self, height, width, image, mask_image)
    saved = ri.scheduler_name
    ri.scheduler_name = ""
    cfg = dict(per_line=True, dilate=D, feather=R, region=REGION, rectify=True, perspective=True)
    try:
        pipe = Pipe()
        out = ri.run_inference(_loader("scene"), _loader("mask"), ["LEVEL", "TRAPEZOID", "SLANT"], num_steps=2, pipe=pipe, paste_back=cfg)
    finally:
        ri.scheduler_name = saved
    assert np.array_equal(np.array(out), both_keys[2][0]) and len(pipe.quad_warps) == 2 and isinstance(pipe.pastes[1]["rect"], ps.Quad)


def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    on = ["--paste_back", "--paste_per_line"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.paste_perspective, a.paste_perspective_max_fit, a.paste_perspective_max_taper) == (False, None, None)
        a = parser.parse_args(base + on + ["--paste_perspective", "--paste_perspective_max_fit", "0.8", "--paste_perspective_max_taper", "3"])
        assert (a.paste_perspective, a.paste_perspective_max_fit, a.paste_perspective_max_taper) == (True, 0.8, 3.0)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(on) == dict(dilate=16, feather=4, region=None, per_line=True)    # without the new flags: the dict it was
    assert parse(on + ["--paste_perspective"])["perspective"] is True
    assert parse(on + ["--paste_perspective_max_taper", "3"])["perspective"] == dict(max_taper=3.0)
    both = parse(on + ["--paste_perspective", "--paste_rectify"])
    assert both["perspective"] is True and both["rectify"] is True
    got = bd._paste_back_cfg(parse(on + ["--paste_perspective", "--paste_perspective_max_fit", "0.8"]))["perspective"]
    assert got == dict(max_fit=0.8, max_taper=4.0, min_aspect=1.5, max_angle=45.0)
    for flag in (["--paste_perspective"], ["--paste_perspective_max_fit", "0.8"], ["--paste_perspective_max_taper", "3"]):
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
    assert "tfx_warp_perspective_u8" in L.SIGNATURES and hasattr(lib, "tfx_warp_perspective_u8")
    assert L.SIGNATURES["tfx_warp_perspective_u8"] == L.SIGNATURES["tfx_warp_affine_u8"]
    assert L.ABI_VERSION == 11 == L.header_abi_version()
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    assert "int tfx_warp_perspective_u8(const void* in, void* out, void* coverage" in hdr and hdr.count("without a new") >= 4
    assert "floor((Nx * 256) / D)" in hdr and "NO read of `in`" in hdr


def test_entry_point_checks_its_arguments(lib):
    p = [k << 20 for k in range(1, 6)]                                           # in, out, coverage, m, taps: never dereferenced, every call is refused
    call = lambda ptrs=p, dims=(2, 8, 8, 3, 4, 4): lib.tfx_warp_perspective_u8(ptrs[0], ptrs[1], ptrs[2], *dims, ptrs[3], ptrs[4], None)
    for k in (0, 1, 3, 4):                                                       # coverage alone may be NULL
        assert call(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_warp_perspective_u8: null pointer" in lib.tfx_last_error()
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
    assert b"warp_perspective_u8" in lib.tfx_last_error()


def test_ops_wrapper_checks_before_it_launches(monkeypatch):
    import inspect
    from textflux_amd import ops
    from textflux_amd.pipeline import FluxFillPipeline
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.warp_perspective_u8(img, IDENT, (4, 4))                              # no CPU fallback
    assert hasattr(FluxFillPipeline, "warp_perspective")
    for f in (bd.prepare_plain, bd.prepare_eval_item, pl.prepare_scene_lines, pl.prepare_lines):
        assert inspect.signature(f).parameters["warp_quad"].default is None
    # the host-array magnitude check, at the destination's four corner pixels; D <= 0 is allowed
    big = IDENT.copy()
    big[0] = 1 << 50
    ops._perspective_magnitudes(big.reshape(1, 9), 4, 16)                        # 15 * 2^50 < 2^54
    for bad, size in ((big, (4, 17)), (np.where(np.arange(9) == 4, 1 << 52, IDENT), (5, 4)), (np.where(np.arange(9) == 8, 1 << 54, IDENT), (4, 4)),
                      (np.where(np.arange(9) == 2, -(1 << 54), IDENT), (1, 1))):
        with pytest.raises(ValueError, match="2\\^54"):
            ops._perspective_magnitudes(np.asarray(bad, np.int64).reshape(1, 9), *size)
    ops._perspective_magnitudes(np.where(np.arange(9) == 8, -(1 << 60), IDENT).reshape(1, 9), 4, 4)
    # ... and the wrapper applies it to a host array before anything is launched
    monkeypatch.setattr(ops, "_chk_dev", lambda *a: None)
    with pytest.raises(ValueError, match="2\\^54"):
        ops.warp_perspective_u8(img, np.where(np.arange(9) == 8, 1 << 54, IDENT), (4, 4))
    with pytest.raises(ValueError, match=r"int64 \[1, 9\] or \[9\]"):
        ops.warp_perspective_u8(img, IDENT[:6], (4, 4))
