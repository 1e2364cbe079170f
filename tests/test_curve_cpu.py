"""Curved per-line edits without a GPU: the numpy restatement of the grid warp against the affine restatement and known answers, the
ribbon recovered from drawn annular sectors, the rule and its place before perspective and rectify, the upright crop's two guarantees,
the control grids' shapes and precision, the batch driver around a stub pipeline whose grid warp IS the restatement, the refusals, the
CLI flags and the new C entry point (exported, bound, refusing bad arguments on the host)."""
import importlib
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from tests.helpers import curve_ref as cref
from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from tests.helpers import perspective_ref as pref
from tests.helpers import rectify_ref as rref
from textflux_amd import batch_driver as bd
from textflux_amd import curve as cv
from textflux_amd import glyph
from textflux_amd import paste_back as pb
from textflux_amd import per_line as pl
from textflux_amd import perspective as ps
from textflux_amd import rectify as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 1 << 16
NONE = cref.NONE

# the issue's annular sectors: radius of the centre arc, thickness, sweep and tilt of the chord in degrees
SECTORS = [(300, 40, 60, 8), (200, 30, 70, -12), (400, 60, 30, 20), (250, 48, 90, 5)]


def sector(R, T, sweep, tilt=0.0, size=None, centre=None, n=64):
    """(uint8 [H, W] mask, the arc's centre): an arch -- the annular sector of radii R -+ T / 2 that sweeps `sweep` degrees around the
    direction `tilt` degrees clockwise of straight up -- filled by glyph.fill_polygon."""
    ang = np.radians(np.linspace(-90 + tilt - sweep / 2, -90 + tilt + sweep / 2, n))
    if size is None:
        size = (int(2 * (R + T) + 40),) * 2
        centre = (size[0] / 2, R + T + 20)
    cx, cy = centre
    outer = [(cx + (R + T / 2) * math.cos(a), cy + (R + T / 2) * math.sin(a)) for a in ang]
    inner = [(cx + (R - T / 2) * math.cos(a), cy + (R - T / 2) * math.sin(a)) for a in ang[::-1]]
    return glyph.fill_polygon(size[1], size[0], outer + inner)[:, :, 0], (cx, cy)


def rotation(deg, src_centre, dst_centre, scale=1.0):
    """test_rectify_gpu's Q16 matrix: destination pixel p reads the source at src_centre + scale R(deg) (p - dst_centre)."""
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    m = [round(c * Q), round(-s * Q), 0, round(s * Q), round(c * Q), 0]
    m[2] = round(src_centre[0] * Q) - m[0] * dst_centre[0] - m[1] * dst_centre[1]
    m[5] = round(src_centre[1] * Q) - m[3] * dst_centre[0] - m[4] * dst_centre[1]
    return np.array(m, np.int64)


BORDER = (rotation(17, (37.3, 18.2), (14, 20)), rotation(-17, (10.0, 2.5), (27, 20), 1.3))    # test_rectify_gpu's "border" case
IDENT6 = np.array([Q, 0, 0, 0, Q, 0], np.int64)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shift", [0, 3, 5])
def test_embedded_affine_grid_is_the_affine_restatement(shift):
    x = np.random.default_rng(1).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    want, want_cov = rref.warp_affine(x, np.stack(BORDER), (29, 41), coverage=True)
    grid = np.stack([cref.embed(a, shift, (29, 41)) for a in BORDER])
    assert grid.shape == (2, ((29 - 1) >> shift) + 2, ((41 - 1) >> shift) + 2, 2)
    got, cov = cref.warp_grid(x, grid, shift, (29, 41), coverage=True)
    assert (want_cov == 0).any() and (want_cov == 255).any()                     # both kinds of pixel are compared
    assert np.array_equal(got, want) and np.array_equal(cov, want_cov)


def test_marked_nodes_give_nothing_even_through_a_weightless_corner():
    x = np.random.default_rng(3).integers(1, 256, (1, 12, 12, 3), dtype=np.uint8)
    grid = cref.embed(IDENT6, 2, (12, 12))
    out, cov = cref.warp_grid(x, grid, 2, (12, 12), coverage=True)
    assert (out == x).all() and (cov == 255).all()
    grid[1, 1, 0] = NONE                                                         # the node of destination pixel (4, 4): a corner of four cells
    out, cov = cref.warp_grid(x, grid, 2, (12, 12), coverage=True)
    off = np.zeros((12, 12), bool)
    off[:8, :8] = True
    assert (out[0][off] == 0).all() and (cov[0][off] == 0).all() and (out[0][~off] == x[0][~off]).all() and (cov[0][~off] == 255).all()
    # pixel (0, 0) sees the marked node only as its g11, whose weight ax ay is 0 there: still nothing
    on, _, _ = cref.positions(grid, 2, (12, 12))
    assert not on[0, 0] and grid[0, 0, 0] != NONE and grid[0, 1, 0] != NONE and grid[1, 0, 0] != NONE
    # a marker in y alone marks nothing
    grid = cref.embed(IDENT6, 2, (12, 12))
    grid[1, 1, 1] = NONE
    assert cref.positions(grid, 2, (12, 12))[0].all()


def _python_positions(grid, shift, out_size):
    """The header's arithmetic per pixel in Python integers, floored (Python's >> floors) and truncated towards zero."""
    c = 1 << shift
    floor, trunc = np.zeros(out_size + (2,), np.int64), np.zeros(out_size + (2,), np.int64)
    for j in range(out_size[0]):
        for i in range(out_size[1]):
            gx, gy, ax, ay = i >> shift, j >> shift, i & (c - 1), j & (c - 1)
            for k in (0, 1):
                g = [int(grid[gy + a, gx + b, k]) for a in (0, 1) for b in (0, 1)]
                total = (c - ax) * (c - ay) * g[0] + ax * (c - ay) * g[1] + (c - ax) * ay * g[2] + ax * ay * g[3]
                floor[j, i, k] = total >> (2 * shift)
                trunc[j, i, k] = -((-total) >> (2 * shift)) if total < 0 else total >> (2 * shift)
    return floor, trunc


def test_negative_positions_with_fractions_floor():
    rng = np.random.default_rng(5)
    shift, size = 3, (19, 27)
    grid = cref.embed(rotation(9, (-6.3, -4.7), (13, 9)), shift, size) + rng.integers(-Q, Q, cref.grid_shape(size, shift) + (2,))
    floor, trunc = _python_positions(grid, shift, size)
    _, X, Y = cref.positions(grid, shift, size)
    assert np.array_equal(X, floor[..., 0]) and np.array_equal(Y, floor[..., 1])
    differ = (floor != trunc).any(axis=2)
    assert differ.mean() > 0.3 and (X < 0).mean() > 0.3 and (X >= 0).any()       # the case holds such pixels, and others
    # ... and the difference reaches the sampler: where the Q16 position differs by one, so may the 8-bit fraction and the integer part
    assert ((floor[..., 0] >> 8) != (trunc[..., 0] >> 8)).any()
    x = rng.integers(0, 256, (1, 23, 31, 1), dtype=np.uint8)
    out, cov = cref.warp_grid(x, grid, shift, size, coverage=True)
    assert (cov == 255).any() and (cov == 0).any()


def test_a_constant_survives_forward_and_back():
    m, _ = sector(200, 30, 70, -12)
    rb = cv.select_ribbon(rc.mask_points(m), 8, 2, pad=0.0, min_side=96)
    x0, y0, x1, y1 = cv.ribbon_window(rb, m.shape[::-1])
    fwd, back, shift = cv.grids(rb, (x0, y0), (y1 - y0, x1 - x0))
    src = np.full((1,) + m.shape + (1,), 137, np.uint8)
    up = cref.warp_grid(src, fwd, shift, (rb.rh, rb.rw))
    again, cov = cref.warp_grid(up, back, shift, (y1 - y0, x1 - x0), coverage=True)
    assert (up == 137).all() and (again[cov == 255] == 137).all() and (again[cov == 0] != 137).sum() == 0 and 0 < (cov == 255).sum() < cov.size


# ---------------------------------------------------------------------------------------------- the ribbon of a region
@pytest.fixture(scope="module")
def fitted():
    """Every sector's (mask, arc centre, points, Line), fitted once."""
    out = {}
    for sec in SECTORS:
        m, c = sector(*sec)
        pts = rc.mask_points(m)
        out[sec] = (m, c, pts, cv.fit_line(pts))
    return out


@pytest.mark.parametrize("sec", SECTORS)
def test_fit_line_recovers_a_drawn_arc_and_encloses_the_region(fitted, sec):
    """Reached here (centre line / half-thickness against the drawn ones, px): 0.60 / 0.64, 0.77 / 0.57, 0.60 / 0.62, 0.83 / 0.61 -- about
    the raster's own uncertainty; the 3 px is a gate against a broken estimator, not an accuracy claim."""
    R, T, sweep, tilt = sec
    m, (cx, cy), pts, line = fitted[sec]
    assert line is not None
    on_line = cv.point_at(line, np.linspace(line.u0, line.u0 + line.length, 400))
    err = float(np.abs(np.hypot(on_line[:, 0] - cx, on_line[:, 1] - cy) - R).max())
    print(f"sector {sec}: centre line within {err:.2f} px, half-thickness {line.half:.2f} against {T / 2}, length {line.length:.1f} "
          f"against {R * math.radians(sweep):.1f}, r_min {line.r_min:.1f}")
    assert err <= 3.0 and abs(line.half - T / 2) <= 3.0
    u, v = cv.project(line, pts)                                                 # EVERY mask pixel, not only the boundary the fit used
    assert (np.abs(v) <= line.half + 1e-9).all() and u.min() >= line.u0 - 1e-9 and u.max() <= line.u0 + line.length + 1e-9
    assert abs(line.length - R * math.radians(sweep)) <= 6.0 and abs(line.r_min - R) <= 0.1 * R
    assert abs(line.sagitta - R * (1 - math.cos(math.radians(sweep / 2)))) <= 3.0 and abs(line.turn - sweep) <= 5.0 and abs(line.angle - tilt) <= 1.0
    # x grows along the line, and v > 0 is below it: the arch's inner side
    a, b = cv.point_at(line, line.u0), cv.point_at(line, line.u0 + line.length)
    assert b[0] > a[0] and np.hypot(*(cv.point_at(line, line.u0 + line.length / 2, 5.0) - (cx, cy))) < R - 3.0


def test_beyond_its_ends_the_line_is_straight_not_a_polynomial(fitted):
    line = fitted[SECTORS[1]][3]
    P, T, S = cv._polyline(line)
    assert S[0] == pytest.approx(-line.ramp) and line.ramp == pytest.approx(line.r_min / 4)
    far = cv.point_at(line, S[-1] + np.array([0.0, 100.0, 1000.0]))
    assert np.allclose(far[1] - far[0], 100 * T[-1]) and np.allclose(far[2] - far[0], 1000 * T[-1])
    # the ramp: the curvature falls to nothing, without a jump at either end of it
    ang = np.unwrap(np.arctan2(T[:, 1], T[:, 0]))
    kappa = np.abs(np.diff(ang) / np.diff(S))
    assert kappa[0] < 0.02 / line.r_min and kappa[-1] < 0.02 / line.r_min and kappa.max() <= 1.001 / line.r_min
    assert np.abs(np.diff(kappa)).max() < 0.01 / line.r_min
    # projecting a point of the continuation finds it again
    u, v = cv.project(line, cv.point_at(line, np.array([S[0] - 50.0, S[-1] + 70.0]), np.array([12.0, -9.0])))
    assert np.allclose(u, [S[0] - 50.0, S[-1] + 70.0]) and np.allclose(v, [12.0, -9.0])


def drawn(length, thickness, deg, centre=(256, 256), size=(512, 512)):
    """test_rectify_cpu's mask: a length x thickness rectangle around `centre` whose long side points along (cos deg, sin deg)."""
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    pts = [np.array(centre) + su * u * length / 2 + sv * v * thickness / 2 for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    im = Image.new("L", size, 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in pts], fill=255)
    return np.array(im)


TAPER2 = [(100, 100), (400, 140), (400, 220), (100, 260)]                        # test_perspective_cpu's 2:1 trapezoid


class Warps:
    """The three warps as the restatements."""

    def __init__(self):
        self.warps, self.quad_warps, self.grid_warps = [], [], []

    def warp_affine(self, image, m, out_size, coverage=False):
        self.warps.append((np.array(image), np.array(m), tuple(out_size)))
        return rref.warp_affine(image, m, out_size, coverage=coverage)

    def warp_perspective(self, image, m, out_size, coverage=False):
        self.quad_warps.append((np.array(image), np.array(m), tuple(out_size)))
        return pref.warp_perspective(image, m, out_size, coverage=coverage)

    def warp_grid(self, image, grid, shift, out_size, coverage=False):
        self.grid_warps.append((np.array(image), np.array(grid), int(shift), tuple(out_size)))
        return cref.warp_grid(image, grid, shift, out_size, coverage=coverage)


def _path(mask, cfg):
    w = Warps()
    scene = Image.fromarray(np.zeros(mask.shape + (3,), np.uint8))
    _, _, extra = bd._edit_inputs(scene, Image.fromarray(mask).convert("RGB"), cfg, w.warp_affine, w.warp_perspective, w.warp_grid)
    return type(extra.get("rect")).__name__


def test_which_lines_take_the_curved_path(fitted):
    cfg = bd._paste_back_cfg(dict(per_line=True, rectify=True, perspective=True, curve=True))
    others = bd._paste_back_cfg(dict(per_line=True, rectify=True, perspective=True))
    claimed = []
    for sec in SECTORS:
        m, _, pts, line = fitted[sec]
        assert cv.is_curved(line) and cv.is_curved(line, cfg["curve"])
        rb = cv.plan(m, cfg)
        assert isinstance(rb, cv.Ribbon) and rb == cv.select_ribbon(pts, 16, 4, line=line)
        claimed += [sec] if ps.plan(m, cfg) is not None else []
        assert cv.plan(m, others) is None
    print("perspective.plan would take", claimed)
    assert len(claimed) >= 1                                                     # so trying the curve first is what keeps these from perspective
    m = fitted[claimed[0]][0]
    assert _path(m, cfg) == "Ribbon" and _path(m, others) == "Quad"
    # a rectangle at 25 degrees and a 2:1 trapezoid have a straight centre line: they keep their paths
    rect, trap = drawn(300, 60, 25), glyph.fill_polygon(400, 512, TAPER2)[:, :, 0]
    for m, path in ((rect, "Rect"), (trap, "Quad")):
        line = cv.fit_line(rc.mask_points(m))
        assert line is not None and line.sagitta < 0.05 * 2 * line.half and not cv.is_curved(line) and cv.plan(m, cfg) is None
        assert _path(m, cfg) == path == _path(m, others)
    # a disc: no bend, no length
    yy, xx = np.mgrid[0:200, 0:200]
    disc = np.where((xx - 100) ** 2 + (yy - 100) ** 2 <= 60 ** 2, 255, 0).astype(np.uint8)
    assert not cv.is_curved(cv.fit_line(rc.mask_points(disc))) and cv.plan(disc, cfg) is None and _path(disc, cfg) == "NoneType"
    assert not cv.is_curved(None) and cv.fit_line(np.zeros((0, 2), np.int64)) is None and cv.plan(np.zeros((8, 8), np.uint8), cfg) is None
    # each limit decides on its own
    line = fitted[SECTORS[0]][3]
    for key, value in (("min_bend", 2.0), ("min_aspect", 20.0), ("min_fill", 0.99), ("max_turn", 30.0), ("max_angle", 5.0)):
        assert not cv.is_curved(line, cv.curve_cfg({key: value})), key


def test_a_bend_too_tight_for_its_crop_falls_back():
    """(150, 36, 50 degrees) with min_side = 256: the crop reaches 128 px from a centre line of radius 150, beyond max_squeeze at every p_k."""
    m, _ = sector(150, 36, 50)
    pts = rc.mask_points(m)
    line = cv.fit_line(pts)
    assert cv.is_curved(line) and abs(line.r_min - 150) <= 25
    assert cv.select_ribbon(pts, 16, 4, min_side=256, line=line) is None
    assert cv.select_ribbon(pts, 8, 2, pad=0.0, min_side=96, line=line) is not None          # ... while a smaller crop serves it
    cfg = bd._paste_back_cfg(dict(per_line=True, curve=True, perspective=True, region=dict(min_side=256)))
    assert cv.plan(m, cfg) is None and _path(m, cfg) in ("Quad", "NoneType")


@pytest.mark.parametrize("region", [{}, dict(pad=0.0, min_side=96)], ids=["default", "tight"])
@pytest.mark.parametrize("sec", SECTORS)
def test_select_ribbon_keeps_its_two_guarantees(fitted, sec, region):
    m, _, pts, line = fitted[sec]
    d, r = (16, 4) if not region else (8, 2)
    rb = cv.select_ribbon(pts, d, r, line=line, **region)
    assert rb is not None and rb.line == line
    h = pb.halo(d, r)
    assert (rb.iw, rb.ih) == (math.ceil(line.length - 1e-6) + 1, math.ceil(2 * line.half - 1e-6) + 1)
    least = math.ceil((h + 1) * math.sqrt(2))
    assert min(rb.ox, rb.rw - rb.ox - rb.iw, rb.oy, rb.rh - rb.oy - rb.ih) >= least
    assert rb.rw >= region.get("min_side", 256) and rb.rh >= region.get("min_side", 256) and (rb.tw, rb.th) == (rb.rw, rb.rh)
    # (a) no fold
    v0 = rb.oy + (rb.ih - 1) / 2
    reach = max(v0, rb.rh - 1 - v0)
    assert (reach + (1 << rb.shift) * math.sqrt(2)) / line.r_min <= 0.75
    assert rb.shift == max(s for s in range(5) if (1 << 2 * s) / (4 * (line.r_min - reach)) <= 1 / 16)       # the issue's formula
    # (b) coverage, on the restated backward warp over the window
    x0, y0, x1, y1 = cv.ribbon_window(rb, m.shape[::-1])
    back = cv.backward_grid(rb, (x0, y0), (y1 - y0, x1 - x0))
    _, cov = cref.warp_grid(np.zeros((1, rb.rh, rb.rw, 1), np.uint8), back, rb.shift, (y1 - y0, x1 - x0), coverage=True)
    alpha = ref.alpha_mask(m[None, y0:y1, x0:x1], d, r)
    assert (alpha > 0).any() and (cov[alpha > 0] == 255).all() and (cov == 0).any()
    # ... and every such pixel maps at least a pixel inside the crop's border
    ys, xs = np.nonzero(alpha[0] > 0)
    xy, dist = cv.scene_to_crop(rb, np.stack([xs + x0, ys + y0], axis=1))
    assert xy.min() >= 1 and xy[:, 0].max() <= rb.rw - 2 and xy[:, 1].max() <= rb.rh - 2 and dist.max() < 0.75 * line.r_min


# ---------------------------------------------------------------------------------------------- the control grids
def _blend(grid, shift, px, py):
    """The restated interpolation at real destination positions: (positions [n, 2] in pixels, whether a marked node takes part)."""
    c = 1 << shift
    gx, gy = np.floor(px / c).astype(int), np.floor(py / c).astype(int)
    ax, ay = (px / c - gx)[:, None], (py / c - gy)[:, None]
    four = [grid[gy, gx], grid[gy, gx + 1], grid[gy + 1, gx], grid[gy + 1, gx + 1]]
    marked = sum(g[:, 0] == NONE for g in four) > 0
    g00, g01, g10, g11 = (g.astype(np.float64) for g in four)
    return ((1 - ax) * (1 - ay) * g00 + ax * (1 - ay) * g01 + (1 - ax) * ay * g10 + ax * ay * g11) / Q, marked


M = 300                               # the margin of the window below around the sector's own raster


@pytest.mark.parametrize("region", [{}, dict(pad=0.0, min_side=96)], ids=["default", "tight"])
@pytest.mark.parametrize("sec", SECTORS)
def test_grids_have_their_shapes_and_compose_to_the_identity_within_a_quarter_pixel(fitted, sec, region):
    """Reached here: 0.17 px at the worst (the 632 x 359 crop of the first sector, on its squeezed inner edge), 0.02 .. 0.09 px elsewhere."""
    m, _, pts, line = fitted[sec]
    rb = cv.select_ribbon(pts, 16, 4, line=line, **region)
    foot = cv.footprint(rb)
    assert foot.min() > -M + 8 and foot[:, 0].max() < m.shape[1] + M - 8 and foot[:, 1].max() < m.shape[0] + M - 8
    H, W = m.shape[0] + 2 * M, m.shape[1] + 2 * M                                 # a window around the whole footprint, and more
    fwd, back, shift = cv.grids(rb, (-M, -M), (H, W))
    assert shift == rb.shift and fwd.dtype == back.dtype == np.int64
    assert fwd.shape == cref.grid_shape((rb.rh, rb.rw), shift) + (2,) and back.shape == cref.grid_shape((H, W), shift) + (2,)
    marked = back[..., 0] == NONE
    assert (fwd != NONE).all() and (back[..., 1] != NONE).all() and np.abs(fwd).max() < 1 << 50 and np.abs(back[~marked]).max() < 1 << 50
    # forward against the map itself
    on, X, Y = cref.positions(fwd, shift, (rb.rh, rb.rw))
    yy, xx = np.mgrid[0:rb.rh, 0:rb.rw]
    exact = cv.crop_to_scene(rb, np.stack([xx, yy], -1).astype(np.float64))
    f_err = float(np.hypot(X / Q - exact[..., 0], Y / Q - exact[..., 1]).max())
    # forward, then backward
    inner = ((xx >= 2) & (xx <= rb.rw - 3) & (yy >= 2) & (yy <= rb.rh - 3)).ravel()
    pos, off = _blend(back, shift, X.ravel() / Q + M, Y.ravel() / Q + M)
    err = np.hypot(pos[:, 0] - xx.ravel(), pos[:, 1] - yy.ravel())
    print(f"sector {sec} {region}: crop {rb.rw} x {rb.rh}, shift {shift}, forward {f_err:.4f} px, forward and back {err[inner].max():.4f} px, "
          f"{int(marked.sum())} marked nodes")
    assert on.all() and not off[inner].any() and f_err <= 1 / 16 and err[inner].max() <= 0.25


def test_the_backward_grid_marks_what_has_no_unique_projection(fitted):
    m, (cx, cy), pts, line = fitted[SECTORS[1]]
    rb = cv.select_ribbon(pts, 16, 4, line=line)
    back = cv.backward_grid(rb, (0, 0), m.shape)
    marked = back[..., 0] == NONE
    c = 1 << rb.shift
    gy, gx = np.nonzero(marked)
    assert marked.any() and not marked.all()
    assert marked[int(round(cy)) // c, int(round(cx)) // c]                       # the arc's own centre: every point of the arc is as near
    d = np.hypot(gx * c - cx, gy * c - cy)
    assert (d[gy * c > cy - 0.05 * line.r_min] >= 0).all() and d.min() < 0.15 * line.r_min
    # the default window is the footprint's own box
    assert cv.backward_grid(rb).shape[0] >= ((int(cv.footprint(rb)[:, 1].max())) >> rb.shift) + 1
    x0, y0, x1, y1 = cv.ribbon_window(rb, m.shape[::-1])
    foot = cv.footprint(rb)
    assert (x0, y0) == (max(math.floor(foot[:, 0].min()), 0), max(math.floor(foot[:, 1].min()), 0)) and x1 <= m.shape[1] and y1 <= m.shape[0]
    with pytest.raises(ValueError, match="outside the image"):
        cv.ribbon_window(rb, (5, 5)) if foot[:, 0].min() > 5 else cv.ribbon_window(rb._replace(line=line._replace(cx=line.cx + 1e6)), (5, 5))


# ---------------------------------------------------------------------------------------------- the batch driver around a stub
T_, J_, P_ = 6, 8, 4
SCENE_WH, FLAT_BOX, ARC = (640, 480), (40, 30, 200, 60), (200, 30, 70, -12)
ARC_CENTRE = (400, 400)
D, R = 8, 2
REGION = dict(pad=0.0, min_side=96)


def _scene():
    return np.random.default_rng(11).integers(0, 256, (SCENE_WH[1], SCENE_WH[0], 3), dtype=np.uint8)


def _line_masks():
    flat = np.zeros((SCENE_WH[1], SCENE_WH[0]), np.uint8)
    x0, y0, x1, y1 = FLAT_BOX
    flat[y0:y1, x0:x1] = 255
    return flat, sector(*ARC, size=SCENE_WH, centre=ARC_CENTRE)[0]


def _loader(kind):
    if kind == "scene":
        return Image.fromarray(_scene())
    flat, arc = _line_masks()
    return Image.fromarray(flat | arc)


ITEMS = [dict(image="scene", mask="mask", text="LEVEL\nARCH")]                   # in the split order: top to bottom


class Stub(Warps):
    """A pipeline whose result is its input canvas inverted, whose warps are the restatements and whose paste is the restated paste; it
    records what it is handed."""

    def __init__(self):
        super().__init__()
        self.calls, self.encodes, self.pastes, self.text_encoder_2 = [], [], [], object()

    def encode_prompt(self, prompt, prompt_2, device=None, max_sequence_length=512, **kw):
        n = 1 if isinstance(prompt_2, str) else len(prompt_2)
        self.encodes.append(prompt_2)
        return torch.zeros(n, T_, J_), torch.zeros(n, P_), torch.zeros(T_, 3)

    def __call__(self, height, width, image, mask_image, **kw):
        self.calls.append((width, height, [np.array(im) for im in image], [np.array(im) for im in mask_image]))
        return SimpleNamespace(images=[Image.fromarray(255 - np.array(im)) for im in image])

    def paste_back(self, original, edited, mask, dilate=None, feather=None, **kw):
        self.pastes.append(dict(original=np.array(original), edited=np.array(edited), mask=np.array(mask), dilate=dilate, feather=feather, **kw))
        o, e, g = np.array(original)[None], np.array(edited)[None], np.array(mask)[None]
        cm = dict(color_match=kw.get("color_match"), color_ref=None if kw.get("color_ref") is None else kw["color_ref"][None])
        if isinstance(kw.get("rect"), cv.Ribbon):
            rb = kw["rect"]
            return cref.paste_ribbon(o, e, g, dilate, feather, cv.backward_grid(rb, kw["origin"], o.shape[1:3]), rb.shift, rb.rw, rb.rh, **cm)
        assert "rect" not in kw
        if "color_match" in kw:
            return plref.paste(o, e, g, dilate, feather, color_ref=kw["color_ref"][None], **kw["color_match"])[0]
        return ref.paste(o, e, g, dilate, feather)


class Old(Stub):
    """A pipeline that predates warp_grid."""
    warp_grid = property()


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
def with_key():
    pipe = Stub()
    res, saved = _run(pipe, paste_back=dict(per_line=True, dilate=D, feather=R, region=REGION, curve=True, perspective=True, rectify=True))
    return pipe, res, saved


def test_the_level_line_stays_plain_and_the_arch_goes_through_its_ribbon(with_key):
    pipe, res, saved = with_key
    scene = _scene()
    flat, arc = _line_masks()
    assert res["all_done"] == [0] and not res["failed"] and len(pipe.pastes) == 2
    assert len(pipe.grid_warps) == 2 and pipe.warps == [] and pipe.quad_warps == []        # the scene and the mask of ONE line, through the grid alone
    level, arch = pipe.pastes
    assert "rect" not in level and isinstance(arch["rect"], cv.Ribbon)
    rb = cv.select_ribbon(rc.mask_points(arc), D, R, **REGION)
    assert arch["rect"] == rb
    x0, y0, x1, y1 = cv.ribbon_window(rb, SCENE_WH)
    assert tuple(arch["origin"]) == (x0, y0) and np.array_equal(arch["mask"], arc[y0:y1, x0:x1]) and (arch["dilate"], arch["feather"]) == (D, R)
    fwd, back, shift = cv.grids(rb, (x0, y0), (y1 - y0, x1 - x0))
    for (img, g, s, size), src in zip(pipe.grid_warps, (scene, np.repeat(arc[:, :, None], 3, 2))):
        assert np.array_equal(img, src) and np.array_equal(g, fwd) and s == shift and size == (rb.rh, rb.rw)
    up_scene = cref.warp_grid(scene, fwd, shift, (rb.rh, rb.rw))[0]
    up_mask = np.where(cref.warp_grid(np.repeat(arc[:, :, None], 3, 2), fwd, shift, (rb.rh, rb.rw))[0] >= 128, 255, 0).astype(np.uint8)
    want = bd.prepare_plain(0, Image.fromarray(up_scene), Image.fromarray(up_mask), ["ARCH"])        # the usual preparation, of the upright crop
    got = next(c for c in pipe.calls if (c[0], c[1]) == want.size and np.array_equal(c[2][0], np.array(want.image)))
    assert np.array_equal(got[3][0], np.array(want.mask))
    # the upright mask is a level bar that fills the inner rectangle: the bend is gone
    bar = up_mask[:, :, 0] > 0
    cols, rows = np.flatnonzero(bar.any(axis=0)), np.flatnonzero(bar.any(axis=1))
    heights = bar[:, cols[5:-5]].sum(axis=0)
    tops = bar[:, cols[5:-5]].argmax(axis=0)
    assert abs(int(heights.max()) - rb.ih) <= 3 and heights.max() - heights.min() <= 3 and tops.max() - tops.min() <= 3
    assert abs(len(cols) - rb.iw) <= 3 and abs(int(cols[0]) - rb.ox) <= 2 and abs(int(rows[0]) - rb.oy) <= 2
    # ---- the pasted scene is the restated composition, line by line onto the running result, in the split order
    out = scene.copy()
    reg = pb.select_region(flat, D, R, **REGION)
    out[reg.y0:reg.y1, reg.x0:reg.x1] = ref.paste(out[None, reg.y0:reg.y1, reg.x0:reg.x1], level["edited"][None],
                                                  flat[None, reg.y0:reg.y1, reg.x0:reg.x1], D, R)[0]
    assert np.array_equal(arch["original"], out[y0:y1, x0:x1])                   # the CURRENT pixels of the window
    edited = (255 - got[2][0])[glyph.crop_box(want.size, want.meta)[1]:]
    assert np.array_equal(arch["edited"], edited)
    out[y0:y1, x0:x1] = cref.paste_ribbon(out[None, y0:y1, x0:x1], edited[None], arc[None, y0:y1, x0:x1], D, R, back, shift, rb.rw, rb.rh)[0]
    assert np.array_equal(saved[0], out)
    grown = np.zeros_like(flat, bool)
    for m in (flat, arc):
        assert not (grown & (ref.dilate(m, D + 3 * R) > 0)).any()
        grown |= ref.dilate(m, D + 3 * R) > 0
    assert (saved[0][~grown] == scene[~grown]).all()
    for m in (flat, arc):
        assert (saved[0][m >= 128] != scene[m >= 128]).any()


def test_a_level_line_yields_the_same_work_as_without_the_key(with_key):
    pipe = Stub()
    base = dict(per_line=True, dilate=D, feather=R, region=REGION)
    cfg0, cfg1 = bd._paste_back_cfg(base), bd._paste_back_cfg(dict(base, curve=True))
    w0 = pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg0)
    w1 = pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg1, warp_grid=pipe.warp_grid)
    assert [type(w.rect).__name__ for w in w0] == ["NoneType", "NoneType"] and [type(w.rect).__name__ for w in w1] == ["NoneType", "Ribbon"]
    _same_work(w0[0], w1[0])
    assert w0[1].size != w1[1].size or not np.array_equal(np.array(w0[1].image), np.array(w1[1].image))
    assert len(pipe.grid_warps) == 2                                             # the level line launched nothing
    # the key set but no grid warp at hand: nobody takes the path
    for a, b in zip(w0, pl.prepare_lines(0, ITEMS[0], _loader, False, None, cfg1)):
        _same_work(a, b)
    # and in the whole run the level line got the paste of a run without the key
    without = Stub()
    _, saved = _run(without, paste_back=base)
    assert without.grid_warps == [] and "rect" not in without.pastes[1]
    assert set(without.pastes[0]) == set(with_key[0].pastes[0])
    for f in ("original", "edited", "mask", "dilate", "feather"):
        assert np.array_equal(without.pastes[0][f], with_key[0].pastes[0][f]), f
    grown = ref.dilate(_line_masks()[0], D + 3 * R) > 0
    assert (saved[0][grown] == with_key[2][0][grown]).all()


def test_color_match_gets_the_original_window_as_its_reference():
    scene = _scene()
    pipe = Stub()
    res, saved = _run(pipe, paste_back=dict(per_line=True, dilate=D, feather=R, region=REGION, curve=True, color_match=dict(ring=40, min_pixels=16)))
    assert res["all_done"] == [0]
    p = pipe.pastes[1]
    x0, y0, x1, y1 = cv.ribbon_window(p["rect"], SCENE_WH)
    assert p["color_match"] == pb.color_match_cfg(dict(ring=40, min_pixels=16)) and np.array_equal(p["color_ref"], scene[y0:y1, x0:x1])
    assert "rect" not in pipe.pastes[0]
    grown = sum((ref.dilate(m, D + 3 * R) > 0) for m in _line_masks()) > 0
    assert (saved[0][~grown] == scene[~grown]).all()


def test_refusals_come_before_anything_is_encoded_or_run():
    pipe = Stub()
    for bad, match in ((dict(curve=True), "curve needs per_line"), (dict(per_line=False, curve=True), "curve needs per_line"),
                       (dict(per_line=True, curve=dict(bend=3)), r"unknown keys \['curve.bend'\]"),
                       (dict(per_line=True, curve=dict(min_bend=0)), "min_bend"), (dict(per_line=True, curve=dict(max_squeeze=0.95)), "max_squeeze"),
                       (dict(per_line=True, curve=dict(max_turn=200)), "max_turn"), (dict(per_line=True, curve=dict(min_aspect=0.5)), "min_aspect"),
                       (dict(per_line=True, curve=dict(min_fill=1.5)), "min_fill"), (dict(per_line=True, curve=dict(max_angle=120)), "max_angle"),
                       (dict(per_line=True, curve=7), "curve")):
        with pytest.raises(ValueError, match="paste_back: .*" + match):
            _run(pipe, paste_back=bad)
    with pytest.raises(ValueError, match="unknown keys"):
        cv.curve_cfg(dict(fill=1))
    old = Old()
    assert not hasattr(old, "warp_grid")
    with pytest.raises(ValueError, match="warp_grid"):
        _run(old, paste_back=dict(per_line=True, curve=True))
    with pytest.raises(ValueError, match="warp_grid"):
        pl.edit_scene(old, _loader("scene"), _loader("mask"), ["A", "B"], bd._paste_back_cfg(dict(per_line=True, curve=True)))
    for p in (pipe, old):
        assert p.encodes == [] and p.calls == [] and p.pastes == [] and p.warps == [] and p.quad_warps == [] and p.grid_warps == []
    # ... while that pipeline still serves the same item without the key, and the key changes nothing else in the cfg
    assert _run(old, paste_back=dict(per_line=True, region=REGION))[0]["all_done"] == [0]
    cfg = bd._paste_back_cfg(dict(per_line=True, curve=dict(max_squeeze=0.5)))
    assert cfg == dict(dilate=16, feather=4, region={}, per_line=True,
                       curve=dict(min_bend=cv.MIN_BEND, max_squeeze=0.5, max_turn=120.0, min_aspect=2.0, min_fill=0.7, max_angle=45.0))
    assert bd._paste_back_cfg(dict(per_line=True, curve=None)) == bd._paste_back_cfg(dict(per_line=True, curve=False)) == \
        dict(dilate=16, feather=4, region={}, per_line=True)


def test_run_inference_takes_the_same_path(with_key):
    sys.path.insert(0, REPO)
    ri = importlib.import_module("run_inference")

    class Pipe(Stub):
        _execution_device = "cpu"

        def __call__(self, height, width, image, mask_image, prompt=None, prompt_2=None, generator=None, **kw):
            return Stub.__call__(self, height, width, image, mask_image)
    saved = ri.scheduler_name
    ri.scheduler_name = ""
    cfg = dict(per_line=True, dilate=D, feather=R, region=REGION, curve=True, perspective=True, rectify=True)
    try:
        pipe = Pipe()
        out = ri.run_inference(_loader("scene"), _loader("mask"), ["LEVEL", "ARCH"], num_steps=2, pipe=pipe, paste_back=cfg)
    finally:
        ri.scheduler_name = saved
    assert np.array_equal(np.array(out), with_key[2][0]) and len(pipe.grid_warps) == 2 and isinstance(pipe.pastes[1]["rect"], cv.Ribbon)


def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    on = ["--paste_back", "--paste_per_line"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.paste_curve, a.paste_curve_min_bend, a.paste_curve_max_squeeze) == (False, None, None)
        a = parser.parse_args(base + on + ["--paste_curve", "--paste_curve_min_bend", "0.4", "--paste_curve_max_squeeze", "0.6"])
        assert (a.paste_curve, a.paste_curve_min_bend, a.paste_curve_max_squeeze) == (True, 0.4, 0.6)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(on) == dict(dilate=16, feather=4, region=None, per_line=True)    # without the new flags: the dict it was
    assert parse(on + ["--paste_curve"])["curve"] is True
    assert parse(on + ["--paste_curve_max_squeeze", "0.6"])["curve"] == dict(max_squeeze=0.6)
    every = parse(on + ["--paste_curve", "--paste_perspective", "--paste_rectify"])
    assert every["curve"] is True and every["perspective"] is True and every["rectify"] is True
    got = bd._paste_back_cfg(parse(on + ["--paste_curve", "--paste_curve_min_bend", "0.4"]))["curve"]
    assert got == dict(min_bend=0.4, max_squeeze=0.75, max_turn=120.0, min_aspect=2.0, min_fill=0.7, max_angle=45.0)
    for flag in (["--paste_curve"], ["--paste_curve_min_bend", "0.4"], ["--paste_curve_max_squeeze", "0.6"]):
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
    assert "tfx_warp_grid_u8" in L.SIGNATURES and hasattr(lib, "tfx_warp_grid_u8")
    assert len(L.SIGNATURES["tfx_warp_grid_u8"][1]) == len(L.SIGNATURES["tfx_warp_affine_u8"][1]) + 1
    assert L.ABI_VERSION == 11 == L.header_abi_version()
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    assert "int tfx_warp_grid_u8(const void* in, void* out, void* coverage" in hdr and hdr.count("without a new") >= 5
    assert "gh = ((out_h - 1) >> shift) + 2" in hdr and "INT64_MIN" in hdr and ">> (2 shift)" in hdr


def test_entry_point_checks_its_arguments(lib):
    p = [k << 20 for k in range(1, 6)]                                           # in, out, coverage, grid, taps: never dereferenced, every call is refused
    call = lambda ptrs=p, dims=(2, 8, 8, 3, 4, 4), shift=3: lib.tfx_warp_grid_u8(ptrs[0], ptrs[1], ptrs[2], *dims, ptrs[3], shift, ptrs[4], None)
    for k in (0, 1, 3, 4):                                                       # coverage alone may be NULL
        assert call(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_warp_grid_u8: null pointer" in lib.tfx_last_error()
    for k in range(6):
        if k != 3:
            dims = [2, 8, 8, 3, 4, 4]
            dims[k] = 0
            assert call(dims=tuple(dims)) != 0 and b"at least 1" in lib.tfx_last_error()
    for c in (0, 5):
        assert call(dims=(2, 8, 8, c, 4, 4)) != 0 and b"1..4 channels" in lib.tfx_last_error()
    for s in (-1, 6, 64):
        assert call(shift=s) != 0 and b"outside 0..5" in lib.tfx_last_error()
    assert call(dims=(65536, 8, 8, 3, 4, 4)) != 0 and b"65535" in lib.tfx_last_error()
    assert call(dims=(2, 8, 8, 3, 600000, 4)) != 0 and b"out_h" in lib.tfx_last_error()
    assert call([p[0], p[0], p[2], p[3], p[4]]) != 0 and b"different buffers" in lib.tfx_last_error()
    assert call([p[0], p[1], p[1], p[3], p[4]]) != 0 and b"different buffers" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2], p[3] + 4, p[4]]) != 0 and b"8-byte aligned" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2], p[3], p[4] + 2]) != 0 and b"8-byte aligned" in lib.tfx_last_error()
    assert b"warp_grid_u8" in lib.tfx_last_error()


def test_ops_wrapper_checks_before_it_launches(monkeypatch):
    import inspect
    from textflux_amd import ops
    from textflux_amd.pipeline import FluxFillPipeline
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    ident = cref.embed(IDENT6, 1, (4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.warp_grid_u8(img, ident, 1, (4, 4))                                  # no CPU fallback
    assert hasattr(FluxFillPipeline, "warp_grid") and ops.GRID_NONE == cv.GRID_NONE == NONE
    for f in (bd.prepare_plain, bd.prepare_eval_item, pl.prepare_scene_lines, pl.prepare_lines):
        assert inspect.signature(f).parameters["warp_grid"].default is None
    monkeypatch.setattr(ops, "_chk_dev", lambda *a: None)                        # every refusal below comes before anything is launched
    big, marked = ident.copy(), ident.copy()
    big[1, 1, 1] = 1 << 50
    marked[1, 1, 0] = NONE
    for bad in ((img, big, 1, (4, 4)), (img, -big, 1, (4, 4)), (img, ident, 6, (4, 4)), (img, ident, -1, (4, 4)), (img, ident, 2, (4, 4)),
                (img, ident[:2], 1, (4, 4)), (img, ident[:, :2], 1, (4, 4)), (img, ident[..., 0], 1, (4, 4)), (img, ident.astype(np.int32), 1, (4, 4)),
                (img, np.stack([ident] * 2), 1, (4, 4)), (img, ident, 1, (0, 4)), (img.float(), ident, 1, (4, 4)), (img[0], ident, 1, (4, 4)),
                (img.permute(0, 2, 1, 3), ident, 1, (4, 4)), (img, torch.from_numpy(ident).int(), 1, (4, 4))):
        with pytest.raises(ValueError):
            ops.warp_grid_u8(*bad)
    with pytest.raises(ValueError, match="2\\^50"):
        ops.warp_grid_u8(img, big, 1, (4, 4))
    with pytest.raises(ValueError, match=r"int64 \[3, 3, 2\] or \[1, 3, 3, 2\]"):
        ops.warp_grid_u8(img, ident[:2], 1, (4, 4))
    # the marker itself passes the magnitude check: the call gets as far as the library (which has no device here)
    monkeypatch.setattr(ops, "_WARP_TAPS", {"cpu": torch.from_numpy(rc.catmull_rom_taps())})
    seen = []
    monkeypatch.setattr(ops.L, "lib", lambda: SimpleNamespace(tfx_warp_grid_u8=lambda *a: seen.append(a) or 0))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    out = ops.warp_grid_u8(img, marked, 1, (4, 4))
    assert tuple(out.shape) == (1, 4, 4, 3) and len(seen) == 1 and seen[0][3:9] == (1, 4, 4, 3, 4, 4) and seen[0][10] == 1
