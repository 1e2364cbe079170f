"""Curved per-line edits (DESIGN.md section 4 "Curved lines"): the host-side geometry.  A text line along a bend -- an arch over a shop
front, a round sign, a bottle -- is no quadrilateral; it is cut as a RIBBON around its own centre line, edited upright next to its level
glyph strip, warped back and blended under the same alpha as any other line.  Here: the centre line and half-thickness of a region
(fit_line), the rule that says which lines take this path (is_curved), the upright crop and its padding (select_ribbon), the scene
window (ribbon_window) and the control grids of both warps (grids; ops.warp_grid_u8 / tfx_warp_grid_u8).  numpy and scipy only:
nothing here resamples anything.

No reference counterpart: the reference edits every line through the axis-aligned scene (run_inference.py:409-467).

Coordinates: rectify.py's pixel-index coordinates, pixel (i, j) has its centre AT (i, j); y points down.  Along the centre line u is
the arc length (0 where the fitted curve begins, negative on the straight continuation before it) and v the signed distance from it,
positive on the side the normal N = (-Ty, Tx) of the tangent T points to -- below a line that reads to the right.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from .perspective import _grow
from .rectify import bounding_window, edit_size, line_frame, mask_points

# Which lines take the curved path (is_curved), and how hard the crop may squeeze the inner edge (select_ribbon).  Starting points, not
# tuned values and no quality claim.
MIN_BEND, MAX_SQUEEZE, MAX_TURN, MIN_ASPECT, MIN_FILL, MAX_ANGLE = 0.2, 0.75, 120.0, 2.0, 0.7, 45.0
DEGREE = 4                           # t(s) across the frame's long axis
REFINE = 2                           # fit_line: rounds in which the fitted line is moved to the middle of the band around it
STEP = 0.125                         # the dense polyline's spacing along s, pixels
VALID = 0.9                          # a backward node further than VALID * r_min from the centre line is marked: no unique projection
GRID_NONE = -(1 << 63)               # ops.GRID_NONE, tfx_warp_grid_u8's "no source" marker (INT64_MIN)
MAX_SHIFT = 4
COARSE = 8                           # project: the k-d tree holds every 8th vertex of the polyline (one per pixel)
MAX_RAMP = 512.0                     # pixels: a nearly straight line needs no longer transition


class Line(NamedTuple):
    cx: float                        # the frame of the region's minimum-area rectangle (rectify.line_frame): centre ...
    cy: float
    theta: float                     # ... and direction of its long axis, degrees, in (-90, 90]: x grows along it
    coef: Tuple[float, ...]          # the centre line t(s) in that frame, numpy.polyval's order
    s0: float                        # ... fitted and used on [s0, s1], the extent of the region's middle along the long axis; beyond both
    s1: float                        # ends the line continues along its end tangents (after a short ramp), never along the polynomial
    u0: float                        # the region's extent along the line: arc lengths u0 .. u0 + length (u = 0 at s0)
    length: float
    half: float                      # the largest distance of a region pixel from the line: the ribbon encloses the region
    r_min: float                     # the smallest radius of curvature on [s0, s1] (inf for a straight line)
    ramp: float                      # beyond s0 and s1 the curvature falls linearly to 0 over this arc length; from there on the line is straight
    sagitta: float                   # the largest distance of the line from its chord
    turn: float                      # the total turning of its tangent, degrees
    angle: float                     # the chord's direction against +x, degrees
    area: int                        # the region's pixel count


class Ribbon(NamedTuple):
    line: Line
    rw: int                          # the upright crop's size: rw along the line, rh across it
    rh: int
    ox: int                          # the region's ribbon maps onto the inner rectangle (ox, oy) .. (ox + iw - 1, oy + ih - 1) of the crop:
    oy: int                          # crop pixel (x, y) is the line's point u = u0 + x - ox moved by v = y - oy - (ih - 1) / 2 along N(u)
    iw: int
    ih: int
    tw: int                          # the size the upright crop is edited at (its own size unless it exceeds max_side)
    th: int
    shift: int                       # the control grids' cell size is 1 << shift destination pixels (grids)

    WARP = "warp_grid"               # rectify.Rect's interface

    def forward(self):
        return forward_grid(self), self.shift

    def backward(self, origin, size):
        return backward_grid(self, origin, size), self.shift

    def window(self, size):
        return ribbon_window(self, size)


# ---------------------------------------------------------------------------------------------- the centre line of a region
def _frame(line: Line):
    a = math.radians(line.theta)
    return np.array([line.cx, line.cy]), np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])


def _ramp(p0: np.ndarray, phi: float, kappa: float, ramp: float, sign: float):
    """The transition beyond an end of the fitted part: from the point p0 with tangent angle phi and curvature kappa, walking along
    sign * tangent, the curvature falls linearly to 0 over the arc length `ramp` (an Euler spiral).  -> (P [n, 2], phi [n]) at arc
    lengths STEP, 2 STEP, .. from p0, integrated with the midpoint rule."""
    n = int(math.ceil(ramp / STEP))
    if n == 0:
        return np.zeros((0, 2)), np.zeros(0)
    a = np.arange(1, n + 1) * (ramp / n)
    turn = lambda x: phi + sign * kappa * (x - x * x / (2.0 * ramp))
    mid = turn(a - 0.5 * ramp / n)
    P = p0 + sign * np.cumsum(np.stack([np.cos(mid), np.sin(mid)], axis=1), axis=0) * (ramp / n)
    return P, turn(a)


@functools.lru_cache(maxsize=8)
def _polyline(line: Line):
    """(P [n, 2], T [n, 2], S [n]): the bent part of the centre line -- the fitted polynomial with a ramp at either end -- as a dense
    polyline in scene coordinates, its unit tangents (from the polynomial's derivative, not from the chords) and the arc length at
    every vertex, 0 at s0.  Beyond P[0] and P[-1] the line is straight along -T[0] and T[-1]."""
    c, e1, e2 = _frame(line)
    n = max(int(math.ceil((line.s1 - line.s0) / STEP)), 1) + 1
    s = np.linspace(line.s0, line.s1, n)
    d1, d2 = np.polyder(np.array(line.coef)), np.polyder(np.array(line.coef), 2)
    t, dt = np.polyval(line.coef, s), np.polyval(d1, s)
    P = c + s[:, None] * e1 + t[:, None] * e2
    phi = math.radians(line.theta) + np.arctan(dt)
    S = np.r_[0.0, np.cumsum(np.hypot(*np.diff(P, axis=0).T))]
    kappa = [float(np.polyval(d2, x) / (1.0 + np.polyval(d1, x) ** 2) ** 1.5) for x in (line.s0, line.s1)]
    P0, phi0 = _ramp(P[0], float(phi[0]), kappa[0], line.ramp, -1.0)
    P1, phi1 = _ramp(P[-1], float(phi[-1]), kappa[1], line.ramp, 1.0)
    step0, step1 = line.ramp / max(len(P0), 1), line.ramp / max(len(P1), 1)
    S = np.r_[-step0 * np.arange(len(P0), 0, -1), S, S[-1] + step1 * np.arange(1, len(P1) + 1)]
    P, phi = np.concatenate([P0[::-1], P, P1]), np.r_[phi0[::-1], phi, phi1]
    return P, np.stack([np.cos(phi), np.sin(phi)], axis=1), S


@functools.lru_cache(maxsize=8)
def _tree(line: Line):
    """Every COARSE-th vertex of the polyline as a k-d tree, built once per line: a paste builds its backward grid on the host, inside
    the call, and a query against all vertices of a curve is slow for points near its centres of curvature."""
    from scipy.spatial import cKDTree
    return cKDTree(_polyline(line)[0][::COARSE])


def point_at(line: Line, u, v=0.0) -> np.ndarray:
    """float64 [..., 2]: the scene position of the line's point at arc length u moved by v along the normal there.  Beyond the fitted
    part and its ramps the line is straight along its end tangent, so the map is an isometry there."""
    P, T, S = _polyline(line)
    u, v = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64))
    uc = np.clip(u, S[0], S[-1])
    C = np.stack([np.interp(uc, S, P[:, 0]), np.interp(uc, S, P[:, 1])], axis=-1)
    Tu = np.stack([np.interp(uc, S, T[:, 0]), np.interp(uc, S, T[:, 1])], axis=-1)
    Tu /= np.linalg.norm(Tu, axis=-1, keepdims=True)
    N = np.stack([-Tu[..., 1], Tu[..., 0]], axis=-1)
    return C + (u - uc)[..., None] * Tu + v[..., None] * N


def project(line: Line, pts) -> Tuple[np.ndarray, np.ndarray]:
    """(u, v), float64 [n] each: the nearest point of the continued centre line to every scene position of pts [n, 2], as its arc length
    and the signed distance from it.  The fitted part is searched through its dense polyline (nearest vertex, then the two segments that
    meet there), the two straight continuations in closed form."""
    P, T, S = _polyline(line)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    best_d = np.full(len(p), np.inf)
    best_u, best_v = np.zeros(len(p)), np.zeros(len(p))

    def take(u, foot, tangent):
        nonlocal best_d, best_u, best_v
        r = p - foot
        d = np.hypot(r[:, 0], r[:, 1])
        v = -tangent[:, 1] * r[:, 0] + tangent[:, 0] * r[:, 1]
        better = d < best_d
        best_d = np.where(better, d, best_d)
        best_u, best_v = np.where(better, u, best_u), np.where(better, np.copysign(d, v), best_v)

    if len(P) > 1:
        _, k = _tree(line).query(p)                                              # the nearest coarse vertex, then the nearest of the fine
        near = np.clip(k[:, None] * COARSE + np.arange(-COARSE, COARSE + 1)[None, :], 0, len(P) - 1)       # vertices around it
        gap = P[near] - p[:, None, :]
        k = near[np.arange(len(p)), (gap * gap).sum(axis=2).argmin(axis=1)]
        for a in (np.maximum(k - 1, 0), np.minimum(k, len(P) - 2)):
            seg = P[a + 1] - P[a]
            ll = np.maximum((seg * seg).sum(axis=1), 1e-300)
            w = np.clip(((p - P[a]) * seg).sum(axis=1) / ll, 0.0, 1.0)
            tang = T[a] + w[:, None] * (T[a + 1] - T[a])
            take(S[a] + w * (S[a + 1] - S[a]), P[a] + w[:, None] * seg, tang / np.linalg.norm(tang, axis=1, keepdims=True))
    a = np.maximum(((p - P[0]) * -T[0]).sum(axis=1), 0.0)                       # the straight continuation before the bent part ...
    take(S[0] - a, P[0] - a[:, None] * T[0], np.broadcast_to(T[0], p.shape))
    a = np.maximum(((p - P[-1]) * T[-1]).sum(axis=1), 0.0)                      # ... and after it
    take(S[-1] + a, P[-1] + a[:, None] * T[-1], np.broadcast_to(T[-1], p.shape))
    return best_u, best_v


def _boundary(points: np.ndarray) -> np.ndarray:
    """The region's pixels that have a 4-neighbour outside it: extremes of any distance over the region lie on them."""
    x0, y0 = points.min(axis=0)
    x1, y1 = points.max(axis=0)
    m = np.zeros((y1 - y0 + 3, x1 - x0 + 3), bool)
    m[points[:, 1] - y0 + 1, points[:, 0] - x0 + 1] = True
    inner = m[1:-1, 1:-1] & m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    ys, xs = np.nonzero(m[1:-1, 1:-1] & ~inner)
    return np.stack([xs + x0, ys + y0], axis=1)


def fit_line(points) -> Optional[Line]:
    """The centre line and the enclosing half-thickness of a region given as [n, 2] (x, y) pixel coordinates, or None when the region
    has no line worth the name (fewer than DEGREE + 4 usable columns).  In the frame of the region's minimum-area rectangle (s along its
    long axis, t across) the RIDGE of the region's Euclidean distance transform is read off per unit column of s -- the mean t of the
    column's pixels within 0.75 of the column's largest distance; a column under an end cap, whose largest distance is below 0.85 of
    that of the columns beside it, has lost its ridge and is dropped -- and a polynomial t(s) of degree 4 is fitted to it by least
    squares.  REFINE rounds then move the line to the middle of the band around it: the boundary pixels are projected onto the line
    (project), the middle between the smallest and the largest signed distance is taken per unit of arc length, and the polynomial is
    refitted through those points; in the line's own coordinates the caps of a bent band stand upright, so only bins that a cap cuts are
    dropped.  The polynomial is used on [s0, s1], the extent of the points it was fitted to, and never beyond: past both ends the line
    continues along its end tangents, after a ramp on which its curvature falls to 0 (Line.ramp, _polyline).  u0, length and half are
    measured last, by projecting the region's boundary pixels onto the continued line, so the ribbon |v| <= half, u0 <= u <= u0 + length
    ENCLOSES the region, as perspective.hull_quad's quad does."""
    from scipy import ndimage
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    if len(pts) < 16:
        return None
    cx, cy, _, _, theta = line_frame(pts)
    a = math.radians(theta)
    e1, e2 = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    x0, y0 = pts.min(axis=0)
    x1, y1 = pts.max(axis=0)
    m = np.zeros((y1 - y0 + 3, x1 - x0 + 3), bool)
    m[pts[:, 1] - y0 + 1, pts[:, 0] - x0 + 1] = True
    dist = ndimage.distance_transform_edt(m)[pts[:, 1] - y0 + 1, pts[:, 0] - x0 + 1]
    rel = pts - np.array([cx, cy])
    s, t = rel @ e1, rel @ e2
    col = np.round(s).astype(np.int64)
    col -= col.min()
    top = np.zeros(col.max() + 1)
    np.maximum.at(top, col, dist)
    ridge = dist >= top[col] - 0.75
    cnt = np.bincount(col[ridge], minlength=len(top)).astype(np.float64)
    # a column under an end cap has lost its ridge: its largest distance is the cap's, well below that of the columns beside it
    reach = 2 * int(math.ceil(top.max())) + 1
    on = (cnt > 0) & (top >= 0.85 * ndimage.maximum_filter1d(top, 2 * reach + 1, mode="nearest"))
    if on.sum() < DEGREE + 4:
        return None
    rs = np.bincount(col[ridge], weights=s[ridge], minlength=len(top))[on] / cnt[on]
    rt = np.bincount(col[ridge], weights=t[ridge], minlength=len(top))[on] / cnt[on]
    edge = _boundary(pts)
    line = _fitted(cx, cy, theta, rs, rt, float(s.min()), float(s.max()), len(pts))
    for _ in range(REFINE):
        if line is None:
            return None
        # in the line's own coordinates the caps of a bent band stand upright: the middle of the band per unit of arc length moves the line
        u, v = project(line, edge)
        b = np.floor(u - u.min()).astype(np.int64)
        lo, hi = np.full(b.max() + 1, np.inf), np.full(b.max() + 1, -np.inf)
        np.minimum.at(lo, b, v)
        np.maximum.at(hi, b, v)
        band = np.where(np.isfinite(lo), hi - lo, 0.0)
        ok = (band > 0) & (band >= 0.9 * ndimage.maximum_filter1d(band, 2 * reach + 1, mode="nearest"))     # a bin a cap cuts says nothing
        lo, hi = np.where(ok, lo, 0.0), np.where(ok, hi, 0.0)
        if ok.sum() < DEGREE + 4:
            return None
        rel = point_at(line, u.min() + np.flatnonzero(ok) + 0.5, 0.5 * (lo + hi)[ok]) - np.array([cx, cy])
        rs, rt = rel @ e1, rel @ e2
        line = _fitted(cx, cy, theta, rs, rt, float(rs.min()), float(rs.max()), len(pts))
    if line is None:
        return None
    u, v = project(line, edge)
    return line._replace(u0=float(u.min()), length=float(u.max() - u.min()), half=float(np.abs(v).max()))


def _fitted(cx, cy, theta, rs, rt, s0, s1, area) -> Optional[Line]:
    """The Line of the least-squares polynomial t(s) through the points (rs, rt) of the frame, used on [s0, s1]; u0, length and half are
    left 0 for fit_line to measure."""
    mid, scale = 0.5 * (s0 + s1), max(0.5 * (s1 - s0), 1.0)
    k = np.polyfit((rs - mid) / scale, rt, DEGREE)
    # back from the normalised abscissa to s: compose with (s - mid) / scale
    coef = np.poly1d(k)(np.poly1d([1.0 / scale, -mid / scale])).coeffs
    coef = tuple(float(c) for c in np.r_[np.zeros(DEGREE + 1 - len(coef)), coef])
    dense = np.linspace(s0, s1, 512)
    d1, d2 = np.polyval(np.polyder(np.array(coef)), dense), np.polyval(np.polyder(np.array(coef), 2), dense)
    kappa = float((np.abs(d2) / (1.0 + d1 * d1) ** 1.5).max())
    phi = np.arctan(d1)
    r_min = 1.0 / kappa if kappa > 1e-12 else math.inf
    # ramp: r_min / 4 is at least v (r_min - v) / r_min for every v, which is what _shift_for's bound asks of it
    line = Line(float(cx), float(cy), float(theta), coef, s0, s1, 0.0, 0.0, 0.0, r_min, min(0.25 * r_min, MAX_RAMP), 0.0,
                float(np.degrees(np.abs(np.diff(phi)).sum())), 0.0, int(area))
    c, e1, e2 = _frame(line)
    P = c + dense[:, None] * e1 + np.polyval(np.array(coef), dense)[:, None] * e2
    chord = P[-1] - P[0]
    cl = float(np.hypot(*chord))
    if cl <= 0:
        return None
    sag = float(np.abs(chord[0] * (P[:, 1] - P[0, 1]) - chord[1] * (P[:, 0] - P[0, 0])).max() / cl)
    return line._replace(sagitta=sag, angle=float(math.degrees(math.atan2(chord[1], chord[0]))))


# ---------------------------------------------------------------------------------------------- the rule
def curve_cfg(curve) -> dict:
    """The curve option (True or a dict of min_bend, max_squeeze, max_turn, min_aspect, min_fill, max_angle) with its defaults filled in
    and checked."""
    p = {} if curve is True else dict(curve)
    keys = dict(min_bend=MIN_BEND, max_squeeze=MAX_SQUEEZE, max_turn=MAX_TURN, min_aspect=MIN_ASPECT, min_fill=MIN_FILL, max_angle=MAX_ANGLE)
    unknown = set(p) - set(keys)
    if unknown:
        raise ValueError(f"unknown keys {sorted('curve.' + k for k in unknown)}")
    cfg = {k: (d if p.get(k) is None else float(p[k])) for k, d in keys.items()}
    if not cfg["min_bend"] > 0.0:
        raise ValueError("curve: min_bend must be positive")
    if not 0.0 < cfg["max_squeeze"] < VALID:
        raise ValueError(f"curve: max_squeeze must lie in (0, {VALID})")
    if not 0.0 < cfg["max_turn"] <= 180.0:
        raise ValueError("curve: max_turn must lie in (0, 180] (degrees)")
    if not cfg["min_aspect"] >= 1.0:
        raise ValueError("curve: min_aspect must be at least 1")
    if not 0.0 < cfg["min_fill"] <= 1.0:
        raise ValueError("curve: min_fill must lie in (0, 1]")
    if not 0.0 <= cfg["max_angle"] <= 90.0:
        raise ValueError("curve: max_angle must lie in 0..90 (degrees)")
    return cfg


cfg = curve_cfg                      # the name all three line paths share


def is_curved(line: Optional[Line], cfg: Optional[dict] = None) -> bool:
    """Whether a line with this centre line (fit_line, or None) is edited through a ribbon.  With thickness = 2 half: sagitta / thickness
    >= min_bend (a rectangle's or a trapezoid's centre line is straight: sagitta 0, rectify's and perspective's ground), arc length /
    thickness >= min_aspect, region area / ribbon area >= min_fill (a blob fills no ribbon), the tangent turns by no more than max_turn
    degrees in all, and the chord lies within max_angle degrees of level."""
    cfg = curve_cfg(True) if cfg is None else cfg
    if line is None or line.half <= 0 or line.length <= 0:
        return False
    thick = 2.0 * line.half
    if line.sagitta < cfg["min_bend"] * thick or line.length < cfg["min_aspect"] * thick:
        return False
    if line.area < cfg["min_fill"] * (line.length + 1.0) * (thick + 1.0):
        return False
    return bool(line.turn <= cfg["max_turn"] and abs(line.angle) <= cfg["max_angle"])


# ---------------------------------------------------------------------------------------------- the crop
def _v0(rb: Ribbon) -> float:
    return rb.oy + (rb.ih - 1) / 2.0


def crop_to_scene(rb: Ribbon, xy) -> np.ndarray:
    """float64 [..., 2]: the scene positions of upright crop positions xy [..., 2]."""
    xy = np.asarray(xy, np.float64)
    return point_at(rb.line, rb.line.u0 + xy[..., 0] - rb.ox, xy[..., 1] - _v0(rb))


def scene_to_crop(rb: Ribbon, pts) -> Tuple[np.ndarray, np.ndarray]:
    """(xy float64 [n, 2], distance float64 [n]): the upright crop positions of scene positions pts [n, 2] by nearest-point projection,
    and their distance from the centre line (the projection is unique below r_min)."""
    u, v = project(rb.line, pts)
    return np.stack([u - rb.line.u0 + rb.ox, v + _v0(rb)], axis=1), np.abs(v)


def _shift_for(line: Line, reach: float) -> Optional[int]:
    """The largest shift in 0..MAX_SHIFT whose cell c = 1 << shift keeps the bilinear interpolation of the ribbon's positions under
    1 / 16 px over a crop that reaches `reach` pixels from the centre line.  Over a c x c cell a map deviates from the bilinear blend of
    its corners by at most c^2 / 8 times its second derivative, per axis.  On an arc of radius r that is 1 / r, c^2 / (4 r) for both
    axes, and r is smallest on the crop's inner edge, r_min - reach.  On a ramp the curvature itself changes, by at most 1 / (r_min ramp)
    per pixel, which moves a point `reach` from the line by reach / (r_min ramp) per pixel squared; with ramp = r_min / 4 that is never
    more than the arc's term.  None when even c = 1 does not pass."""
    room = line.r_min - reach
    if not room > 0:
        return None
    second = max(1.0 / room, reach / (line.r_min * line.ramp) if line.ramp > 0 else 0.0)
    for shift in range(MAX_SHIFT, -1, -1):
        if (1 << (2 * shift)) * second / 4.0 <= 1.0 / 16.0:
            return shift
    return None


def select_ribbon(points, dilate: int = 16, feather: int = 4, pad: float = 0.5, min_side: int = 256, max_side: int = 1024,
                  max_squeeze: float = MAX_SQUEEZE, line: Optional[Line] = None) -> Optional[Ribbon]:
    """The upright crop a curved line is edited through: rectify.select_rect's sizes around the line's ribbon (fit_line(points), or the
    `line` already fitted).  u runs along the crop's width, v across it.  With L = ceil(length) + 1 and T = ceil(2 half) + 1 the ribbon
    maps onto an inner L x T rectangle, padded by p and then grown evenly to min_side per axis; a crop whose longer side exceeds
    max_side is edited at select_rect's (tw, th).  p is the first of p_k = max(ceil(pad L / 2^k), ceil((halo + 1) sqrt 2)), k = 0..3
    -- the sqrt 2 because alpha's support is a square in the SCENE's axes while the ribbon is isometric along its normals and along
    its straight continuations -- whose crop passes
      (a) no fold: (the largest |v| in the crop + c sqrt 2) / r_min <= max_squeeze, c = 1 << shift the grids' cell (_shift_for): the
          inner edge of the crop, and every grid node around it, is then compressed to no less than 1 - max_squeeze of its length and
          stays clear of the centres of curvature, where the nearest-point projection stops being unique; and
      (b) coverage, checked numerically on the finished plan: every boundary pixel of the region moved by (+-(halo + 1), +-(halo + 1))
          projects into the crop.  Alpha's support is the region grown by a square of half-width halo - 1, two pixels less, so every
          pixel with alpha > 0 maps into the crop at least one pixel from its border and lies inside what the warp back covers.
    Along a ramp the ribbon is NOT isometric on its inner side: a scene pixel there spans up to 1 / (1 - max_squeeze) crop pixels.  So,
    as perspective.select_quad does, each side gets max(p, what (b) needs there), the need read off the moved pixels' own projections;
    the inner rectangle is then not always centred.  None when there is no line, no p_k passes (a), or (b) fails on the finished crop
    all the same: the line then falls back to the other paths."""
    from .paste_back import halo
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    line = fit_line(pts) if line is None else line
    if line is None:
        return None
    L, T = int(math.ceil(line.length - 1e-6)) + 1, int(math.ceil(2.0 * line.half - 1e-6)) + 1
    h = halo(dilate, feather)
    least = int(math.ceil((h + 1) * math.sqrt(2.0)))
    moved = np.concatenate([_boundary(pts) + np.array([sx, sy]) * (h + 1) for sx in (-1, 1) for sy in (-1, 1)])
    mu, mv = project(line, moved)
    if not (np.abs(mv) < VALID * line.r_min).all():
        return None
    need = [max(int(math.ceil(x - 1e-9)), 0) for x in (line.u0 - mu.min(), mu.max() - (line.u0 + L - 1),
                                                        -mv.min() - (T - 1) / 2.0, mv.max() - (T - 1) / 2.0)]
    tried = set()
    for k in range(4):
        p = max(int(math.ceil(pad * L / (1 << k))), least)
        if p in tried:
            continue
        tried.add(p)
        (l, r), (t, b) = _grow(max(need[0], p), max(need[1], p), L, min_side), _grow(max(need[2], p), max(need[3], p), T, min_side)
        rw, rh = L + l + r, T + t + b
        reach = max(t + (T - 1) / 2.0, b + (T - 1) / 2.0)
        shift = _shift_for(line, reach)
        if shift is None or reach + (1 << shift) * math.sqrt(2.0) > max_squeeze * line.r_min:
            continue
        tw, th = edit_size(rw, rh, max_side)
        rb = Ribbon(line, rw, rh, l, t, L, T, tw, th, shift)
        xy = np.stack([mu - line.u0 + rb.ox, mv + _v0(rb)], axis=1)
        if (xy >= 0).all() and (xy[:, 0] <= rw - 1).all() and (xy[:, 1] <= rh - 1).all():
            return rb
        return None
    return None


def footprint(rb: Ribbon) -> np.ndarray:
    """float64 [n, 2]: the scene positions of the crop's border pixels, in cyclic order."""
    x, y = np.arange(rb.rw, dtype=np.float64), np.arange(rb.rh, dtype=np.float64)
    edge = np.concatenate([np.stack([x, np.zeros_like(x)], 1), np.stack([np.full_like(y, rb.rw - 1), y], 1),
                           np.stack([x[::-1], np.full_like(x, rb.rh - 1)], 1), np.stack([np.zeros_like(y), y[::-1]], 1)])
    return crop_to_scene(rb, edge)


def ribbon_window(rb: Ribbon, size: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1), half-open: the footprint's bounding box cut at the image (size = (W, H)) -- the scene window a curved line is
    pasted into (rectify.rect_window's rule).  ValueError when the footprint misses the image."""
    return bounding_window(footprint(rb), size, "ribbon_window: the ribbon's footprint lies outside the image")


# ---------------------------------------------------------------------------------------------- the control grids
def _nodes(h: int, w: int, shift: int) -> np.ndarray:
    """float64 [gh, gw, 2]: the destination pixels (q << shift, r << shift) the nodes of a grid over [h, w] stand for."""
    gh, gw = ((h - 1) >> shift) + 2, ((w - 1) >> shift) + 2
    q, r = np.meshgrid(np.arange(gw, dtype=np.float64) * (1 << shift), np.arange(gh, dtype=np.float64) * (1 << shift))
    return np.stack([q, r], axis=-1)


def _q16(pos: np.ndarray) -> np.ndarray:
    return np.round(np.clip(pos, -(2.0 ** 33), 2.0 ** 33) * 65536.0).astype(np.int64)


def grids(rb: Ribbon, origin: Tuple[int, int] = (0, 0), size: Optional[Tuple[int, int]] = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """(forward, backward, shift) for tfx_warp_grid_u8, int64 [gh, gw, 2] each of Q16 source positions (x, y), one node per
    c = 1 << shift destination pixels.  forward: destination = the upright crop [rh, rw], source = the scene; node (r, q) holds
    C(u) + v N(u) of crop pixel (q c, r c).  backward: destination = the scene window [size = (h, w)] whose top-left pixel is scene
    pixel `origin` (None: from the origin to the footprint's far corner), source = the upright crop; a node holds the crop position of
    its scene pixel's nearest point on the continued centre line, (arc length, signed distance), and carries the marker GRID_NONE in
    x where that distance is >= 0.9 r_min: beyond it the projection stops being unique.  select_ribbon's rule (a) keeps the whole crop
    band, and every node of a cell that touches it, inside the unmarked zone.  shift is the ribbon's (_shift_for): the largest of
    0..4 whose interpolation error bound, c^2 / (4 (r_min - reach)) on an arc, stays <= 1 / 16 px."""
    return forward_grid(rb), backward_grid(rb, origin, size), rb.shift


def forward_grid(rb: Ribbon) -> np.ndarray:
    """grids' forward grid alone (what preparing a line needs)."""
    return _q16(crop_to_scene(rb, _nodes(rb.rh, rb.rw, rb.shift)))


def backward_grid(rb: Ribbon, origin: Tuple[int, int] = (0, 0), size: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """grids' backward grid alone (what pasting a line needs)."""
    if size is None:
        far = footprint(rb).max(axis=0)
        size = (max(int(math.ceil(far[1])) + 1 - int(origin[1]), 1), max(int(math.ceil(far[0])) + 1 - int(origin[0]), 1))
    nodes = _nodes(int(size[0]), int(size[1]), rb.shift)
    xy, d = scene_to_crop(rb, nodes.reshape(-1, 2) + np.array(origin, np.float64))
    back = _q16(xy)
    back[d >= VALID * rb.line.r_min, 0] = GRID_NONE
    return back.reshape(nodes.shape)


def plan(mask_grey, cfg: dict) -> Optional[Ribbon]:
    """The Ribbon a line's mask is edited through under the paste_back cfg (batch_driver._paste_back_cfg), or None when the line stays on
    the other paths: curve absent, an empty mask, no centre line, a line outside the rule, or no padding that serves it."""
    p = cfg.get("curve")
    if not p:
        return None
    pts = mask_points(mask_grey)
    line = fit_line(pts) if len(pts) else None
    if not is_curved(line, p):
        return None
    return select_ribbon(pts, cfg["dilate"], cfg["feather"], max_squeeze=p["max_squeeze"], line=line, **(cfg.get("region") or {}))
