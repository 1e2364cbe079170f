"""Perspective per-line edits (DESIGN.md section 4 "Perspective lines"): the host-side geometry.  A text line seen at an angle has a
QUADRILATERAL outline whose far side is shorter than its near side; it is cut through the homography that maps an upright rectangle onto
that quad, edited upright next to its level glyph strip, warped back and blended under the same alpha as any other line.  Here: the
quad of a region (hull_quad, order_quad), the rule that says which lines take this path (is_perspective), the upright crop and its
padding (select_quad), the scene window (quad_window) and the integer matrices of both warps (matrices; ops.warp_perspective_u8 /
tfx_warp_perspective_u8).  numpy only: nothing here resamples anything.

No reference counterpart: the reference edits every line through the axis-aligned scene (run_inference.py:409-467); the four-point
`polygon` entries of its annos.json are the quads this module recovers from the filled mask.

Coordinates: rectify.py's pixel-index coordinates, pixel (i, j) has its centre AT (i, j); y points down, "clockwise" is meant on
screen.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import glyph
from .rectify import bounding_window, edit_size, mask_points

# Which lines take the perspective path (is_perspective).  fit = area(quad) / area(its minimum-area rectangle): 1 for a rectangle at any
# angle (that is rectify's ground), about 0.75 for a 2:1 taper.  A starting point, not a tuned value and no quality claim.
MAX_FIT, MAX_TAPER, MIN_ASPECT, MAX_ANGLE = 0.9, 4.0, 1.5, 45.0
MIN_QUAD_SIDE = 8.0                  # pixels: a shorter side has no direction worth trusting
D_BITS = 30                          # matrices(): D = 2^30 at the destination's centre


class Quad(NamedTuple):
    corners: Tuple[Tuple[float, float], ...]     # TL, TR, BR, BL of the line in the scene (order_quad), pixel-index coordinates
    rw: int                          # the upright crop's size: rw along the line, rh across it
    rh: int
    ox: int                          # the line's quad maps onto the inner rectangle (ox, oy) .. (ox + iw - 1, oy + ih - 1) of the crop
    oy: int
    iw: int                          # the inner rectangle's size: the pixel extents L and T of the line (select_quad)
    ih: int
    tw: int                          # the size the upright crop is edited at (its own size unless it exceeds max_side)
    th: int

    WARP = "warp_perspective"        # rectify.Rect's interface

    def forward(self):
        return (matrices(self)[0],)

    def backward(self, origin, size):
        return (matrices(self, origin)[1],)

    def window(self, size):
        return quad_window(self, size)


# ---------------------------------------------------------------------------------------------- the quad of a region
def _hull(points) -> np.ndarray:
    """float64 [n, 2]: the convex hull's vertices in cyclic order (glyph.min_area_rect's hull), [] for a degenerate set.  Only the first and
    last pixel of every row can be a hull vertex, so the rest is dropped first."""
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    if len(pts) == 0:
        return np.zeros((0, 2))
    order = np.lexsort((pts[:, 0], pts[:, 1]))
    pts = pts[order]
    first = np.flatnonzero(np.r_[True, pts[1:, 1] != pts[:-1, 1]])
    last = np.r_[first[1:] - 1, len(pts) - 1]
    pts = np.unique(np.concatenate([pts[first], pts[last]]), axis=0).astype(np.float64)
    if len(pts) < 3:
        return np.zeros((0, 2))
    try:
        from scipy.spatial import ConvexHull
        return pts[ConvexHull(pts).vertices]
    except Exception:                # collinear
        return np.zeros((0, 2))


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def hull_quad(points) -> Optional[np.ndarray]:
    """float64 [4, 2] (cyclic order), or None: the convex hull of the region's pixels reduced to four sides.  One step removes the edge
    whose removal adds the least area: its two neighbouring edges are extended until they meet, which is allowed only when they meet
    BEYOND the edge (otherwise they diverge there and nothing encloses the hull).  Every step only adds area, so the result encloses
    every point.  None: fewer than 4 hull vertices, or a hull on which no edge can be removed."""
    v = _hull(points)
    if len(v) < 4:
        return None
    while len(v) > 4:
        a, b, c, d = np.roll(v, 1, axis=0), v, np.roll(v, -1, axis=0), np.roll(v, -2, axis=0)      # edge k: b -> c; neighbours a -> b, c -> d
        e1, e2 = b - a, c - d        # the two rays: from b along e1, from c along e2
        den = _cross(e1, e2)
        ok = np.abs(den) > 1e-12
        t = np.where(ok, _cross(c - b, e2) / np.where(ok, den, 1.0), -1.0)       # b + t e1 = c + s e2
        s = np.where(ok, _cross(c - b, e1) / np.where(ok, den, 1.0), -1.0)
        ok &= (t >= 0) & (s >= 0)
        if not ok.any():
            return None
        p = b + t[:, None] * e1
        area = np.where(ok, 0.5 * np.abs(_cross(p - b, c - b)), np.inf)
        k = int(np.argmin(area))
        v[k] = p[k]
        v = np.delete(v, (k + 1) % len(v), axis=0)
    return v


def _sides(q: np.ndarray) -> np.ndarray:
    """The lengths of q0 -> q1, q1 -> q2, q2 -> q3, q3 -> q0."""
    return np.hypot(*(np.roll(q, -1, axis=0) - q).T)


def order_quad(q) -> np.ndarray:
    """float64 [4, 2]: the corners of a quad given in either cyclic order, as TL, TR, BR, BL.  They run clockwise on screen; the pair of
    opposite sides with the larger summed length is top and bottom (a tie goes to the more level pair); the direction from the left
    side's midpoint to the right side's has x > 0, and a vertical line reads downward."""
    q = np.asarray(q, np.float64).reshape(4, 2)
    if np.sum(_cross(q, np.roll(q, -1, axis=0))) < 0:        # shoelace, y down: positive is clockwise on screen
        q = q[::-1]
    best = None
    for k in range(4):
        r = np.roll(q, -k, axis=0)
        s = _sides(r)
        dx, dy = (r[1] + r[2] - r[0] - r[3]) / 2
        if dx < -1e-9 or (abs(dx) <= 1e-9 and dy < 0):
            continue
        key = (round(float(s[0] + s[2]), 6), abs(dx))
        if best is None or key > best[0]:
            best = (key, r)
    return best[1].copy()


def _area(q: np.ndarray) -> float:
    return 0.5 * abs(float(np.sum(_cross(q, np.roll(q, -1, axis=0)))))


def _convex(q: np.ndarray) -> bool:
    e = np.roll(q, -1, axis=0) - q
    c = _cross(e, np.roll(e, -1, axis=0))
    return bool((c > 1e-9).all() or (c < -1e-9).all())


# ---------------------------------------------------------------------------------------------- the rule
def perspective_cfg(perspective) -> dict:
    """The perspective option (True or a dict of max_fit, max_taper, min_aspect, max_angle) with its defaults filled in and checked."""
    p = {} if perspective is True else dict(perspective)
    unknown = set(p) - {"max_fit", "max_taper", "min_aspect", "max_angle"}
    if unknown:
        raise ValueError(f"unknown keys {sorted('perspective.' + k for k in unknown)}")
    get = lambda k, default: default if p.get(k) is None else float(p[k])
    cfg = dict(max_fit=get("max_fit", MAX_FIT), max_taper=get("max_taper", MAX_TAPER), min_aspect=get("min_aspect", MIN_ASPECT),
               max_angle=get("max_angle", MAX_ANGLE))
    if not 0.0 < cfg["max_fit"] <= 1.0:
        raise ValueError("perspective: max_fit must lie in (0, 1]")
    if not cfg["max_taper"] >= 1.0:
        raise ValueError("perspective: max_taper must be at least 1")
    if not cfg["min_aspect"] >= 1.0:
        raise ValueError("perspective: min_aspect must be at least 1")
    if not 0.0 <= cfg["max_angle"] <= 90.0:
        raise ValueError("perspective: max_angle must lie in 0..90 (degrees)")
    return cfg


cfg = perspective_cfg                # the name all three line paths share


def is_perspective(quad, cfg: Optional[dict] = None) -> bool:
    """Whether a line whose quad is `quad` (order_quad's TL, TR, BR, BL, or None) is edited through a homography: the quad exists and is
    convex, every side is at least 8 px, fit = area(quad) / area(its minimum-area rectangle) <= max_fit (a rectangle at any angle has
    fit 1 and stays with rectify), both ratios of opposite sides are <= max_taper, length / thickness >= min_aspect (the means of top and
    bottom, and of left and right), and the reading direction lies within max_angle degrees of level."""
    cfg = perspective_cfg(True) if cfg is None else cfg
    if quad is None:
        return False
    q = np.asarray(quad, np.float64).reshape(4, 2)
    if not _convex(q):
        return False
    top, right, bottom, left = _sides(q)
    if min(top, right, bottom, left) < MIN_QUAD_SIDE:
        return False
    (_, _), (w, h), _ = glyph.min_area_rect(q)
    if w * h <= 0 or _area(q) / (w * h) > cfg["max_fit"]:
        return False
    if max(top, bottom) > cfg["max_taper"] * min(top, bottom) or max(left, right) > cfg["max_taper"] * min(left, right):
        return False
    if (top + bottom) < cfg["min_aspect"] * (left + right):
        return False
    dx, dy = (q[1] + q[2] - q[0] - q[3]) / 2
    return bool(abs(math.degrees(math.atan2(dy, dx))) <= cfg["max_angle"])


# ---------------------------------------------------------------------------------------------- the homography
def _homography(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """float64 [3, 3], h22 = 1: the homography that takes the four points src onto dst."""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        b += [u, v]
    return np.append(np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64)), 1.0).reshape(3, 3)


def _apply(h: np.ndarray, pts) -> np.ndarray:
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    w = np.c_[p, np.ones(len(p))] @ h.T
    return w[:, :2] / w[:, 2:3]


def _inner(ox: int, oy: int, iw: int, ih: int) -> np.ndarray:
    return np.array([(ox, oy), (ox + iw - 1, oy), (ox + iw - 1, oy + ih - 1), (ox, oy + ih - 1)], np.float64)


def _outer(rw: int, rh: int) -> np.ndarray:
    """The crop's four corner PIXELS: the warp back covers a position x exactly when 0 <= floor(x) < rw, so what their footprint
    contains is covered."""
    return np.array([(0, 0), (rw - 1, 0), (rw - 1, rh - 1), (0, rh - 1)], np.float64)


def upright_to_scene(quad: Quad) -> np.ndarray:
    """float64 [3, 3]: the homography from the upright crop's pixel coordinates to the scene's, normalised to D = 1 at the crop's centre
    pixel (rw // 2, rh // 2)."""
    h = _homography(_inner(quad.ox, quad.oy, quad.iw, quad.ih), np.asarray(quad.corners, np.float64))
    return h / float(h[2] @ np.array([quad.rw // 2, quad.rh // 2, 1.0]))


def footprint(quad: Quad) -> np.ndarray:
    """float64 [4, 2]: the scene positions of the crop's four corner pixels, a convex quad (select_quad keeps D > 0 on them)."""
    return _apply(upright_to_scene(quad), _outer(quad.rw, quad.rh))


def _inside(poly: np.ndarray, pts: np.ndarray) -> bool:
    """Whether every point lies in the convex polygon (either orientation), its border included."""
    e = np.roll(poly, -1, axis=0) - poly
    c = _cross(e[None], pts[:, None, :] - poly[None])
    return bool((c >= -1e-9).all() or (c <= 1e-9).all())


def _grow(lo: int, hi: int, inner: int, min_side: int) -> Tuple[int, int]:
    """One axis: the margins (lo, hi) around `inner` pixels, grown evenly (floor on the low side) until the axis has min_side pixels."""
    extra = max(int(min_side) - (inner + lo + hi), 0)
    return lo + extra // 2, hi + extra - extra // 2


def _select(q: np.ndarray, dilate: int = 16, feather: int = 4, pad: float = 0.5, min_side: int = 256, max_side: int = 1024,
            max_taper: float = MAX_TAPER) -> Optional[Quad]:
    from .paste_back import halo
    top, right, bottom, left = _sides(q)
    L, T = int(math.ceil(max(top, bottom) + 1 - 1e-6)), int(math.ceil(max(left, right) + 1 - 1e-6))
    h = halo(dilate, feather)
    moved = np.concatenate([q + np.array([sx, sy], np.float64) * (h + 1) for sx in (-1, 1) for sy in (-1, 1)])
    # what rule (b) needs on each side: the moved corners in the frame of the inner rectangle (0, 0) .. (L - 1, T - 1)
    back = np.linalg.inv(_homography(_inner(0, 0, L, T), q))
    w = np.c_[moved, np.ones(len(moved))] @ (back / float(back[2] @ np.append(q.mean(axis=0), 1.0))).T
    if not (w[:, 2] > 1e-9).all():   # a moved corner at or beyond the scene's vanishing line: no upright crop holds it
        return None
    uv = w[:, :2] / w[:, 2:3]
    need = [max(int(math.ceil(v - 1e-9)), 0) for v in (-uv[:, 0].min(), uv[:, 0].max() - (L - 1), -uv[:, 1].min(), uv[:, 1].max() - (T - 1))]
    corners = tuple((float(x), float(y)) for x, y in q)
    tried = set()
    for k in range(4):
        p = max(int(math.ceil(pad * L / (1 << k))), h)
        if p in tried:
            continue
        tried.add(p)
        (l, r), (t, b) = _grow(max(need[0], p), max(need[1], p), L, min_side), _grow(max(need[2], p), max(need[3], p), T, min_side)
        rw, rh = L + l + r, T + t + b
        tw, th = edit_size(rw, rh, max_side)
        quad = Quad(corners, rw, rh, l, t, L, T, tw, th)
        d = np.c_[_outer(rw, rh), np.ones(4)] @ upright_to_scene(quad)[2]
        if (d >= 1.0 / max_taper).all() and _inside(footprint(quad), moved):
            return quad
    return None


def select_quad(points, dilate: int = 16, feather: int = 4, pad: float = 0.5, min_side: int = 256, max_side: int = 1024,
                max_taper: float = MAX_TAPER) -> Optional[Quad]:
    """The upright crop a perspective line is edited through: rectify.select_rect's sizes around the line's quad (order_quad(hull_quad(
    points))).  With L = ceil(max(|top|, |bottom|)) + 1 and T = ceil(max(|left|, |right|)) + 1 (the pixel extents select_rect counts)
    the quad maps onto an inner L x T rectangle of the crop, and a crop whose longer side exceeds max_side is edited at select_rect's
    (tw, th).  Two guarantees decide the margins around the inner rectangle:
      (a) D of the upright -> scene homography, normalised to 1 at the crop's centre pixel, is >= 1 / max_taper at the crop's four corner
          pixels -- D is linear, so it is that over the whole crop and the crop never nears the horizon; and
      (b) the footprint of the crop in the scene (the convex quad of its corner pixels) contains every corner of the line's quad moved by
          (+-(halo + 1), +-(halo + 1)).  The quad encloses the mask and alpha's support is the mask grown by a square of half-width
          halo - 1, so every pixel with alpha > 0, and a pixel more around it, lies inside what the warp back covers.
    Padding in the upright frame is not padding in the scene: a pixel of it is a full scene pixel beside the near side and a fraction of
    one beside the far side.  So each side gets its own margin, max(p, what (b) needs on that side) with the need read off the moved
    corners' positions in the inner rectangle's frame (the inner rectangle is therefore NOT centred in the crop), then each axis grows
    evenly to min_side.  p is the first of p_k = max(ceil(pad L / 2^k), halo(dilate, feather)), k = 0..3, whose crop passes (a); (b) is
    then checked on the finished crop all the same.  None when there is no quad, a moved corner lies beyond the vanishing line, or no
    p_k passes: the line then falls back to the other paths."""
    hq = hull_quad(points)
    if hq is None:
        return None
    return _select(order_quad(hq), dilate, feather, pad, min_side, max_side, max_taper)


def quad_window(quad: Quad, size: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1), half-open: the footprint's bounding box cut at the image (size = (W, H)) -- the scene window a perspective line
    is pasted into (rectify.rect_window's rule).  ValueError when the footprint misses the image."""
    return bounding_window(footprint(quad), size, "quad_window: the quad's footprint lies outside the image")


def _fixed(h: np.ndarray, at) -> np.ndarray:
    """int64 [9]: h scaled so that D = 2^30 at the destination pixel `at`, rounded to integers; m8 then takes up what the rounding of
    m6 and m7 left, so that D is exactly 2^30 there."""
    d = float(h[2] @ np.array([at[0], at[1], 1.0]))
    m = [int(round(float(v))) for v in (h * ((1 << D_BITS) / d)).reshape(9)]
    m[8] = (1 << D_BITS) - m[6] * int(at[0]) - m[7] * int(at[1])
    return np.array(m, np.int64)


def matrices(quad: Quad, origin: Tuple[int, int] = (0, 0)) -> Tuple[np.ndarray, np.ndarray]:
    """(forward, backward), int64 [9] each, for tfx_warp_perspective_u8.  forward: destination = the upright crop [rh, rw], source = the
    scene.  backward: destination = the scene window whose top-left pixel is scene pixel `origin`, source = the upright crop.  Both are
    the float64 homography (and its inverse, shifted by the origin) scaled so that D = 2^30 at the destination's centre -- the crop's
    centre pixel (rw // 2, rh // 2), and the window pixel nearest to where that pixel lands -- and rounded.  With D >= 2^30 / max_taper
    over the crop, rounding m6 and m7 moves D by up to a pixel coordinate's worth of halves, a relative 2^-30 times that coordinate:
    composing the two returns every crop pixel of a 600-pixel crop to within 2e-4 px (tests/test_perspective_cpu.py prints it and
    holds it under 1 / 256, the resampler's own step), and |Nx| = x D stays below 2^44 for scenes up to 2^12 pixels wide."""
    h = upright_to_scene(quad)
    centre = (quad.rw // 2, quad.rh // 2)
    back = np.linalg.inv(h) @ np.array([[1, 0, origin[0]], [0, 1, origin[1]], [0, 0, 1]], np.float64)
    landed = _apply(h, [centre])[0] - np.array(origin, np.float64)
    return _fixed(h, centre), _fixed(back, (round(float(landed[0])), round(float(landed[1]))))


def plan(mask_grey, cfg: dict) -> Optional[Quad]:
    """The Quad a line's mask is edited through under the paste_back cfg (batch_driver._paste_back_cfg), or None when the line stays on
    the other paths: perspective absent, an empty mask, no quad, a quad outside the rule, or no padding that serves it."""
    p = cfg.get("perspective")
    if not p:
        return None
    pts = mask_points(mask_grey)
    hq = hull_quad(pts) if len(pts) else None
    if hq is None:
        return None
    q = order_quad(hq)
    if not is_perspective(q, p):
        return None
    return _select(q, cfg["dilate"], cfg["feather"], max_taper=p["max_taper"], **(cfg.get("region") or {}))
