"""Rectified per-line edits (DESIGN.md section 4 "Rectified lines"): the host-side geometry.  A slanted text line is cut from the scene
as an ORIENTED rectangle, warped upright, edited upright next to its horizontal glyph strip, warped back and blended under the same
alpha as an unrectified line.  Here: the line's frame (line_frame), the rule that says which lines are rectified (is_rectified), the
oriented rectangle (select_rect: paste_back.select_region's rule in the rotated frame), the Q16 matrices of both warps (matrices)
and the tap table of the device resampler (catmull_rom_taps; ops.warp_affine_u8 / tfx_warp_affine_u8).  numpy only: nothing here
resamples anything.

No reference counterpart: the reference's single-line path stacks a horizontal strip on the axis-aligned scene whatever the line's
orientation (run_inference.py:409-467); only its multi-line canvas follows the minimum-area rectangle (draw_glyph2).

Coordinates: pixel-index coordinates, in which pixel (i, j) has its centre AT (i, j) -- the coordinates of glyph.mask_regions'
points and of the kernel's sample positions.  Angles are in degrees, in image coordinates (y points down): theta > 0 is a line that
descends to the right.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import glyph

# Which lines are rectified: min_angle <= |theta| <= max_angle (degrees) and length / thickness >= min_aspect.  Below min_angle the
# axis-aligned box already fits; above max_angle the line is closer to vertical text, which stays on the unrectified path; a blob
# has no direction worth trusting.  A starting point, not a tuned value and no quality claim.
MIN_ANGLE, MAX_ANGLE, MIN_ASPECT = 5.0, 45.0, 1.5


class Rect(NamedTuple):
    cx: float                        # centre, pixel-index coordinates of the scene
    cy: float
    rw: int                          # the upright crop's size: rw along the line, rh across it (whole pixels, unit scale)
    rh: int
    theta: float                     # degrees; the upright crop's +x axis is the scene direction (cos theta, sin theta)
    tw: int                          # the size the upright crop is edited at (its own size unless it exceeds max_side)
    th: int

    # What batch_driver and paste_back ask of a line's shape (perspective.Quad and curve.Ribbon answer the same four)
    WARP = "warp_affine"             # the pipeline's warp; ops' is WARP + "_u8"

    def forward(self):
        """The warp's arguments after the image, scene -> upright crop."""
        return (matrices(self)[0],)

    def backward(self, origin, size):
        """The same, upright crop -> the scene window [size = (h, w)] whose top-left pixel is scene pixel `origin`."""
        return (matrices(self, origin)[1],)

    def window(self, size):
        return rect_window(self, size)


def catmull_rom_taps() -> np.ndarray:
    """int16 [256][4]: row f = the Catmull-Rom (a = -0.5) weights of the taps at distances 1 + t, t, 1 - t, 2 - t for t = f / 256, with
    14 fractional bits.  Computed in Python integers: with d = 256 |x|, 2 w 256^3 = 3 d^3 - 5 256 d^2 + 2 256^3 for d <= 256 and
    -d^3 + 5 256 d^2 - 8 256^2 d + 4 256^3 beyond, rounded half up to 1 / 2^14; the largest tap then absorbs what the rounding left, so
    that every row sums to exactly 1 << 14."""
    def num(d: int) -> int:
        if d <= 256:
            return 3 * d ** 3 - 5 * 256 * d * d + 2 * 256 ** 3
        return -d ** 3 + 5 * 256 * d * d - 8 * 256 * 256 * d + 4 * 256 ** 3
    out = np.zeros((256, 4), np.int16)
    for f in range(256):
        row = [(num(d) + (1 << 10)) >> 11 for d in (256 + f, f, 256 - f, 512 - f)]      # 2 w 256^3 / 2^25 * 2^14
        row[max(range(4), key=lambda k: row[k])] += (1 << 14) - sum(row)
        out[f] = row
    return out


def line_frame(points) -> Tuple[float, float, float, float, float]:
    """(cx, cy, length, thickness, theta) of a line given as [n, 2] (x, y) pixel coordinates (glyph.mask_regions' points): the
    minimum-area rectangle of the points (glyph.box_points(glyph.min_area_rect(points))).  (cx, cy) is its centre; length and
    thickness are its long and short side, measured between pixel CENTRES (a level run of n pixels is n - 1 long); theta is the
    direction of the long side against +x, normalised into (-90, 90]."""
    box = np.asarray(glyph.box_points(glyph.min_area_rect(np.asarray(points))), np.float64)
    cx, cy = box.mean(axis=0)
    e1, e2 = box[1] - box[0], box[2] - box[1]
    l1, l2 = float(np.hypot(*e1)), float(np.hypot(*e2))
    long_, length, thickness = (e1, l1, l2) if l1 >= l2 else (e2, l2, l1)
    theta = math.degrees(math.atan2(long_[1], long_[0])) if length > 0 else 0.0
    if theta > 90.0 + 1e-9:
        theta -= 180.0
    elif theta <= -90.0 + 1e-9:
        theta += 180.0
    return float(cx), float(cy), length, thickness, float(min(theta, 90.0))


def rectify_cfg(rectify) -> dict:
    """The rectify option (True or a dict of min_angle, max_angle, min_aspect) with its defaults filled in and checked."""
    r = {} if rectify is True else dict(rectify)
    unknown = set(r) - {"min_angle", "max_angle", "min_aspect"}
    if unknown:
        raise ValueError(f"unknown keys {sorted('rectify.' + k for k in unknown)}")
    lo = MIN_ANGLE if r.get("min_angle") is None else float(r["min_angle"])
    hi = MAX_ANGLE if r.get("max_angle") is None else float(r["max_angle"])
    aspect = MIN_ASPECT if r.get("min_aspect") is None else float(r["min_aspect"])
    if not 0.0 <= lo <= hi <= 90.0:
        raise ValueError("rectify: min_angle and max_angle must satisfy 0 <= min_angle <= max_angle <= 90 (degrees)")
    if not aspect >= 1.0:
        raise ValueError("rectify: min_aspect must be at least 1")
    return dict(min_angle=lo, max_angle=hi, min_aspect=aspect)


cfg = rectify_cfg                    # the name all three line paths share (perspective.cfg, curve.cfg)


def is_rectified(frame, min_angle: float = MIN_ANGLE, max_angle: float = MAX_ANGLE, min_aspect: float = MIN_ASPECT) -> bool:
    """Whether a line of this line_frame is edited upright: min_angle <= |theta| <= max_angle and length / thickness >= min_aspect."""
    _, _, length, thickness, theta = frame
    return bool(min_angle <= abs(theta) <= max_angle and length >= min_aspect * thickness)


def _axes(theta: float) -> Tuple[float, float]:
    a = math.radians(theta)
    return math.cos(a), math.sin(a)


def _centre_offsets(rect: Rect) -> Tuple[int, int, float, float]:
    """(ic, jc, da, db): the upright crop's centre pixel (rw // 2, rh // 2) and its offset from the rectangle's centre along the two axes
    (0 for an odd side, half a pixel for an even one)."""
    ic, jc = rect.rw // 2, rect.rh // 2
    return ic, jc, ic + 0.5 - rect.rw / 2.0, jc + 0.5 - rect.rh / 2.0


def edit_size(rw: int, rh: int, max_side: int) -> Tuple[int, int]:
    """(tw, th): the size an upright crop [rh, rw] is edited at: its own, unless its longer side m exceeds max_side; then
    (max(32, rw max_side // m), max(32, rh max_side // m))."""
    longer = max(rw, rh)
    return (max(32, rw * max_side // longer), max(32, rh * max_side // longer)) if longer > max_side else (rw, rh)


def select_rect(points, dilate: int = 16, feather: int = 4, pad: float = 0.5, min_side: int = 256, max_side: int = 1024) -> Rect:
    """The oriented rectangle of the scene that is edited: paste_back.select_region's rule in the line's own frame.  With
    (L, T) = the frame's length and thickness + 1 (the pixels' own extent, as a half-open bounding box counts) rounded up to whole
    pixels, each side is grown by p = max(ceil(halo(dilate, feather) k),
    ceil(pad L)) at both ends, then to min_side: rw = max(L + 2 p, min_side), rh = max(T + 2 p, min_side).  k = |cos theta| +
    |sin theta| (1 for an axis-aligned frame, where this is select_region's p): alpha's support is the mask dilated by a window that is
    square in the SCENE's axes, and along the frame's axes a square of half-width h reaches h k; with it every pixel with alpha > 0,
    and a pixel of alpha = 0 around them, lies inside the rectangle.  A rectangle whose longer
    side m exceeds max_side is edited at (max(32, rw max_side // m), max(32, rh max_side // m)).  The rectangle is never shifted or
    clipped into the image: what sticks out is filled by edge replication and is never pasted.  The centre is moved by less than
    a pixel so that the upright crop's centre pixel lies exactly on a scene pixel (matrices() maps the two onto each other)."""
    from .paste_back import halo
    cx, cy, length, thickness, theta = line_frame(points)
    L, T = int(math.ceil(length + 1 - 1e-6)), int(math.ceil(thickness + 1 - 1e-6))
    c, s = _axes(theta)
    p = max(int(math.ceil(halo(dilate, feather) * (abs(c) + abs(s)) - 1e-9)), int(math.ceil(pad * L)))
    rw, rh = max(L + 2 * p, int(min_side)), max(T + 2 * p, int(min_side))
    tw, th = edit_size(rw, rh, max_side)
    _, _, da, db = _centre_offsets(Rect(cx, cy, rw, rh, theta, tw, th))
    px, py = round(cx + da * c - db * s), round(cy + da * s + db * c)
    return Rect(px - da * c + db * s, py - da * s - db * c, rw, rh, theta, tw, th)


def rect_corners(rect: Rect) -> np.ndarray:
    """float64 [4, 2]: the scene positions of the rectangle's corners (the outer edges of its corner pixels)."""
    c, s = _axes(rect.theta)
    out = []
    for u, v in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
        out.append((rect.cx + u * rect.rw * c - v * rect.rh * s, rect.cy + u * rect.rw * s + v * rect.rh * c))
    return np.array(out, np.float64)


def bounding_window(pts: np.ndarray, size: Tuple[int, int], missed: str) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1), half-open: the bounding box of the scene positions pts [n, 2] cut at the image (size = (W, H)) -- the window
    rule of all three line paths.  ValueError(missed) when the box misses the image."""
    x0, y0 = max(int(math.floor(pts[:, 0].min())), 0), max(int(math.floor(pts[:, 1].min())), 0)
    x1, y1 = min(int(math.ceil(pts[:, 0].max())) + 1, int(size[0])), min(int(math.ceil(pts[:, 1].max())) + 1, int(size[1]))
    if x1 <= x0 or y1 <= y0:
        raise ValueError(missed)
    return x0, y0, x1, y1


def rect_window(rect: Rect, size: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1), half-open: the rectangle's bounding box cut at the image (size = (W, H)) -- the scene window a rectified line
    is pasted into.  ValueError when the rectangle misses the image."""
    return bounding_window(rect_corners(rect), size, "rect_window: the rectangle lies outside the image")


def matrices(rect: Rect, origin: Tuple[int, int] = (0, 0)) -> Tuple[np.ndarray, np.ndarray]:
    """(forward, backward), int64 [6] each, Q16, for tfx_warp_affine_u8.  forward: destination = the upright crop [rh, rw], source =
    the scene (scene -> upright).  backward: destination = the scene window whose top-left pixel is scene pixel `origin`, source = the
    upright crop (upright -> scene), at unit scale.  The rotation is round(cos 2^16), round(sin 2^16) in both; the translations are
    chosen so that the upright crop's centre pixel (rw // 2, rh // 2) and the scene pixel under it (select_rect put one there) map
    onto each other with a zero fraction in both directions."""
    q = 1 << 16
    c, s = _axes(rect.theta)
    ic, jc, da, db = _centre_offsets(rect)
    px, py = int(round(rect.cx + da * c - db * s)), int(round(rect.cy + da * s + db * c))
    C, S = int(round(c * q)), int(round(s * q))
    fwd = [C, -S, px * q - C * ic + S * jc, S, C, py * q - S * ic - C * jc]
    wx, wy = px - int(origin[0]), py - int(origin[1])
    bwd = [C, S, ic * q - C * wx - S * wy, -S, C, jc * q + S * wx - C * wy]
    return np.array(fwd, np.int64), np.array(bwd, np.int64)


def mask_points(mask_grey) -> np.ndarray:
    """[n, 2] (x, y) coordinates of the pixels >= 128 of a host uint8 [H, W] mask (what paste_back.select_region takes the box of)."""
    ys, xs = np.nonzero(np.asarray(mask_grey) >= 128)
    return np.stack([xs, ys], axis=1)


def plan(mask_grey, cfg: dict) -> Optional[Rect]:
    """The Rect a line's mask is edited through under the paste_back cfg (batch_driver._paste_back_cfg), or None when the line stays on
    the unrectified path: rectify absent, an empty mask (the region rule refuses it), or a frame outside the rule."""
    r = cfg.get("rectify")
    if not r:
        return None
    pts = mask_points(mask_grey)
    if len(pts) == 0 or not is_rectified(line_frame(pts), r["min_angle"], r["max_angle"], r["min_aspect"]):
        return None
    return select_rect(pts, cfg["dilate"], cfg["feather"], **(cfg.get("region") or {}))
