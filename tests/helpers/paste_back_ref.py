"""numpy restatement of the paste-back arithmetic (include/textflux_hip.h: tfx_mask_dilate_u8, tfx_mask_feather_u8, tfx_overlay_u8;
textflux_amd/paste_back.py: alpha_mask, select_region, paste), written from the specification, loop for loop, with no code shared
with the package.  Everything is integer arithmetic, so the device results are compared bit for bit.  PIL's Image.resize serves the
resample (the device resampler is pinned to it bit for bit in tests/test_imageops_gpu.py)."""
import math

import numpy as np
from PIL import Image


def dilate(m: np.ndarray, r: int) -> np.ndarray:
    """[..., H, W] u8: max over the (2r+1)^2 window clipped at the border -- x pass, then y pass."""
    def axis_pass(v, axis):
        L = v.shape[axis]
        out = np.zeros_like(v)
        for i in range(L):
            lo, hi = max(i - r, 0), min(i + r, L - 1)
            sl = [slice(None)] * v.ndim
            sl[axis] = slice(lo, hi + 1)
            dst = [slice(None)] * v.ndim
            dst[axis] = i
            out[tuple(dst)] = v[tuple(sl)].max(axis=axis)
        return out
    return axis_pass(axis_pass(np.asarray(m, np.uint8), -1), -2)


def box_pass(v: np.ndarray, r: int, axis: int) -> np.ndarray:
    """One box pass: s = sum_{k=-r..r} v[clamp(i+k, 0, L-1)], out = (2 s + n) // (2 n), n = 2r+1."""
    L, n = v.shape[axis], 2 * r + 1
    s = np.zeros(v.shape, np.int64)
    idx = np.arange(L)
    for k in range(-r, r + 1):
        s += np.take(v, np.clip(idx + k, 0, L - 1), axis=axis).astype(np.int64)
    return ((2 * s + n) // (2 * n)).astype(np.uint8)


def feather(m: np.ndarray, r: int) -> np.ndarray:
    v = np.asarray(m, np.uint8)
    for axis in (-1, -1, -1, -2, -2, -2):
        v = box_pass(v, r, axis)
    return v


def overlay(orig: np.ndarray, edit: np.ndarray, alpha: np.ndarray) -> np.ndarray:
    """orig, edit [..., C], alpha [...]: (orig (255 - a) + edit a + 127) // 255."""
    a = np.asarray(alpha, np.int64)[..., None]
    return ((np.asarray(orig, np.int64) * (255 - a) + np.asarray(edit, np.int64) * a + 127) // 255).astype(np.uint8)


def alpha_mask(grey: np.ndarray, d: int, r: int) -> np.ndarray:
    return feather(dilate(np.where(np.asarray(grey) >= 128, 255, 0).astype(np.uint8), d), r)


def resize(img: np.ndarray, hw) -> np.ndarray:
    """[B, h, w, 3] u8 -> [B, H, W, 3] with PIL's default (bicubic) resize."""
    return np.stack([np.array(Image.fromarray(a).resize((hw[1], hw[0]))) for a in img])


def paste(original: np.ndarray, edited: np.ndarray, grey: np.ndarray, d: int, r: int) -> np.ndarray:
    if edited.shape[1:3] != original.shape[1:3]:
        edited = resize(edited, original.shape[1:3])
    return overlay(original, edited, alpha_mask(grey, d, r))


def select_region(grey: np.ndarray, d: int, r: int, pad=0.5, min_side=256, max_side=1024):
    """-> (x0, y0, x1, y1, tw, th), the seven steps of the specification in order."""
    H, W = grey.shape
    ys, xs = np.nonzero(grey >= 128)
    if ys.size == 0:
        raise ValueError("empty mask")
    x0, x1, y0, y1 = xs.min(), xs.max() + 1, ys.min(), ys.max() + 1                 # 1. half-open bounding box
    h_ = d + 3 * r + 1                                                             # 2. halo
    p = max(h_, math.ceil(pad * max(x1 - x0, y1 - y0)))                            # 3.
    x0, x1, y0, y1 = x0 - p, x1 + p, y0 - p, y1 + p                                # 4.

    def axis(lo, hi, size):
        if hi - lo < min_side:                                                     # 5. symmetric growth, floor on the low side
            lo = lo - (min_side - (hi - lo)) // 2
            hi = lo + min_side
        if hi - lo >= size:                                                        # 6. shift, do not shrink
            return 0, size
        if lo < 0:
            hi, lo = hi - lo, 0
        if hi > size:
            lo, hi = lo - (hi - size), size
        return lo, hi
    x0, x1 = axis(x0, x1, W)
    y0, y1 = axis(y0, y1, H)
    w, h = x1 - x0, y1 - y0
    m = max(w, h)
    tw, th = (max(32, w * max_side // m), max(32, h * max_side // m)) if m > max_side else (w, h)   # 7.
    return tuple(int(v) for v in (x0, y0, x1, y1, tw, th))


def bbox_grown(grey: np.ndarray, by: int):
    """Half-open bounding box of the pixels >= 128 grown by `by`, cut at the image border."""
    H, W = grey.shape
    ys, xs = np.nonzero(grey >= 128)
    return max(int(xs.min()) - by, 0), max(int(ys.min()) - by, 0), min(int(xs.max()) + 1 + by, W), min(int(ys.max()) + 1 + by, H)
