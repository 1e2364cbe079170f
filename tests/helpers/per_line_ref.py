"""numpy / Python-int restatement of the colour-matched paste (include/textflux_hip.h: tfx_masked_moments_u8, tfx_overlay_lut_u8;
textflux_amd/paste_back.py: ring_mask, fit_luts, paste(color_match=...)), written from the specification with no code shared with the
package.  The moments and the blend are integer arithmetic and the fit is float64 on exact integers, so the device results are
compared bit for bit."""
import math

import numpy as np

from tests.helpers import paste_back_ref as ref


def moments(a: np.ndarray, b: np.ndarray, weight: np.ndarray):
    """a, b [B, H, W, C] u8, weight [B, H, W] u8 -> nested list [B][C][5] of Python ints (n, sum a, sum b, sum a a, sum a b) over the
    pixels with weight != 0."""
    out = []
    for s in range(a.shape[0]):
        on = weight[s] != 0
        rows = []
        for c in range(a.shape[3]):
            x = [int(v) for v in a[s, :, :, c][on]]
            y = [int(v) for v in b[s, :, :, c][on]]
            rows.append([len(x), sum(x), sum(y), sum(v * v for v in x), sum(v * w for v, w in zip(x, y))])
        out.append(rows)
    return out


def moments_np(a: np.ndarray, b: np.ndarray, weight: np.ndarray) -> np.ndarray:
    """The same as an int64 array, summed with numpy in uint64 (for images too large to walk in Python)."""
    on = (weight != 0)[..., None]
    x, y = np.where(on, a, 0).astype(np.uint64), np.where(on, b, 0).astype(np.uint64)
    n = np.broadcast_to((weight != 0).sum(axis=(1, 2), dtype=np.uint64)[:, None], (a.shape[0], a.shape[3]))
    s = lambda v: v.sum(axis=(1, 2), dtype=np.uint64)
    return np.stack([n, s(x), s(y), s(x * x), s(x * y)], axis=2).astype(np.int64)


def fit_luts(mom, gain=(0.8, 1.25), max_shift=32, min_pixels=256) -> np.ndarray:
    """[B][C][5] -> u8 [B, C, 256], entry by entry."""
    mom = [[[int(v) for v in ch] for ch in smp] for smp in mom]
    out = np.zeros((len(mom), len(mom[0]), 256), np.uint8)
    for s, smp in enumerate(mom):
        for c, (n, sa, sb, saa, sab) in enumerate(smp):
            den = n * saa - sa * sa
            fit = n >= min_pixels and den > 0
            if fit:
                g = (n * sab - sa * sb) / den
                g = gain[0] if g < gain[0] else gain[1] if g > gain[1] else g
                o = (sb - g * sa) / n
            for v in range(256):
                t = v
                if fit:
                    t = math.floor(g * v + o + 0.5)
                    t = max(v - max_shift, min(v + max_shift, t))
                    t = max(0, min(255, t))
                out[s, c, v] = t
    return out


def overlay_lut(orig: np.ndarray, edit: np.ndarray, alpha: np.ndarray, lut: np.ndarray) -> np.ndarray:
    """orig, edit [B, H, W, C], alpha [B, H, W], lut [B, C, 256]: (orig (255 - a) + lut[b, c, edit] a + 127) // 255."""
    mapped = np.empty_like(edit)
    for s in range(edit.shape[0]):
        for c in range(edit.shape[3]):
            mapped[s, :, :, c] = lut[s, c][edit[s, :, :, c]]
    return ref.overlay(orig, mapped, alpha)


def ring_mask(alpha: np.ndarray, ring: int) -> np.ndarray:
    """255 within `ring` (square window) of alpha's support but not in it, else 0."""
    support = np.where(alpha > 0, 255, 0).astype(np.uint8)
    out = ref.dilate(support, ring)
    out[support > 0] = 0
    return out


def paste(original, edited, grey, d, r, ring=24, gain=(0.8, 1.25), max_shift=32, min_pixels=256, color_ref=None):
    """-> (pasted, lut, ring): the colour-matched paste of the specification."""
    if edited.shape[1:3] != original.shape[1:3]:
        edited = ref.resize(edited, original.shape[1:3])
    alpha = ref.alpha_mask(grey, d, r)
    rm = ring_mask(alpha, ring)
    lut = fit_luts(moments_np(edited, original if color_ref is None else color_ref, rm), gain, max_shift, min_pixels)
    return overlay_lut(original, edited, alpha, lut), lut, rm


# ---- the synthetic colour drift of the paste tests: the original's values lie in [40, 215] and edit = round(g orig + o), so that no
# value clips for any of these (g, o); 1 / g lies inside the default gain clamp and the shift inside the default max_shift
DRIFTS = ((1.0, 0.0), (1.1, -9.0), (0.9, 12.0), (1.2, -20.0), (0.85, 25.0))
DRIFT_HW, DRIFT_BOX = (96, 131), (50, 40, 90, 56)          # (x0, y0, x1, y1) of the mask


def drift_case(g: float, o: float):
    """-> (orig [1, H, W, 3] u8, edit, grey [1, H, W] u8); the same original for every drift."""
    h, w = DRIFT_HW
    orig = np.random.default_rng(17).integers(40, 216, (1, h, w, 3), dtype=np.uint8)
    edit = np.floor(g * orig.astype(np.float64) + o + 0.5).astype(np.uint8)
    grey = np.zeros((1, h, w), np.uint8)
    x0, y0, x1, y1 = DRIFT_BOX
    grey[0, y0:y1, x0:x1] = 255
    return orig, edit, grey
