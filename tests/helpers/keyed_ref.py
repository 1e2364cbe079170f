"""numpy restatement of the keyed paste (include/textflux_hip.h: tfx_change_metric_u8, tfx_hysteresis_u8; textflux_amd/paste_back.py:
keyed_sigma, keyed_levels, change_key, paste(keyed=...)), written from the specification with no code shared with the package.  The
metric and the hysteresis are integer arithmetic and the host arithmetic is float64 on exact integers, so the device results are compared
bit for bit.  The hysteresis is written twice, independently: as a repeated 3 x 3 dilation clipped to m >= lo, and as a flood fill from
the seeds over a stack."""
import math

import numpy as np

from tests.helpers import grain_ref as gref
from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from tests.helpers import seamless_ref as sref

DEFAULTS = dict(lo=10, hi=28, dilate=6, feather=2, noise=3.0, ring=24, min_pixels=256)
STENCIL = ((1, 2, 1), (2, 4, 2), (1, 2, 1))


def change_metric(a, b) -> np.ndarray:
    """a, b u8 [B, H, W, C] -> u8 [B, H, W]: max over c of (|sum w (a - b)| + 8) >> 4, the neighbour indices clamped to the image."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    _, H, W, _ = d.shape
    ys, xs = np.arange(H), np.arange(W)
    s = np.zeros_like(d)
    for dy in (-1, 0, 1):
        rows = d[:, np.clip(ys + dy, 0, H - 1)]
        for dx in (-1, 0, 1):
            s += STENCIL[dy + 1][dx + 1] * rows[:, :, np.clip(xs + dx, 0, W - 1)]
    return ((np.abs(s) + 8) >> 4).max(axis=3).astype(np.uint8)


def hysteresis_dilation(m, lo: int, hi: int) -> np.ndarray:
    """m u8 [B, H, W] -> u8 [B, H, W] in {0, 255}: the seeds m >= hi, grown by one pixel in the eight directions and cut to m >= lo, until
    nothing is added."""
    m = np.asarray(m).astype(np.int64)
    weak, on = m >= lo, m >= hi
    while True:
        p = np.pad(on, ((0, 0), (1, 1), (1, 1)))
        grown = np.zeros_like(on)
        H, W = on.shape[1:]
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                grown |= p[:, dy:dy + H, dx:dx + W]
        grown &= weak
        if np.array_equal(grown, on):
            return np.where(on, 255, 0).astype(np.uint8)
        on = grown


def hysteresis_flood(m, lo: int, hi: int) -> np.ndarray:
    """The same set by a flood fill: every seed goes on a stack; a popped pixel marks and pushes its unmarked neighbours with m >= lo."""
    m = np.asarray(m)
    B, H, W = m.shape
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        field = m[b].astype(int).tolist()
        mark = [[False] * W for _ in range(H)]
        stack = []
        for y in range(H):
            for x in range(W):
                if field[y][x] >= hi:
                    mark[y][x] = True
                    stack.append((y, x))
        while stack:
            y, x = stack.pop()
            for ny in range(max(y - 1, 0), min(y + 2, H)):
                for nx in range(max(x - 1, 0), min(x + 2, W)):
                    if not mark[ny][nx] and field[ny][nx] >= lo:
                        mark[ny][nx] = True
                        stack.append((ny, nx))
        out[b] = np.where(np.array(mark, bool).reshape(H, W), 255, 0)
    return out


def levels(cfg=None, sigma: float = 0.0):
    """(lo_eff, hi_eff): lo_eff = max(lo, ceil(noise sigma)), hi_eff = hi + (lo_eff - lo), both at most 256."""
    k = dict(DEFAULTS)
    k.update(cfg or {})
    lo_eff = min(max(k["lo"], math.ceil(k["noise"] * sigma)), 256)
    return lo_eff, min(k["hi"] + lo_eff - k["lo"], 256)


def scene_sigma(scene, ring, cfg=None) -> np.ndarray:
    """float64 [B]: the largest per-channel noise level of the scene on the ring; 0 with fewer than min_pixels ring pixels or noise = 0."""
    k = dict(DEFAULTS)
    k.update(cfg or {})
    B = np.asarray(scene).shape[0]
    if k["noise"] == 0:
        return np.zeros(B)
    hist = gref.highpass_hist(scene, ring, 255, 255)
    sig = gref.noise_sigma(hist)
    return np.array([sig[b].max() if int((np.asarray(ring)[b] == 255).sum()) >= k["min_pixels"] else 0.0 for b in range(B)])


def change_key(original, result, cfg=None, sigma=None, hysteresis=hysteresis_dilation) -> np.ndarray:
    """u8 [B, H, W]: feather(dilate(hysteresis(metric(result, original), levels of the sample))), sample by sample."""
    k = dict(DEFAULTS)
    k.update(cfg or {})
    m = change_metric(result, original)
    B = m.shape[0]
    sg = np.zeros(B) if sigma is None else np.broadcast_to(np.asarray(sigma, np.float64), (B,))
    marked = np.concatenate([hysteresis(m[b:b + 1], *levels(k, float(sg[b]))) for b in range(B)])
    return ref.feather(ref.dilate(marked, k["dilate"]), k["feather"])


def blend(original, edited, grey, d, r, color_match=None, seamless=None, color_ref=None):
    """Today's paste without the key and without grain -> (result, alpha): plain, colour-matched and / or seamless."""
    resized = edited if edited.shape[1:3] == original.shape[1:3] else ref.resize(edited, original.shape[1:3])
    alpha = ref.alpha_mask(grey, d, r)
    against = original if color_ref is None else color_ref
    if seamless is not None:
        return sref.paste(original, edited, grey, d, r, seamless=seamless, color_match=color_match, color_ref=color_ref), alpha
    if color_match is not None:
        ring = plref.ring_mask(alpha, color_match["ring"])
        lut = plref.fit_luts(plref.moments_np(resized, against, ring), color_match["gain"], color_match["max_shift"], color_match["min_pixels"])
        return plref.overlay_lut(original, resized, alpha, lut), alpha
    return ref.overlay(original, resized, alpha), alpha


def paste(original, edited, grey, d, r, keyed=None, color_match=None, seamless=None, grain=None, color_ref=None, origin=(0, 0)):
    """The keyed paste of the specification -> (final, key, result): the blend as before; the scene's noise level on the ring just
    outside it; the key; the result over the original under the key; then, with grain, the grain match on that under min(alpha, key)
    where it took alpha (the ring stays alpha's).  color_match, seamless and grain: complete dicts (the package's *_cfg)."""
    k = dict(DEFAULTS)
    k.update(keyed or {})
    result, alpha = blend(original, edited, grey, d, r, color_match, seamless, color_ref)
    against = original if color_ref is None else color_ref
    sigma = scene_sigma(against, plref.ring_mask(alpha, k["ring"]), k)
    key = change_key(original, result, k, sigma)
    final = ref.overlay(original, result, key)
    if grain is not None:
        final = gref.match(final, against, np.minimum(alpha, key), plref.ring_mask(alpha, grain["ring"]), grain, origin)[0]
    return final, key, result
