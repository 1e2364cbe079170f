"""numpy restatement of the grain match (include/textflux_hip.h: tfx_highpass_hist_u8, tfx_grain_u8; textflux_amd/paste_back.py:
noise_sigma, grain_levels, grain_gains, paste(grain=...)), written from the specification with no code shared with the package.  The
histogram and the grain are integer arithmetic and the host arithmetic is float64 on exact integers, so the device results are compared
bit for bit."""
import math

import numpy as np

from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from tests.helpers import seamless_ref as sref

BINS = 1024
SIGMA0 = math.sqrt(4 * (256 ** 2 - 1) / 12)          # of the sum of four independent uniform bytes: 147.8005
K = 1.4826 / math.sqrt(164)                          # grey levels per bin: the MAD factor over the filter's L2 norm sqrt(164) (in units of 1/16)
DEFAULTS = dict(ring=24, max_sigma=6.0, strength=1.0, min_pixels=256, seed=0)
M32 = np.uint64(0xFFFFFFFF)


def _mix(h):
    """uint32 wrap-around arithmetic, carried in uint64 and cut back after every product."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & M32
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & M32
    return h ^ (h >> np.uint64(16))


def noise_field(h: int, w: int, c: int, origin=(0, 0), seed: int = 0) -> np.ndarray:
    """int64 [h, w, c]: n in [-510, 510] of the window whose top-left pixel is scene pixel origin = (x, y)."""
    x = ((np.arange(w, dtype=np.uint64) + np.uint64(int(origin[0]) % 2 ** 32)) & M32)[None, :, None]
    y = ((np.arange(h, dtype=np.uint64) + np.uint64(int(origin[1]) % 2 ** 32)) & M32)[:, None, None]
    ch = np.arange(c, dtype=np.uint64)[None, None, :]
    k = ((x * np.uint64(0x9E3779B1)) & M32) + ((y * np.uint64(0x85EBCA77)) & M32) + ((ch * np.uint64(0xC2B2AE3D)) & M32)
    hh = _mix(_mix(k & M32) ^ np.uint64(int(seed) % 2 ** 32))
    b = lambda s: ((hh >> np.uint64(s)) & np.uint64(255)).astype(np.int64)
    return b(0) + b(8) + b(16) + b(24) - 510


def grain(img, alpha, gain, origin=None, seed: int = 0) -> np.ndarray:
    """img u8 [B, H, W, C], alpha u8 [B, H, W], gain int [B, C], origin None / (x, y) / int [B, 2] -> u8 [B, H, W, C]."""
    img, alpha, gain = np.asarray(img), np.asarray(alpha), np.asarray(gain, np.int64)
    B, H, W, C = img.shape
    org = np.zeros((B, 2), np.int64) if origin is None else np.broadcast_to(np.asarray(origin, np.int64), (B, 2))
    out = np.empty_like(img)
    for s in range(B):
        n = noise_field(H, W, C, org[s], seed)
        num = n * gain[s][None, None, :] * alpha[s].astype(np.int64)[:, :, None] + 255 * 32768
        d = num // (255 * 65536)                      # numpy's // on int64 is floor division
        out[s] = np.clip(img[s].astype(np.int64) + d, 0, 255).astype(np.uint8)
    return out


def highpass_hist(img, sel, lo: int = 255, hi: int = 255) -> np.ndarray:
    """img u8 [B, H, W, C], sel u8 [B, H, W] -> int64 [B, C, 1024]."""
    img, sel = np.asarray(img), np.asarray(sel)
    B, H, W, C = img.shape
    p = img.astype(np.int64)
    ys, xs = np.arange(H), np.arange(W)
    blur = np.zeros_like(p)
    for dy, wy in ((-1, 1), (0, 2), (1, 1)):
        rows = p[:, np.clip(ys + dy, 0, H - 1)]
        for dx, wx in ((-1, 1), (0, 2), (1, 1)):
            blur += wy * wx * rows[:, :, np.clip(xs + dx, 0, W - 1)]
    v = np.minimum(np.abs(16 * p - blur), BINS - 1)
    on = (sel >= lo) & (sel <= hi)
    out = np.zeros((B, C, BINS), np.int64)
    for s in range(B):
        for c in range(C):
            out[s, c] = np.bincount(v[s, :, :, c][on[s]], minlength=BINS)
    return out


def noise_sigma(hist) -> np.ndarray:
    """[B, C, 1024] -> float64 [B, C]: K times the lower median bin, entry by entry."""
    hist = np.asarray(hist)
    out = np.zeros(hist.shape[:2], np.float64)
    for s in range(hist.shape[0]):
        for c in range(hist.shape[1]):
            counts = [int(v) for v in hist[s, c]]
            target, run, m = (sum(counts) + 1) // 2, 0, 0
            for m, v in enumerate(counts):
                run += v
                if run >= target:
                    break
            out[s, c] = K * m
    return out


def grain_levels(hist_scene, hist_edit, cfg=None):
    """-> (sigma_scene, sigma_edit, sigma_add), float64 [B, C] each."""
    g = dict(DEFAULTS)
    g.update(cfg or {})
    hs, he = np.asarray(hist_scene), np.asarray(hist_edit)
    ss, se = noise_sigma(hs), noise_sigma(he)
    add = np.zeros_like(ss)
    for s in range(ss.shape[0]):
        for c in range(ss.shape[1]):
            if int(hs[s, c].sum()) < g["min_pixels"] or int(he[s, c].sum()) < g["min_pixels"] or ss[s, c] <= se[s, c]:
                continue
            add[s, c] = min(g["strength"] * math.sqrt(ss[s, c] ** 2 - se[s, c] ** 2), g["max_sigma"])
    return ss, se, add


def grain_gains(hist_scene, hist_edit, cfg=None) -> np.ndarray:
    add = grain_levels(hist_scene, hist_edit, cfg)[2]
    return np.array([[math.floor(v / SIGMA0 * 65536 + 0.5) for v in row] for row in add], np.int32)


def match(result, scene, alpha, ring, cfg=None, origin=None):
    """The three steps after the blend: the scene's histogram on `ring`, the result's where alpha == 255, the grain under alpha."""
    g = dict(DEFAULTS)
    g.update(cfg or {})
    gains = grain_gains(highpass_hist(scene, ring, 255, 255), highpass_hist(result, alpha, 255, 255), g)
    return grain(result, alpha, gains, origin, g["seed"]), gains


def paste(original, edited, grey, d, r, grain_cfg=None, origin=(0, 0), seamless=None, color_match=None, color_ref=None, warped=None):
    """The grain-matched paste of the specification: today's paste (plain, colour-matched and / or seamless; warped: None or (the edit
    already warped into the window, its coverage)), then match() against color_ref (None: original) on the ring cut to the coverage.
    -> (pasted, gains)."""
    g = dict(DEFAULTS)
    g.update(grain_cfg or {})
    covered = None
    if warped is not None:
        resized, covered = warped
    else:
        resized = edited if edited.shape[1:3] == original.shape[1:3] else ref.resize(edited, original.shape[1:3])
    alpha = ref.alpha_mask(grey, d, r)
    against = original if color_ref is None else color_ref
    if seamless is not None:
        result = sref.paste(original, edited, grey, d, r, seamless=seamless, color_match=color_match, color_ref=color_ref, warped=warped)
    elif color_match is not None:
        ring = plref.ring_mask(alpha, color_match["ring"])
        if covered is not None:
            ring = ring & covered
        lut = plref.fit_luts(plref.moments_np(resized, against, ring), color_match["gain"], color_match["max_shift"], color_match["min_pixels"])
        result = plref.overlay_lut(original, resized, alpha, lut)
    else:
        result = ref.overlay(original, resized, alpha)
    ring = plref.ring_mask(alpha, g["ring"])
    if covered is not None:
        ring = ring & covered
    return match(result, against, alpha, ring, g, origin)
