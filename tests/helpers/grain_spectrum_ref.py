"""numpy restatement of the grain spectrum match (include/textflux_hip.h: tfx_highpass_hist_step_u8, tfx_grain_shaped_u8;
textflux_amd/paste_back.py: grain_shape, grain_shaped_gains, paste(grain=dict(spectrum=...))), written from the specification with no
code shared with the package; it builds on grain_ref.noise_field.  The histogram and the grain are integer arithmetic and the host
arithmetic is float64 on exact integers, so the device results are compared bit for bit."""
import math

import numpy as np

from tests.helpers import grain_ref as gref
from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from tests.helpers import seamless_ref as sref

BINS = 1024
SPECTRUM = dict(max_blur=64, luma=True)
MAX_GAIN = 2 ** 18


# ---------------------------------------------------------------------------------------------- the device's arithmetic
def highpass_hist_step(img, sel, lo: int = 255, hi: int = 255, step: int = 1) -> np.ndarray:
    """img u8 [B, H, W, C], sel u8 [B, H, W] -> int64 [B, C + 1, 1024]: rows 0..C-1 of |r_c|, row C of |sum_c r_c|."""
    img, sel = np.asarray(img), np.asarray(sel)
    B, H, W, C = img.shape
    p = img.astype(np.int64)
    ys, xs = np.arange(H), np.arange(W)
    blur = np.zeros_like(p)
    for dy, wy in ((-step, 1), (0, 2), (step, 1)):
        rows = p[:, np.clip(ys + dy, 0, H - 1)]
        for dx, wx in ((-step, 1), (0, 2), (step, 1)):
            blur += wy * wx * rows[:, :, np.clip(xs + dx, 0, W - 1)]
    r = 16 * p - blur
    v = np.minimum(np.abs(np.concatenate([r, r.sum(axis=3, keepdims=True)], axis=3)), BINS - 1)
    on = (sel >= lo) & (sel <= hi)
    out = np.zeros((B, C + 1, BINS), np.int64)
    for b in range(B):
        for c in range(C + 1):
            out[b, c] = np.bincount(v[b, :, :, c][on[b]], minlength=BINS)
    return out


def noise_channels(h: int, w: int, channels, origin=(0, 0), seed: int = 0) -> np.ndarray:
    """grain_ref.noise_field for an explicit list of channel indices (noise_field(h, w, c) is channels 0..c-1; a test holds the two
    together): int64 [h, w, len(channels)]."""
    M32 = gref.M32
    x = ((np.arange(w, dtype=np.uint64) + np.uint64(int(origin[0]) % 2 ** 32)) & M32)[None, :, None]
    y = ((np.arange(h, dtype=np.uint64) + np.uint64(int(origin[1]) % 2 ** 32)) & M32)[:, None, None]
    ch = np.array(channels, dtype=np.uint64)[None, None, :]
    key = ((x * np.uint64(0x9E3779B1)) & M32) + ((y * np.uint64(0x85EBCA77)) & M32) + ((ch * np.uint64(0xC2B2AE3D)) & M32)
    hh = gref._mix(gref._mix(key & M32) ^ np.uint64(int(seed) % 2 ** 32))
    byte = lambda sh: ((hh >> np.uint64(sh)) & np.uint64(255)).astype(np.int64)
    return byte(0) + byte(8) + byte(16) + byte(24) - 510


def shaped_field(h: int, w: int, c: int, s: int, lam: int, origin=(0, 0), seed: int = 0) -> np.ndarray:
    """int64 [h, w, c]: f (Q24) of the window whose top-left pixel is scene pixel origin; the neighbours are scene pixels, window or not."""
    x, y = int(origin[0]), int(origin[1])
    n = noise_channels(h + 2, w + 2, list(range(c)) + [255], (x - 1, y - 1), seed)
    m = (256 - lam) * n[:, :, :c] + lam * n[:, :, c:]
    k = (s, 256 - 2 * s, s)
    f = np.zeros((h, w, c), np.int64)
    for dy in range(3):
        for dx in range(3):
            f += k[dy] * k[dx] * m[dy:dy + h, dx:dx + w]
    return f


def grain_shaped(img, alpha, gain, shape, origin=None, seed: int = 0) -> np.ndarray:
    """img u8 [B, H, W, C], alpha u8 [B, H, W], gain int [B, C], shape (s, lam) / int [B, 2], origin None / (x, y) / int [B, 2]."""
    img, alpha, gain = np.asarray(img), np.asarray(alpha), np.asarray(gain, np.int64)
    B, H, W, C = img.shape
    org = np.zeros((B, 2), np.int64) if origin is None else np.broadcast_to(np.asarray(origin, np.int64), (B, 2))
    shp = np.broadcast_to(np.asarray(shape, np.int64), (B, 2))
    out = np.empty_like(img)
    for b in range(B):
        f = shaped_field(H, W, C, int(shp[b, 0]), int(shp[b, 1]), org[b], seed)
        num = f * gain[b][None, None, :] * alpha[b].astype(np.int64)[:, :, None] + 255 * 2 ** 39
        out[b] = np.clip(img[b].astype(np.int64) + num // (255 * 2 ** 40), 0, 255).astype(np.uint8)      # //: floor division
    return out


# ---------------------------------------------------------------------------------------------- the host's model
def _response(s: int, m: int) -> np.ndarray:
    """The impulse response of `blur by k x k / 65536, then high-pass at distance m` on a (2 m + 3)^2 grid, float64."""
    k1 = np.array([s, 256 - 2 * s, s], np.float64) / 256.0
    n = 2 * m + 3
    resp = np.zeros((n, n))
    b = {-m: 1.0, 0: 2.0, m: 1.0}
    for dy, wy in b.items():
        for dx, wx in b.items():
            weight = (16.0 if (dy, dx) == (0, 0) else 0.0) - wy * wx
            resp[m + dy:m + dy + 3, m + dx:m + dx + 3] += weight * np.outer(k1, k1)
    return resp


def variance(s: int, m: int) -> float:
    """V_m(s): the variance of the step-m residual of unit white noise blurred by s (the sum of the squared impulse response, which is
    the specification's double sum over the autocorrelation)."""
    return float((_response(s, m) ** 2).sum())


def q_model(s: int) -> float:
    return math.sqrt(variance(s, 2) / variance(s, 1))


def levels(s: int, lam: int):
    """(w, t): the step-1 white-equivalent level and the true deviation of shaped grain driven by unit white noise."""
    mix = math.sqrt((256 - lam) ** 2 + lam ** 2) / 256.0
    return math.sqrt(variance(s, 1) / 164.0) * mix, (2 * s * s + (256 - 2 * s) ** 2) / 65536.0 * mix


def median_bin(counts) -> int:
    counts = [int(v) for v in counts]
    target, run, m = (sum(counts) + 1) // 2, 0, 0
    for m, v in enumerate(counts):
        run += v
        if run >= target:
            break
    return m


def grain_shape(h1, h2, cfg=None) -> np.ndarray:
    """int [B, C + 1, 1024] at steps 1 and 2 -> int32 [B, 2] = (s, lam)."""
    g = dict(gref.DEFAULTS)
    g.update(cfg or {})
    sp = dict(SPECTRUM)
    if isinstance(g.get("spectrum"), dict):
        sp.update(g["spectrum"])
    h1, h2 = np.asarray(h1), np.asarray(h2)
    B, C = h1.shape[0], h1.shape[1] - 1
    out = np.zeros((B, 2), np.int32)
    for b in range(B):
        p1, p2 = h1[b, :C].sum(axis=0), h2[b, :C].sum(axis=0)
        M1, M2 = median_bin(p1), median_bin(p2)
        if M1 > 0 and M2 > M1 and int(p1.sum()) >= g["min_pixels"] * C and int(p2.sum()) >= g["min_pixels"] * C:
            q, best = M2 / M1, None
            for s in range(sp["max_blur"] + 1):
                d = abs(q_model(s) - q)
                if best is None or d < best:
                    best, out[b, 0] = d, s
        if C > 1 and sp["luma"]:
            Mc = [float(median_bin(h1[b, c])) for c in range(C)]
            MS = float(median_bin(h1[b, C]))
            own = sum(v * v for v in Mc)
            den = sum(Mc) ** 2 - own
            if den > 0:
                rho, best = min(max((MS * MS - own) / den, 0.0), 1.0), None
                for lam in range(257):
                    d = abs(lam * lam / ((256 - lam) ** 2 + lam * lam) - rho)
                    if best is None or d < best:
                        best, out[b, 1] = d, lam
    return out


def grain_shaped_gains(hist_scene, hist_edit, shape, cfg=None) -> np.ndarray:
    g = dict(gref.DEFAULTS)
    g.update({k: v for k, v in (cfg or {}).items() if k != "spectrum"})
    hs, he = np.asarray(hist_scene), np.asarray(hist_edit)
    add = gref.grain_levels(hs[:, :-1], he[:, :-1], g)[2]
    out = np.zeros(add.shape, np.int32)
    for b in range(add.shape[0]):
        w, t = levels(int(shape[b][0]), int(shape[b][1]))
        for c in range(add.shape[1]):
            level = min(add[b, c] / w, g["max_sigma"] / t)
            out[b, c] = min(math.floor(level / gref.SIGMA0 * 65536 + 0.5), MAX_GAIN)
    return out


def match(result, scene, alpha, ring, cfg=None, origin=None):
    """The steps after the blend: the scene's histograms on `ring` at steps 1 and 2, the result's where alpha == 255, the shaped grain
    under alpha.  -> (out, gains, shape)"""
    g = dict(gref.DEFAULTS)
    g.update(cfg or {})
    h1, h2 = highpass_hist_step(scene, ring, 255, 255, 1), highpass_hist_step(scene, ring, 255, 255, 2)
    shape = grain_shape(h1, h2, g)
    gains = grain_shaped_gains(h1, highpass_hist_step(result, alpha, 255, 255, 1), shape, g)
    return grain_shaped(result, alpha, gains, shape, origin, g["seed"]), gains, shape


def paste(original, edited, grey, d, r, grain_cfg=None, origin=(0, 0), seamless=None, warped=None):
    """The spectrum-matched paste: the plain or seamless paste (warped: None or (the edit already warped into the window, its
    coverage)), then match() against the original on the ring cut to the coverage.  -> (pasted, gains, shape)"""
    g = dict(gref.DEFAULTS)
    g.update(grain_cfg or {})
    covered = None
    if warped is not None:
        resized, covered = warped
    else:
        resized = edited if edited.shape[1:3] == original.shape[1:3] else ref.resize(edited, original.shape[1:3])
    alpha = ref.alpha_mask(grey, d, r)
    if seamless is not None:
        result = sref.paste(original, edited, grey, d, r, seamless=seamless, color_match=None, color_ref=None, warped=warped)
    else:
        result = ref.overlay(original, resized, alpha)
    ring = plref.ring_mask(alpha, g["ring"])
    if covered is not None:
        ring = ring & covered
    return match(result, original, alpha, ring, g, origin)
