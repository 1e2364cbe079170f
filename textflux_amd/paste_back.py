"""Paste-back and region editing (DESIGN.md section 4 "Paste-back"): the pipeline's result goes back into the ORIGINAL image, at
its original size, under a dilated and feathered mask, so that every pixel outside the edit keeps its bytes; and a large photo is
edited through a region cut around the mask instead of being resized whole.

No reference counterpart: FluxFillPipeline never calls its image processor's crop / overlay helpers (the idea is in
diffusers/src/diffusers/image_processor.py: get_crop_region :293, blur :276, apply_overlay :773) and the reference's callers
return the VAE round trip of the whole canvas.  The arithmetic here is this project's own, exact in integers:

    alpha = feather(dilate(mask >= 128 ? 255 : 0, d), r)          ops.mask_dilate / ops.mask_feather
    out   = (orig (255 - alpha) + edit alpha + 127) // 255        ops.overlay

The feather's support grows by at most 3 r per axis, so alpha is 0 outside the mask dilated by d + 3 r; with d >= 3 r every
original mask pixel has alpha = 255 (the seam lies outside the edited text).  The defaults satisfy that; they are a starting
point, not a tuned value.

Colour matching (opt-in, paste(color_match=...); DESIGN.md section 4 "Per-line edits"): before the blend the edit goes through a per-channel
look-up table, the least-squares line from the edit's colours to the original's on a ring just outside alpha's support:

    moments = (n, sum a, sum b, sum a a, sum a b) over ring_mask(alpha)    ops.masked_moments (exact 64-bit integer sums)
    lut     = fit_luts(moments)                                            host, Python integers up to the division
    out     = (orig (255 - alpha) + lut[edit] alpha + 127) // 255          ops.overlay_lut

Seamless paste (opt-in, paste(seamless=...); DESIGN.md section 4 "Seamless paste"): the final blend becomes ops.seamless_overlay, which
first adds a membrane to the (table-mapped) edit: the difference to the scene, known just outside the blend, interpolated across alpha's
support by a pull-push pyramid, so that the edit meets the scene at the seam and keeps its own gradients inside.

Grain match (opt-in, paste(grain=...); DESIGN.md section 4 "Grain match"): after the final blend the pasted pixels get the scene's noise level:

    hist  = histogram of |16 p - [1 2 1] x [1 2 1] p|                      ops.highpass_hist (exact integer counts)
    sigma = 1.4826 / sqrt(164) * lower median of hist                      host: on the ring for the scene, where alpha == 255 for the edit
    gain  = min(strength sqrt(sigma_scene^2 - sigma_edit^2), max_sigma)    host, in Q16 of the hash's own standard deviation
    out   = clamp(result + grain(scene position, channel, seed) gain alpha)  ops.grain

Grain spectrum (opt-in, grain=dict(spectrum=...); DESIGN.md section 4 "Grain spectrum"): the grain also gets the SHAPE of the scene's noise:

    h1, h2 = the histogram with its neighbours at distance 1 and 2, and of the channel sum     ops.highpass_hist_step
    s      = the [s, 256 - 2 s, s] blur whose model ratio is nearest to median(h2) / median(h1)   host: grain_shape
    lam    = the share of one field common to the channels, from the channel sum's median      host: grain_shape
    gain   = sigma_add / w(s, lam), its true deviation held below max_sigma                    host: grain_shaped_gains
    out    = clamp(result + blurred, channel-mixed grain gain alpha)                           ops.grain_shaped

Keyed paste (opt-in, paste(keyed=...); DESIGN.md section 4 "Keyed paste"): behind the blend and in front of the grain, a pixel inside the
blend keeps the scene's byte unless the blend really differs there:

    m     = max over the channels of (|[1 2 1] x [1 2 1] (result - orig)| + 8) >> 4            ops.change_metric
    key   = feather(dilate(hysteresis(m, lo_eff, hi_eff), dilate), feather)                    ops.hysteresis, ops.mask_dilate / mask_feather
    final = (orig (255 - key) + result key + 127) // 255                                       ops.overlay
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops

DILATE, FEATHER = 16, 4
PAD, MIN_SIDE, MAX_SIDE = 0.5, 256, 1024


class Region(NamedTuple):
    x0: int
    y0: int
    x1: int                          # half-open: columns [x0, x1), rows [y0, y1) of the original image
    y1: int
    tw: int                          # the size the crop is edited at (the crop's own size unless it exceeds max_side)
    th: int


def halo(dilate: int, feather: int) -> int:
    """Pixels around the mask's bounding box that a region must keep: alpha's support (dilate + 3 feather) and one pixel of
    alpha = 0, so that the region's border is untouched and the paste leaves no seam there."""
    return int(dilate) + 3 * int(feather) + 1


def _fit(lo: int, hi: int, size: int, min_side: int) -> Tuple[int, int]:
    """One axis: grown symmetrically (floor on the low side) to min_side, then shifted -- not shrunk -- into [0, size)."""
    if hi - lo < min_side:
        lo -= (min_side - (hi - lo)) // 2
        hi = lo + min_side
    if hi - lo >= size:
        return 0, size
    if lo < 0:
        lo, hi = 0, hi - lo
    if hi > size:
        lo, hi = lo - (hi - size), size
    return lo, hi


def select_region(mask_grey, dilate: int = DILATE, feather: int = FEATHER, pad: float = PAD, min_side: int = MIN_SIDE,
                  max_side: int = MAX_SIDE, size: Optional[Tuple[int, int]] = None) -> Region:
    """The rectangle of the original image that is edited.  mask_grey: host uint8 [H, W]; None with size = (W, H) is the whole image
    at its own size, (0, 0, W, H, W, H).
    Bounding box of the pixels >= 128 (none: ValueError), grown on every side by p = max(halo, ceil(pad * max(bw, bh))), each axis
    then grown to min_side and shifted into the image (an axis longer than the image is the whole axis).  A region whose longer
    side m exceeds max_side is edited at (max(32, w max_side // m), max(32, h max_side // m))."""
    if mask_grey is None:
        if size is None:
            raise ValueError("select_region: the whole-image region needs size=(width, height)")
        return Region(0, 0, int(size[0]), int(size[1]), int(size[0]), int(size[1]))
    m = np.asarray(mask_grey)
    if m.ndim != 2:
        raise ValueError(f"select_region: the mask must be [H, W], got {m.shape}")
    H, W = m.shape
    on = m >= 128
    rows, cols = np.flatnonzero(on.any(axis=1)), np.flatnonzero(on.any(axis=0))
    if rows.size == 0:
        raise ValueError("select_region: the mask is empty (no pixel >= 128)")
    x0, x1, y0, y1 = int(cols[0]), int(cols[-1]) + 1, int(rows[0]), int(rows[-1]) + 1
    p = max(halo(dilate, feather), int(math.ceil(pad * max(x1 - x0, y1 - y0))))
    x0, x1 = _fit(x0 - p, x1 + p, W, min_side)
    y0, y1 = _fit(y0 - p, y1 + p, H, min_side)
    w, h = x1 - x0, y1 - y0
    longer = max(w, h)
    if longer > max_side:
        return Region(x0, y0, x1, y1, max(32, w * max_side // longer), max(32, h * max_side // longer))
    return Region(x0, y0, x1, y1, w, h)


def alpha_mask(mask_grey: torch.Tensor, dilate: int = DILATE, feather: int = FEATHER) -> torch.Tensor:
    """uint8 [B, H, W] grey mask on the device -> the blend weight: binarised at >= 128 (VaeImageProcessor.binarize of grey / 255 at
    0.5), dilated, feathered."""
    if mask_grey.dtype != torch.uint8 or mask_grey.dim() != 3:
        raise ValueError(f"alpha_mask: the mask must be uint8 [B, H, W], got {mask_grey.dtype} {tuple(mask_grey.shape)}")
    binary = (mask_grey >= 128).to(torch.uint8).mul_(255).contiguous()
    return ops.mask_feather(ops.mask_dilate(binary, dilate), feather)


# Colour matching (DESIGN.md section 4 "Per-line edits"): the ring's width, the clamps of the fitted gain and of a table entry's shift,
# and the fewest ring pixels a fit is trusted with.  A starting point, not a tuned value and no quality claim.
RING, GAIN, MAX_SHIFT, MIN_PIXELS = 24, (0.8, 1.25), 32, 256


def color_match_cfg(color_match) -> dict:
    """paste's color_match argument (True or a dict of ring, gain, max_shift, min_pixels) with its defaults filled in and checked."""
    cm = {} if color_match is True else dict(color_match)
    unknown = set(cm) - {"ring", "gain", "max_shift", "min_pixels"}
    if unknown:
        raise ValueError(f"color_match: unknown keys {sorted(unknown)}")
    ring = RING if cm.get("ring") is None else int(cm["ring"])
    gain = GAIN if cm.get("gain") is None else (float(cm["gain"][0]), float(cm["gain"][1]))
    max_shift = MAX_SHIFT if cm.get("max_shift") is None else int(cm["max_shift"])
    min_pixels = MIN_PIXELS if cm.get("min_pixels") is None else int(cm["min_pixels"])
    if not 1 <= ring <= 255:
        raise ValueError("color_match: ring must be in [1, 255]")
    if not 0 < gain[0] <= gain[1]:
        raise ValueError("color_match: gain must be (lo, hi) with 0 < lo <= hi")
    if not 0 <= max_shift <= 255 or min_pixels < 1:
        raise ValueError("color_match: max_shift must be in [0, 255] and min_pixels at least 1")
    return dict(ring=ring, gain=gain, max_shift=max_shift, min_pixels=min_pixels)


# Seamless paste (DESIGN.md section 4 "Seamless paste"): the Jacobi sweeps after the push and the clamp of the correction in grey levels.
# A starting point, not a tuned value and no quality claim.
SEAMLESS_SMOOTH, SEAMLESS_MAX_SHIFT = 8, 32


def seamless_cfg(seamless) -> dict:
    """paste's seamless argument (True or a dict of smooth, max_shift) with its defaults filled in and checked."""
    if seamless is not True and not isinstance(seamless, dict):
        raise ValueError("seamless: must be True or a dict")
    sm = {} if seamless is True else dict(seamless)
    unknown = set(sm) - {"smooth", "max_shift"}
    if unknown:
        raise ValueError(f"seamless: unknown keys {sorted(unknown)}")
    smooth = SEAMLESS_SMOOTH if sm.get("smooth") is None else int(sm["smooth"])
    max_shift = SEAMLESS_MAX_SHIFT if sm.get("max_shift") is None else int(sm["max_shift"])
    if not 0 <= smooth <= 255 or not 0 <= max_shift <= 255:
        raise ValueError("seamless: smooth and max_shift must be in [0, 255]")
    return dict(smooth=smooth, max_shift=max_shift)


# Grain match (DESIGN.md section 4 "Grain match"): the largest standard deviation that is ever added, in grey levels, and the share of the
# missing noise that is.  The ring and the fewest pixels an estimate is trusted with are colour matching's.  A starting point, not a tuned
# value and no quality claim.
GRAIN_MAX_SIGMA, GRAIN_STRENGTH = 6.0, 1.0
# Grey levels of noise per histogram bin: a Gaussian's sigma is 1.4826 times the median of its absolute value (the MAD estimate), and the
# filter 16 delta - [1 2 1] x [1 2 1] turns white noise of sigma s into noise of sigma s sqrt(164) (its L2 norm: 12^2 + 4 2^2 + 4 1^2 = 164).
GRAIN_K = 1.4826 / math.sqrt(164.0)


def grain_cfg(grain) -> dict:
    """paste's grain argument (True or a dict of ring, max_sigma, strength, min_pixels, seed, spectrum) with its defaults filled in and
    checked.  spectrum (DESIGN.md section 4 "Grain spectrum"): True or a dict of max_blur (0..64, default 64) and luma (a bool, default
    True); the result carries the key only when the caller gave it."""
    if grain is not True and not isinstance(grain, dict):
        raise ValueError("grain: must be True or a dict")
    gr = {} if grain is True else dict(grain)
    unknown = set(gr) - {"ring", "max_sigma", "strength", "min_pixels", "seed", "spectrum"}
    if unknown:
        raise ValueError(f"grain: unknown keys {sorted(unknown)}")
    spectrum = gr.pop("spectrum", None)
    if spectrum is not None and spectrum is not False:
        if spectrum is not True and not isinstance(spectrum, dict):
            raise ValueError("grain: spectrum must be True or a dict")
        sp = {} if spectrum is True else dict(spectrum)
        if set(sp) - {"max_blur", "luma"}:
            raise ValueError(f"grain: unknown spectrum keys {sorted(set(sp) - {'max_blur', 'luma'})}")
        max_blur = ops.GRAIN_MAX_BLUR if sp.get("max_blur") is None else sp["max_blur"]
        luma = True if sp.get("luma") is None else sp["luma"]
        if isinstance(max_blur, bool) or not isinstance(max_blur, (int, np.integer)) or not 0 <= max_blur <= ops.GRAIN_MAX_BLUR:
            raise ValueError(f"grain: spectrum max_blur must be an integer in [0, {ops.GRAIN_MAX_BLUR}]")
        if not isinstance(luma, (bool, np.bool_)):
            raise ValueError("grain: spectrum luma must be a bool")
        return dict(grain_cfg(gr or True), spectrum=dict(max_blur=int(max_blur), luma=bool(luma)))
    ring = RING if gr.get("ring") is None else int(gr["ring"])
    max_sigma = GRAIN_MAX_SIGMA if gr.get("max_sigma") is None else float(gr["max_sigma"])
    strength = GRAIN_STRENGTH if gr.get("strength") is None else float(gr["strength"])
    min_pixels = MIN_PIXELS if gr.get("min_pixels") is None else int(gr["min_pixels"])
    seed = 0 if gr.get("seed") is None else int(gr["seed"])
    if not 1 <= ring <= 255:
        raise ValueError("grain: ring must be in [1, 255]")
    if not 0.0 <= max_sigma <= 64.0:                 # also refuses NaN
        raise ValueError("grain: max_sigma must be in [0, 64]")
    if not 0.0 <= strength <= 4.0:
        raise ValueError("grain: strength must be in [0, 4]")
    if min_pixels < 1 or not 0 <= seed < 2 ** 32:
        raise ValueError("grain: min_pixels must be at least 1 and seed in [0, 2^32)")
    return dict(ring=ring, max_sigma=max_sigma, strength=strength, min_pixels=min_pixels, seed=seed)


# Keyed paste (DESIGN.md section 4 "Keyed paste"): the two thresholds of the change metric in grey levels, how far the key is grown and
# feathered, and how many standard deviations of the scene's noise the lower threshold is kept above.  The ring and the fewest pixels a
# noise estimate is trusted with are colour matching's.  A starting point, not a tuned value and no quality claim.
KEYED_LO, KEYED_HI, KEYED_DILATE, KEYED_FEATHER, KEYED_NOISE = 10, 28, 6, 2, 3.0


def keyed_cfg(keyed) -> dict:
    """paste's keyed argument (True or a dict of lo, hi, dilate, feather, noise, ring, min_pixels) with its defaults filled in and
    checked: 0 <= lo <= hi <= 256, dilate >= 3 feather (every pixel the hysteresis marks then has key = 255), 0 <= noise <= 64."""
    if keyed is not True and not isinstance(keyed, dict):
        raise ValueError("keyed: must be True or a dict")
    kd = {} if keyed is True else dict(keyed)
    unknown = set(kd) - {"lo", "hi", "dilate", "feather", "noise", "ring", "min_pixels"}
    if unknown:
        raise ValueError(f"keyed: unknown keys {sorted(unknown)}")
    for k in ("lo", "hi", "dilate", "feather", "ring", "min_pixels"):
        if kd.get(k) is not None and (isinstance(kd[k], bool) or not isinstance(kd[k], (int, np.integer))):
            raise ValueError(f"keyed: {k} must be an integer")
    lo = KEYED_LO if kd.get("lo") is None else int(kd["lo"])
    hi = KEYED_HI if kd.get("hi") is None else int(kd["hi"])
    dilate = KEYED_DILATE if kd.get("dilate") is None else int(kd["dilate"])
    feather = KEYED_FEATHER if kd.get("feather") is None else int(kd["feather"])
    noise = KEYED_NOISE if kd.get("noise") is None else float(kd["noise"])
    ring = RING if kd.get("ring") is None else int(kd["ring"])
    min_pixels = MIN_PIXELS if kd.get("min_pixels") is None else int(kd["min_pixels"])
    if not 0 <= lo <= hi <= 256:
        raise ValueError("keyed: lo and hi must satisfy 0 <= lo <= hi <= 256")
    if not (0 <= feather and 3 * feather <= dilate <= 255):
        raise ValueError("keyed: dilate and feather must satisfy 0 <= 3 feather <= dilate <= 255")
    if not 0.0 <= noise <= 64.0:                     # also refuses NaN
        raise ValueError("keyed: noise must be in [0, 64]")
    if not 1 <= ring <= 255 or min_pixels < 1:
        raise ValueError("keyed: ring must be in [1, 255] and min_pixels at least 1")
    return dict(lo=lo, hi=hi, dilate=dilate, feather=feather, noise=noise, ring=ring, min_pixels=min_pixels)


def keyed_sigma(hist, cfg=True) -> np.ndarray:
    """hist int [B, C, 1024] (ops.highpass_hist of the scene on the ring) -> float64 [B]: the largest per-channel noise_sigma of every
    sample under keyed_cfg(cfg); 0 where the histogram counts fewer than min_pixels pixels."""
    cfg = keyed_cfg(cfg)
    h = _hist(hist)
    return np.where(h.sum(axis=2).min(axis=1) >= cfg["min_pixels"], noise_sigma(h).max(axis=1), 0.0)


def keyed_levels(cfg=True, sigma: float = 0.0) -> Tuple[int, int]:
    """(lo_eff, hi_eff), the hysteresis thresholds of one sample whose scene has the noise level sigma, under keyed_cfg(cfg):
    lo_eff = max(lo, ceil(noise sigma)) and hi_eff = hi + (lo_eff - lo), both at most 256.  The difference between a clean edit and a
    noisy scene has the scene's noise level; that noise is not keyed as change."""
    cfg = keyed_cfg(cfg)
    lo_eff = min(max(cfg["lo"], int(math.ceil(cfg["noise"] * float(sigma)))), 256)
    return lo_eff, min(cfg["hi"] + (lo_eff - cfg["lo"]), 256)


def change_key(original: torch.Tensor, result: torch.Tensor, cfg=True, sigma=None) -> torch.Tensor:
    """uint8 [B, H, W], the key of the keyed paste: ops.change_metric(result, original), thresholded by ops.hysteresis at
    keyed_levels(cfg, sigma[b]) per sample, grown by cfg's dilate (ops.mask_dilate) and feathered by its feather (ops.mask_feather).
    original, result: uint8 [B, H, W, C] on the device; sigma: None (0), a number or one per sample.  Every pixel whose metric reaches
    hi_eff has key = 255; a pixel farther than dilate + 3 feather (per axis) from every marked pixel has key = 0."""
    cfg = keyed_cfg(cfg)
    B = original.shape[0]
    sg = np.broadcast_to(np.zeros(1) if sigma is None else np.asarray(sigma, np.float64), (B,))
    levels = [keyed_levels(cfg, s) for s in sg]
    m = ops.change_metric(result, original)
    if len(set(levels)) == 1:
        marked = ops.hysteresis(m, *levels[0])
    else:                                            # the thresholds are the call's, not the sample's: one call per sample
        marked = torch.cat([ops.hysteresis(m[b:b + 1], *levels[b]) for b in range(B)])
    return ops.mask_feather(ops.mask_dilate(marked, cfg["dilate"]), cfg["feather"])


def _hist(hist) -> np.ndarray:
    h = hist.cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
    if h.ndim != 3 or h.shape[2] != ops.HIGHPASS_BINS:
        raise ValueError(f"noise_sigma: the histogram must be [B, C, {ops.HIGHPASS_BINS}], got {h.shape}")
    return h.astype(np.int64)


def noise_sigma(hist) -> np.ndarray:
    """hist int [B, C, 1024] (ops.highpass_hist) -> float64 [B, C], the noise level in grey levels: GRAIN_K m with m the lower median of the
    residual's magnitude, the smallest bin whose cumulative count reaches (n + 1) // 2 (0 for an empty histogram).  Edges and glyph
    strokes are outliers of the magnitude; the median ignores them while they cover less than half of the counted pixels."""
    h = _hist(hist)
    cum = np.cumsum(h, axis=2)
    target = (cum[:, :, -1] + 1) // 2
    return GRAIN_K * (cum < target[:, :, None]).sum(axis=2).astype(np.float64)


def grain_levels(hist_scene, hist_edit, cfg=True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(sigma_scene, sigma_edit, sigma_add), float64 [B, C] each, of the two histograms under grain_cfg(cfg): noise_sigma of both and the
    standard deviation of the grain that is added, min(strength sqrt(sigma_scene^2 - sigma_edit^2), max_sigma); 0 where either histogram
    counts fewer than min_pixels pixels or the edit is already at least as noisy as the scene (nothing is denoised)."""
    cfg = grain_cfg(cfg)
    hs, he = _hist(hist_scene), _hist(hist_edit)
    if hs.shape != he.shape:
        raise ValueError(f"grain_levels: the histograms must agree, got {hs.shape} and {he.shape}")
    ss, se = noise_sigma(hs), noise_sigma(he)
    add = np.minimum(cfg["strength"] * np.sqrt(np.maximum(ss * ss - se * se, 0.0)), cfg["max_sigma"])
    trusted = (hs.sum(axis=2) >= cfg["min_pixels"]) & (he.sum(axis=2) >= cfg["min_pixels"]) & (ss > se)
    return ss, se, np.where(trusted, add, 0.0)


def grain_gains(hist_scene, hist_edit, cfg=True) -> np.ndarray:
    """int32 [B, C]: ops.grain's gain for grain_levels' sigma_add, floor(sigma_add / ops.GRAIN_SIGMA0 * 65536 + 0.5) in float64."""
    add = grain_levels(hist_scene, hist_edit, cfg)[2]
    return np.floor(add / ops.GRAIN_SIGMA0 * 65536.0 + 0.5).astype(np.int32)


# Grain spectrum (DESIGN.md section 4 "Grain spectrum").  ops.grain_shaped blurs unit white noise by K = k x k / 65536, k = [s, 256 - 2 s, s],
# whose autocorrelation is A_s(du, dv) = a(du) a(dv) with a(d) = sum_i k[i] k[i + d] / 65536.  The high-pass 16 delta - [1 2 1] x [1 2 1]
# with its neighbours at distance m, h_m, then sees the variance V_m(s) = sum over u, v of h_m[u] h_m[v] A_s(u - v); V_1(0) = 164.
@functools.lru_cache(maxsize=None)                   # 65 x 2 values, asked for on every paste: the device waits for the host meanwhile
def _highpass_variance(s: int, m: int) -> float:
    k = (s, 256 - 2 * s, s)
    a = {d: sum(k[i] * k[i + d] for i in range(3) if 0 <= i + d < 3) / 65536.0 for d in range(-2, 3)}
    h = {(m * dx, m * dy): -float((2 - abs(dx)) * (2 - abs(dy))) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    h[(0, 0)] += 16.0
    return sum(hu * hv * a.get(ux - vx, 0.0) * a.get(uy - vy, 0.0) for (ux, uy), hu in h.items() for (vx, vy), hv in h.items())


def grain_q_model(s: int) -> float:
    """sqrt(V_2(s) / V_1(s)): how much larger the step-2 residual of grain blurred by s is than its step-1 residual.  1 for white noise
    (s = 0), rising with s to 1.926 at 64."""
    return math.sqrt(_highpass_variance(s, 2) / _highpass_variance(s, 1))


def grain_shape_levels(s: int, lam: int) -> Tuple[float, float]:
    """(w, t) of ops.grain_shaped driven by unit white noise: w the level the step-1 estimator (noise_sigma) reads, its white
    equivalent, and t the true standard deviation.  (1, 1) at (0, 0)."""
    mix = math.sqrt((256 - lam) ** 2 + lam ** 2) / 256.0
    return math.sqrt(_highpass_variance(s, 1) / 164.0) * mix, (s * s + (256 - 2 * s) ** 2 + s * s) / 65536.0 * mix


@functools.lru_cache(maxsize=None)
def _shape_models(max_blur: int) -> Tuple[np.ndarray, np.ndarray]:
    """(grain_q_model of s = 0..max_blur, the channels' correlation lam^2 / ((256 - lam)^2 + lam^2) of lam = 0..256), float64."""
    lams = np.arange(257, dtype=np.float64)
    return np.array([grain_q_model(s) for s in range(max_blur + 1)]), lams ** 2 / ((256.0 - lams) ** 2 + lams ** 2)


def _median_bin(h: np.ndarray) -> np.ndarray:
    """int [..., 1024] -> the lower median bin, as noise_sigma's."""
    cum = np.cumsum(h, axis=-1)
    return (cum < ((cum[..., -1] + 1) // 2)[..., None]).sum(axis=-1)


def grain_shape(h1, h2, cfg=True) -> np.ndarray:
    """int32 [B, 2] = (s, lam), ops.grain_shaped's shape, from the SCENE ring's histograms at steps 1 and 2 (ops.highpass_hist_step,
    int [B, C + 1, 1024]) under grain_cfg(cfg).
    s: rows 0..C-1 pooled over the channels, M1 and M2 their lower median bins, q = M2 / M1; the s in 0..max_blur whose grain_q_model is
    nearest to q (ties: the smaller); 0 when q <= 1, M1 = 0 or either pooled histogram counts fewer than min_pixels C.
    lam: with M_c the step-1 median bins of rows 0..C-1 and M_S that of row C (the channel sum),
    rho = clamp((M_S^2 - sum M_c^2) / ((sum M_c)^2 - sum M_c^2), 0, 1), the share of the variance that the channels have in common; the
    lam in 0..256 whose lam^2 / ((256 - lam)^2 + lam^2) is nearest to rho (ties: the smaller); 0 when C = 1, the denominator is 0 or
    luma is False."""
    cfg = grain_cfg(cfg)
    sp = cfg.get("spectrum") or dict(max_blur=ops.GRAIN_MAX_BLUR, luma=True)
    h1, h2 = _hist(h1), _hist(h2)
    if h1.shape != h2.shape or h1.shape[1] < 2:
        raise ValueError(f"grain_shape: the histograms must be [B, C + 1, {ops.HIGHPASS_BINS}] and agree, got {h1.shape} and {h2.shape}")
    B, C = h1.shape[0], h1.shape[1] - 1
    q_model, rho_model = _shape_models(sp["max_blur"])
    pooled1, pooled2 = h1[:, :C].sum(axis=1), h2[:, :C].sum(axis=1)
    m1, m2, mc = _median_bin(pooled1), _median_bin(pooled2), _median_bin(h1).astype(np.float64)
    out = np.zeros((B, 2), np.int32)
    for b in range(B):
        trusted = min(int(pooled1[b].sum()), int(pooled2[b].sum())) >= cfg["min_pixels"] * C
        if trusted and m1[b] > 0 and m2[b] > m1[b]:
            out[b, 0] = int(np.argmin(np.abs(q_model - float(m2[b]) / float(m1[b]))))
        own = float((mc[b, :C] ** 2).sum())
        den = float(mc[b, :C].sum()) ** 2 - own
        if C > 1 and sp["luma"] and den > 0:
            rho = min(max((mc[b, C] ** 2 - own) / den, 0.0), 1.0)
            out[b, 1] = int(np.argmin(np.abs(rho_model - rho)))
    return out


def grain_shaped_gains(hist_scene, hist_edit, shape, cfg=True) -> np.ndarray:
    """int32 [B, C]: ops.grain_shaped's gain.  sigma_add is grain_levels' of rows 0..C-1 of the two step-1 histograms (int
    [B, C + 1, 1024]): the missing level as the step-1 high-pass sees it.  Grain of shape (s, lam) and input level L reads as L w there
    and has the true deviation L t (grain_shape_levels), so L = sigma_add / w, brought down to max_sigma / t where its true deviation
    would pass max_sigma; gain = floor(L / ops.GRAIN_SIGMA0 * 65536 + 0.5), at most 2^18."""
    cfg = grain_cfg(cfg)
    hs, he = _hist(hist_scene), _hist(hist_edit)
    add = grain_levels(hs[:, :-1], he[:, :-1], cfg)[2]
    out = np.zeros(add.shape, np.int32)
    for b, (s, lam) in enumerate(np.asarray(shape).tolist()):
        w, t = grain_shape_levels(s, lam)
        level = np.minimum(add[b] / w, cfg["max_sigma"] / t)
        out[b] = np.minimum(np.floor(level / ops.GRAIN_SIGMA0 * 65536.0 + 0.5), ops.GRAIN_MAX_GAIN).astype(np.int32)
    return out


def ring_mask(alpha: torch.Tensor, ring: int = RING) -> torch.Tensor:
    """uint8 [B, H, W] blend weight -> 255 on the pixels within `ring` (square window) of alpha's support that are not in it, else 0:
    support = 255 where alpha > 0, ring = mask_dilate(support, ring) with the support's own pixels cleared.  These pixels lie just
    outside the blend, where the edit shows unchanged scene content."""
    if alpha.dtype != torch.uint8 or alpha.dim() != 3:
        raise ValueError(f"ring_mask: alpha must be uint8 [B, H, W], got {alpha.dtype} {tuple(alpha.shape)}")
    if not 1 <= int(ring) <= 255:
        raise ValueError(f"ring_mask: ring must be in [1, 255], got {ring}")
    support = (alpha > 0).to(torch.uint8).mul_(255).contiguous()
    return ops.mask_dilate(support, int(ring)).masked_fill_(support > 0, 0)


def fit_luts(moments, gain: Tuple[float, float] = GAIN, max_shift: int = MAX_SHIFT, min_pixels: int = MIN_PIXELS) -> np.ndarray:
    """moments int [B, C, 5] = (n, sum a, sum b, sum a a, sum a b) with a the edit and b the colour reference (ops.masked_moments) ->
    uint8 [B, C, 256] tables t with t[a] ~ b, the least-squares line b = g a + o per (sample, channel), on the host:
    den = n sum aa - (sum a)^2 in Python integers; the identity table when n < min_pixels or den <= 0; else
    g = (n sum ab - sum a sum b) / den clamped to `gain`, o = (sum b - g sum a) / n in float64, and
    t[v] = floor(g v + o + 0.5) clamped to [v - max_shift, v + max_shift], then to [0, 255]."""
    m = moments.cpu().numpy() if isinstance(moments, torch.Tensor) else np.asarray(moments)
    if m.ndim != 3 or m.shape[2] != 5:
        raise ValueError(f"fit_luts: moments must be [B, C, 5], got {m.shape}")
    v = np.arange(256, dtype=np.float64)
    ident = np.arange(256, dtype=np.int64)
    out = np.empty(m.shape[:2] + (256,), np.uint8)
    for b in range(m.shape[0]):
        for c in range(m.shape[1]):
            n, sa, sb, saa, sab = (int(x) for x in m[b, c])
            den = n * saa - sa * sa
            if n < min_pixels or den <= 0:
                out[b, c] = ident
                continue
            g = min(max((n * sab - sa * sb) / den, float(gain[0])), float(gain[1]))
            o = (sb - g * sa) / n
            t = np.floor(g * v + o + 0.5).astype(np.int64)
            t = np.minimum(np.maximum(t, ident - int(max_shift)), ident + int(max_shift))
            out[b, c] = np.clip(t, 0, 255)
    return out


def paste(original: torch.Tensor, edited: torch.Tensor, mask_grey: torch.Tensor, dilate: int = DILATE, feather: int = FEATHER,
          color_match=None, color_ref: Optional[torch.Tensor] = None, rect=None, origin: Tuple[int, int] = (0, 0), seamless=None,
          grain=None, keyed=None) -> torch.Tensor:
    """original uint8 [B, H, W, 3], edited uint8 [B, h, w, 3], mask_grey uint8 [B, H, W], all on the device -> [B, H, W, 3]: the edit,
    resampled to (H, W) when its size differs (ops.resample_u8: Pillow's bicubic), blended over the original under alpha_mask computed at
    the ORIGINAL resolution.  Outside the mask dilated by dilate + 3 feather the result is the original byte for byte; with
    dilate >= 3 feather it is the resampled edit on every mask pixel.
    color_match: None, or True / dict(ring, gain, max_shift, min_pixels): the resampled edit goes through a per-channel table fitted
    (fit_luts) on the ring just outside the blend (ring_mask) to the colours of color_ref (uint8 [B, H, W, 3]; None: `original`) before
    it is blended (ops.overlay_lut).  The alpha is the same, so the bytes outside the grown mask are still the original's.
    rect (a rectify.Rect; DESIGN.md section 4 "Rectified lines"): `edited` is the UPRIGHT result of a rectified line and `original` the
    scene window whose top-left pixel is scene pixel `origin`.  The edit is resampled to the rectangle's own size (rh, rw) and warped
    into the window (ops.warp_affine_u8 under rectify.matrices' upright -> scene matrix) instead of being resized to it; the alpha is
    still that of mask_grey, the line's ORIGINAL mask, so the bytes outside the grown mask stay the original's; with color_match the
    ring is cut to the pixels the warp covered (their sample position lies inside the upright crop).
    rect may also be a perspective.Quad (DESIGN.md section 4 "Perspective lines"): the same, with the edit resampled to the quad's crop
    (rh, rw) and warped by ops.warp_perspective_u8 under perspective.matrices' upright -> scene homography.
    Or a curve.Ribbon (DESIGN.md section 4 "Curved lines"): the same through ops.warp_grid_u8 under curve.grids' backward grid.
    seamless: None, or True / dict(smooth, max_shift) (DESIGN.md section 4 "Seamless paste"): the final blend is ops.seamless_overlay
    instead: the difference between color_ref (None: `original`) and the edit -- after the table, when color_match is set too -- is
    taken on the pixels with alpha == 0 (that the warp covered, when there was one), interpolated across alpha's support and added to
    the edit before the blend.  The alpha is the same, so the bytes outside the grown mask are still the original's.  color_ref may then
    be given without color_match.  Without the key the calls are those above, unchanged.
    grain: None, or True / dict(ring, max_sigma, strength, min_pixels, seed) (DESIGN.md section 4 "Grain match"): after the final blend
    above, the noise level of color_ref (None: `original`) on the ring just outside the blend (cut to what the warp covered) and that of
    the result where alpha == 255 are estimated (ops.highpass_hist, noise_sigma) and the missing variance is added as hashed white grain
    under alpha (grain_gains, ops.grain), anchored at the scene position `origin` + the pixel's place in the window.  The alpha is the
    same, so the bytes outside the grown mask are still the original's.  color_ref may then be given without color_match.  Without the
    key the calls are those above, unchanged.
    grain=dict(spectrum=True | dict(max_blur, luma), ...) (DESIGN.md section 4 "Grain spectrum"): the three histograms become
    ops.highpass_hist_step (the ring at steps 1 and 2, the result at step 1), grain_shape estimates the scene noise's blur and the share
    its channels have in common, and ops.grain_shaped adds grain of that shape at grain_shaped_gains' level.  Without the sub-key the
    grain's calls are those above, unchanged; with max_blur=0, luma=False the bytes are.
    keyed: None, or True / dict(lo, hi, dilate, feather, noise, ring, min_pixels) (DESIGN.md section 4 "Keyed paste"): behind the blend
    above (plain, colour-matched and / or seamless) and in front of the grain, a pixel keeps `original`'s byte unless the blend really
    differs there: key = change_key(original, result, keyed, sigma) and the result goes over `original` once more under it
    (ops.overlay).  sigma, per sample, is the largest per-channel noise level of color_ref (None: `original`) on the ring just outside
    the blend, cut to what the warp covered (ops.highpass_hist, keyed_sigma): the lower threshold stays `noise` standard deviations above
    it (keyed_levels); noise = 0 takes no estimate.  The grain then runs on the keyed result under min(alpha, key) where it took alpha.
    Exactly: the result is `original` wherever the key is 0 and, as before, everywhere outside the grown mask; it carries the blend's
    byte wherever the metric reaches hi_eff; it lies between `original` and the blend; and hi_eff = 0 (lo = hi = 0 on a ring without
    noise, or with noise = 0) gives the bytes of the call without the key.  color_ref may then be given without color_match.  Without
    the key the calls are those above, unchanged."""
    if original.dtype != torch.uint8 or original.dim() != 4 or edited.dtype != torch.uint8 or edited.dim() != 4:
        raise ValueError("paste: original and edited must be uint8 [B, H, W, C]")
    if edited.shape[0] != original.shape[0] or edited.shape[3] != original.shape[3] or mask_grey.shape != original.shape[:3]:
        raise ValueError(f"paste: original {tuple(original.shape)}, edited {tuple(edited.shape)} and mask {tuple(mask_grey.shape)} do not agree")
    if color_match is None and seamless is None and grain is None and keyed is None and color_ref is not None:
        raise ValueError("paste: color_ref needs color_match")
    sm = None if seamless is None else seamless_cfg(seamless)
    gr = None if grain is None else grain_cfg(grain)
    kd = None if keyed is None else keyed_cfg(keyed)
    original, edited = original.contiguous(), edited.contiguous()
    covered = None
    if rect is not None:
        if tuple(edited.shape[1:3]) != (rect.rh, rect.rw):
            edited = ops.resample_u8(edited, (rect.rh, rect.rw))
        size = (original.shape[1], original.shape[2])
        edited, covered = getattr(ops, rect.WARP + "_u8")(edited, *rect.backward(origin, size), size, coverage=True)
    elif edited.shape[1:3] != original.shape[1:3]:
        edited = ops.resample_u8(edited, (original.shape[1], original.shape[2]))
    alpha = alpha_mask(mask_grey.contiguous(), dilate, feather)
    if color_match is None and sm is None and gr is None and kd is None:
        return ops.overlay(original, edited, alpha)
    cm = None if color_match is None else color_match_cfg(color_match)
    ref = original if color_ref is None else color_ref.contiguous()
    if ref.shape != original.shape or ref.dtype != torch.uint8:
        raise ValueError(f"paste: color_ref must be uint8 of original's shape {tuple(original.shape)}, got {ref.dtype} {tuple(ref.shape)}")
    rings = {}

    def ring_of(width):                              # colour matching and the grain match share the ring when their widths agree
        if width not in rings:
            rings[width] = ring_mask(alpha, width) if covered is None else ring_mask(alpha, width) & covered
        return rings[width]

    if cm is None and sm is None:
        result = ops.overlay(original, edited, alpha)
    elif cm is None:
        result = ops.seamless_overlay(original, ref, edited, alpha, covered=covered, smooth=sm["smooth"], max_shift=sm["max_shift"])
    else:
        luts = fit_luts(ops.masked_moments(edited, ref, ring_of(cm["ring"])), cm["gain"], cm["max_shift"], cm["min_pixels"])
        luts = torch.from_numpy(luts).to(original.device)
        if sm is not None:
            result = ops.seamless_overlay(original, ref, edited, alpha, covered=covered, lut=luts, smooth=sm["smooth"], max_shift=sm["max_shift"])
        else:
            result = ops.overlay_lut(original, edited, alpha, luts)
    under = alpha                                    # the weight the grain is added under
    if kd is not None:
        sigma = keyed_sigma(ops.highpass_hist(ref, ring_of(kd["ring"]), 255, 255), kd) if kd["noise"] > 0 else None
        key = change_key(original, result, kd, sigma)
        result = ops.overlay(original, result, key)
        under = torch.minimum(alpha, key)
    if gr is None:
        return result
    if "spectrum" in gr:
        ring = ring_of(gr["ring"])
        h1, h2 = ops.highpass_hist_step(ref, ring, 255, 255, 1), ops.highpass_hist_step(ref, ring, 255, 255, 2)
        shape = grain_shape(h1, h2, gr)
        gains = grain_shaped_gains(h1, ops.highpass_hist_step(result, under, 255, 255, 1), shape, gr)
        if not gains.any():
            return result
        return ops.grain_shaped(result, under, gains, shape, origin, gr["seed"], out=result)
    gains = grain_gains(ops.highpass_hist(ref, ring_of(gr["ring"]), 255, 255), ops.highpass_hist(result, under, 255, 255), gr)
    if not gains.any():
        return result                                # nothing to add: the scene is no noisier than the edit, or too few pixels to tell
    return ops.grain(result, under, gains, origin, gr["seed"], out=result)


def grey_of(mask) -> np.ndarray:
    """Host uint8 [H, W] grey value of a mask given as a PIL image or an [H, W] / [H, W, 3] uint8 array: PIL's convert("L")."""
    from PIL import Image
    if isinstance(mask, Image.Image):
        return np.array(mask.convert("L"))
    m = np.asarray(mask)
    return np.array(Image.fromarray(m).convert("L")) if m.ndim == 3 else m
