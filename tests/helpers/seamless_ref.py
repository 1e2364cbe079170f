"""numpy restatement of the seamless paste (include/textflux_hip.h: tfx_seamless_overlay_u8; textflux_amd/paste_back.py:
paste(seamless=...)), written from the specification with no code shared with the package: 64-bit integers, Python floor division,
one level after the other.  Everything is integer arithmetic, so the device results are compared bit for bit.  The rest of the paste
(alpha, ring, fit, warp) is the restatement of the neighbouring helpers, imported."""
import numpy as np

from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref


def _pull(v: np.ndarray, filled: np.ndarray):
    """One pull: v int64 [h, w, C], filled bool [h, w] -> the level ((h + 1) // 2, (w + 1) // 2)."""
    h, w, C = v.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    s = np.zeros((hc, wc, C), np.int64)
    n = np.zeros((hc, wc), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            sub_f = filled[dy::2, dx::2]
            sub_v = np.where(sub_f[..., None], v[dy::2, dx::2], 0)
            s[:sub_f.shape[0], :sub_f.shape[1]] += sub_v
            n[:sub_f.shape[0], :sub_f.shape[1]] += sub_f
    nn = np.maximum(n, 1)[..., None]
    return np.where((n > 0)[..., None], (2 * s + nn) // (2 * nn), 0), n > 0


def _push(v: np.ndarray, filled: np.ndarray, c: np.ndarray) -> np.ndarray:
    """One push: the unfilled pixels of the level v take the 2x upsample of the complete coarse level c."""
    h, w, _ = v.shape
    hc, wc = c.shape[:2]
    y, x = np.arange(h), np.arange(w)
    i, j = y >> 1, x >> 1
    i2 = np.clip(i + np.where(y & 1, 1, -1), 0, hc - 1)
    j2 = np.clip(j + np.where(x & 1, 1, -1), 0, wc - 1)
    up = (9 * c[i][:, j] + 3 * c[i][:, j2] + 3 * c[i2][:, j] + c[i2][:, j2] + 8) >> 4
    return np.where(filled[..., None], v, up)


def membrane(d: np.ndarray, known: np.ndarray, free: np.ndarray, smooth: int) -> np.ndarray:
    """d int [H, W, C] (ref - e; read on the known pixels only), known, free bool [H, W] -> v int64 [H, W, C] with 6 fractional bits:
    64 d on the known pixels, pulled up to 1 x 1, pushed back down into every unfilled pixel, then `smooth` Jacobi sweeps of the free
    pixels."""
    known, free = np.asarray(known, bool), np.asarray(free, bool)
    v0 = np.where(known[..., None], np.asarray(d, np.int64) * 64, 0)
    vals, fills = [v0], [known]
    while vals[-1].shape[:2] != (1, 1):
        v, f = _pull(vals[-1], fills[-1])
        vals.append(v)
        fills.append(f)
    c = vals[-1]                                     # an unfilled top is 0 already
    for l in range(len(vals) - 2, -1, -1):
        c = _push(vals[l], fills[l], c)
    v = c
    for _ in range(int(smooth)):
        p = np.pad(v, ((1, 1), (1, 1), (0, 0)), mode="edge")       # a neighbour outside the window is the centre's own value
        nb = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + 2) >> 2
        v = np.where(free[..., None], nb, v)
    return v


def seamless_overlay(orig, ref_img, edit, alpha, covered=None, lut=None, smooth=8, max_shift=32) -> np.ndarray:
    """orig, ref_img, edit u8 [B, H, W, C], alpha u8 [B, H, W], covered u8 [B, H, W] or None, lut u8 [B, C, 256] or None -> u8
    [B, H, W, C]."""
    orig, ref_img, edit, alpha = (np.asarray(t) for t in (orig, ref_img, edit, alpha))
    out = np.empty_like(orig)
    for s in range(orig.shape[0]):
        e = edit[s].astype(np.int64)
        if lut is not None:
            e = np.stack([np.asarray(lut)[s, c][edit[s, :, :, c]] for c in range(edit.shape[3])], axis=2).astype(np.int64)
        a = alpha[s].astype(np.int64)
        free = a > 0
        known = (a == 0) if covered is None else (a == 0) & (np.asarray(covered)[s] != 0)
        v = membrane(ref_img[s].astype(np.int64) - e, known, free, smooth)
        delta = np.clip((v + 32) >> 6, -int(max_shift), int(max_shift))
        e2 = np.clip(e + delta, 0, 255)
        o = orig[s].astype(np.int64)
        blend = (o * (255 - a[..., None]) + e2 * a[..., None] + 127) // 255
        out[s] = np.where(free[..., None], blend, o).astype(np.uint8)
    return out


def paste(original, edited, grey, d, r, seamless=None, color_match=None, color_ref=None, warped=None):
    """The seamless paste of the specification: original u8 [B, H, W, 3], edited u8 [B, h, w, 3] (resized with PIL's bicubic when its
    size differs), grey u8 [B, H, W].  seamless: dict(smooth, max_shift); color_match: None or dict(ring, gain, max_shift, min_pixels)
    (the table is fitted as in per_line_ref.paste); color_ref: the image the difference and the fit are taken against (None:
    original); warped: None, or (the edit already warped into the window, its coverage) for a rectified line."""
    sm = dict(smooth=8, max_shift=32)
    sm.update(seamless or {})
    covered = None
    if warped is not None:
        edited, covered = warped
    elif edited.shape[1:3] != original.shape[1:3]:
        edited = ref.resize(edited, original.shape[1:3])
    alpha = ref.alpha_mask(grey, d, r)
    against = original if color_ref is None else color_ref
    lut = None
    if color_match is not None:
        ring = plref.ring_mask(alpha, color_match["ring"])
        if covered is not None:
            ring = ring & covered
        lut = plref.fit_luts(plref.moments_np(edited, against, ring), color_match["gain"], color_match["max_shift"], color_match["min_pixels"])
    return seamless_overlay(original, against, edited, alpha, covered, lut, sm["smooth"], sm["max_shift"])
