"""numpy restatement of the perspective-line arithmetic (include/textflux_hip.h: tfx_warp_perspective_u8; textflux_amd/paste_back.py:
paste(rect=Quad)), written from the header's text.  The one thing shared with the package is the tap table's builder: the
specification says "the same array".  Everything is integer arithmetic, so the device results are compared bit for bit.  The rest of
the paste (alpha, ring, fit, blend) is the restatement of tests/helpers/paste_back_ref.py and per_line_ref.py, imported."""
import numpy as np

from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from textflux_amd.rectify import catmull_rom_taps

TAPS = catmull_rom_taps()


def positions(m, out_size):
    """(D, PX, PY), int64 [out_h, out_w] each, of one matrix m int64 [9]: D = m6 i + m7 j + m8 and, where D > 0, PX = floor(Nx 256 / D),
    PY = floor(Ny 256 / D) (numpy's // floors; the int64 product wraps); where D <= 0, PX = PY = 0 (unused)."""
    Ho, Wo = out_size
    i = np.arange(Wo, dtype=np.int64)[None, :]
    j = np.arange(Ho, dtype=np.int64)[:, None]
    Nx, Ny, D = (m[k] * i + m[k + 1] * j + m[k + 2] for k in (0, 3, 6))
    on = D > 0
    Ds = np.where(on, D, 1)
    return D, np.where(on, (Nx * 256) // Ds, 0), np.where(on, (Ny * 256) // Ds, 0)


def warp_perspective(x, m, out_size, coverage=False, taps=TAPS):
    """x u8 [B, H, W, C] or [H, W, C]; m int64 [B, 9] or [9]; out_size = (out_h, out_w) -> u8 [B, out_h, out_w, C] (and the coverage u8
    [B, out_h, out_w]).  Per destination pixel (i, j): D <= 0 gives 0 on every channel and coverage 0; otherwise xi = PX >> 8,
    fx = PX & 255 (yi, fy alike), 4 x 4 taps at rows yi - 1 .. yi + 2, columns xi - 1 .. xi + 2, indices clamped into the image, weights
    taps[fy][r] taps[fx][k]; out = clamp((acc + 2^27) >> 28, 0, 255); coverage = 255 where 0 <= xi < W and 0 <= yi < H."""
    x = np.asarray(x)
    x = x[None] if x.ndim == 3 else x
    assert x.dtype == np.uint8 and x.ndim == 4
    B, H, W, C = x.shape
    m = np.broadcast_to(np.asarray(m, np.int64).reshape(-1, 9), (B, 9))
    Ho, Wo = out_size
    t = taps.astype(np.int64)
    out = np.empty((B, Ho, Wo, C), np.uint8)
    cov = np.empty((B, Ho, Wo), np.uint8)
    for b in range(B):
        D, PX, PY = positions(m[b], (Ho, Wo))
        xi, yi, fx, fy = PX >> 8, PY >> 8, PX & 255, PY & 255
        acc = np.zeros((Ho, Wo, C), np.int64)
        for r in range(4):
            yy = np.clip(yi - 1 + r, 0, H - 1)
            for k in range(4):
                xx = np.clip(xi - 1 + k, 0, W - 1)
                acc += (t[fy, r] * t[fx, k])[:, :, None] * x[b][yy, xx].astype(np.int64)
        on = D > 0
        out[b] = np.where(on[:, :, None], np.clip((acc + (1 << 27)) >> 28, 0, 255), 0)
        cov[b] = np.where(on & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H), 255, 0)
    return (out, cov) if coverage else out


def embed(affine):
    """The Q16 affine matrix int64 [..., 6] as a homography int64 [..., 9]: m6 = m7 = 0, m8 = 2^16."""
    a = np.asarray(affine, np.int64)
    tail = np.broadcast_to(np.array([0, 0, 1 << 16], np.int64), a.shape[:-1] + (3,))
    return np.concatenate([a, tail], axis=-1)


def paste_quad(original, edited, grey, d, r, m_back, rw, rh, color_match=None, color_ref=None):
    """The perspective line's paste (rectify_ref.paste_rect with the other warp): original u8 [1, H, W, 3] (the scene window), edited u8
    [1, h, w, 3] (the upright result), grey u8 [1, H, W] (the line's ORIGINAL mask over the window), m_back = the upright -> window
    matrix.  The edit is resized to (rh, rw) with PIL's bicubic when its size differs, warped into the window, and blended under
    alpha_mask(grey); with color_match (a dict of ring, gain, max_shift, min_pixels) the ring is ANDed with the coverage and the table is
    fitted against color_ref (None: original)."""
    if edited.shape[1:3] != (rh, rw):
        edited = ref.resize(edited, (rh, rw))
    warped, cov = warp_perspective(edited, m_back, original.shape[1:3], coverage=True)
    alpha = ref.alpha_mask(grey, d, r)
    if color_match is None:
        return ref.overlay(original, warped, alpha)
    ring = plref.ring_mask(alpha, color_match["ring"]) & cov
    lut = plref.fit_luts(plref.moments_np(warped, original if color_ref is None else color_ref, ring), color_match["gain"],
                         color_match["max_shift"], color_match["min_pixels"])
    return plref.overlay_lut(original, warped, alpha, lut)
