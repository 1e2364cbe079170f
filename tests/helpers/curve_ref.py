"""numpy restatement of the curved-line arithmetic (include/textflux_hip.h: tfx_warp_grid_u8; textflux_amd/paste_back.py:
paste(rect=Ribbon)), written from the header's text.  The one thing shared with the package is the tap table's builder: the
specification says "the same array".  Everything is integer arithmetic, so the device results are compared bit for bit.  The rest of
the paste (alpha, ring, fit, blend) is the restatement of tests/helpers/paste_back_ref.py and per_line_ref.py, imported."""
import numpy as np

from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from textflux_amd.rectify import catmull_rom_taps

TAPS = catmull_rom_taps()
NONE = np.iinfo(np.int64).min


def grid_shape(out_size, shift):
    Ho, Wo = out_size
    return ((Ho - 1) >> shift) + 2, ((Wo - 1) >> shift) + 2


def positions(grid, shift, out_size):
    """(on, X, Y), [out_h, out_w] each, of one grid int64 [gh, gw, 2]: on = none of the pixel's four nodes carries the marker in x; X, Y
    = the Q16 blend ((c - ax)(c - ay) g00 + ax (c - ay) g01 + (c - ax) ay g10 + ax ay g11) >> (2 shift), the int64 products wrapping and
    the shift arithmetic (numpy's >> on int64 floors); 0 where the pixel is off."""
    Ho, Wo = out_size
    c = 1 << shift
    i = np.arange(Wo, dtype=np.int64)[None, :]
    j = np.arange(Ho, dtype=np.int64)[:, None]
    gx, gy, ax, ay = i >> shift, j >> shift, i & (c - 1), j & (c - 1)
    g00, g01, g10, g11 = grid[gy, gx], grid[gy, gx + 1], grid[gy + 1, gx], grid[gy + 1, gx + 1]
    on = (g00[..., 0] != NONE) & (g01[..., 0] != NONE) & (g10[..., 0] != NONE) & (g11[..., 0] != NONE)
    w00, w01, w10, w11 = (c - ax) * (c - ay), ax * (c - ay), (c - ax) * ay, ax * ay
    with np.errstate(over="ignore"):
        X, Y = ((w00 * g00[..., k] + w01 * g01[..., k] + w10 * g10[..., k] + w11 * g11[..., k]) >> (2 * shift) for k in (0, 1))
    return on, np.where(on, X, 0), np.where(on, Y, 0)


def warp_grid(x, grid, shift, out_size, coverage=False, taps=TAPS):
    """x u8 [B, H, W, C] or [H, W, C]; grid int64 [B, gh, gw, 2] or [gh, gw, 2]; out_size = (out_h, out_w) -> u8 [B, out_h, out_w, C] (and
    the coverage u8 [B, out_h, out_w]).  Per destination pixel: a marked node among its four gives 0 on every channel and coverage 0;
    otherwise xi = X >> 16, fx = (X >> 8) & 255 (yi, fy alike), 4 x 4 taps at rows yi - 1 .. yi + 2, columns xi - 1 .. xi + 2, indices
    clamped into the image, weights taps[fy][r] taps[fx][k]; out = clamp((acc + 2^27) >> 28, 0, 255); coverage = 255 where 0 <= xi < W and
    0 <= yi < H."""
    x = np.asarray(x)
    x = x[None] if x.ndim == 3 else x
    assert x.dtype == np.uint8 and x.ndim == 4 and 0 <= shift <= 5
    B, H, W, C = x.shape
    Ho, Wo = out_size
    grid = np.asarray(grid)
    assert grid.dtype == np.int64 and grid.shape[-3:] == grid_shape(out_size, shift) + (2,)
    grid = np.broadcast_to(grid.reshape((-1,) + grid.shape[-3:]), (B,) + grid.shape[-3:])
    t = taps.astype(np.int64)
    out = np.empty((B, Ho, Wo, C), np.uint8)
    cov = np.empty((B, Ho, Wo), np.uint8)
    for b in range(B):
        on, X, Y = positions(grid[b], shift, (Ho, Wo))
        xi, yi, fx, fy = X >> 16, Y >> 16, (X >> 8) & 255, (Y >> 8) & 255
        acc = np.zeros((Ho, Wo, C), np.int64)
        for r in range(4):
            yy = np.clip(yi - 1 + r, 0, H - 1)
            for k in range(4):
                xx = np.clip(xi - 1 + k, 0, W - 1)
                acc += (t[fy, r] * t[fx, k])[:, :, None] * x[b][yy, xx].astype(np.int64)
        out[b] = np.where(on[:, :, None], np.clip((acc + (1 << 27)) >> 28, 0, 255), 0)
        cov[b] = np.where(on & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H), 255, 0)
    return (out, cov) if coverage else out


def embed(affine, shift, out_size):
    """The Q16 affine matrix int64 [6] as a grid int64 [gh, gw, 2]: the matrix evaluated at the nodes' pixels (q << shift, r << shift)."""
    a = [int(v) for v in np.asarray(affine).reshape(6)]
    gh, gw = grid_shape(out_size, shift)
    q = (np.arange(gw, dtype=np.int64) << shift)[None, :]
    r = (np.arange(gh, dtype=np.int64) << shift)[:, None]
    return np.stack([a[0] * q + a[1] * r + a[2], a[3] * q + a[4] * r + a[5]], axis=-1)


def paste_ribbon(original, edited, grey, d, r, grid_back, shift, rw, rh, color_match=None, color_ref=None):
    """The curved line's paste (perspective_ref.paste_quad with the other warp): original u8 [1, H, W, 3] (the scene window), edited u8
    [1, h, w, 3] (the upright result), grey u8 [1, H, W] (the line's ORIGINAL mask over the window), grid_back = the upright -> window
    grid.  The edit is resized to (rh, rw) with PIL's bicubic when its size differs, warped into the window, and blended under
    alpha_mask(grey); with color_match (a dict of ring, gain, max_shift, min_pixels) the ring is ANDed with the coverage and the table is
    fitted against color_ref (None: original)."""
    if edited.shape[1:3] != (rh, rw):
        edited = ref.resize(edited, (rh, rw))
    warped, cov = warp_grid(edited, grid_back, shift, original.shape[1:3], coverage=True)
    alpha = ref.alpha_mask(grey, d, r)
    if color_match is None:
        return ref.overlay(original, warped, alpha)
    ring = plref.ring_mask(alpha, color_match["ring"]) & cov
    lut = plref.fit_luts(plref.moments_np(warped, original if color_ref is None else color_ref, ring), color_match["gain"],
                         color_match["max_shift"], color_match["min_pixels"])
    return plref.overlay_lut(original, warped, alpha, lut)
