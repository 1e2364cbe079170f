"""Curved per-line edits on the GPU: the control-grid warp kernel (imageops.hip: warp_grid_u8) and paste_back.paste(rect=Ribbon) against
the numpy restatement in tests/helpers/curve_ref.py, bit for bit (integer arithmetic only), and batch_driver.run_items(curve=True) end to
end on the tiny synthetic checkpoint of the e2e tests."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import curve_ref as cref
from tests.helpers import paste_back_ref as ref
from tests.helpers import rectify_ref as rref

pytestmark = pytest.mark.gpu
Q = 1 << 16
NONE = cref.NONE
IDENT6 = np.array([Q, 0, 0, 0, Q, 0], np.int64)


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def rotation(deg, src_centre, dst_centre, scale=1.0):
    """test_rectify_gpu's Q16 matrix: destination pixel p reads the source at src_centre + scale R(deg) (p - dst_centre)."""
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    m = [round(c * Q), round(-s * Q), 0, round(s * Q), round(c * Q), 0]
    m[2] = round(src_centre[0] * Q) - m[0] * dst_centre[0] - m[1] * dst_centre[1]
    m[5] = round(src_centre[1] * Q) - m[3] * dst_centre[0] - m[4] * dst_centre[1]
    return np.array(m, np.int64)


BORDER = (rotation(17, (37.3, 18.2), (14, 20)), rotation(-17, (10.0, 2.5), (27, 20), 1.3))    # test_rectify_gpu's "border" case


def node_pixels(size, shift):
    """(x, y), float64 [gh, gw] each: the destination pixels the nodes stand for."""
    gh, gw = cref.grid_shape(size, shift)
    return np.meshgrid(np.arange(gw, dtype=np.float64) * (1 << shift), np.arange(gh, dtype=np.float64) * (1 << shift))


def q16(x, y):
    return np.stack([np.round(x * Q), np.round(y * Q)], axis=-1).astype(np.int64)


def arc(size, shift, radius, centre, top, scale=1.0):
    """An arch unrolled: destination column i is the arc length, row j the depth below the arch's outer edge; the source is the point
    at angle (i - w / 2) scale / radius from straight up, radius - j scale + top from `centre`."""
    x, y = node_pixels(size, shift)
    a, r = (x - size[1] / 2) * scale / radius, radius + top - y * scale
    return q16(centre[0] + r * np.sin(a), centre[1] - r * np.cos(a))


def smooth(size, seed):
    """A per-pixel map: the identity plus a few low waves of some pixels' amplitude."""
    rng = np.random.default_rng(seed)
    x, y = node_pixels(size, 0)
    dx, dy = (sum(rng.uniform(-3, 3) * np.sin(x * rng.uniform(0.05, 0.3) + y * rng.uniform(0.05, 0.3) + rng.uniform(0, 6)) for _ in range(3))
              for _ in range(2))
    return q16(x + dx, y + dy)


def negative(size, shift, seed):
    """Positions that are negative, with fractions, on most pixels, and nodes whose blend leaves a remainder: where flooring differs
    from truncating."""
    rng = np.random.default_rng(seed)
    return cref.embed(rotation(9, (-6.3 + seed, -4.7), (13, 9)), shift, size) + rng.integers(-Q, Q, cref.grid_shape(size, shift) + (2,))


def marked(size, shift, nodes):
    g = cref.embed(rotation(5, (20.0, 12.0), (16, 4)), shift, size)
    for r, q in nodes:
        g[r, q, 0] = NONE
    return g


# case: (source H, W), (destination h, w), shift, the two samples' grids
CASES = {
    **{f"embedded{s}": ((37, 53), (29, 41), s, tuple(cref.embed(a, s, (29, 41)) for a in BORDER)) for s in (0, 3, 5)},
    # the arch leaves the source at the top and on the right / at the top and on the left
    "arc": ((37, 53), (29, 41), 3, (arc((29, 41), 3, 60.0, (34.0, 70.0), 12.0), arc((29, 41), 3, 45.0, (14.0, 55.0), 12.0, 1.2))),
    "per_pixel": ((37, 53), (37, 53), 0, (smooth((37, 53), 1), smooth((37, 53), 2))),
    "negative": ((23, 31), (19, 27), 2, (negative((19, 27), 2, 0), negative((19, 27), 2, 3))),
    # marked nodes: at shift 4 node (0, 0) takes out columns 0..15 and node (0, 2) columns 16..32, so the first 32 x 8 tile holds both
    # kinds; at shift 5 node (1, 2) is seen by the last column alone (as its g11) and node (0, 0) by all others.  The last cell is
    # one pixel wide (33 = 2 * 16 + 1 = 32 + 1) and the second tile row is one line
    "marked4": ((37, 53), (9, 33), 4, (marked((9, 33), 4, [(0, 0)]), marked((9, 33), 4, [(0, 2)]))),
    "marked5": ((37, 53), (9, 33), 5, (marked((9, 33), 5, [(1, 2)]), marked((9, 33), 5, [(0, 0)]))),
    "large": ((300, 500), (128, 512), 3, (arc((128, 512), 3, 700.0, (250.0, 760.0), 10.0), arc((128, 512), 3, 420.0, (240.0, 470.0), 30.0, 0.8))),
    "identity": ((37, 53), (37, 53), 4, (cref.embed(IDENT6, 4, (37, 53)),) * 2),
}


@pytest.fixture(scope="module")
def expected():
    """The restatement's answer per (case, channels), computed once."""
    cache = {}

    def get(case, c):
        if (case, c) not in cache:
            (H, W), (h, w), shift, gs = CASES[case]
            x = np.random.default_rng(H * W + c).integers(0, 256, (2, H, W, c), dtype=np.uint8)     # the two samples differ: a batch-stride slip shows
            cache[case, c] = (x,) + cref.warp_grid(x, np.stack(gs), shift, (h, w), coverage=True)
        return cache[case, c]
    return get


def test_the_cases_exercise_what_they_claim():
    for case, ((H, W), (h, w), shift, gs) in CASES.items():
        for k, g in enumerate(gs):
            assert g.shape == cref.grid_shape((h, w), shift) + (2,) and g.dtype == np.int64
            assert np.abs(np.where(g == NONE, 0, g)).max() < 1 << 50, case
            on, X, Y = cref.positions(g, shift, (h, w))
            xi, yi = X >> 16, Y >> 16
            if case == "arc":
                assert on.all() and (yi < 0).any() and ((xi >= W) if k == 0 else (xi < 0)).any() and not (yi >= H).any()
                assert 0.3 < ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).mean() < 0.95
            if case == "per_pixel":
                x, y = node_pixels((h, w), 0)
                d = np.hypot(X / Q - x[:h, :w], Y / Q - y[:h, :w])
                assert shift == 0 and d.max() > 2 and (np.abs(np.diff(X, axis=1) / Q - 1) < 1).all()
            if case == "negative":
                # floor and truncation differ exactly where the weighted sum is negative and leaves a remainder
                ws, four = _weights(g, shift, (h, w))
                low = (1 << 2 * shift) - 1
                tx, ty = (sum(wt * node[..., a] for wt, node in zip(ws, four)) for a in (0, 1))
                differ = ((tx < 0) & (tx & low != 0)) | ((ty < 0) & (ty & low != 0))
                assert differ.mean() > 0.5 and ((xi >= 0) & (yi >= 0) & (xi < W) & (yi < H)).mean() > 0.05    # ... also on pixels that show the image
            if case.startswith("marked"):
                assert 0.02 < (~on).mean() < 0.98 and w % 32 != 0 and (w - 1) % (1 << shift) == 0     # both kinds; a ragged last cell
                assert case == "marked5" or (on[:8, :32].any() and not on[:8, :32].all())             # the first 32 x 8 tile holds both
            if case in ("large", "identity"):
                assert on.all()
            if case == "large":
                assert (w + 31) // 32 > 4 and (h + 7) // 8 > 4 and ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).mean() > 0.5


def _weights(g, shift, size):
    h, w = size
    c = 1 << shift
    i, j = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    gx, gy, ax, ay = i >> shift, j >> shift, i & (c - 1), j & (c - 1)
    return ((c - ax) * (c - ay), ax * (c - ay), (c - ax) * ay, ax * ay), (g[gy, gx], g[gy, gx + 1], g[gy + 1, gx], g[gy + 1, gx + 1])


@pytest.mark.parametrize("c", [3, 1, 4, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_warp_is_the_restatement_exactly(ops, expected, case, c):
    (H, W), (h, w), shift, gs = CASES[case]
    x, want, want_cov = expected(case, c)
    g = np.stack(gs)
    if case == "identity":
        assert (want == x).all() and (want_cov == 255).all()
    if case.startswith("marked"):
        assert (want_cov == 0).any() and (want_cov == 255).any()
    xd = torch.from_numpy(x).cuda()
    got, cov = ops.warp_grid_u8(xd, torch.from_numpy(g).cuda(), shift, (h, w), coverage=True)
    assert got.dtype == cov.dtype == torch.uint8 and tuple(got.shape) == (2, h, w, c) and tuple(cov.shape) == (2, h, w)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(cov.cpu().numpy(), want_cov)
    assert torch.equal(ops.warp_grid_u8(xd, g, shift, (h, w)), got)              # a host array for the grid, no coverage asked: the same pixels
    one = ops.warp_grid_u8(xd, gs[1], shift, (h, w))                             # one grid for the whole batch
    assert np.array_equal(one[1].cpu().numpy(), want[1])
    assert np.array_equal(one[0].cpu().numpy(), cref.warp_grid(x[:1], gs[1], shift, (h, w))[0])
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                            # the input is untouched
    if case.startswith("embedded"):                                              # ... and the affine kernel's result, bit for bit, on the device
        a, a_cov = ops.warp_affine_u8(xd, np.stack(BORDER), (h, w), coverage=True)
        assert torch.equal(a, got) and torch.equal(a_cov, cov)
        assert np.array_equal(want, rref.warp_affine(x, np.stack(BORDER), (h, w)))


def arch_mask(sec, size, centre, n=64):
    """uint8 [H, W]: the annular sector (radius, thickness, sweep in degrees) around straight up from `centre`, filled."""
    from textflux_amd import glyph
    R, T, sweep = sec
    ang = np.radians(np.linspace(-90 - sweep / 2, -90 + sweep / 2, n))
    outer = [(centre[0] + (R + T / 2) * math.cos(a), centre[1] + (R + T / 2) * math.sin(a)) for a in ang]
    inner = [(centre[0] + (R - T / 2) * math.cos(a), centre[1] + (R - T / 2) * math.sin(a)) for a in ang[::-1]]
    return glyph.fill_polygon(size[1], size[0], outer + inner)[:, :, 0]


# ---------------------------------------------------------------------------------------------- the curved paste
D, R = 8, 2
REGION = dict(pad=0.0, min_side=96)
PASTE_WH, PASTE_ARCH, PASTE_CENTRE = (220, 150), (150, 24, 60), (110, 190)


@pytest.mark.parametrize("c", [3, 1])
def test_a_constant_survives_forward_and_back(ops, c):
    """Every tap row sums to one, so a constant source comes back as that constant on every covered pixel; any deviation is an indexing
    or a rounding slip."""
    from textflux_amd import curve as cv
    from textflux_amd import rectify as rc
    rb = cv.select_ribbon(rc.mask_points(arch_mask(PASTE_ARCH, PASTE_WH, PASTE_CENTRE)), D, R, **REGION)
    fwd, back, shift = cv.grids(rb, (0, 0), (PASTE_WH[1], PASTE_WH[0]))
    for value in (0, 1, 137, 255):
        src = torch.full((2, PASTE_WH[1], PASTE_WH[0], c), value, dtype=torch.uint8, device="cuda")
        up = ops.warp_grid_u8(src, fwd, shift, (rb.rh, rb.rw))
        again, cov = ops.warp_grid_u8(up, back, shift, (PASTE_WH[1], PASTE_WH[0]), coverage=True)
        assert bool((up == value).all()) and bool((again[cov == 255] == value).all()) and 0 < int((cov == 255).sum()) < cov.numel()


def test_wrapper_refuses_what_it_cannot_serve(ops):
    img = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device="cuda")
    ident = cref.embed(IDENT6, 1, (4, 4))
    big = ident.copy()
    big[1, 1, 1] = 1 << 50
    for bad in ((img.float(), ident, 1, (4, 4)), (img[0], ident, 1, (4, 4)), (img[..., :0], ident, 1, (4, 4)), (img, ident, 1, (0, 4)),
                (img, ident.astype(np.int32), 1, (4, 4)), (img, np.stack([ident] * 3), 1, (4, 4)), (img, ident[:2], 1, (4, 4)),
                (img, ident[:, :2], 1, (4, 4)), (img, ident[..., 0], 1, (4, 4)), (img, ident, 2, (4, 4)), (img, ident, 6, (4, 4)), (img, ident, -1, (4, 4)),
                (img.repeat(1, 1, 1, 2)[..., :5].contiguous(), ident, 1, (4, 4)), (img.permute(0, 2, 1, 3), ident, 1, (4, 4)),
                (img, big, 1, (4, 4)), (img, -big, 1, (4, 4)), (img, torch.from_numpy(ident).int().cuda(), 1, (4, 4))):
        with pytest.raises(ValueError):
            ops.warp_grid_u8(*bad)
    out, cov = ops.warp_grid_u8(img + 7, ident, 1, (4, 4), coverage=True)        # what it does serve
    assert bool((out == 7).all()) and bool((cov == 255).all())


@pytest.mark.parametrize("color", [None, dict(ring=40, min_pixels=16)])
def test_paste_of_a_curved_line_is_the_restatement(ops, color):
    """paste_back.paste(rect=Ribbon) on a window cut at the image (the crop's footprint sticks out of it): resample to the crop's size, warp,
    blend -- and with color_match a ring wider than the crop's margin, so that cutting it to the coverage matters."""
    from textflux_amd import curve as cv
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    rng = np.random.default_rng(5)
    arch = arch_mask(PASTE_ARCH, PASTE_WH, PASTE_CENTRE)
    rb = cv.select_ribbon(rc.mask_points(arch), D, R, **REGION)
    assert rb is not None and cv.is_curved(rb.line)
    x0, y0, x1, y1 = cv.ribbon_window(rb, PASTE_WH)
    foot = cv.footprint(rb)
    assert foot[:, 1].min() < 0 and y0 == 0 and (foot[:, 0].min() < 0 or foot[:, 0].max() > PASTE_WH[0] - 1)    # cut at the image
    back = cv.backward_grid(rb, (x0, y0), (y1 - y0, x1 - x0))
    orig = rng.integers(40, 216, (1, y1 - y0, x1 - x0, 3), dtype=np.uint8)
    edit = rng.integers(0, 256, (1, rb.rh - 9, rb.rw + 14, 3), dtype=np.uint8)                      # another size: resampled to (rh, rw) first
    grey = arch[None, y0:y1, x0:x1]
    cm = None if color is None else pb.color_match_cfg(color)
    want = cref.paste_ribbon(orig, edit, grey, D, R, back, rb.shift, rb.rw, rb.rh, color_match=cm)
    od, ed, gd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (orig, edit, grey))
    got = pb.paste(od, ed, gd, D, R, rect=rb, origin=(x0, y0), **({} if color is None else dict(color_match=color))).cpu().numpy()
    assert np.array_equal(got, want)
    outside = ref.dilate(grey, D + 3 * R) == 0
    assert outside.any() and (got[outside] == orig[outside]).all() and (got[~outside] != orig[~outside]).any()
    alpha = ref.alpha_mask(grey, D, R)
    _, cov = cref.warp_grid(ref.resize(edit, (rb.rh, rb.rw)), back, rb.shift, orig.shape[1:3], coverage=True)
    assert (cov[alpha > 0] == 255).all()                                         # alpha's support lies inside the coverage
    if color is not None:
        from tests.helpers import per_line_ref as plref
        ring = plref.ring_mask(alpha, cm["ring"])
        assert (ring & ~cov).any() and (ring & cov).sum() // 255 >= cm["min_pixels"]                # the ring does leave the coverage


# ---------------------------------------------------------------------------------------------- end to end, through run_items
SCENE_WH, FLAT_BOX, ARCH, ARCH_CENTRE = (320, 256), (40, 30, 160, 54), (150, 24, 50), (215, 290)


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_curve"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def test_end_to_end_one_level_line_one_arch(pipe):
    from textflux_amd import batch_driver
    from textflux_amd import curve as cv
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    sc = np.random.default_rng(0).integers(0, 256, (SCENE_WH[1], SCENE_WH[0], 3), dtype=np.uint8)
    flat = np.zeros((SCENE_WH[1], SCENE_WH[0]), np.uint8)
    flat[FLAT_BOX[1]:FLAT_BOX[3], FLAT_BOX[0]:FLAT_BOX[2]] = 255
    arch = arch_mask(ARCH, SCENE_WH, ARCH_CENTRE)
    item = dict(image=Image.fromarray(sc), mask=Image.fromarray(flat | arch).convert("RGB"), text="LEVEL\nARCH")
    rb = cv.select_ribbon(rc.mask_points(arch), D, R, **REGION)
    assert rb is not None and cv.is_curved(rb.line)
    x0, y0, x1, y1 = cv.ribbon_window(rb, SCENE_WH)
    grown_flat, grown_arch = ref.dilate(flat, D + 3 * R) > 0, ref.dilate(arch, D + 3 * R) > 0
    assert not (grown_flat & grown_arch).any()
    outs, recs = {}, {}
    for name, extra in (("plain", {}), ("ribbon", dict(curve=True)), ("matched", dict(curve=True, color_match=True))):
        saved, pastes = {}, []
        real = pipe.paste_back

        def spy(o_, e, m, **k):
            out = real(o_, e, m, **k)
            pastes.append(dict(original=np.array(o_), edited=np.array(e), mask=np.array(m), out=out.cpu().numpy(), kw=k))
            return out
        pipe.paste_back = spy
        try:
            res = batch_driver.run_items([item], pipe, None, batch_size=2, num_inference_steps=2, guidance_scale=30.0, seed=42,
                                         loader=lambda x: x, save=lambda i, im: saved.__setitem__(i, np.array(im)),
                                         paste_back=dict(per_line=True, dilate=D, feather=R, region=REGION, **extra))
        finally:
            del pipe.paste_back
        assert res["all_done"] == [0] and not res["failed"] and len(pastes) == 2
        outs[name], recs[name] = saved[0], pastes
        assert saved[0].shape == sc.shape
        assert (saved[0][~(grown_flat | grown_arch)] == sc[~(grown_flat | grown_arch)]).all()        # outside the grown masks: the original
        assert (saved[0][flat >= 128] != sc[flat >= 128]).any() and (saved[0][arch >= 128] != sc[arch >= 128]).any()
    # the level line: rect never reached its paste, and its pasted bytes are those of the run without the key
    for name in outs:
        assert "rect" not in recs[name][0]["kw"] and ("rect" in recs[name][1]["kw"]) == (name != "plain")
    assert np.array_equal(recs["plain"][0]["edited"], recs["ribbon"][0]["edited"])
    assert (outs["ribbon"][grown_flat] == outs["plain"][grown_flat]).all()
    assert (outs["ribbon"][grown_arch] != outs["plain"][grown_arch]).any()       # the arch was edited another way
    # the arch: the scene window is the restated paste of the pipeline's own cropped output
    p = recs["ribbon"][1]
    assert p["kw"]["rect"] == rb and tuple(p["kw"]["origin"]) == (x0, y0) and p["edited"].shape[:2] != (rb.rh, rb.rw)
    assert np.array_equal(p["mask"], arch[y0:y1, x0:x1])
    back = cv.backward_grid(rb, (x0, y0), (y1 - y0, x1 - x0))
    want = cref.paste_ribbon(p["original"][None], p["edited"][None], p["mask"][None], D, R, back, rb.shift, rb.rw, rb.rh)
    assert np.array_equal(p["out"], want) and np.array_equal(outs["ribbon"][y0:y1, x0:x1], want[0])
    # colour matching: the same alpha, so it differs from the unmatched result only where alpha > 0 -- and the restatement agrees
    alpha = np.maximum(ref.alpha_mask(flat, D, R), ref.alpha_mask(arch, D, R))
    differs = (outs["matched"] != outs["ribbon"]).any(axis=2)
    assert not differs[alpha == 0].any()
    q = recs["matched"][1]
    assert np.array_equal(q["kw"]["color_ref"], sc[y0:y1, x0:x1]) and np.array_equal(q["edited"], p["edited"])
    want = cref.paste_ribbon(q["original"][None], q["edited"][None], q["mask"][None], D, R, back, rb.shift, rb.rw, rb.rh,
                             color_match=pb.color_match_cfg(True), color_ref=sc[None, y0:y1, x0:x1])
    assert np.array_equal(q["out"], want)
