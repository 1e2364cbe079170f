"""Perspective per-line edits on the GPU: the homography warp kernel (imageops.hip: warp_perspective_u8) and paste_back.paste(rect=Quad)
against the numpy restatement in tests/helpers/perspective_ref.py, bit for bit (integer arithmetic only), and
batch_driver.run_items(perspective=True) end to end on the tiny synthetic checkpoint of the e2e tests."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import paste_back_ref as ref
from tests.helpers import perspective_ref as pref
from tests.helpers import rectify_ref as rref

pytestmark = pytest.mark.gpu
Q = 1 << 16
ONE = 1 << 30
IDENT = np.array([ONE, 0, 0, 0, ONE, 0, 0, 0, ONE], np.int64)


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


def homography(dst_size, src_quad):
    """int64 [9]: the destination's corner pixels (h, w = dst_size; TL, TR, BR, BL) read the source at src_quad; D = 2^30 (up to the
    rounding) at the destination's centre."""
    h, w = dst_size
    A, b = [], []
    for (x, y), (u, v) in zip(((0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)), src_quad):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        b += [u, v]
    m = np.append(np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64)), 1.0)
    m *= ONE / (m[6] * (w // 2) + m[7] * (h // 2) + m[8])
    return np.round(m).astype(np.int64)


def horizon(a, b, c):
    """A matrix whose D = u (a i + b j + c), u = 2^30 // c, crosses zero inside the destination, over a mild projective numerator."""
    m = homography((9, 33), ((2.0, 3.0), (50.0, 1.0), (48.0, 30.0), (4.0, 33.0)))
    u = ONE // c
    m[6], m[7], m[8] = a * u, b * u, c * u
    return m


# (source H, W), (destination h, w), the two samples' matrices
CASES = {
    # the embedded affine matrices of test_rectify_gpu's "border" case
    "embedded": ((37, 53), (29, 41), tuple(pref.embed(a) for a in (rotation(17, (37.3, 18.2), (14, 20)), rotation(-17, (10.0, 2.5), (27, 20), 1.3)))),
    # a 1.5:1 taper (the source quad's left side is 1.5 times its right side) that leaves the source on the left and at the top
    "mild": ((37, 53), (29, 41), (homography((29, 41), ((-24.0, -8.0), (40.0, 4.5), (40.0, 28.5), (-24.0, 28.0))),
                                  homography((29, 41), ((8.0, 7.0), (60.0, -5.0), (60.0, 31.0), (8.0, 31.0))))),
    # the source positions are negative, with fractions, on most pixels: where truncating division differs from floor
    "negative": ((23, 31), (19, 27), (homography((19, 27), ((-20.3, -11.7), (12.2, -9.1), (14.9, 9.3), (-18.6, 14.2))),
                                      homography((19, 27), ((-3.3, -30.7), (33.2, -21.1), (30.9, 11.3), (-6.6, 6.2))))),
    # D crosses zero inside the destination (at i = 20.5, and along 4 i = 45 + 3 j, which pixel (12, 1) hits exactly); a second tile row
    # of one line, a width that is no multiple of 32
    "horizon": ((37, 53), (9, 33), (horizon(-4, 0, 82), horizon(-4, 3, 45))),
    "large": ((300, 500), (128, 512), (homography((128, 512), ((20.5, 40.25), (480.0, 90.0), (470.0, 200.0), (10.0, 280.0))),
                                       homography((128, 512), ((60.0, 150.0), (430.0, 10.0), (520.0, 170.0), (140.0, 310.0))))),
    "identity": ((37, 53), (37, 53), (IDENT, IDENT)),
}


@pytest.fixture(scope="module")
def expected():
    """The restatement's answer per (case, channels), computed once."""
    cache = {}

    def get(case, c):
        if (case, c) not in cache:
            (H, W), (h, w), ms = CASES[case]
            x = np.random.default_rng(H * W + c).integers(0, 256, (2, H, W, c), dtype=np.uint8)     # the two samples differ: a batch-stride slip shows
            cache[case, c] = (x,) + pref.warp_perspective(x, np.stack(ms), (h, w), coverage=True)
        return cache[case, c]
    return get


def test_the_cases_exercise_what_they_claim():
    for case, ((H, W), (h, w), ms) in CASES.items():
        for k, m in enumerate(ms):
            i, j = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
            Nx, Ny, D = (m[a] * i + m[a + 1] * j + m[a + 2] for a in (0, 3, 6))
            assert max(np.abs(Nx).max(), np.abs(Ny).max(), np.abs(D).max()) < 1 << 54, case
            _, PX, PY = pref.positions(m, (h, w))
            uncovered = ~((D > 0) & ((PX >> 8) >= 0) & ((PX >> 8) < W) & ((PY >> 8) >= 0) & ((PY >> 8) < H))
            if case == "mild" and k == 0:
                left, right = (Ny[-1, 0] / D[-1, 0] - Ny[0, 0] / D[0, 0]), (Ny[-1, -1] / D[-1, -1] - Ny[0, -1] / D[0, -1])
                assert abs(left / right - 1.5) < 0.01 and 0.28 < uncovered.mean() < 0.4
            if case == "negative":
                # floor and truncation differ exactly where the numerator is negative and the remainder is not zero
                differ = ((Nx < 0) & ((Nx * 256) % D != 0)) | ((Ny < 0) & ((Ny * 256) % D != 0))
                assert (D > 0).all() and differ.mean() > 0.5
                trunc = np.where(Nx < 0, -((-Nx * 256) // D), (Nx * 256) // D)
                assert (trunc != PX).mean() > 0.1 and (~uncovered).mean() > 0.1                      # ... also on pixels that show the image
            if case == "horizon":
                assert 0.2 < (D <= 0).mean() < 0.8 and (D > 0).any() and (D == 0).any() == (k == 1)  # both signs; sample 1 also hits D = 0 exactly
            if case in ("large", "identity"):
                assert (D > 0).all()


@pytest.mark.parametrize("c", [3, 1, 4, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_warp_is_the_restatement_exactly(ops, expected, case, c):
    (H, W), (h, w), ms = CASES[case]
    x, want, want_cov = expected(case, c)
    m = np.stack(ms)
    if case == "identity":
        assert (want == x).all() and (want_cov == 255).all()
    if case == "horizon":
        assert (want_cov == 0).any() and (want_cov == 255).any()
    xd = torch.from_numpy(x).cuda()
    got, cov = ops.warp_perspective_u8(xd, torch.from_numpy(m).cuda(), (h, w), coverage=True)
    assert got.dtype == cov.dtype == torch.uint8 and tuple(got.shape) == (2, h, w, c) and tuple(cov.shape) == (2, h, w)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(cov.cpu().numpy(), want_cov)
    assert torch.equal(ops.warp_perspective_u8(xd, m, (h, w)), got)              # a host array for m, no coverage asked: the same pixels
    one = ops.warp_perspective_u8(xd, ms[1], (h, w))                             # one matrix for the whole batch
    assert np.array_equal(one[1].cpu().numpy(), want[1])
    assert np.array_equal(one[0].cpu().numpy(), pref.warp_perspective(x[:1], ms[1], (h, w))[0])
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                            # the input is untouched
    if case == "embedded":                                                       # ... and the affine kernel's result, bit for bit, on the device
        a, a_cov = ops.warp_affine_u8(xd, m[:, :6].copy(), (h, w), coverage=True)
        assert torch.equal(a, got) and torch.equal(a_cov, cov)
        assert np.array_equal(want, rref.warp_affine(x, m[:, :6], (h, w)))


def trapezoid_mask(quad, size):
    from textflux_amd import glyph
    return glyph.fill_polygon(size[1], size[0], quad)[:, :, 0]


@pytest.mark.parametrize("c", [3, 1])
def test_a_constant_survives_forward_and_back(ops, c):
    """Every tap row sums to one, so a constant source comes back as that constant on every pixel in front of the horizon; any deviation
    is an indexing or a rounding slip."""
    from textflux_amd import perspective as ps
    from textflux_amd import rectify as rc
    quad = ps.select_quad(rc.mask_points(trapezoid_mask(PASTE_QUAD, PASTE_WH)), D, R, **REGION)
    fwd, back = ps.matrices(quad)
    for value in (0, 1, 137, 255):
        src = torch.full((2, PASTE_WH[1], PASTE_WH[0], c), value, dtype=torch.uint8, device="cuda")
        up = ops.warp_perspective_u8(src, fwd, (quad.rh, quad.rw))
        again, cov = ops.warp_perspective_u8(up, back, (PASTE_WH[1], PASTE_WH[0]), coverage=True)
        assert bool((up == value).all()) and bool((again == value).all()) and 0 < int((cov == 255).sum()) < cov.numel()


def test_wrapper_refuses_what_it_cannot_serve(ops):
    img = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device="cuda")
    for bad in ((img.float(), IDENT, (4, 4)), (img[0], IDENT, (4, 4)), (img[..., :0], IDENT, (4, 4)), (img, IDENT, (0, 4)),
                (img, IDENT.astype(np.int32), (4, 4)), (img, np.stack([IDENT] * 3), (4, 4)), (img, IDENT[:8], (4, 4)), (img, IDENT[:6], (4, 4)),
                (img.repeat(1, 1, 1, 2)[..., :5].contiguous(), IDENT, (4, 4)), (img.permute(0, 2, 1, 3), IDENT, (4, 4)),
                (img, np.where(np.arange(9) == 8, 1 << 54, IDENT), (4, 4))):
        with pytest.raises(ValueError):
            ops.warp_perspective_u8(*bad)


# ---------------------------------------------------------------------------------------------- the perspective paste
D, R = 8, 2
REGION = dict(pad=0.0, min_side=96)
PASTE_WH, PASTE_QUAD = (220, 150), [(40, 50), (190, 30), (190, 110), (40, 90)]   # 2:1, the near side at the image's right edge


@pytest.mark.parametrize("color", [None, dict(ring=40, min_pixels=16)])
def test_paste_of_a_perspective_line_is_the_restatement(ops, color):
    """paste_back.paste(rect=Quad) on a window cut at the image (the crop's footprint sticks out of it): resample to the crop's size, warp,
    blend -- and with color_match a ring wider than the crop's margin, so that cutting it to the coverage matters."""
    from textflux_amd import paste_back as pb
    from textflux_amd import perspective as ps
    from textflux_amd import rectify as rc
    rng = np.random.default_rng(5)
    trap = trapezoid_mask(PASTE_QUAD, PASTE_WH)
    quad = ps.select_quad(rc.mask_points(trap), D, R, **REGION)
    x0, y0, x1, y1 = ps.quad_window(quad, PASTE_WH)
    foot = ps.footprint(quad)
    assert foot[:, 0].max() > PASTE_WH[0] and (x1, y0) == (PASTE_WH[0], 0) and foot[:, 1].min() < 0            # cut at the image
    back = ps.matrices(quad, (x0, y0))[1]
    orig = rng.integers(40, 216, (1, y1 - y0, x1 - x0, 3), dtype=np.uint8)
    edit = rng.integers(0, 256, (1, quad.rh - 9, quad.rw + 14, 3), dtype=np.uint8)                  # another size: resampled to (rh, rw) first
    grey = trap[None, y0:y1, x0:x1]
    cm = None if color is None else pb.color_match_cfg(color)
    want = pref.paste_quad(orig, edit, grey, D, R, back, quad.rw, quad.rh, color_match=cm)
    od, ed, gd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (orig, edit, grey))
    got = pb.paste(od, ed, gd, D, R, rect=quad, origin=(x0, y0), **({} if color is None else dict(color_match=color))).cpu().numpy()
    assert np.array_equal(got, want)
    outside = ref.dilate(grey, D + 3 * R) == 0
    assert outside.any() and (got[outside] == orig[outside]).all() and (got[~outside] != orig[~outside]).any()
    alpha = ref.alpha_mask(grey, D, R)
    _, cov = pref.warp_perspective(ref.resize(edit, (quad.rh, quad.rw)), back, orig.shape[1:3], coverage=True)
    assert (cov[alpha > 0] == 255).all()                                         # alpha's support lies inside the coverage
    if color is not None:
        from tests.helpers import per_line_ref as plref
        ring = plref.ring_mask(alpha, cm["ring"])
        assert (ring & ~cov).any() and (ring & cov).sum() // 255 >= cm["min_pixels"]                # the ring does leave the coverage


# ---------------------------------------------------------------------------------------------- end to end, through run_items
SCENE_WH, FLAT_BOX, TRAP = (320, 256), (40, 30, 160, 54), [(170, 120), (300, 135), (300, 185), (170, 215)]


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_perspective"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def test_end_to_end_one_level_line_one_trapezoid(pipe):
    from textflux_amd import batch_driver
    from textflux_amd import paste_back as pb
    from textflux_amd import perspective as ps
    from textflux_amd import rectify as rc
    sc = np.random.default_rng(0).integers(0, 256, (SCENE_WH[1], SCENE_WH[0], 3), dtype=np.uint8)
    flat = np.zeros((SCENE_WH[1], SCENE_WH[0]), np.uint8)
    flat[FLAT_BOX[1]:FLAT_BOX[3], FLAT_BOX[0]:FLAT_BOX[2]] = 255
    trap = trapezoid_mask(TRAP, SCENE_WH)
    item = dict(image=Image.fromarray(sc), mask=Image.fromarray(flat | trap).convert("RGB"), text="LEVEL\nTRAPEZOID")
    quad = ps.select_quad(rc.mask_points(trap), D, R, **REGION)
    assert quad is not None and ps.is_perspective(np.array(quad.corners))
    x0, y0, x1, y1 = ps.quad_window(quad, SCENE_WH)
    grown_flat, grown_trap = ref.dilate(flat, D + 3 * R) > 0, ref.dilate(trap, D + 3 * R) > 0
    assert not (grown_flat & grown_trap).any()
    outs, recs = {}, {}
    for name, extra in (("plain", {}), ("quad", dict(perspective=True)), ("matched", dict(perspective=True, color_match=True))):
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
        assert (saved[0][~(grown_flat | grown_trap)] == sc[~(grown_flat | grown_trap)]).all()        # outside the grown masks: the original
        assert (saved[0][flat >= 128] != sc[flat >= 128]).any() and (saved[0][trap >= 128] != sc[trap >= 128]).any()
    # the level line: rect never reached its paste, and its pasted bytes are those of the run without the key
    for name in outs:
        assert "rect" not in recs[name][0]["kw"] and ("rect" in recs[name][1]["kw"]) == (name != "plain")
    assert np.array_equal(recs["plain"][0]["edited"], recs["quad"][0]["edited"])
    assert (outs["quad"][grown_flat] == outs["plain"][grown_flat]).all()
    assert (outs["quad"][grown_trap] != outs["plain"][grown_trap]).any()         # the trapezoid was edited another way
    # the trapezoid: the scene window is the restated paste of the pipeline's own cropped output
    p = recs["quad"][1]
    assert p["kw"]["rect"] == quad and tuple(p["kw"]["origin"]) == (x0, y0) and p["edited"].shape[:2] != (quad.rh, quad.rw)
    assert np.array_equal(p["mask"], trap[y0:y1, x0:x1])
    back = ps.matrices(quad, (x0, y0))[1]
    want = pref.paste_quad(p["original"][None], p["edited"][None], p["mask"][None], D, R, back, quad.rw, quad.rh)
    assert np.array_equal(p["out"], want) and np.array_equal(outs["quad"][y0:y1, x0:x1], want[0])
    # colour matching: the same alpha, so it differs from the unmatched result only where alpha > 0 -- and the restatement agrees
    alpha = np.maximum(ref.alpha_mask(flat, D, R), ref.alpha_mask(trap, D, R))
    differs = (outs["matched"] != outs["quad"]).any(axis=2)
    assert not differs[alpha == 0].any()
    q = recs["matched"][1]
    assert np.array_equal(q["kw"]["color_ref"], sc[y0:y1, x0:x1]) and np.array_equal(q["edited"], p["edited"])
    want = pref.paste_quad(q["original"][None], q["edited"][None], q["mask"][None], D, R, back, quad.rw, quad.rh,
                           color_match=pb.color_match_cfg(True), color_ref=sc[None, y0:y1, x0:x1])
    assert np.array_equal(q["out"], want)
