"""Rectified per-line edits on the GPU: the affine warp kernel (imageops.hip: warp_affine_u8) and paste_back.paste(rect=...) against the
numpy restatement in tests/helpers/rectify_ref.py, bit for bit (integer arithmetic only), and batch_driver.run_items(rectify=True) end
to end on the tiny synthetic checkpoint of the e2e tests."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from tests.helpers import paste_back_ref as ref
from tests.helpers import rectify_ref as rref

pytestmark = pytest.mark.gpu
Q = 1 << 16


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def rotation(deg, src_centre, dst_centre, scale=1.0):
    """Q16 matrix: destination pixel p reads the source at src_centre + scale R(deg) (p - dst_centre)."""
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    m = [round(c * Q), round(-s * Q), 0, round(s * Q), round(c * Q), 0]
    m[2] = round(src_centre[0] * Q) - m[0] * dst_centre[0] - m[1] * dst_centre[1]
    m[5] = round(src_centre[1] * Q) - m[3] * dst_centre[0] - m[4] * dst_centre[1]
    return np.array(m, np.int64)


# (source H, W), (destination h, w), the two samples' matrices.  37 x 53 -> 29 x 41 at 17 degrees, shifted so that a third of the
# destination reads outside the source (border replication, coverage 0); a 7 x 130 destination (rows shorter than the 8-row tile, a
# width that is no multiple of 32 or 64, five tiles across); 300 x 500 -> 128 x 512 at -33 degrees (64 x 16 tiles); the identity; an
# exact quarter turn.
CASES = {
    "border": ((37, 53), (29, 41), (rotation(17, (37.3, 18.2), (14, 20)), rotation(-17, (10.0, 2.5), (27, 20), 1.3))),
    "thin": ((37, 53), (7, 130), (rotation(5, (26, 18), (65, 3), 0.4), rotation(-80, (26, 18), (65, 3), 0.3))),
    "large": ((300, 500), (128, 512), (rotation(-33, (250.5, 149.25), (256, 64)), rotation(33, (249, 150), (255.5, 63.5), 0.9))),
    "identity": ((37, 53), (37, 53), (np.array([Q, 0, 0, 0, Q, 0], np.int64),) * 2),
    "quarter": ((37, 53), (53, 37), (np.array([0, -Q, 52 * Q, Q, 0, 0], np.int64), np.array([0, Q, 0, -Q, 0, 36 * Q], np.int64))),
}


@pytest.mark.parametrize("c", [3, 1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_warp_is_the_restatement_exactly(ops, case, c):
    (H, W), (h, w), ms = CASES[case]
    x = np.random.default_rng(H * W + c).integers(0, 256, (2, H, W, c), dtype=np.uint8)     # the two samples differ: a batch-stride slip shows
    m = np.stack(ms)
    want, want_cov = rref.warp_affine(x, m, (h, w), coverage=True)
    if case == "border":
        assert 0.3 < (want_cov[0] == 0).mean() < 0.37 and (want_cov[1] == 0).any()
    if case == "identity":
        assert (want == x).all() and (want_cov == 255).all()
    if case == "quarter":
        assert (want[0] == np.rot90(x[0])).all() and (want[1] == np.rot90(x[1], -1)).all() and (want_cov == 255).all()
    xd = torch.from_numpy(x).cuda()
    got, cov = ops.warp_affine_u8(xd, torch.from_numpy(m).cuda(), (h, w), coverage=True)
    assert got.dtype == cov.dtype == torch.uint8 and tuple(got.shape) == (2, h, w, c) and tuple(cov.shape) == (2, h, w)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(cov.cpu().numpy(), want_cov)
    assert torch.equal(ops.warp_affine_u8(xd, m, (h, w)), got)                   # a host array for m, no coverage asked: the same pixels
    one = ops.warp_affine_u8(xd, ms[1], (h, w))                                  # one matrix for the whole batch
    assert np.array_equal(one[1].cpu().numpy(), want[1]) and np.array_equal(one[0].cpu().numpy(), rref.warp_affine(x[:1], ms[1], (h, w))[0])
    assert torch.equal(xd.cpu(), torch.from_numpy(x))


def affine_three_ways(ms, out_size):
    """{entry point: its arguments between the image and out_size} for one batch of Q16 affine matrices said three ways: as they are, as
    homographies (m6 = m7 = 0, m8 = 2^16) and as control grids whose node (r, q) is the affine image of (q << shift, r << shift), at
    shift 0 and 3.  All of them name the same position for every destination pixel, exactly: the blend of an affine map's nodes is the map."""
    from tests.helpers import curve_ref as cref
    from tests.helpers import perspective_ref as pref
    m = np.stack(ms)
    ways = {"warp_affine": (m,), "warp_perspective": (pref.embed(m),)}
    for shift in (0, 3):
        ways[f"warp_grid, shift {shift}"] = (np.stack([cref.embed(a, shift, out_size) for a in ms]), shift)
    return ways


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("case", ["border", "thin"])
def test_one_affine_map_through_all_three_entry_points(ops, case, c):
    """The three maps share one kernel body: a map wired to the wrong entry point, or a lost zero / uncovered tail, shows here."""
    (H, W), (h, w), ms = CASES[case]
    x = np.random.default_rng(H * W + c).integers(0, 256, (2, H, W, c), dtype=np.uint8)
    want, want_cov = rref.warp_affine(x, np.stack(ms), (h, w), coverage=True)
    if case == "border":
        assert (want_cov == 0).mean() > 0.3 and (want_cov == 255).any()          # coverage is exercised
    xd = torch.from_numpy(x).cuda()
    for way, args in affine_three_ways(ms, (h, w)).items():
        got, cov = getattr(ops, way.split(",")[0] + "_u8")(xd, *args, (h, w), coverage=True)
        assert np.array_equal(got.cpu().numpy(), want), way
        assert np.array_equal(cov.cpu().numpy(), want_cov), way


@pytest.mark.parametrize("c", [3, 1])
def test_a_constant_survives_forward_and_back(ops, c):
    """Every tap row sums to one, so a constant source comes back as that constant on every covered pixel -- and, by edge replication,
    on the others too; any deviation is an indexing or a rounding slip."""
    from textflux_amd import rectify as rc
    for value in (0, 1, 137, 255):
        src = torch.full((2, 61, 83, c), value, dtype=torch.uint8, device="cuda")
        rect = rc.Rect(41.0, 30.0, 70, 31, 25.0, 70, 31)
        fwd, back = rc.matrices(rect)
        up = ops.warp_affine_u8(src, fwd, (rect.rh, rect.rw))
        again, cov = ops.warp_affine_u8(up, back, (61, 83), coverage=True)
        assert bool((up == value).all()) and bool((again == value).all()) and 0 < int((cov == 255).sum()) < cov.numel()


def test_wrapper_refuses_what_it_cannot_serve(ops):
    img = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device="cuda")
    ident = np.array([Q, 0, 0, 0, Q, 0], np.int64)
    for bad in ((img.float(), ident, (4, 4)), (img[0], ident, (4, 4)), (img[..., :0], ident, (4, 4)), (img, ident, (0, 4)),
                (img, ident.astype(np.int32), (4, 4)), (img, np.stack([ident] * 3), (4, 4)), (img, ident[:5], (4, 4)),
                (img.repeat(1, 1, 1, 2)[..., :5].contiguous(), ident, (4, 4)), (img.permute(0, 2, 1, 3), ident, (4, 4))):
        with pytest.raises(ValueError):
            ops.warp_affine_u8(*bad)


# ---------------------------------------------------------------------------------------------- the rectified paste
def drawn(length, thickness, deg, centre, size):
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    pts = [np.array(centre) + su * u * length / 2 + sv * v * thickness / 2 for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    im = Image.new("L", size, 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in pts], fill=255)
    return np.array(im)


SCENE_WH, FLAT_BOX, SLANT = (320, 256), (40, 30, 160, 54), (140, 20, 25, (200, 170))
D, R = 8, 2
REGION = dict(pad=0.0, min_side=96)


@pytest.mark.parametrize("color", [None, dict(ring=40, min_pixels=16)])
def test_paste_of_a_rectified_line_is_the_restatement(ops, color):
    """paste_back.paste(rect=...) on a window at the image's corner (the rectangle sticks out of it): resample to the rectangle's size,
    warp, blend -- and with color_match a ring wider than the rectangle's margin, so that cutting it to the coverage matters."""
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    rng = np.random.default_rng(5)
    slant = drawn(140, 20, 25, (80, 60), (240, 160))
    rect = rc.select_rect(rc.mask_points(slant), D, R, **REGION)
    x0, y0, x1, y1 = rc.rect_window(rect, (240, 160))
    assert (x0, y0) == (0, 0) and min(rc.rect_corners(rect).min(axis=0)) < 0     # cut at the image
    back = rc.matrices(rect, (x0, y0))[1]
    orig = rng.integers(40, 216, (1, y1 - y0, x1 - x0, 3), dtype=np.uint8)
    edit = rng.integers(0, 256, (1, rect.rh - 9, rect.rw + 14, 3), dtype=np.uint8)                  # another size: resampled to (rh, rw) first
    grey = slant[None, y0:y1, x0:x1]
    cm = None if color is None else pb.color_match_cfg(color)
    want = rref.paste_rect(orig, edit, grey, D, R, back, rect.rw, rect.rh, color_match=cm)
    od, ed, gd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (orig, edit, grey))
    got = pb.paste(od, ed, gd, D, R, rect=rect, origin=(x0, y0), **({} if color is None else dict(color_match=color))).cpu().numpy()
    assert np.array_equal(got, want)
    outside = ref.dilate(grey, D + 3 * R) == 0
    assert outside.any() and (got[outside] == orig[outside]).all() and (got[~outside] != orig[~outside]).any()
    if color is not None:
        from tests.helpers import per_line_ref as plref
        alpha = ref.alpha_mask(grey, D, R)
        _, cov = rref.warp_affine(ref.resize(edit, (rect.rh, rect.rw)), back, orig.shape[1:3], coverage=True)
        ring = plref.ring_mask(alpha, cm["ring"])
        assert (ring & ~cov).any() and (ring & cov).sum() // 255 >= cm["min_pixels"]                # the ring does leave the coverage
        assert (cov[alpha > 0] == 255).all()                                     # ... while alpha's support never does


# ---------------------------------------------------------------------------------------------- end to end, through run_items
@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_rectify"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def test_end_to_end_one_level_line_one_slanted(pipe):
    from textflux_amd import batch_driver
    from textflux_amd import paste_back as pb
    from textflux_amd import rectify as rc
    sc = np.random.default_rng(0).integers(0, 256, (SCENE_WH[1], SCENE_WH[0], 3), dtype=np.uint8)
    flat = np.zeros((SCENE_WH[1], SCENE_WH[0]), np.uint8)
    flat[FLAT_BOX[1]:FLAT_BOX[3], FLAT_BOX[0]:FLAT_BOX[2]] = 255
    slant = drawn(SLANT[0], SLANT[1], SLANT[2], SLANT[3], SCENE_WH)
    item = dict(image=Image.fromarray(sc), mask=Image.fromarray(flat | slant).convert("RGB"), text="LEVEL\nSLANT")
    rect = rc.select_rect(rc.mask_points(slant), D, R, **REGION)
    x0, y0, x1, y1 = rc.rect_window(rect, SCENE_WH)
    grown_flat, grown_slant = ref.dilate(flat, D + 3 * R) > 0, ref.dilate(slant, D + 3 * R) > 0
    assert not (grown_flat & grown_slant).any()
    outs, recs = {}, {}
    for name, extra in (("plain", {}), ("rect", dict(rectify=True)), ("matched", dict(rectify=True, color_match=True))):
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
        assert (saved[0][~(grown_flat | grown_slant)] == sc[~(grown_flat | grown_slant)]).all()      # outside the grown masks: the original
        assert (saved[0][flat >= 128] != sc[flat >= 128]).any() and (saved[0][slant >= 128] != sc[slant >= 128]).any()
    # the level line: rect never reached its paste, and its pasted bytes are those of the run without the key
    for name in outs:
        assert "rect" not in recs[name][0]["kw"] and ("rect" in recs[name][1]["kw"]) == (name != "plain")
    assert np.array_equal(recs["plain"][0]["edited"], recs["rect"][0]["edited"])
    assert (outs["rect"][grown_flat] == outs["plain"][grown_flat]).all()
    assert (outs["rect"][grown_slant] != outs["plain"][grown_slant]).any()       # the slanted line was edited another way
    # the slanted line: the scene window is the restated paste of the pipeline's own cropped output
    p = recs["rect"][1]
    assert p["kw"]["rect"] == rect and tuple(p["kw"]["origin"]) == (x0, y0) and p["edited"].shape[:2] != (rect.rh, rect.rw)
    assert np.array_equal(p["mask"], slant[y0:y1, x0:x1])
    back = rc.matrices(rect, (x0, y0))[1]
    want = rref.paste_rect(p["original"][None], p["edited"][None], p["mask"][None], D, R, back, rect.rw, rect.rh)
    assert np.array_equal(p["out"], want) and np.array_equal(outs["rect"][y0:y1, x0:x1], want[0])
    # colour matching: the same alpha, so it differs from the unmatched result only where alpha > 0 -- and the restatement agrees
    alpha = np.maximum(ref.alpha_mask(flat, D, R), ref.alpha_mask(slant, D, R))
    differs = (outs["matched"] != outs["rect"]).any(axis=2)
    print(f"colour matching changed {int(differs.sum())} pixels, all of the {int((alpha > 0).sum())} with alpha > 0: {not differs[alpha == 0].any()}")
    assert not differs[alpha == 0].any()
    q = recs["matched"][1]
    assert np.array_equal(q["kw"]["color_ref"], sc[y0:y1, x0:x1]) and np.array_equal(q["edited"], p["edited"])
    want = rref.paste_rect(q["original"][None], q["edited"][None], q["mask"][None], D, R, back, rect.rw, rect.rh,
                           color_match=pb.color_match_cfg(True), color_ref=sc[None, y0:y1, x0:x1])
    assert np.array_equal(q["out"], want)
