"""Paste-back on the GPU: the three uint8 kernels (imageops.hip: mask_dilate_u8, mask_feather_u8, overlay_u8) and
textflux_amd/paste_back.py against the numpy restatement in tests/helpers/paste_back_ref.py, bit for bit (the arithmetic is exact in
integers), and the batch driver end to end on the tiny synthetic checkpoint of the e2e tests."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import paste_back_ref as ref

pytestmark = pytest.mark.gpu
H, W = 37, 53
RADII = (0, 1, 3, 40, 64)            # inside the image, across both borders (H = 37 < 2 * 40 + 1), beyond the image (64 > W)


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def _pairs(h, w):
    """B = 2 batches whose two samples DIFFER (a batch-stride slip shows): name -> uint8 [2, h, w]."""
    rng = np.random.default_rng(h * 1000 + w)
    z = lambda: np.zeros((h, w), np.uint8)
    corner, centre, far = z(), z(), z()
    corner[0, 0], centre[h // 2, w // 2], far[h - 1, w - 1] = 255, 255, 255
    rb = lambda p: (rng.random((h, w)) < p).astype(np.uint8) * 255
    return {"corner|centre": np.stack([corner, centre]), "full|empty": np.stack([np.full((h, w), 255, np.uint8), z()]),
            "far corner|random": np.stack([far, rb(0.02)]), "random|random": np.stack([rb(0.05), rb(0.3)]),
            "grey|grey": rng.integers(0, 256, (2, h, w), dtype=np.uint8)}


@pytest.fixture(scope="module")
def masks():
    return {(h, w): _pairs(h, w) for h, w in ((H, W), (1, W), (H, 1))}


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("hw", [(H, W), (1, W), (H, 1)])
def test_dilate_is_the_restatement_bit_for_bit(ops, masks, hw, r):
    for name, m in masks[hw].items():
        got = ops.mask_dilate(torch.from_numpy(m).cuda(), r).cpu()
        assert torch.equal(got, torch.from_numpy(ref.dilate(m, r))), (name, hw, r)
        if r == 0:
            assert torch.equal(got, torch.from_numpy(m))


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("hw", [(H, W), (1, W), (H, 1)])
def test_feather_is_the_restatement_bit_for_bit(ops, masks, hw, r):
    for name, m in masks[hw].items():
        x = torch.from_numpy(m).cuda()
        got = ops.mask_feather(x, r).cpu()
        assert torch.equal(got, torch.from_numpy(ref.feather(m, r))), (name, hw, r)
        assert torch.equal(x.cpu(), torch.from_numpy(m))                   # the input is left alone (out / tmp ping-pong)
        if r == 0:
            assert torch.equal(got, torch.from_numpy(m))
    full = torch.full((2,) + hw, 255, dtype=torch.uint8, device="cuda")
    assert bool((ops.mask_feather(full, r) == 255).all()) and not bool(ops.mask_feather(torch.zeros_like(full), r).any())


def test_window_radius_255_and_a_one_pixel_image(ops):
    m = _pairs(H, W)["grey|grey"]
    assert torch.equal(ops.mask_dilate(torch.from_numpy(m).cuda(), 255).cpu(), torch.from_numpy(ref.dilate(m, 255)))
    assert torch.equal(ops.mask_feather(torch.from_numpy(m).cuda(), 255).cpu(), torch.from_numpy(ref.feather(m, 255)))
    one = torch.tensor([[[93]]], dtype=torch.uint8, device="cuda")
    assert int(ops.mask_dilate(one, 7)) == 93 and int(ops.mask_feather(one, 7)) == 93
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="radius"):
            ops.mask_dilate(one, bad)
    with pytest.raises(ValueError):
        ops.mask_feather(one.float(), 1)
    with pytest.raises(ValueError):
        ops.mask_dilate(one[0], 1)


def test_overlay_all_triples_in_one_launch(ops):
    """Every (orig, edit, alpha) in [0, 255]^3 as one [1, 4096, 4096, 1] image: index = orig * 65536 + edit * 256 + alpha."""
    i = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
    o, e, a = (i >> 16).to(torch.uint8), ((i >> 8) & 255).to(torch.uint8), (i & 255).to(torch.uint8)
    got = ops.overlay(o.view(1, 4096, 4096, 1), e.view(1, 4096, 4096, 1), a.view(1, 4096, 4096)).view(-1)
    on, en, an = o.cpu().numpy(), e.cpu().numpy(), a.cpu().numpy()
    want = torch.from_numpy(ref.overlay(on[:, None], en[:, None], an)[:, 0])
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got[a == 0], o[a == 0]) and torch.equal(got[a == 255], e[a == 255])
    assert bool((got >= torch.minimum(o, e)).all()) and bool((got <= torch.maximum(o, e)).all())


def test_overlay_random_rgb_and_in_place(ops):
    rng = np.random.default_rng(11)
    o, e = (rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8) for _ in range(2))
    a = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
    a[0, :5], a[1, -5:] = 0, 255
    want = torch.from_numpy(ref.overlay(o, e, a))
    od, ed, ad = (torch.from_numpy(x).cuda() for x in (o, e, a))
    assert torch.equal(ops.overlay(od, ed, ad).cpu(), want) and torch.equal(od.cpu(), torch.from_numpy(o))
    same = ops.overlay(od, ed, ad, out=od)                                  # out aliases orig
    assert same.data_ptr() == od.data_ptr() and torch.equal(od.cpu(), want)
    with pytest.raises(ValueError):
        ops.overlay(od, ed[:, :-1].contiguous(), ad)
    with pytest.raises(ValueError):
        ops.overlay(od, ed, ad[:1])


def test_alpha_mask_binarises_dilates_feathers(ops):
    from textflux_amd import paste_back as pb
    for name, m in _pairs(H, W).items():
        for d, r in ((0, 0), (9, 3), (3, 5)):
            got = pb.alpha_mask(torch.from_numpy(m).cuda(), d, r).cpu()
            assert torch.equal(got, torch.from_numpy(ref.alpha_mask(m, d, r))), (name, d, r)
    edge = torch.tensor([[[127, 128]]], dtype=torch.uint8, device="cuda")
    assert pb.alpha_mask(edge, 0, 0).tolist() == [[[0, 255]]]


def test_paste_with_a_size_change(ops):
    """Edited 64 x 96 into the original 67 x 101: byte-identical outside the mask dilated by dilate + 3 feather, the resampled edit on
    the mask itself (dilate >= 3 feather), the restatement everywhere."""
    from textflux_amd import paste_back as pb
    rng = np.random.default_rng(5)
    orig = rng.integers(0, 256, (2, 67, 101, 3), dtype=np.uint8)
    edit = rng.integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)
    grey = np.zeros((2, 67, 101), np.uint8)
    grey[0, 30:40, 40:70], grey[1, 0:6, 90:101], grey[1, 50:52, 10:12] = 255, 200, 129
    grey[0, 5, 5] = 127                                                     # below the threshold: not part of the mask
    d, r = 9, 3
    got = pb.paste(*(torch.from_numpy(x).cuda() for x in (orig, edit, grey)), d, r).cpu().numpy()
    assert (got == ref.paste(orig, edit, grey, d, r)).all()
    binary = np.where(grey >= 128, 255, 0).astype(np.uint8)
    outside = ref.dilate(binary, d + 3 * r) == 0
    assert outside.any() and (got[outside] == orig[outside]).all()
    core = binary == 255
    assert (got[core] == ref.resize(edit, (67, 101))[core]).all()
    same = pb.paste(torch.from_numpy(orig).cuda(), torch.from_numpy(orig).cuda(), torch.from_numpy(grey).cuda(), d, r)
    assert torch.equal(same.cpu(), torch.from_numpy(orig))                  # no size change, edit == original: nothing moves


# ---------------------------------------------------------------------------------------------- end to end, through run_items
@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_paste"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def _scene(spec):
    kind, w, h, box = spec
    if kind == "scene":
        return Image.fromarray(np.random.default_rng(w * h).integers(0, 256, (h, w, 3), dtype=np.uint8))
    m = np.zeros((h, w), np.uint8)
    m[box[1]:box[3], box[0]:box[2]] = 255
    return Image.fromarray(m)


def _run(pipe, item, paste_back):
    from textflux_amd import batch_driver
    saved, edits = {}, []
    if paste_back is not None:
        real = pipe.paste_back
        pipe.paste_back = lambda o, e, m, **k: (edits.append(np.array(e)), real(o, e, m, **k))[1]
    try:
        res = batch_driver.run_items([item], pipe, None, batch_size=2, num_inference_steps=2, guidance_scale=30.0, seed=42,
                                     loader=_scene, save=lambda i, im: saved.__setitem__(i, np.array(im)), paste_back=paste_back)
    finally:
        if paste_back is not None:
            del pipe.paste_back
    assert res["all_done"] == [0] and not res["failed"]
    return saved[0], (edits[0] if edits else None)


def test_end_to_end_whole_scene(pipe):
    w, h, box = 250, 130, (60, 50, 180, 80)                                  # not a multiple of 32 in either direction
    item = dict(image=("scene", w, h, None), mask=("mask", w, h, box), text="HELLO")
    scene, grey = np.array(_scene(item["image"])), np.array(_scene(item["mask"]))
    plain, _ = _run(pipe, item, None)
    again, _ = _run(pipe, item, None)
    assert plain.shape[1] == 224 and plain.shape[:2] != (h, w) and (plain == again).all()   # off: the pipeline's pixels at pipeline size
    d, r = 12, 4
    out, edit = _run(pipe, item, dict(dilate=d, feather=r))
    assert (edit == plain).all()                                           # the pipeline's own cropped result went into the paste
    assert out.shape == scene.shape
    alpha = ref.alpha_mask(grey, d, r)
    assert (alpha == 0).any() and (out[alpha == 0] == scene[alpha == 0]).all()
    core = grey >= 128
    assert (out[core] == ref.resize(edit[None], (h, w))[0][core]).all()
    assert (out == ref.paste(scene[None], edit[None], grey[None], d, r)[0]).all()
    assert (out[core] != scene[core]).any()


def test_end_to_end_region(pipe):
    from textflux_amd import paste_back as pb
    w, h, box = 603, 401, (300, 200, 340, 216)
    item = dict(image=("scene", w, h, None), mask=("mask", w, h, box), text="HELLO")
    scene, grey = np.array(_scene(item["image"])), np.array(_scene(item["mask"]))
    d, r = 16, 4
    reg = pb.select_region(grey, d, r, min_side=150)
    assert tuple(reg) == ref.select_region(grey, d, r, min_side=150)
    assert (reg.x1 - reg.x0, reg.y1 - reg.y0) == (150, 150) and reg.x0 > 0 and reg.y0 > 0 and reg.x1 < w and reg.y1 < h
    out, edit = _run(pipe, item, dict(region=dict(min_side=150)))
    assert edit.shape[1] == 128 and edit.shape[0] < 150                    # the pipeline ran on the region (150 -> 128 wide), not on the scene
    assert out.shape == scene.shape
    alpha = ref.alpha_mask(grey, d, r)
    assert (out[alpha == 0] == scene[alpha == 0]).all()
    ra = ref.alpha_mask(grey[reg.y0:reg.y1, reg.x0:reg.x1], d, r)          # alpha as the paste saw it: of the crop
    assert not ra[0].any() and not ra[-1].any() and not ra[:, 0].any() and not ra[:, -1].any()
    assert (ra == alpha[reg.y0:reg.y1, reg.x0:reg.x1]).all()
    core = grey >= 128
    want = scene.copy()
    want[reg.y0:reg.y1, reg.x0:reg.x1] = ref.resize(edit[None], (150, 150))[0]
    assert (out[core] == want[core]).all()
    crop = lambda a: a[reg.y0:reg.y1, reg.x0:reg.x1]
    assert (crop(out) == ref.paste(crop(scene)[None], edit[None], crop(grey)[None], d, r)[0]).all()
