"""Paste-back and region editing without a GPU: the properties of the integer arithmetic (on its numpy restatement, which the GPU
tests compare the kernels with bit for bit), the region rule's known answers, the three new C entry points (exported, bound,
refusing bad arguments on the host), and the batch driver / CLI plumbing around a stub pipeline."""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import paste_back_ref as ref
from textflux_amd import batch_driver as bd
from textflux_amd import paste_back as pb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("tfx_mask_dilate_u8", "tfx_mask_feather_u8", "tfx_overlay_u8")


# ---------------------------------------------------------------------------------------------- the arithmetic's properties
def _masks(h, w, seed):
    rng = np.random.default_rng(seed)
    out = {"corner": np.zeros((h, w), np.uint8), "centre": np.zeros((h, w), np.uint8),
           "random": (rng.random((h, w)) < 0.03).astype(np.uint8) * 255,
           "grey": rng.integers(0, 256, (h, w), dtype=np.uint8)}
    out["corner"][0, 0] = 255
    out["centre"][h // 2, w // 2] = 200          # >= 128: binarised to 255
    return out


@pytest.mark.parametrize("h,w,d,r", [(37, 53, 0, 0), (37, 53, 9, 3), (37, 53, 12, 4), (37, 53, 40, 1), (5, 1, 2, 1), (64, 80, 3, 5)])
def test_alpha_support_and_core(h, w, d, r):
    for name, m in _masks(h, w, h * w + d).items():
        binary = np.where(m >= 128, 255, 0).astype(np.uint8)
        a = ref.alpha_mask(m, d, r)
        assert not a[ref.dilate(binary, d + 3 * r) == 0].any(), name        # the support grows by at most d + 3 r per axis
        if d >= 3 * r:
            assert (a[binary == 255] == 255).all(), name                    # the seam condition: the mask itself is fully the edit
        if d == 0 and r == 0:
            assert (a == binary).all()
    for r_ in (r, 255):
        assert (ref.feather(np.full((h, w), 255, np.uint8), r_) == 255).all() and not ref.feather(np.zeros((h, w), np.uint8), r_).any()
        assert (ref.dilate(np.full((h, w), 255, np.uint8), r_) == 255).all() and not ref.dilate(np.zeros((h, w), np.uint8), r_).any()
    assert not ref.alpha_mask(np.full((h, w), 127, np.uint8), d, r).any()   # 127 is below the threshold


def test_dilate_is_the_clipped_square_maximum():
    m = np.random.default_rng(3).integers(0, 256, (2, 11, 13), dtype=np.uint8)
    for r in (0, 1, 4, 20):
        got = ref.dilate(m, r)
        for b, y, x in ((0, 0, 0), (1, 10, 12), (0, 5, 6), (1, 0, 12), (0, 3, 1)):
            assert got[b, y, x] == m[b, max(y - r, 0): y + r + 1, max(x - r, 0): x + r + 1].max()


def test_box_pass_rounds_half_up_and_replicates_the_edge():
    v = np.array([[0, 0, 255, 0, 0, 10]], np.uint8)
    # n = 3: sums 0, 255, 255, 255, 10, 20 (last: 0 + 10 + the replicated 10) -> (2 s + 3) // 6
    assert ref.box_pass(v, 1, -1).tolist() == [[0, 85, 85, 85, 3, 7]]
    assert ref.box_pass(np.array([[1, 2]], np.uint8), 0, -1).tolist() == [[1, 2]]


def test_overlay_is_exact_at_the_ends_and_bounded_over_all_triples():
    o, e = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    o, e = o.reshape(-1, 1), e.reshape(-1, 1)
    lo, hi = np.minimum(o, e), np.maximum(o, e)
    for a in range(256):
        out = ref.overlay(o, e, np.full(o.shape[0], a, np.uint8))
        assert (lo <= out).all() and (out <= hi).all()
        if a == 0:
            assert (out == o).all()
        if a == 255:
            assert (out == e).all()


# ---------------------------------------------------------------------------------------------- the region rule
def _rect(H, W, x0, y0, x1, y1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


REGION_CASES = {  # name: (mask, kwargs, expected Region)
    "middle of 4000x3000": (_rect(3000, 4000, 1500, 1400, 2500, 1600), {}, (1000, 900, 3000, 2100, 1024, 614)),
    "touching a corner": (_rect(800, 1000, 0, 0, 40, 20), {}, (0, 0, 256, 256, 256, 256)),
    "near the far corner": (_rect(800, 1000, 950, 770, 1000, 800), {}, (744, 544, 1000, 800, 256, 256)),
    "mask larger than max_side": (_rect(2000, 3000, 200, 300, 1800, 700), {}, (0, 0, 3000, 2000, 1024, 682)),
    "image smaller than min_side": (_rect(150, 200, 50, 50, 60, 60), {}, (0, 0, 200, 150, 200, 150)),
    # 1 x 3 mask, pad 0: p = halo = 29 -> x [271, 330) (59), y [271, 332) (61); to 100 the low side gets 41 // 2 = 20 and 39 // 2 = 19
    "odd growth": (_rect(600, 700, 300, 300, 301, 303), dict(min_side=100, pad=0.0), (251, 252, 351, 352, 100, 100)),
    "thin and long": (_rect(400, 5000, 100, 190, 4100, 210), dict(max_side=512), (0, 0, 5000, 400, 512, 40)),
}


@pytest.mark.parametrize("name", sorted(REGION_CASES))
def test_select_region_known_answers(name):
    mask, kw, want = REGION_CASES[name]
    d, r = 16, 4
    got = pb.select_region(mask, d, r, **kw)
    assert tuple(got) == want == ref.select_region(mask, d, r, **kw)
    H, W = mask.shape
    assert 0 <= got.x0 < got.x1 <= W and 0 <= got.y0 < got.y1 <= H
    gx0, gy0, gx1, gy1 = ref.bbox_grown(mask, pb.halo(d, r))                # the bbox grown by the halo, cut by the image border
    assert got.x0 <= gx0 and got.y0 <= gy0 and got.x1 >= gx1 and got.y1 >= gy1
    w, h = got.x1 - got.x0, got.y1 - got.y0
    if max(w, h) > kw.get("max_side", 1024):
        assert max(got.tw, got.th) == kw.get("max_side", 1024)
    else:
        assert (got.tw, got.th) == (w, h)


def test_select_region_refuses_an_empty_mask_and_knows_the_whole_image():
    with pytest.raises(ValueError, match="empty"):
        pb.select_region(np.full((64, 64), 127, np.uint8), 16, 4)
    assert tuple(pb.select_region(None, size=(4000, 3000))) == (0, 0, 4000, 3000, 4000, 3000)
    with pytest.raises(ValueError):
        pb.select_region(None)


# ---------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


def test_symbols_are_exported_bound_and_the_abi_version_stays(lib):
    from textflux_amd import _lib as L
    for s in SYMS:
        assert s in L.SIGNATURES and hasattr(lib, s)
    assert L.ABI_VERSION == 11 == L.header_abi_version()
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    assert "without a new TFX_ABI_VERSION" in hdr


@pytest.mark.parametrize("sym", SYMS[:2])
def test_window_entry_points_check_their_arguments(lib, sym):
    fn = getattr(lib, sym)
    a, b, c = 1 << 20, 2 << 20, 3 << 20                                   # never dereferenced: every call below is refused on the host
    for args in ((None, b, c), (a, None, c), (a, b, None)):
        assert fn(*args, 1, 4, 4, 1, None) != 0 and b"null pointer" in lib.tfx_last_error()
    for radius in (-1, 256):
        assert fn(a, b, c, 1, 4, 4, radius, None) != 0 and b"radius must be in [0, 255]" in lib.tfx_last_error()
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert fn(a, b, c, B, H, W, 1, None) != 0 and b"at least 1" in lib.tfx_last_error()
    for args in ((a, a, c), (a, b, a), (a, b, b)):
        assert fn(*args, 1, 4, 4, 1, None) != 0 and b"three different buffers" in lib.tfx_last_error()


def test_overlay_entry_point_checks_its_arguments(lib):
    fn = lib.tfx_overlay_u8
    o, e, a, out = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    for args in ((None, e, a, out), (o, None, a, out), (o, e, None, out), (o, e, a, None)):
        assert fn(*args, 1, 4, 4, 3, None) != 0 and b"null pointer" in lib.tfx_last_error()
    for dims in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 3), (1, 4, 4, 0)):
        assert fn(o, e, a, out, *dims, None) != 0 and b"at least 1" in lib.tfx_last_error()
    assert fn(o, e, a, e, 1, 4, 4, 3, None) != 0 and b"alias orig only" in lib.tfx_last_error()
    assert fn(o, e, a, a, 1, 4, 4, 3, None) != 0 and b"alias orig only" in lib.tfx_last_error()


def test_ops_wrappers_check_before_they_launch():
    from textflux_amd import ops
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    for f in (ops.mask_dilate, ops.mask_feather):
        with pytest.raises(RuntimeError, match="ROCm device"):
            f(m, 1)                                                         # no CPU fallback
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.overlay(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), m)
    from textflux_amd.pipeline import FluxFillPipeline
    assert FluxFillPipeline.supports_paste_back is True and callable(FluxFillPipeline.paste_back)


# ---------------------------------------------------------------------------------------------- the batch driver
T, J, P = 6, 8, 4


def _loader(spec):
    kind, w, h, i = spec
    if kind == "scene":
        return Image.fromarray(np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8))
    m = np.zeros((h, w), np.uint8)
    m[h // 2: h // 2 + 40, w // 2: w // 2 + 100] = 255
    return Image.fromarray(m)


class Stub:
    """A pipeline of flat grey images that records what it is handed."""

    def __init__(self):
        self.calls, self.encodes, self.pastes, self.text_encoder_2 = [], [], [], object()

    def encode_prompt(self, prompt, prompt_2, device=None, max_sequence_length=512, **kw):
        n = 1 if isinstance(prompt_2, str) else len(prompt_2)
        self.encodes.append(n)
        return torch.zeros(n, T, J), torch.zeros(n, P), torch.zeros(T, 3)

    def __call__(self, height, width, image, mask_image, **kw):
        self.calls.append((width, height, [np.array(im) for im in image]))
        return SimpleNamespace(images=[Image.fromarray(np.full((height, width, 3), 200, np.uint8)) for _ in image])


class PasteStub(Stub):
    def paste_back(self, original, edited, mask, dilate=None, feather=None):
        self.pastes.append((np.array(original), edited.size, np.array(mask), dilate, feather))
        return np.full((1,) + original.shape, 7, np.uint8)


ITEMS = [dict(image=("scene", 500, 250, 1), mask=("mask", 500, 250, 1), text="WORD"),
         dict(image=("scene", 500, 250, 2), mask=("mask", 500, 250, 2), text="OTHER")]


def _run(pipe, items=ITEMS, **kw):
    saved = {}
    res = bd.run_items(items, pipe, None, batch_size=4, num_inference_steps=2, device="cpu", loader=_loader,
                       save=lambda i, im: saved.__setitem__(i, np.array(im)), **kw)
    return res, saved


def test_off_never_touches_paste_back():
    class Trap(Stub):
        def paste_back(self, *a, **k):
            raise AssertionError("paste_back=None must not call pipe.paste_back")
    (res, saved), (res0, saved0) = _run(Trap()), _run(Stub())
    assert res["all_done"] == res0["all_done"] == [0, 1]
    for i in (0, 1):
        assert saved[i].shape == saved0[i].shape and saved[i].shape[:2] != (250, 500) and (saved[i] == saved0[i]).all()
    w = bd.prepare_item(0, ITEMS[0], _loader)
    assert w.orig_scene is None and w.orig_mask is None and w.region is None


def test_on_hands_over_scene_mask_and_crop_and_saves_at_the_scene_size():
    pipe = PasteStub()
    res, saved = _run(pipe, paste_back=dict(dilate=9, feather=3))
    assert res["all_done"] == [0, 1] and len(pipe.pastes) == 2 and len(pipe.calls) == 1
    cw, ch, _ = pipe.calls[0]
    for i, (orig, esize, mask, d, r) in enumerate(pipe.pastes):
        scene = np.array(_loader(ITEMS[i]["image"]))
        assert (orig == scene).all() and (mask == np.array(_loader(ITEMS[i]["mask"]))).all() and (d, r) == (9, 3)
        assert esize[0] == cw and 0 < esize[1] < ch                       # the cropped result: the canvas without its glyph strip
        assert saved[i].shape == (250, 500, 3) and (saved[i] == 7).all()  # what paste_back returned, at the ORIGINAL size
    _, _ = _run(pipe, paste_back={})
    assert pipe.pastes[-1][3:] == (16, 4)                                 # the defaults


def test_refusals_come_before_anything_is_encoded():
    pipe = Stub()
    with pytest.raises(ValueError, match="paste_back needs a pipeline with paste_back"):
        _run(pipe, paste_back={})
    pipe = PasteStub()
    pipe.call_mixed = lambda **k: None
    with pytest.raises(NotImplementedError, match="mixed-geometry"):
        _run(pipe, paste_back={}, mixed_pad=0.25)
    with pytest.raises(ValueError, match="unknown keys"):
        _run(pipe, paste_back=dict(radius=3))
    with pytest.raises(ValueError, match="unknown keys"):
        _run(pipe, paste_back=dict(region=dict(side=3)))
    with pytest.raises(ValueError, match=r"\[0, 255\]"):
        _run(pipe, paste_back=dict(dilate=256))
    assert pipe.encodes == [] and pipe.calls == [] and pipe.pastes == []


def test_region_mode_hands_the_pipeline_the_region_not_the_scene():
    items = [dict(image=("scene", 1210, 905, 5), mask=("mask", 1210, 905, 5), text="WORD")]
    whole, part = PasteStub(), PasteStub()
    _run(whole, items, paste_back={})
    res, saved = _run(part, items, paste_back=dict(region=dict(min_side=256)))
    scene, mask = np.array(_loader(items[0]["image"])), np.array(_loader(items[0]["mask"]))
    reg = pb.select_region(mask, 16, 4, min_side=256)
    assert tuple(reg) == ref.select_region(mask, 16, 4, min_side=256)
    w, h = reg.x1 - reg.x0, reg.y1 - reg.y0
    assert (w, h) == (256, 256) and 0 < reg.x0 and reg.x1 < 1210 and 0 < reg.y0 and reg.y1 < 905      # a proper sub-rectangle
    assert whole.calls[0][0] == 1184 and part.calls[0][0] == 256         # canvas width: the scene's / the region's, floored to 32
    canvas = part.calls[0][2][0]
    assert canvas.shape[1] == 256
    orig, esize, m, _, _ = part.pastes[0]
    assert (orig == scene[reg.y0:reg.y1, reg.x0:reg.x1]).all() and (m == mask[reg.y0:reg.y1, reg.x0:reg.x1]).all()
    out = saved[0]
    assert out.shape == scene.shape and (out[reg.y0:reg.y1, reg.x0:reg.x1] == 7).all()
    outside = np.ones(scene.shape[:2], bool)
    outside[reg.y0:reg.y1, reg.x0:reg.x1] = False
    assert (out[outside] == scene[outside]).all()
    # a region above max_side is edited smaller: the pipeline sees (tw, th), the paste still gets the crop at its own size
    small = PasteStub()
    _run(small, items, paste_back=dict(region=dict(min_side=512, max_side=320)))
    reg2 = pb.select_region(mask, 16, 4, min_side=512, max_side=320)
    assert (reg2.tw, reg2.th) == (320, 320) and small.calls[0][0] == 320 and small.pastes[0][0].shape == (512, 512, 3)


def test_eval_schema_writes_the_pasted_scene_and_keeps_the_raw_canvas(tmp_path):
    from textflux_amd import glyph
    data = [dict(img_name="a.png", annotations=[dict(text="HELLO", polygon=[[100, 60], [400, 60], [400, 120], [100, 120]])])]
    loader = lambda p: Image.fromarray(np.full((260, 520, 3), 77, np.uint8))
    cfg = dict(original_images_dir="imgs", font=glyph.load_font(None), text_height_ratio=0.1667)
    os.makedirs(tmp_path / "full_images"), os.makedirs(tmp_path / "cropped_images")
    pipe = PasteStub()
    res = bd.run_items(data, pipe, str(tmp_path), device="cpu", loader=loader, eval_cfg=cfg, paste_back={})
    assert res["all_done"] == [0]
    assert Image.open(tmp_path / "full_images" / "a.png").size == (512, 320)          # the raw canvas, as without paste-back
    assert Image.open(tmp_path / "cropped_images" / "a.png").size == (520, 260)       # the original scene's size
    assert pipe.pastes[0][0].shape == (260, 520, 3) and pipe.pastes[0][2][60:121, 100:401].min() == 255


def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    on = ["--paste_back", "--paste_dilate", "20", "--paste_feather", "5", "--paste_region", "--paste_region_max", "768"]
    for parser, base in ((ri.build_parser(), ["--image", "i", "--mask", "m", "--words", "w"]),
                         (rl.build_parser(), ["--image", "i", "--mask", "m", "--words", "w"]),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.paste_back, a.paste_dilate, a.paste_feather, a.paste_region, a.paste_region_max) == (False, 16, 4, False, 1024)
        a = parser.parse_args(base + on)
        assert (a.paste_back, a.paste_dilate, a.paste_feather, a.paste_region, a.paste_region_max) == (True, 20, 5, True, 768)
    a = ri.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w"] + on)
    assert ri.paste_back_from_args(a) == dict(dilate=20, feather=5, region=dict(max_side=768))
    assert ri.paste_back_from_args(ri.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w"])) is None
    with pytest.raises(SystemExit):
        ri.paste_back_from_args(ri.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w", "--paste_region"]))
    with pytest.raises(SystemExit):
        re_.main(["--json_path", "j", "--original_images_dir", "o", "--weights_path", "w", "--paste_back", "--mixed_pad", "0.2"])
    import inspect
    assert inspect.signature(ri.run_inference).parameters["paste_back"].default is None
    assert inspect.signature(bd.run_items).parameters["paste_back"].default is None
