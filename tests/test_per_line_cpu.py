"""Per-line region edits and the colour-matched paste without a GPU: line splitting, the table fit against its Python restatement,
the batch driver around a stub pipeline (composition order, the colour reference, item sharding, failures), the CLI flags and the two
new C entry points (exported, bound, refusing bad arguments on the host)."""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import per_line_ref as plref
from textflux_amd import batch_driver as bd
from textflux_amd import glyph
from textflux_amd import paste_back as pb
from textflux_amd import per_line as pl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("tfx_masked_moments_u8", "tfx_overlay_lut_u8")


# ---------------------------------------------------------------------------------------------- line splitting
def test_split_lines_order_pairing_and_masks():
    m = np.zeros((120, 200), np.uint8)
    m[70:90, 20:120] = 255            # lower line
    m[10:30, 100:180] = 200           # upper line, its own grey value
    m[50:54, 5:9] = 255               # 4 x 4 = 16 < min_area: not a line
    m[30, 180] = 90                   # touches the upper line diagonally: 8-connectivity makes it part of it
    lines = pl.split_lines(Image.fromarray(m), ["UP", "LOW", "NOBODY"])
    assert [(i, t) for i, t, _ in lines] == [(0, "UP"), (1, "LOW")]              # top-to-bottom; the small region never counted
    up, low = lines[0][2], lines[1][2]
    assert up.shape == m.shape and up.dtype == np.uint8
    assert (up[10:30, 100:180] == 200).all() and up[30, 180] == 90 and int((up != 0).sum()) == 20 * 80 + 1
    assert (low[70:90, 20:120] == 255).all() and int((low != 0).sum()) == 20 * 100
    assert not (up[50:54, 5:9].any() or low[50:54, 5:9].any())
    # fewer texts than regions: the regions beyond them are dropped; a blank text drops its region but keeps the pairing
    assert [(i, t) for i, t, _ in pl.split_lines(Image.fromarray(m), ["ONLY"])] == [(0, "ONLY")]
    assert [(i, t) for i, t, _ in pl.split_lines(Image.fromarray(m), ["  ", "LOW"])] == [(1, "LOW")]
    assert pl.split_lines(Image.fromarray(m), []) == []
    big = pl.split_lines(Image.fromarray(m), ["a", "b", "c"], min_area=10)        # the 16-pixel region now counts, between the two
    assert [i for i, _, _ in big] == [0, 1, 2] and int((big[1][2] != 0).sum()) == 16
    rgb = pl.split_lines(Image.fromarray(np.repeat(m[:, :, None], 3, 2)), ["UP", "LOW"])
    assert rgb[0][2].shape == (120, 200, 3) and (rgb[0][2][:, :, 1] == up).all()


# ---------------------------------------------------------------------------------------------- the fit
def _mom(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return [int(a.size), int(a.sum()), int(b.sum()), int((a * a).sum()), int((a * b).sum())]


def test_fit_luts_is_the_restatement_and_its_clamps_bite():
    rng = np.random.default_rng(0)
    a = rng.integers(40, 216, 5000)
    ident = np.arange(256, dtype=np.uint8)
    cases = {
        "plain": _mom(a, np.round(1.1 * a - 9)),
        "few pixels": _mom(a[:255], np.round(1.1 * a[:255] - 9)),
        "den = 0": _mom(np.full(400, 77), rng.integers(0, 256, 400)),
        "gain clamp high": _mom(a, np.clip(2.0 * a - 100, 0, 255)),
        "gain clamp low": _mom(a, np.round(0.3 * a + 60)),
        "shift clamp": _mom(a, np.clip(a + 60, 0, 255)),
        "negative slope": _mom(a, 255 - a),
    }
    mom = [[cases[k] for k in cases]]                                            # one sample, seven "channels"
    got = pb.fit_luts(np.array(mom, dtype=np.int64))
    want = plref.fit_luts(mom)
    assert got.dtype == np.uint8 and got.shape == (1, 7, 256) and (got == want).all()
    t = dict(zip(cases, got[0].astype(int)))
    v = np.arange(256)
    assert (t["few pixels"] == ident).all() and (t["den = 0"] == ident).all()
    assert not (t["plain"] == ident).all() and abs(int(t["plain"][100]) - 101) <= 1
    # the clamped gains: the table's slope in its unclipped middle is the bound, not the data's 2.0 / 0.3 / -1
    assert abs((t["gain clamp high"][130] - t["gain clamp high"][90]) / 40 - 1.25) < 0.03
    assert abs((t["gain clamp low"][130] - t["gain clamp low"][90]) / 40 - 0.8) < 0.03
    assert abs((t["negative slope"][130] - t["negative slope"][90]) / 40 - 0.8) < 0.03
    assert (np.abs(got[0].astype(int) - v) <= 32).all()                          # no entry moves further than max_shift
    assert (t["shift clamp"][:224] == v[:224] + 32).all() and (t["shift clamp"][224:] == 255).all()
    # the arguments reach the fit
    wide = pb.fit_luts(np.array(mom, dtype=np.int64), gain=(0.1, 4.0), max_shift=255, min_pixels=1)
    assert (wide == plref.fit_luts(mom, (0.1, 4.0), 255, 1)).all() and not (wide[0, 1] == ident).all()
    # exact in Python integers where float64 would not be: n sum aa and (sum a)^2 near 2^70 that differ by little
    n = 1 << 24
    big = [[[n, 255 * n - 1, 200 * n, 255 * 255 * n - 509, 255 * 200 * n - 200]]]  # one pixel at 254, the rest at 255; b = 200
    assert (pb.fit_luts(np.array(big, dtype=np.int64), min_pixels=1) == plref.fit_luts(big, min_pixels=1)).all()
    with pytest.raises(ValueError):
        pb.fit_luts(np.zeros((2, 5), np.int64))


def test_synthetic_drifts_are_undone_to_within_one_level_by_the_restatement():
    """The GPU test's inputs, on the CPU: for every drift (g, o) the table fitted on the ring takes the edit back to within one level
    of the original there -- the bound the GPU test holds the kernels to."""
    for g, o in plref.DRIFTS:
        orig, edit, grey = plref.drift_case(g, o)
        assert orig.min() == 40 and orig.max() == 215 and 0 <= g * 40 + o and g * 215 + o <= 255      # no value clips
        _, lut, ring = plref.paste(orig, edit, grey, 9, 3)
        on = ring[0] != 0
        assert on.sum() >= 256
        for c in range(3):
            back = lut[0, c][edit[0, :, :, c][on]].astype(int)
            assert np.abs(back - orig[0, :, :, c][on].astype(int)).max() <= 1, (g, o, c)


def test_color_match_cfg_defaults_and_refusals():
    assert pb.color_match_cfg(True) == dict(ring=24, gain=(0.8, 1.25), max_shift=32, min_pixels=256) == pb.color_match_cfg({})
    assert pb.color_match_cfg(dict(ring=7, gain=[0.5, 2]))["gain"] == (0.5, 2.0)
    for bad in (dict(ring=0), dict(ring=256), dict(gain=(0, 1)), dict(gain=(2, 1)), dict(max_shift=-1), dict(min_pixels=0), dict(width=3)):
        with pytest.raises(ValueError):
            pb.color_match_cfg(bad)


# ---------------------------------------------------------------------------------------------- the batch driver
T, J, P = 6, 8, 4


def _loader(spec):
    kind, w, h, boxes = spec
    if kind == "scene":
        return Image.fromarray(np.random.default_rng(w * h).integers(0, 256, (h, w, 3), dtype=np.uint8))
    m = np.zeros((h, w), np.uint8)
    for x0, y0, x1, y1 in boxes:
        m[y0:y1, x0:x1] = 255
    return Image.fromarray(m)


class Stub:
    """A pipeline of flat images (value 100 + the call's number) that records what it is handed."""
    fail_width = None

    def __init__(self):
        self.calls, self.encodes, self.pastes, self.text_encoder_2 = [], [], [], object()

    def encode_prompt(self, prompt, prompt_2, device=None, max_sequence_length=512, **kw):
        n = 1 if isinstance(prompt_2, str) else len(prompt_2)
        self.encodes.append(prompt_2)
        return torch.zeros(n, T, J), torch.zeros(n, P), torch.zeros(T, 3)

    def __call__(self, height, width, image, mask_image, **kw):
        if width == self.fail_width:
            raise RuntimeError("this geometry fails")
        self.calls.append((width, height, [np.array(im) for im in image]))
        return SimpleNamespace(images=[Image.fromarray(np.full((height, width, 3), 100 + len(self.calls), np.uint8)) for _ in image])


class PasteStub(Stub):
    """paste_back with the OLD signature: adds 1 to every byte of what it is handed as the original."""

    def paste_back(self, original, edited, mask, dilate=None, feather=None):
        self.pastes.append(dict(original=np.array(original), edited=edited.size, mask=np.array(mask), dilate=dilate, feather=feather))
        return (np.array(original) + 1)[None]


class ColorStub(Stub):
    def paste_back(self, original, edited, mask, dilate=None, feather=None, color_match=None, color_ref=None):
        self.pastes.append(dict(original=np.array(original), edited=edited.size, mask=np.array(mask), dilate=dilate, feather=feather,
                                color_match=color_match, color_ref=None if color_ref is None else np.array(color_ref)))
        return (np.array(original) + 1)[None]


def _run(pipe, items, **kw):
    saved = {}
    res = bd.run_items(items, pipe, None, batch_size=4, num_inference_steps=2, device="cpu", loader=_loader,
                       save=lambda i, im: saved.__setitem__(i, np.array(im)), **kw)
    return res, saved


ONE = [dict(image=("scene", 1210, 905, None), mask=("mask", 1210, 905, [(605, 452, 705, 492)]), text="WORD")]
# two lines whose 256-pixel regions overlap: 100 x 30 boxes, 120 pixels apart vertically
TWO = [dict(image=("scene", 900, 700, None), mask=("mask", 900, 700, [(300, 200, 400, 230), (320, 320, 420, 350)]), text="UPPER\nLOWER")]


def test_a_single_line_item_equals_region_mode_byte_for_byte():
    class Blend(Stub):               # a paste that depends on everything it is handed
        def paste_back(self, original, edited, mask, dilate=None, feather=None):
            self.pastes.append((np.array(original), np.array(edited), np.array(mask), dilate, feather))
            e = np.array(edited.resize((original.shape[1], original.shape[0])))
            return np.where(np.array(mask)[..., None] >= 128, e, original)[None]
    region, line = Blend(), Blend()
    r0, s0 = _run(region, ONE, paste_back=dict(region=dict(min_side=256), dilate=9, feather=3))
    r1, s1 = _run(line, ONE, paste_back=dict(region=dict(min_side=256), dilate=9, feather=3, per_line=True))
    assert r0["all_done"] == r1["all_done"] == [0] and (r0["batches"], r0["rounds"]) == (r1["batches"], r1["rounds"]) == (1, 1)
    assert s0[0].shape == (905, 1210, 3) and (s0[0] == s1[0]).all() and (s0[0] != np.array(_loader(ONE[0]["image"]))).any()
    assert len(region.calls) == len(line.calls) == 1 and region.calls[0][:2] == line.calls[0][:2]
    assert (region.calls[0][2][0] == line.calls[0][2][0]).all()                  # the same canvas went into the pipeline
    assert region.encodes == line.encodes
    for a, b in zip(region.pastes[0], line.pastes[0]):
        assert np.array_equal(a, b)
    # per_line implies region: without the key the line still runs on a region (default min_side 256), not on the 1210-wide scene
    alone = PasteStub()
    _run(alone, ONE, paste_back=dict(per_line=True))
    assert alone.calls[0][0] == 256 and alone.pastes[0]["original"].shape == (256, 256, 3)


def test_two_overlapping_lines_are_pasted_in_order_onto_the_running_result():
    scene = np.array(_loader(TWO[0]["image"]))
    grey = np.array(_loader(TWO[0]["mask"]))
    for color in (None, True, dict(ring=7)):
        pipe = ColorStub() if color else PasteStub()
        res, saved = _run(pipe, TWO, paste_back=dict(per_line=True, **({"color_match": color} if color else {})))
        assert res["all_done"] == [0] and not res["failed"] and len(pipe.pastes) == 2
        assert len(pipe.calls) == 1 and len(pipe.calls[0][2]) == 2                # equal editing size: the two lines share one batch
        assert pipe.encodes[1] == [glyph.generate_prompt(["UPPER"]), glyph.generate_prompt(["LOWER"])]
        up = np.zeros_like(grey)
        up[200:230, 300:400] = 255
        regs = [pb.select_region(up, 16, 4), pb.select_region(grey - up, 16, 4)]
        crop = lambda a, g: a[g.y0:g.y1, g.x0:g.x1]
        assert regs[0].y1 > regs[1].y0                                           # the regions do overlap
        want = scene.copy()
        for k, (g, p) in enumerate(zip(regs, pipe.pastes)):
            assert (p["original"] == crop(want, g)).all()                        # the CURRENT pixels: line 1 sees line 0's paste
            assert (p["mask"] == crop(up if k == 0 else grey - up, g)).all()     # the line's own mask, not the item's
            assert (p["dilate"], p["feather"]) == (16, 4)
            if color:
                assert p["color_match"] == pb.color_match_cfg(color)
                assert (p["color_ref"] == crop(scene, g)).all()                  # the ORIGINAL pixels, whatever was pasted since
            else:
                assert "color_match" not in p                                    # the old signature was enough: nothing new was passed
            want[g.y0:g.y1, g.x0:g.x1] = crop(want, g) + 1
        assert (pipe.pastes[1]["original"] != crop(scene, regs[1])).any()
        assert (saved[0] == want).all()
        assert (saved[0][regs[1].y0:regs[0].y1, max(regs[0].x0, regs[1].x0):regs[0].x1] ==
                scene[regs[1].y0:regs[0].y1, max(regs[0].x0, regs[1].x0):regs[0].x1] + 2).all()      # where the regions overlap: pasted twice


def test_color_match_without_per_line_passes_only_color_match():
    pipe = ColorStub()
    _run(pipe, ONE, paste_back=dict(color_match=True))
    assert pipe.pastes[0]["color_match"] == pb.color_match_cfg(True) and pipe.pastes[0]["color_ref"] is None
    old = PasteStub()
    _run(old, ONE, paste_back={})
    assert len(old.pastes) == 1                                                  # and without it the old signature still serves


def _works(sizes_per_item):
    return [bd.Work(i, None, None, "", {}, s, parent=i, line=k) for i, sizes in enumerate(sizes_per_item) for k, s in enumerate(sizes)]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_plans_keep_todays_dealing_and_shard_per_line_by_item(world):
    a, b, c = (256, 288), (512, 320), (128, 160)
    works = _works([[a], [b], [a], [a], [c], [b], [a], [a], [a], [c], [b]])
    plan = bd.plan_batches(works, 2)
    plans = bd.rank_plans(works, world, 2)
    assert len(plans) == world and sum(len(p) for p in plans) == len(plan)
    for k in range(world):
        for r, batch in enumerate(plans[k]):
            assert batch is not None and [w.index for w in batch.items] == [w.index for w in plan[r * world + k].items]
            assert batch.size == plan[r * world + k].size
    assert max(len(p) for p in plans) == (len(plan) + world - 1) // world        # rounds, as before
    lines = _works([[a, a, b], [a], [c, b], [b, b, b, a], [a, c], [c], [a, a]])
    plans = bd.rank_plans(lines, world, 2, per_line=True)
    owner, seen = {}, []
    for k, p in enumerate(plans):
        for batch in p:
            assert len({w.size for w in batch.items}) == 1 and len(batch.items) <= 2
            for w in batch.items:
                assert owner.setdefault(w.index, k) == k                         # all lines of an item on one rank
                seen.append((w.index, w.line))
    assert sorted(seen) == sorted((w.index, w.line) for w in lines) and len(set(seen)) == len(seen)   # every line exactly once
    assert owner == {i: i % world for i in range(7)}
    # lines of equal editing size share batches ACROSS the items of a rank
    if world == 1:
        assert [len(bt.items) for bt in plans[0] if bt.size == a] == [2, 2, 2, 1]


def _annos(n):
    polys = [[[40, 30], [200, 30], [200, 70], [40, 70]], [[260, 150], [470, 150], [470, 200], [260, 200]], [[50, 200], [120, 200], [120, 230], [50, 230]]]
    return [dict(img_name="dir/a.png", annotations=[dict(text=f"LINE{k}", polygon=polys[k]) for k in range(n)])]


def test_every_annotation_is_a_line_only_under_per_line(tmp_path):
    loader = lambda p: Image.fromarray(np.full((260, 520, 3), 77, np.uint8))
    cfg = dict(original_images_dir="imgs", font=glyph.load_font(None), text_height_ratio=0.1667)
    for sub in ("off", "on"):
        os.makedirs(tmp_path / sub / "full_images"), os.makedirs(tmp_path / sub / "cropped_images")
    off, on = PasteStub(), PasteStub()
    bd.run_items(_annos(2), off, str(tmp_path / "off"), device="cpu", loader=loader, eval_cfg=cfg, paste_back=dict(region={}))
    res = bd.run_items(_annos(2), on, str(tmp_path / "on"), device="cpu", loader=loader, eval_cfg=cfg, paste_back=dict(per_line=True))
    assert len(off.pastes) == 1 and off.encodes[1] == [glyph.generate_prompt(["LINE0"])]       # annotations[0] alone, as the reference
    assert res["all_done"] == [0] and len(on.pastes) == 2
    assert [p for e in on.encodes[1:] for p in e] == [glyph.generate_prompt(["LINE0"]), glyph.generate_prompt(["LINE1"])]
    assert on.pastes[0]["mask"].max() == 255 and on.pastes[1]["mask"].max() == 255
    assert sorted(os.listdir(tmp_path / "on" / "full_images")) == ["a.png", "a_line1.png"]
    assert os.listdir(tmp_path / "on" / "cropped_images") == ["a.png"] and os.listdir(tmp_path / "off" / "full_images") == ["a.png"]
    out = np.array(Image.open(tmp_path / "on" / "cropped_images" / "a.png"))
    assert out.shape == (260, 520, 3) and out[50, 100, 0] in (78, 79) and out[175, 400, 0] in (78, 79)   # both lines' regions were pasted
    works = pl.prepare_lines(0, _annos(3)[0], loader, False, cfg, bd._paste_back_cfg(dict(per_line=True)))
    assert [(w.parent, w.line, w.name, w.meta["mode"]) for w in works] == [(0, k, "a.png", "singleline") for k in range(3)]
    assert bd.prepare_item(0, _annos(3)[0], loader, eval_cfg=cfg).parent is None
    blank = _annos(3)[0]
    blank["annotations"][1]["text"] = " "
    assert [w.prompt for w in pl.prepare_lines(0, blank, loader, False, cfg, bd._paste_back_cfg(dict(per_line=True)))] == \
        [glyph.generate_prompt(["LINE0"]), glyph.generate_prompt(["LINE2"])]


def test_a_failing_line_fails_its_item_and_nothing_is_written():
    # item 0: a narrow line (256-wide region) and a wide one (300 + 2 * 150 -> 600-wide region, edited at 576); item 1: a narrow line
    items = [dict(image=("scene", 1000, 800, None), mask=("mask", 1000, 800, [(100, 100, 200, 130), (300, 500, 600, 540)]), text="A\nB"),
             dict(image=("scene", 1000, 800, None), mask=("mask", 1000, 800, [(100, 100, 200, 130)]), text="C")]
    ok = PasteStub()
    res, saved = _run(ok, items, paste_back=dict(per_line=True))
    assert res["all_done"] == [0, 1] and sorted({c[0] for c in ok.calls}) == [256, 576] and len(ok.pastes) == 3
    for fail_width in (576, 256):
        pipe = PasteStub()
        pipe.fail_width = fail_width
        res, saved = _run(pipe, items, paste_back=dict(per_line=True))
        if fail_width == 576:        # item 0's second line: item 0 fails although its first line ran; item 1 is untouched by that
            assert res["failed"] == [0] and res["all_done"] == [1] and list(saved) == [1] and len(pipe.pastes) == 1
        else:                        # the batch that holds a line of each item
            assert sorted(res["failed"]) == [0, 1] and res["all_done"] == [] and saved == {} and pipe.pastes == []
    # a text line without a mask region to go to is no failure (the region rule drops it); no usable line at all is
    res, saved = _run(PasteStub(), [dict(items[1], text="C\nD"), dict(items[1], text="  ")], paste_back=dict(per_line=True))
    assert res["all_done"] == [0] and res["failed"] == [1]


def test_unknown_keys_and_bad_values_are_refused_before_anything_runs():
    pipe = PasteStub()
    for bad, match in ((dict(per_lines=True), "unknown keys"), (dict(color_match=dict(radius=3)), "unknown keys"),
                       (dict(per_line="yes"), "per_line"), (dict(color_match=3), "color_match"),
                       (dict(color_match=dict(ring=0)), "ring"), (dict(color_match=dict(gain=(2, 1))), "gain")):
        with pytest.raises(ValueError, match=match):
            _run(pipe, ONE, paste_back=bad)
    pipe.call_mixed = lambda **k: None
    with pytest.raises(NotImplementedError, match="mixed-geometry"):
        _run(pipe, ONE, paste_back=dict(per_line=True), mixed_pad=0.25)          # the existing refusal is not lifted
    assert pipe.encodes == [] and pipe.calls == [] and pipe.pastes == []
    cfg = bd._paste_back_cfg(dict(per_line=True, color_match=True))
    assert cfg == dict(dilate=16, feather=4, region={}, per_line=True, color_match=pb.color_match_cfg(True))
    assert bd._paste_back_cfg(dict(per_line=False, color_match=None)) == dict(dilate=16, feather=4, region=None) == bd._paste_back_cfg({})
    assert bd._paste_back_cfg(dict(per_line=True, region=dict(max_side=512)))["region"] == dict(max_side=512)


def test_work_keeps_its_old_constructions():
    w = bd.Work(3, None, None, "p", {}, (64, 64))
    assert w.parent is None and w.line is None


# ---------------------------------------------------------------------------------------------- callers and CLIs
def test_run_inference_takes_the_same_path():
    sys.path.insert(0, REPO)
    ri = importlib.import_module("run_inference")

    class Pipe(ColorStub):
        _execution_device = "cpu"    # where the per-line path makes its generators

        def __call__(self, height, width, image, mask_image, prompt=None, prompt_2=None, generator=None, **kw):
            assert len(prompt) == len(prompt_2) == len(generator) == len(image)
            self.encodes.append(list(prompt_2))
            return Stub.__call__(self, height, width, image, mask_image)
    scene, mask = _loader(TWO[0]["image"]), _loader(TWO[0]["mask"])
    saved = ri.scheduler_name
    ri.scheduler_name = ""
    try:
        pipe, via_driver = Pipe(), ColorStub()
        out = ri.run_inference(scene, mask, ["UPPER", "LOWER"], num_steps=2, pipe=pipe, paste_back=dict(per_line=True, color_match=True))
    finally:
        ri.scheduler_name = saved
    _, want = _run(via_driver, TWO, paste_back=dict(per_line=True, color_match=True))
    assert out.size == scene.size and (np.array(out) == want[0]).all()
    assert len(pipe.calls) == 1 and pipe.encodes == [[glyph.generate_prompt(["UPPER"]), glyph.generate_prompt(["LOWER"])]]
    for a, b in zip(pipe.pastes, via_driver.pastes):
        assert (a["color_ref"] == b["color_ref"]).all() and (a["original"] == b["original"]).all() and (a["mask"] == b["mask"]).all()


def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        a = parser.parse_args(base)
        assert (a.paste_per_line, a.paste_color_match, a.paste_color_ring) == (False, False, None)
        a = parser.parse_args(base + ["--paste_back", "--paste_per_line", "--paste_color_match", "--paste_color_ring", "12"])
        assert (a.paste_back, a.paste_per_line, a.paste_color_match, a.paste_color_ring) == (True, True, True, 12)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(["--paste_back"]) == dict(dilate=16, feather=4, region=None)     # without the new flags: the dict it was
    assert parse(["--paste_back", "--paste_per_line"]) == dict(dilate=16, feather=4, region=None, per_line=True)
    assert parse(["--paste_back", "--paste_color_match"])["color_match"] is True
    assert parse(["--paste_back", "--paste_color_ring", "12"])["color_match"] == dict(ring=12)
    assert bd._paste_back_cfg(parse(["--paste_back", "--paste_per_line", "--paste_color_ring", "12"]))["color_match"]["ring"] == 12
    for flag in (["--paste_per_line"], ["--paste_color_match"], ["--paste_color_ring", "12"]):
        with pytest.raises(SystemExit, match="needs --paste_back"):
            parse(flag)
        with pytest.raises(SystemExit, match="needs --paste_back"):
            re_.main(["--json_path", "j", "--original_images_dir", "o", "--weights_path", "w"] + flag)
        with pytest.raises(SystemExit, match="needs --paste_back"):
            re_.main(["--json_path", "j", "--original_images_dir", "o", "--lora_weights_path", "l"] + flag, lora=True)


# ---------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


def test_symbols_are_exported_bound_and_the_abi_version_stays(lib):
    from textflux_amd import _lib as L
    from textflux_amd import ops
    for s in SYMS:
        assert s in L.SIGNATURES and hasattr(lib, s)
    assert L.ABI_VERSION == 11 == L.header_abi_version()
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    assert hdr.count("without a new") >= 2 and f"#define TFX_MASKED_MOMENTS_SCRATCH_BYTES {ops.MASKED_MOMENTS_SCRATCH_BYTES}" in hdr


def test_entry_points_check_their_arguments(lib):
    p = [k << 20 for k in range(1, 6)]                                           # never dereferenced: every call below is refused on the host
    need = 34816
    mm = lambda ptrs=p, scratch=4 * need, dims=(2, 4, 4, 3): lib.tfx_masked_moments_u8(*ptrs, scratch, *dims, None)
    for k in range(5):
        assert mm(p[:k] + [None] + p[k + 1:]) != 0 and b"null pointer" in lib.tfx_last_error()
    for dims in ((0, 4, 4, 3), (2, 0, 4, 3), (2, 4, 0, 3), (-1, 4, 4, 3)):
        assert mm(dims=dims) != 0 and b"at least 1" in lib.tfx_last_error()
    for c in (0, 5):
        assert mm(dims=(2, 4, 4, c)) != 0 and b"1..4 channels" in lib.tfx_last_error()
    assert mm(scratch=2 * need - 1) != 0 and b"scratch" in lib.tfx_last_error()  # one byte short of B = 2 samples' worth
    ol = lambda ptrs=p, dims=(2, 4, 4, 3): lib.tfx_overlay_lut_u8(*ptrs, *dims, None)
    for k in range(5):
        assert ol(p[:k] + [None] + p[k + 1:]) != 0 and b"null pointer" in lib.tfx_last_error()
    for dims in ((0, 4, 4, 3), (2, 0, 4, 3), (2, 4, 0, 3)):
        assert ol(dims=dims) != 0 and b"at least 1" in lib.tfx_last_error()
    for c in (0, 5):
        assert ol(dims=(2, 4, 4, c)) != 0 and b"1..4 channels" in lib.tfx_last_error()
    for k in (1, 2, 3):                                                          # out may be orig, and nothing else
        assert ol(p[:4] + [p[k]]) != 0 and b"alias orig only" in lib.tfx_last_error()


def test_ops_wrappers_check_before_they_launch():
    from textflux_amd import ops
    from textflux_amd.pipeline import FluxFillPipeline
    import inspect
    img, w = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.masked_moments(img, img, w)                                          # no CPU fallback
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.overlay_lut(img, img, w, torch.zeros(1, 3, 256, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pb.ring_mask(w, 3)
    with pytest.raises(ValueError):
        pb.ring_mask(w, 0)
    for f in (FluxFillPipeline.paste_back, pb.paste):
        sig = inspect.signature(f).parameters
        assert sig["color_match"].default is None and sig["color_ref"].default is None
