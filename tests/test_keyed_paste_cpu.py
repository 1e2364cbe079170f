"""Keyed paste without a GPU (DESIGN.md section 4 "Keyed paste"): the two restatements of the hysteresis against each other and the set's
properties, the metric's identities (tests/helpers/keyed_ref.py), the package's host arithmetic against the restatement, and the
plumbing: the configuration, what the batch driver, the per-line composer and the pipeline method hand on, the CLIs' flags, and the C
entry points' declarations and refusals (none of which touches a device)."""
import importlib
import inspect
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from tests.helpers import keyed_ref as kref
from tests.test_paste_back_cpu import ITEMS, Stub, _loader
from textflux_amd import batch_driver as bd
from textflux_amd import paste_back as pb
from textflux_amd import per_line as pl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = ((0, 0), (0, 256), (40, 40), (10, 28), (1, 255))
H, W = 130, 257                                       # the constructed fields: three tiles of 64 wide and a rest, eight of 16 high and a rest
LO, HI = 10, 28


@pytest.fixture(autouse=True)
def feature():
    """The restatement is only worth its tests beside the thing it restates: without the feature every test of this file fails."""
    from textflux_amd import _lib as L
    from textflux_amd import ops
    assert hasattr(pb, "keyed_cfg") and hasattr(ops, "hysteresis") and "tfx_hysteresis_u8" in L.SIGNATURES, "this tree has no keyed paste"


# ---------------------------------------------------------------------------------------------- constructed fields (shared with the GPU tests)
def serpentine(gap=None):
    """A one-pixel-wide path of LO pixels that runs along every second row, joined at alternating ends, with one HI seed at its start:
    it crosses every vertical tile boundary on every second row and every horizontal one once.  gap: the index of a path pixel that is
    left out.  -> (field u8 [2, H, W], the path as (y, x) in order): sample 1 holds the same path mirrored left to right."""
    path = []
    for k, y in enumerate(range(0, H, 2)):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, W - 1 if k % 2 == 0 else 0))
    m = np.zeros((2, H, W), np.uint8)
    for i, (y, x) in enumerate(path):
        if i != gap:
            m[0, y, x] = m[1, y, W - 1 - x] = HI if i == 0 else LO
    return m, path


def blobs(apart: int):
    """Two 5 x 5 blobs of LO pixels, the first with a HI seed, whose corners meet diagonally at the tile corner (row 16 | column 64):
    the first ends at (15, 63), the second begins at (16 + apart, 64 + apart).  -> field u8 [2, H, W] (sample 1: the same, transposed)."""
    m = np.zeros((2, H, W), np.uint8)
    m[0, 11:16, 59:64] = LO
    m[0, 13, 61] = HI
    m[0, 16 + apart:21 + apart, 64 + apart:69 + apart] = LO
    m[1, 59:64, 11:16] = LO                           # the same transposed: the corners meet across the tile edge between rows 63 and 64
    m[1, 61, 13] = HI
    m[1, 64 + apart:69 + apart, 16 + apart:21 + apart] = LO
    return m


def one_sample_seed():
    """Both samples all LO; a HI seed in sample 0 only."""
    m = np.full((2, H, W), LO, np.uint8)
    m[0, 77, 200] = HI
    return m


def constructed():
    """name -> (field, the expected result written down by hand)."""
    out = {}
    m, path = serpentine()
    out["serpentine"] = (m, np.where(m > 0, 255, 0).astype(np.uint8))
    cut = len(path) // 2
    m, path = serpentine(gap=cut)
    want = np.zeros_like(m)
    for y, x in path[:cut]:
        want[0, y, x] = want[1, y, W - 1 - x] = 255
    out["serpentine_cut"] = (m, want)
    m = blobs(0)
    out["blobs_touch"] = (m, np.where(m > 0, 255, 0).astype(np.uint8))
    m = blobs(1)
    want = np.zeros_like(m)
    want[0, 11:16, 59:64] = want[1, 59:64, 11:16] = 255
    out["blobs_apart"] = (m, want)
    m = one_sample_seed()
    want = np.zeros_like(m)
    want[0] = 255
    out["one_sample"] = (m, want)
    return out


# ---------------------------------------------------------------------------------------------- the hysteresis
@pytest.mark.parametrize("shape", ((1, 1, 1), (1, 1, 300), (2, 67, 131), (2, 40, 57)))
def test_the_two_restatements_agree_on_random_fields(shape):
    rng = np.random.default_rng(sum(shape))
    fields = dict(bytes=rng.integers(0, 256, shape, dtype=np.uint8),
                  sparse=np.where(rng.random(shape) < 0.02, 255, rng.integers(0, 60, shape)).astype(np.uint8))
    for (name, m), (lo, hi) in ((f, l) for f in fields.items() for l in LEVELS):
        a, b = kref.hysteresis_dilation(m, lo, hi), kref.hysteresis_flood(m, lo, hi)
        assert np.array_equal(a, b), (name, lo, hi)
        assert set(np.unique(a)) <= {0, 255}
        if hi == 256:
            assert not a.any()
        if hi == 0:
            assert (a == 255).all()
        if lo == hi:
            assert np.array_equal(a == 255, m >= hi)  # no hysteresis: the plain threshold


@pytest.mark.parametrize("name", ("serpentine", "serpentine_cut", "blobs_touch", "blobs_apart", "one_sample"))
def test_the_two_restatements_give_the_constructed_results(name):
    m, want = constructed()[name]
    assert np.array_equal(kref.hysteresis_dilation(m, LO, HI), want)
    assert np.array_equal(kref.hysteresis_flood(m, LO, HI), want)
    if name == "serpentine_cut":
        assert (want == 0).sum() > (m == 0).sum()     # the far part is weak and stays 0
    if name == "one_sample":
        assert not want[1].any() and (m[1] >= LO).all()


def test_set_properties():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 256, (2, 48, 70), dtype=np.uint8)
    m[rng.random(m.shape) < 0.5] //= 4
    f = kref.hysteresis_dilation
    for lo, hi in ((10, 28), (40, 200), (1, 255), (60, 61)):
        on = f(m, lo, hi) == 255
        assert (on <= (m >= lo)).all() and (on >= (m >= hi)).all()                   # between the two plain thresholds
        assert np.array_equal(f(np.where(on, 255, 0).astype(np.uint8), lo, hi) == 255, on)                  # idempotent on its own output
        again = np.where(on, m, 0).astype(np.uint8)
        assert np.array_equal(f(again, lo, hi) == 255, on)                           # idempotent: the unreached pixels removed, the same set
        if lo > 0:
            assert (f(m, lo - 1, hi) == 255)[on].all()                               # monotone in lo: a lower lo reaches no less
        assert ((f(m, lo + 1, hi) == 255) <= on).all() if lo < hi else True
        if hi > lo:
            assert (f(m, lo, hi - 1) == 255)[on].all()                               # monotone in hi: a lower hi seeds no less
        if hi < 256:
            assert ((f(m, lo, hi + 1) == 255) <= on).all()


# ---------------------------------------------------------------------------------------------- the metric
def test_metric_identities():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    assert not kref.change_metric(a, a).any()                                        # equal inputs
    for k in (1, 7, 100):
        base = rng.integers(100, 150, (1, 6, 8, 3), dtype=np.uint8)
        assert (kref.change_metric(base + k, base) == k).all() and (kref.change_metric(base - k, base) == k).all()      # a constant difference, either sign
    z = np.zeros((1, 7, 7, 4), np.uint8)
    assert (kref.change_metric(np.full_like(z, 255), z) == 255).all()                # the range's top: (16 * 255 + 8) >> 4
    for v in (1, 3, 4, 255):
        imp = z.copy()
        imp[0, 3, 3, 2] = v                           # a one-pixel impulse in one channel: the stencil times v, divided by 16 and rounded
        want = np.zeros((7, 7), np.int64)
        want[2:5, 2:5] = (np.array(kref.STENCIL) * v + 8) >> 4
        assert np.array_equal(kref.change_metric(imp, z)[0], want) and np.array_equal(kref.change_metric(z, imp)[0], want)
    corner = z.copy()
    corner[0, 0, 0, 0] = 160                          # at the corner the clamped indices fold the stencil: (4 + 2 + 2 + 1) / 16 of it
    assert kref.change_metric(corner, z)[0, 0, 0] == (9 * 160 + 8) >> 4 and kref.change_metric(corner, z)[0, 1, 1] == 10
    one = rng.integers(0, 256, (1, 1, 1, 1), dtype=np.uint8)
    assert kref.change_metric(one, np.zeros_like(one))[0, 0, 0] == one[0, 0, 0, 0]   # a single pixel is its own neighbourhood


# ---------------------------------------------------------------------------------------------- the configuration and the host arithmetic
def test_keyed_cfg_defaults_and_refusals():
    full = dict(lo=10, hi=28, dilate=6, feather=2, noise=3.0, ring=24, min_pixels=256)
    assert pb.keyed_cfg(True) == full == kref.DEFAULTS == pb.keyed_cfg({}) == pb.keyed_cfg(dict(lo=None))
    assert pb.keyed_cfg(dict(lo=0, hi=0, noise=0)) == dict(full, lo=0, hi=0, noise=0.0)
    assert pb.keyed_cfg(dict(hi=256, dilate=255, feather=85)) == dict(full, hi=256, dilate=255, feather=85)
    assert pb.keyed_cfg(dict(dilate=0, feather=0))["dilate"] == 0
    for bad, match in ((dict(dilate=5), "dilate"), (dict(feather=3), "dilate"), (dict(dilate=256, feather=2), "dilate"), (dict(feather=-1), "dilate"),
                       (dict(lo=29), "lo and hi"), (dict(lo=40, hi=39), "lo and hi"), (dict(lo=-1), "lo and hi"), (dict(hi=257), "lo and hi"),
                       (dict(lo=2.5), "lo must be an integer"), (dict(hi=True), "hi must be an integer"), (dict(noise=-1), "noise"),
                       (dict(noise=65), "noise"), (dict(noise=float("nan")), "noise"), (dict(ring=0), "ring"), (dict(min_pixels=0), "min_pixels"),
                       (dict(low=3), r"unknown keys \['low'\]"), (dict(lo=1, sigma=2), r"unknown keys \['sigma'\]"), (7, "True or a dict")):
        with pytest.raises(ValueError, match="keyed: .*" + match):
            pb.keyed_cfg(bad)
        with pytest.raises(ValueError, match="paste_back: .*keyed"):
            bd._paste_back_cfg(dict(keyed=bad))
    assert bd._paste_back_cfg(dict(keyed=True)) == dict(dilate=16, feather=4, region=None, keyed=full)
    assert bd._paste_back_cfg(dict(per_line=True, keyed=dict(hi=40), curve=True, seamless=True, grain=True))["keyed"] == dict(full, hi=40)
    assert bd._paste_back_cfg(dict(keyed=None)) == bd._paste_back_cfg(dict(keyed=False)) == bd._paste_back_cfg({}) == dict(dilate=16, feather=4, region=None)
    with pytest.raises(ValueError, match="unknown keys"):
        bd._paste_back_cfg(dict(key=True))


def test_levels_and_sigma_are_the_restatement():
    for cfg in (True, dict(lo=0, hi=0), dict(lo=5, hi=250), dict(noise=0), dict(noise=64.0), dict(lo=256, hi=256)):
        plain = None if cfg is True else cfg
        for sigma in (0.0, 0.1, 3.3, 10 / 3, 4.0, 50.0, 118.4):
            got = pb.keyed_levels(cfg, sigma)
            assert got == kref.levels(plain, sigma) and 0 <= got[0] <= got[1] <= 256
    assert pb.keyed_levels(True, 0.0) == (10, 28) and pb.keyed_levels(True, 3.0) == (10, 28)        # ceil(9) stays below lo
    assert pb.keyed_levels(True, 4.0) == (12, 30) and pb.keyed_levels(True, 4.01) == (13, 31)       # lo_eff = ceil(3 sigma), hi follows
    assert pb.keyed_levels(dict(lo=0, hi=0), 2.0) == (6, 6) and pb.keyed_levels(dict(lo=0, hi=0, noise=0), 2.0) == (0, 0)
    assert pb.keyed_levels(dict(hi=250), 50.0) == (150, 256) and pb.keyed_levels(dict(noise=64), 50.0) == (256, 256)
    hist = np.zeros((3, 3, 1024), np.int64)
    hist[0, :, 20], hist[0, 1, 20], hist[0, 1, 50] = 300, 0, 300      # sample 0: channel 1 is the noisiest
    hist[1, :, 30] = 255                              # sample 1: one pixel short of min_pixels
    hist[2, :, 0] = 1000                              # sample 2: a flat ring
    got = pb.keyed_sigma(hist)
    assert np.allclose(got, [50 * 1.4826 / math.sqrt(164), 0.0, 0.0], rtol=0, atol=1e-12)
    assert pb.keyed_sigma(hist, dict(min_pixels=255))[1] == 30 * pb.GRAIN_K


# ---------------------------------------------------------------------------------------------- what a pipeline is handed
class Recorder:
    """A pipeline stand-in whose paste returns the window unchanged and records its keyword arguments."""

    def __init__(self):
        self.pastes = []

    def paste_back(self, original, edited, mask, dilate=None, feather=None, **kw):
        self.pastes.append(kw)
        return np.array(original)


def _works():
    rng = np.random.default_rng(1)
    scene = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    mask = np.zeros((40, 60, 3), np.uint8)
    mask[10:14, 8:30] = 255
    mask[26:30, 20:50] = 255
    regs = (pb.Region(0, 0, 40, 24, 40, 24), pb.Region(10, 16, 60, 40, 50, 24))
    works = [bd.Work(0, None, None, "", {}, (r.tw, r.th), orig_scene=scene, orig_mask=mask, region=r, parent=0, line=k) for k, r in enumerate(regs)]
    return scene, works, [np.zeros((r.th, r.tw, 3), np.uint8) for r in regs]


@pytest.mark.parametrize("keyed", (True, dict(lo=4, hi=9, noise=0)))
@pytest.mark.parametrize("others", ({}, dict(color_match=True), dict(seamless=True, grain=True)))
def test_compose_lines_and_the_driver_pass_the_key_exactly_when_configured(keyed, others):
    scene, works, crops = _works()
    base = dict(per_line=True, dilate=2, feather=1, **others)
    cfg0, cfg1 = bd._paste_back_cfg(base), bd._paste_back_cfg(dict(base, keyed=keyed))
    p0, p1 = Recorder(), Recorder()
    pl.compose_lines(p0, works, crops, cfg0)
    out = pl.compose_lines(p1, works, crops, cfg1)
    assert np.array_equal(np.array(out), scene) and len(p0.pastes) == len(p1.pastes) == 2
    for w, k0, k1 in zip(works, p0.pastes, p1.pastes):
        assert "keyed" not in k0 and set(k1) == set(k0) | {"keyed", "color_ref"}
        r = w.region
        assert k1["keyed"] == pb.keyed_cfg(keyed) and np.array_equal(k1["color_ref"], scene[r.y0:r.y1, r.x0:r.x1])
        assert all(k1[k] is k0[k] or k1[k] == k0[k] for k in k0 if k != "color_ref")
    q0, q1 = Recorder(), Recorder()
    bd._paste_into_original(q0, works[1], crops[1], cfg0)
    bd._paste_into_original(q1, works[1], crops[1], cfg1)
    assert "keyed" not in q0.pastes[0] and q1.pastes[0] == dict(q0.pastes[0], keyed=pb.keyed_cfg(keyed))


def test_the_pipeline_method_hands_the_key_on_only_when_given(monkeypatch):
    from textflux_amd.pipeline import FluxFillPipeline
    assert inspect.signature(pb.paste).parameters["keyed"].default is None
    assert inspect.signature(FluxFillPipeline.paste_back).parameters["keyed"].default is None
    calls = []
    monkeypatch.setattr(pb, "paste", lambda original, edited, mask, dilate, feather, **kw: (calls.append(kw), original)[1])
    me = types.SimpleNamespace(_execution_device="cpu")
    img, m = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)
    FluxFillPipeline.paste_back(me, img, img, m)
    FluxFillPipeline.paste_back(me, img, img, m, keyed=dict(hi=30))
    FluxFillPipeline.paste_back(me, img, img, m, keyed=True, color_ref=img, grain=True)
    assert calls[0] == {} and calls[1] == dict(keyed=dict(hi=30))
    assert set(calls[2]) == {"keyed", "grain", "origin", "color_match", "color_ref"} and calls[2]["keyed"] is True and calls[2]["color_match"] is None


def test_paste_refuses_before_it_launches_and_has_no_cpu_path():
    from textflux_amd import ops
    img, m = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="keyed: unknown keys"):
        pb.paste(img, img, m, keyed=dict(sigma=1))
    with pytest.raises(ValueError, match="keyed: .*dilate"):
        pb.paste(img, img, m, keyed=dict(dilate=2, feather=1))
    for call in (lambda: ops.change_metric(img, img), lambda: ops.hysteresis(m, 1, 2), lambda: pb.change_key(img, img),
                 lambda: pb.paste(img, img, m, keyed=True, color_ref=img)):          # color_ref is allowed with the key
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


def test_ops_wrappers_check_before_they_launch(monkeypatch):
    from textflux_amd import ops
    monkeypatch.setattr(ops, "_chk_dev", lambda *a: None)
    monkeypatch.setattr(ops.L, "lib", lambda: pytest.fail("a refused call reached the library"))
    img, m = torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8)
    for bad in (dict(a=img.float()), dict(b=img[:1]), dict(a=img.permute(0, 2, 1, 3)), dict(a=torch.zeros(2, 4, 4, 5, dtype=torch.uint8)),
                dict(a=img[0]), dict(out=m[:1]), dict(out=m.float()), dict(out=torch.zeros(2, 4, 4, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="change_metric"):
            ops.change_metric(**dict(dict(a=img, b=img), **bad))
    for bad in (dict(m=m.float()), dict(m=m[0]), dict(m=m[:, :, ::2]), dict(m=m[:0]), dict(lo=-1), dict(hi=257), dict(lo=5, hi=4), dict(lo=1.5)):
        with pytest.raises(ValueError, match="hysteresis"):
            ops.hysteresis(**dict(dict(m=m, lo=1, hi=2), **bad))


# ---------------------------------------------------------------------------------------------- the batch driver
class PasteStub(Stub):
    def paste_back(self, original, edited, mask, dilate=None, feather=None, **kw):
        self.pastes.append(kw)
        return np.full((1,) + original.shape, 7, np.uint8)


def _run(pipe, **kw):
    saved = {}
    res = bd.run_items(ITEMS, pipe, None, batch_size=4, num_inference_steps=2, device="cpu", loader=_loader,
                       save=lambda i, im: saved.__setitem__(i, np.array(im)), **kw)
    return res, saved


def test_run_items_accepts_the_key_on_the_stub_pipeline():
    pipe = PasteStub()
    res, saved = _run(pipe, paste_back=dict(keyed=dict(lo=3, hi=30)))
    assert res["all_done"] == [0, 1] and len(pipe.pastes) == 2
    assert all(k == dict(keyed=pb.keyed_cfg(dict(lo=3, hi=30))) for k in pipe.pastes) and (saved[0] == 7).all()
    pipe = PasteStub()
    _run(pipe, paste_back=dict(keyed=True, grain=dict(seed=1), region={}))
    assert all(set(k) == {"keyed", "grain", "origin"} and k["keyed"] == pb.keyed_cfg(True) for k in pipe.pastes)
    pipe = PasteStub()
    _run(pipe, paste_back={})
    assert pipe.pastes == [{}, {}]                                                    # without the key: the call as it was
    with pytest.raises(ValueError, match="paste_back: keyed: unknown keys"):
        _run(PasteStub(), paste_back=dict(keyed=dict(high=3)))
    with pytest.raises(ValueError, match="paste_back: keyed: .*dilate"):
        _run(PasteStub(), paste_back=dict(keyed=dict(dilate=4, feather=2)))
    with pytest.raises(TypeError):
        _run(PasteStub(), keyed=True)                                                 # it is a key of paste_back, not an argument of its own
    assert "keyed" not in inspect.signature(bd.run_items).parameters


# ---------------------------------------------------------------------------------------------- the CLIs
def test_clis_carry_the_flags():
    sys.path.insert(0, REPO), sys.path.insert(0, os.path.join(REPO, "scripts"))
    ri, rl, re_ = (importlib.import_module(n) for n in ("run_inference", "run_inference_lora", "run_eval"))
    single = ["--image", "i", "--mask", "m", "--words", "w"]
    flags = lambda a: (a.paste_keyed, a.paste_keyed_lo, a.paste_keyed_hi, a.paste_keyed_dilate, a.paste_keyed_feather, a.paste_keyed_noise)
    for parser, base in ((ri.build_parser(), single), (rl.build_parser(), single),
                         (re_.build_parser(), ["--json_path", "j"]), (re_.build_parser(lora=True), ["--json_path", "j"])):
        assert flags(parser.parse_args(base)) == (False, None, None, None, None, None)
        a = parser.parse_args(base + ["--paste_back", "--paste_keyed", "--paste_keyed_lo", "4", "--paste_keyed_hi", "40", "--paste_keyed_dilate", "9",
                                      "--paste_keyed_feather", "3", "--paste_keyed_noise", "2.5"])
        assert flags(a) == (True, 4, 40, 9, 3, 2.5)
    parse = lambda extra: ri.paste_back_from_args(ri.build_parser().parse_args(single + extra))
    assert parse(["--paste_back"]) == dict(dilate=16, feather=4, region=None)          # without the new flags: the dict it was
    assert parse(["--paste_back", "--paste_keyed"]) == dict(dilate=16, feather=4, region=None, keyed=True)
    assert parse(["--paste_back", "--paste_keyed_hi", "40"])["keyed"] == dict(hi=40)
    assert parse(["--paste_back", "--paste_keyed_lo", "0", "--paste_keyed_noise", "0"])["keyed"] == dict(lo=0, noise=0.0)
    assert parse(["--paste_back", "--paste_per_line", "--paste_curve", "--paste_seamless", "--paste_grain", "--paste_keyed_dilate", "7"])["keyed"] == dict(dilate=7)
    assert bd._paste_back_cfg(parse(["--paste_back", "--paste_keyed_feather", "1"]))["keyed"] == dict(kref.DEFAULTS, feather=1)
    # the flags reach run_items: the lora CLI uses the function above, the two eval CLIs build the same dict in their common main
    src = inspect.getsource(re_.main)                 # one main serves both eval CLIs
    assert 'paste_back["keyed"] = values or True' in src and "paste_back=paste_back" in src
    assert "base.paste_back_from_args(a)" in inspect.getsource(rl)
    for flag in (["--paste_keyed"], ["--paste_keyed_lo", "0"], ["--paste_keyed_hi", "40"], ["--paste_keyed_dilate", "6"], ["--paste_keyed_feather", "0"],
                 ["--paste_keyed_noise", "0"]):
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


NAMES = ("tfx_change_metric_u8", "tfx_hysteresis_workspace_bytes", "tfx_hysteresis_u8")


def test_symbols_are_declared_bound_exported_and_the_abi_version_stays(lib):
    from textflux_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in NAMES:
        assert sym in L.SIGNATURES and hasattr(lib, sym) and re.search(r"\b" + sym + r"\s*\(", code)
    assert "int tfx_change_metric_u8(const void* a, const void* b, void* out, int32_t B, int32_t H, int32_t W, int32_t C, tfx_stream stream);" in code
    assert "int64_t tfx_hysteresis_workspace_bytes(int32_t B, int32_t H, int32_t W);" in code
    assert "int tfx_hysteresis_u8(const void* m, void* out, int32_t lo, int32_t hi, void* workspace, int64_t workspace_bytes, int32_t* rounds, int32_t B," in code
    assert [len(L.SIGNATURES[s][1]) for s in NAMES] == [8, 3, 11]
    assert L.ABI_VERSION == L.header_abi_version()
    text = " ".join(hdr.split())
    for phrase in ("SYNCHRONISES `stream` ONCE PER ROUND", "REFUSED, with tfx_last_error, ON A CAPTURING STREAM", "8-connected",
                   "final == orig wherever key == 0", "min(orig, result) <= final <= max(orig, result)", "(|s_c| + 8) >> 4"):
        assert phrase in text, phrase


def test_entry_points_check_their_arguments(lib):
    p = [k << 20 for k in range(1, 5)]               # never dereferenced: every call is refused

    def metric(ptrs=p, dims=(2, 8, 8, 3)):
        return lib.tfx_change_metric_u8(ptrs[0], ptrs[1], ptrs[2], *dims, None)

    def hyst(ptrs=p, lo=10, hi=28, ws=64, dims=(2, 8, 8)):
        return lib.tfx_hysteresis_u8(ptrs[0], ptrs[1], lo, hi, ptrs[2], ws, None, *dims, None)
    for k in range(3):
        assert metric(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_change_metric_u8: null pointer" in lib.tfx_last_error()
        assert hyst(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_hysteresis_u8: null pointer" in lib.tfx_last_error()
    for c in (0, 5):
        assert metric(dims=(2, 8, 8, c)) != 0 and b"1..4 channels" in lib.tfx_last_error()
    for k in range(3):
        dims = [2, 8, 8]
        dims[k] = 0
        assert metric(dims=tuple(dims) + (3,)) != 0 and b"at least 1" in lib.tfx_last_error()
        assert hyst(dims=tuple(dims)) != 0 and b"at least 1" in lib.tfx_last_error()
        assert lib.tfx_hysteresis_workspace_bytes(*dims) == -1
    assert metric(dims=(65536, 8, 8, 3)) != 0 and hyst(dims=(65536, 8, 8)) != 0 and b"65535" in lib.tfx_last_error()
    for k in (0, 1):
        assert metric([p[0], p[1], p[k]]) != 0 and b"alias" in lib.tfx_last_error()
    for lo, hi in ((-1, 5), (6, 5), (0, 257)):
        assert hyst(lo=lo, hi=hi) != 0 and b"0 <= lo <= hi <= 256" in lib.tfx_last_error()
    need = lib.tfx_hysteresis_workspace_bytes(2, 8, 8)
    assert need >= 4 and need == lib.tfx_hysteresis_workspace_bytes(1, 4000, 4000)
    assert hyst(ws=need - 1) != 0 and b"workspace" in lib.tfx_last_error()
    assert hyst([p[0], p[1], p[2] + 2]) != 0 and b"4-byte aligned" in lib.tfx_last_error()
    for ptrs in ([p[0], p[0], p[2]], [p[0], p[1], p[0]], [p[0], p[1], p[1]]):
        assert hyst(ptrs) != 0 and b"different buffers" in lib.tfx_last_error()
