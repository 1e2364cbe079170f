"""Keyed paste on the GPU (DESIGN.md section 4 "Keyed paste"): ops.change_metric and ops.hysteresis (imageops.hip: change_metric_kernel,
hysteresis_kernel) and paste_back.paste(keyed=...) against the numpy restatement in tests/helpers/keyed_ref.py, bit for bit (integer
arithmetic only; the host arithmetic is float64 on exact integers), the exact guarantees asserted directly, and
batch_driver.run_items(per_line=True, keyed=...) end to end on the tiny synthetic checkpoint of the e2e tests."""
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import grain_ref as gref
from tests.helpers import keyed_ref as kref
from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref
from tests.test_keyed_paste_cpu import HI, LEVELS, LO, constructed

pytestmark = pytest.mark.gpu
# a single pixel; one row over five tiles of 64; two samples of several tiles with a rest on both axes; the constructed fields' size
SHAPES = ((1, 1, 1, 1), (1, 1, 300, 3), (2, 67, 131, 3), (2, 130, 257, 4))


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def _dev(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays)


# ---------------------------------------------------------------------------------------------- ops.change_metric
@pytest.mark.parametrize("shape", SHAPES)
def test_change_metric_is_the_restatement_exactly(ops, shape):
    rng = np.random.default_rng(sum(shape))
    a, b = (rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(2))        # random bytes: both signs, and the clamped borders
    want = kref.change_metric(a, b)
    ad, bd = _dev(a, b)
    got = ops.change_metric(ad, bd)
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape[:3] and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.change_metric(bd, ad).cpu().numpy(), want)          # symmetric
    assert np.array_equal(ad.cpu().numpy(), a) and np.array_equal(bd.cpu().numpy(), b)
    out = torch.full(shape[:3], 7, dtype=torch.uint8, device="cuda")
    assert ops.change_metric(ad, bd, out=out).data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)
    assert int(ops.change_metric(ad, ad).max()) == 0                              # equal inputs
    k = 37
    base = rng.integers(40, 200, shape, dtype=np.uint8)
    assert bool((ops.change_metric(*_dev(base + k, base)) == k).all()) and bool((ops.change_metric(*_dev(base, base + k)) == k).all())
    with pytest.raises(RuntimeError, match="alias"):
        ops.change_metric(ad, bd, out=ad.view(-1)[:got.numel()].view(got.shape))


# ---------------------------------------------------------------------------------------------- ops.hysteresis
def _fields(rng, shape):
    """Random bytes (at (10, 28) nearly everything joins), and a field of weak pixels with few seeds, where the paths matter."""
    return dict(bytes=rng.integers(0, 256, shape, dtype=np.uint8),
                sparse=np.where(rng.random(shape) < 0.004, 255, np.where(rng.random(shape) < 0.45, 20, 0)).astype(np.uint8))


@pytest.mark.parametrize("shape", [s[:3] for s in SHAPES])
def test_hysteresis_is_the_restatement_on_random_fields(ops, shape):
    rng = np.random.default_rng(10 + sum(shape))
    for name, m in _fields(rng, shape).items():
        md = _dev(m)[0]
        for lo, hi in LEVELS:
            want = kref.hysteresis_flood(m, lo, hi)
            got, rounds = ops.hysteresis(md, lo, hi, rounds=True)
            print(f"{shape} {name} ({lo}, {hi}): {rounds} rounds, {int((want == 255).sum())} of {want.size} on")
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (name, lo, hi)
            assert rounds >= 1 and torch.equal(ops.hysteresis(md, lo, hi), got)
            if hi == 256:
                assert int(got.max()) == 0
            if hi == 0:
                assert int(got.min()) == 255
            if name == "sparse" and (lo, hi) == (10, 28) and shape[1] > 1:           # strictly between the two plain thresholds: the paths matter
                assert not np.array_equal(want == 255, m >= hi) and not np.array_equal(want == 255, m >= lo)
        assert np.array_equal(md.cpu().numpy(), m)                                # the input is untouched


@pytest.mark.parametrize("name", ("serpentine", "serpentine_cut", "blobs_touch", "blobs_apart", "one_sample"))
def test_hysteresis_on_the_constructed_fields(ops, name):
    """The expected results are written down by hand (tests/test_keyed_paste_cpu.py: constructed) and both restatements give them."""
    m, want = constructed()[name]
    got, rounds = ops.hysteresis(_dev(m)[0], LO, HI, rounds=True)
    print(f"{name}: {rounds} rounds")
    assert rounds >= 1 and np.array_equal(got.cpu().numpy(), want)
    if name in ("serpentine", "serpentine_cut"):
        assert rounds >= 2                             # several tiles and a seed: the round that marks it is followed by one that confirms
    if name == "one_sample":
        assert int(got[1].max()) == 0 and int(got[0].min()) == 255


def test_hysteresis_is_refused_on_a_capturing_stream(ops):
    """The call reads a word back after every round, so it cannot be captured: on a capturing stream it is refused before anything is
    launched.  The capture is begun and ended through the HIP runtime the process has loaded; the buffers are made before it begins."""
    import ctypes as C
    from textflux_amd import _lib as L
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    m = torch.zeros(1, 40, 80, dtype=torch.uint8, device="cuda")
    out, ws = torch.full_like(m, 9), torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stream, graph, rounds = C.c_void_p(), C.c_void_p(), C.c_int32(-1)
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        assert hip.hipStreamBeginCapture(stream, 2) == 0                          # hipStreamCaptureModeRelaxed
        try:
            rc = L.lib().tfx_hysteresis_u8(m.data_ptr(), out.data_ptr(), 1, 2, ws.data_ptr(), 64, C.byref(rounds), 1, 40, 80, stream)
            err = L.lib().tfx_last_error()
        finally:
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
            if graph.value:
                hip.hipGraphDestroy(graph)
    finally:
        hip.hipStreamDestroy(stream)
    assert rc != 0 and b"capturing" in err and rounds.value == -1
    torch.cuda.synchronize()
    assert int(out.min()) == int(out.max()) == 9                                  # nothing was written
    got, n = ops.hysteresis(m, 1, 2, rounds=True)                                 # and the same call outside a capture is served
    assert n == 1 and int(got.max()) == 0


# ---------------------------------------------------------------------------------------------- paste(keyed=...)
D, R = 8, 2
HW = (96, 160)
KEYED = dict(ring=12, min_pixels=64)
GRAIN = dict(ring=12, seed=3, min_pixels=64)
COLOR = dict(ring=20, min_pixels=16)
SEAMLESS = dict(smooth=3, max_shift=12)
BOX = (36, 60, 50, 110)                               # the mask: rows 36..59, columns 50..109
# y0, y1, x0, x1: drawn at the left, columns 90 and up stay background; apart, so that no 3 x 3 neighbourhood sees a dark and a bright stroke cancel
STROKES = ((40, 56, 54, 57), (40, 43, 62, 76), (52, 56, 62, 76))


def _scene(noisy: bool):
    """A colour ramp in flat bands of ten columns (more than half of the pixels have no high-pass residual at all, so the noise estimate
    is exactly 0), clean or with the restatement's grain of standard deviation 4 (a photo with sensor noise)."""
    h, w = HW
    ramp = (70 + 6 * (np.arange(w) // 10))[None, None, :, None] + np.array([0, 8, -12])
    flat = np.ascontiguousarray(np.broadcast_to(ramp, (1, h, w, 3))).astype(np.uint8)
    if not noisy:
        return flat
    gain = np.full((1, 3), math.floor(4.0 / gref.SIGMA0 * 65536 + 0.5))
    return gref.grain(flat, np.full((1, h, w), 255, np.uint8), gain, (40, 30), 21)


@pytest.fixture(scope="module")
def cases():
    """name -> (orig, edit, grey): the synthetic edit is the CLEAN ramp plus a few drawn strokes plus noise of +-2."""
    rng = np.random.default_rng(3)
    edit = _scene(False).astype(np.int64)
    for k, (y0, y1, x0, x1) in enumerate(STROKES):
        edit[0, y0:y1, x0:x1] = (20, 235, 30)[k]
    edit = np.clip(edit + rng.integers(-2, 3, edit.shape), 0, 255).astype(np.uint8)
    grey = np.zeros((1,) + HW, np.uint8)
    grey[0, BOX[0]:BOX[1], BOX[2]:BOX[3]] = 255
    out = dict(clean=(_scene(False), edit, grey), noisy=(_scene(True), edit, grey))
    for arrays in out.values():
        for a in arrays:
            a.setflags(write=False)
    return out


def _stroke_mask():
    s = np.zeros((1,) + HW, bool)
    for y0, y1, x0, x1 in STROKES:
        s[0, y0:y1, x0:x1] = True
    return s


@pytest.mark.parametrize("scene,options", [("clean", ()), ("clean", ("color_match",)), ("clean", ("seamless",)), ("noisy", ()), ("noisy", ("grain",)),
                                           ("noisy", ("color_match", "seamless", "grain"))])
def test_paste_is_the_restatement_and_keeps_its_guarantees(ops, cases, scene, options):
    from textflux_amd import paste_back as pb
    orig, edit, grey = cases[scene]
    given = dict(color_match=COLOR, seamless=SEAMLESS, grain=GRAIN)
    kw = {k: given[k] for k in options}
    full = dict(color_match=pb.color_match_cfg(COLOR) if "color_match" in options else None,
                seamless=pb.seamless_cfg(SEAMLESS) if "seamless" in options else None, grain=pb.grain_cfg(GRAIN) if "grain" in options else None)
    if "grain" in options:
        kw["origin"] = (40, 30)
    od, ed, gd = _dev(orig, edit, grey)
    want, key, result = kref.paste(orig, edit, grey, D, R, keyed=KEYED, origin=(40, 30), **full)
    got = pb.paste(od, ed, gd, D, R, keyed=KEYED, **kw).cpu().numpy()
    plain = pb.paste(od, ed, gd, D, R, **kw).cpu().numpy()
    alpha = ref.alpha_mask(grey, D, R)
    m = kref.change_metric(result, orig)
    sigma = kref.scene_sigma(orig, plref.ring_mask(alpha, KEYED["ring"]), KEYED)
    lo_eff, hi_eff = kref.levels(KEYED, float(sigma[0]))
    print(f"{scene} {options}: sigma {sigma[0]:.3f}, levels ({lo_eff}, {hi_eff}), key 0 on {int((key == 0).sum())}, 255 on {int((key == 255).sum())} pixels; "
          f"inside the mask {int(((key == 0) & (grey >= 128)).sum())} keep the scene's byte")
    assert np.array_equal(got, want)
    assert np.array_equal(od.cpu().numpy(), orig) and np.array_equal(ed.cpu().numpy(), edit)         # the inputs are untouched
    assert (sigma[0] == 0) == (scene == "clean") and (lo_eff > 10) == (scene == "noisy")
    # final == original wherever key == 0: in particular on the background inside the mask, where the plain paste carries the edit's noise
    kept = (key == 0) & (grey >= 128)
    assert kept[0, BOX[0]:BOX[1], 100:BOX[3]].all() and np.array_equal(got[kept], orig[kept]) and not np.array_equal(plain[kept], orig[kept])
    assert np.array_equal(got[key == 0], orig[key == 0])
    # bytes outside the grown mask are untouched, whatever the key holds
    outside = ref.dilate(grey, D + 3 * R) == 0
    assert outside.any() and np.array_equal(got[outside], orig[outside])
    # every pixel with m >= hi_eff has key = 255; the strokes are such pixels; without grain they carry the blend's bytes
    strokes = _stroke_mask()
    assert (m[strokes] >= hi_eff).all() and (key[m >= hi_eff] == 255).all()
    if "grain" not in options:
        assert np.array_equal(result, plain)
        assert np.array_equal(got[key == 255], result[key == 255]) and np.array_equal(got[strokes], plain[strokes])
        lo_, hi_ = np.minimum(orig, result), np.maximum(orig, result)
        assert (got >= lo_).all() and (got <= hi_).all()
    assert not np.array_equal(got, plain) and not np.array_equal(got, orig)      # the key does something, and so does the edit
    # hi_eff = 0 reproduces the unkeyed call: lo = hi = 0 on a ring without noise, lo = hi = noise = 0 on any
    if scene == "clean":
        assert np.array_equal(pb.paste(od, ed, gd, D, R, keyed=dict(KEYED, lo=0, hi=0), **kw).cpu().numpy(), plain)
    assert np.array_equal(pb.paste(od, ed, gd, D, R, keyed=dict(KEYED, lo=0, hi=0, noise=0), **kw).cpu().numpy(), plain)
    # hi = 256: nothing is keyed, the scene stays
    assert np.array_equal(pb.paste(od, ed, gd, D, R, keyed=dict(KEYED, lo=256, hi=256), **kw).cpu().numpy(), orig)


def test_two_samples_with_their_own_levels_and_change_key(ops, cases):
    """A clean and a noisy scene in one call: every sample gets its own thresholds (one hysteresis call per sample).  A faint bar, 34
    grey levels off the scene, is a change on the clean scene (hi_eff = 28) and none on the noisy one, whose thresholds noise = 6 lifts
    to (26, 44): there the bar's metric is 34 plus the smoothed noise, whose deviation is 4.3 * 6 / 16 = 1.6."""
    from textflux_amd import paste_back as pb
    cfg = dict(KEYED, noise=6.0)
    orig = np.concatenate([cases["clean"][0], cases["noisy"][0]])
    edit = np.array(cases["clean"][1])
    edit[0, 44:52, 94:102] += 34
    edit, grey = np.concatenate([edit] * 2), np.concatenate([cases["clean"][2]] * 2)
    want, key, result = kref.paste(orig, edit, grey, D, R, keyed=cfg)
    od, ed, gd = _dev(orig, edit, grey)
    assert np.array_equal(pb.paste(od, ed, gd, D, R, keyed=cfg).cpu().numpy(), want)
    assert (key[0, 44:52, 94:102] == 255).all() and (key[1, 44:52, 94:102] == 0).all()
    assert np.array_equal(want[0, 44:52, 94:102], edit[0, 44:52, 94:102]) and np.array_equal(want[1, 44:52, 94:102], orig[1, 44:52, 94:102])
    assert (key[:, 40:56, 54:57] == 255).all()        # the strong strokes are keyed in both
    rd = _dev(result)[0]
    for sigma in (None, 0.0, 4.0, np.array([0.0, 4.0])):
        assert np.array_equal(pb.change_key(od, rd, KEYED, sigma).cpu().numpy(), kref.change_key(orig, result, KEYED, sigma)), sigma
        assert np.array_equal(kref.change_key(orig, result, KEYED, sigma), kref.change_key(orig, result, KEYED, sigma, hysteresis=kref.hysteresis_flood))


# ---------------------------------------------------------------------------------------------- end to end, through run_items
REGION = dict(pad=0.0, min_side=96)


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_keyed"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def test_end_to_end_two_lines(pipe, monkeypatch):
    """The synthetic two-line case with and without the key.  Outside the lines' grown masks, where alone a key can act, the keyed run is
    the plain run (both are the scene); wherever every key that covers a pixel is 0, the keyed run is the scene; and the keyed run is
    the restated composition of what the pipeline was handed, line by line."""
    from textflux_amd import batch_driver, glyph
    from textflux_amd import paste_back as pb
    from textflux_amd import per_line as pl
    scene, mask, words = glyph.synthetic_case(384, 256, multiline=True)
    item = dict(image=scene, mask=mask, text="\n".join(words))
    sc = np.array(scene)
    lines = pl.split_lines(mask, words)
    assert len(lines) == 2
    grown = np.zeros(sc.shape[:2], bool)
    for _, _, lm in lines:
        grown |= ref.dilate(np.where(lm[:, :, 0] >= 128, 255, 0).astype(np.uint8), D + 3 * R) > 0
    keyed = dict(lo=120, hi=150, noise=0)             # the scene is white noise: its own level would lift the thresholds out of reach
    keys = []
    real_key = pb.change_key
    monkeypatch.setattr(pb, "change_key", lambda *a, **k: (keys.append(real_key(*a, **k)), keys[-1])[1])
    outs = {}
    for name, kd in (("plain", None), ("keyed", keyed)):
        saved, pastes = {}, []
        real = pipe.paste_back
        pipe.paste_back = lambda o_, e, m, **k: (pastes.append(dict(k, original=np.array(o_), edited=np.array(e), mask=np.array(m))), real(o_, e, m, **k))[1]
        try:
            cfg = dict(per_line=True, dilate=D, feather=R, region=REGION, **({} if kd is None else dict(keyed=kd)))
            res = batch_driver.run_items([item], pipe, None, batch_size=2, num_inference_steps=2, guidance_scale=30.0, seed=42,
                                         loader=lambda x: x, save=lambda i, im: saved.__setitem__(i, np.array(im)), paste_back=cfg)
        finally:
            del pipe.paste_back
        assert res["all_done"] == [0] and not res["failed"] and len(pastes) == 2
        assert all(("keyed" in k) == (kd is not None) and ("color_ref" in k) == (kd is not None) for k in pastes)
        out = outs[name] = saved[0]
        assert out.shape == sc.shape and np.array_equal(out[~grown], sc[~grown])
        works = pl.prepare_lines(0, item, lambda x: x, False, None, batch_driver._paste_back_cfg(cfg))
        want = sc.copy()
        for w, k in zip(works, pastes):
            reg = w.region
            assert np.array_equal(k["original"], want[reg.y0:reg.y1, reg.x0:reg.x1])
            if kd is None:
                pasted = ref.paste(k["original"][None], k["edited"][None], k["mask"][None], D, R)
            else:
                assert k["keyed"] == pb.keyed_cfg(kd) and np.array_equal(k["color_ref"], sc[reg.y0:reg.y1, reg.x0:reg.x1])
                pasted = kref.paste(k["original"][None], k["edited"][None], k["mask"][None], D, R, keyed=k["keyed"], color_ref=k["color_ref"][None])[0]
            want[reg.y0:reg.y1, reg.x0:reg.x1] = pasted[0]
        assert np.array_equal(out, want)
        if kd is None:
            assert not keys                           # without the key nothing of it runs
        else:
            assert len(keys) == 2
            touched = np.zeros(sc.shape[:2], bool)    # where some line's key is not 0
            for w, key in zip(works, keys):
                reg = w.region
                touched[reg.y0:reg.y1, reg.x0:reg.x1] |= key[0].cpu().numpy() > 0
            print(f"keys: {int(touched.sum())} pixels keyed, {int((grown & ~touched).sum())} pixels inside the grown masks keep the scene's byte")
            assert np.array_equal(out[~touched], sc[~touched])
    assert np.array_equal(outs["keyed"][~grown], outs["plain"][~grown]) and not np.array_equal(outs["keyed"], outs["plain"])
