"""Per-line edits on the GPU: the two uint8 kernels of the colour-matched paste (imageops.hip: masked_moments_u8, overlay_lut_u8) and
paste_back.paste(color_match=...) against the restatement in tests/helpers/per_line_ref.py, bit for bit (integer sums, and a float64 fit
on exact integers), and batch_driver.run_items(per_line=True) end to end on the tiny synthetic checkpoint of the e2e tests."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import paste_back_ref as ref
from tests.helpers import per_line_ref as plref

pytestmark = pytest.mark.gpu
# 37 x 53 (1961 pixels: odd, so the byte path, two workgroups), its one-row and one-column forms, and 36 x 52 (a multiple of 4: the
# 32-bit path)
SHAPES = ((37, 53), (1, 53), (37, 1), (36, 52))


@pytest.fixture(scope="module")
def ops():
    from textflux_amd import ops as o
    return o


def _images(h, w, c, seed):
    """B = 2 with DIFFERING samples (a batch-stride slip shows); the weight mixes 0, small and 255 values."""
    rng = np.random.default_rng(seed)
    a, b = (rng.integers(0, 256, (2, h, w, c), dtype=np.uint8) for _ in range(2))
    wt = rng.choice(np.array([0, 0, 1, 128, 255], np.uint8), (2, h, w))
    return a, b, wt


def _offset_by_one(x: torch.Tensor) -> torch.Tensor:
    """The same contiguous tensor at an address that is no multiple of 4."""
    buf = torch.empty(x.numel() + 1, dtype=torch.uint8, device=x.device)
    buf[1:] = x.reshape(-1)
    return buf[1:].view(x.shape)


@pytest.mark.parametrize("hw,c", [(hw, 3) for hw in SHAPES] + [(hw, c) for c in (1, 4, 2) for hw in ((37, 53), (36, 52))])
def test_moments_are_the_restatement_exactly(ops, hw, c):
    a, b, wt = _images(*hw, c, 100 * hw[0] + hw[1] + c)
    want = plref.moments(a, b, wt)
    assert want[0] != want[1] and (plref.moments_np(a, b, wt) == np.array(want, dtype=np.int64)).all()
    da, db, dw = (torch.from_numpy(x).cuda() for x in (a, b, wt))
    got = ops.masked_moments(da, db, dw)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, c, 5)
    assert got.cpu().tolist() == want
    assert ops.masked_moments(_offset_by_one(da), db, _offset_by_one(dw)).cpu().tolist() == want     # unaligned: the byte path, same sums
    assert not bool(ops.masked_moments(da, db, torch.zeros_like(dw)).any())                          # all-zero weight: zeros


def test_moments_keep_64_bits(ops):
    """1024 x 1024 x 3, all 255, full weight: sum a a = 65025 * 2^20 = 6.8e10 does not fit 32 bits; 256 workgroups, each thread walks
    four groups."""
    full = torch.full((1, 1024, 1024, 3), 255, dtype=torch.uint8, device="cuda")
    wt = torch.full((1, 1024, 1024), 255, dtype=torch.uint8, device="cuda")
    n = 1 << 20
    assert ops.masked_moments(full, full, wt).cpu().tolist() == [[[n, 255 * n, 255 * n, 65025 * n, 65025 * n]] * 3]
    wt[0, 512:] = 0
    wt[0, 0, 0] = 0
    half = n // 2 - 1
    assert ops.masked_moments(full, full, wt).cpu().tolist() == [[[half, 255 * half, 255 * half, 65025 * half, 65025 * half]] * 3]


def test_moments_wrapper_refuses_what_it_cannot_serve(ops):
    img, wt = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda"), torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    for bad in ((img.float(), img, wt), (img, img[:, :2], wt), (img, img, wt[:, :2]), (img[..., :0], img[..., :0], wt),
                (img.repeat(1, 1, 1, 2)[..., :5].contiguous(),) * 2 + (wt,)):
        with pytest.raises(ValueError):
            ops.masked_moments(*bad)


@pytest.mark.parametrize("c", [3, 1, 4])
@pytest.mark.parametrize("hw", [(37, 53), (36, 52)])
def test_overlay_lut(ops, hw, c):
    rng = np.random.default_rng(7 * hw[0] + c)
    o, e = (rng.integers(0, 256, (2,) + hw + (c,), dtype=np.uint8) for _ in range(2))
    al = rng.integers(0, 256, (2,) + hw, dtype=np.uint8)
    al[0, :5], al[1, -5:] = 0, 255
    od, ed, ad = (torch.from_numpy(x).cuda() for x in (o, e, al))
    ident = torch.arange(256, dtype=torch.uint8, device="cuda").expand(2, c, 256).contiguous()
    assert torch.equal(ops.overlay_lut(od, ed, ad, ident), ops.overlay(od, ed, ad))                  # the identity table: overlay, bit for bit
    assert torch.equal(ops.overlay_lut(_offset_by_one(od), _offset_by_one(ed), ad, ident), ops.overlay(od, ed, ad))
    lut = rng.integers(0, 256, (2, c, 256), dtype=np.uint8)                                         # the two samples' tables differ
    want = torch.from_numpy(plref.overlay_lut(o, e, al, lut))
    ld = torch.from_numpy(lut).cuda()
    assert torch.equal(ops.overlay_lut(od, ed, ad, ld).cpu(), want) and torch.equal(od.cpu(), torch.from_numpy(o))
    same = ops.overlay_lut(od, ed, ad, ld, out=od)                                                   # out aliases orig
    assert same.data_ptr() == od.data_ptr() and torch.equal(od.cpu(), want)
    with pytest.raises(ValueError):
        ops.overlay_lut(od, ed, ad, ld[:1])
    with pytest.raises(ValueError):
        ops.overlay_lut(od, ed, ad[:1], ld)


def test_ring_mask_is_the_restatement(ops):
    from textflux_amd import paste_back as pb
    alpha = np.zeros((2, 37, 53), np.uint8)
    alpha[0, 10:20, 20:30], alpha[1, 0:3, 50:53], alpha[1, 30, 5] = 255, 7, 1
    for ring in (1, 5, 24, 255):
        got = pb.ring_mask(torch.from_numpy(alpha).cuda(), ring).cpu().numpy()
        assert (got == plref.ring_mask(alpha, ring)).all() and not got[alpha > 0].any() and got.max() == 255


@pytest.mark.parametrize("g,o", plref.DRIFTS)
def test_paste_undoes_a_synthetic_drift(ops, g, o):
    """edit = round(g orig + o) everywhere: the table fitted on the ring takes the edit back to the original to within one level there
    (the restatement's own figure on these inputs: tests/test_per_line_cpu.py), the pasted image is the restatement bit for bit, and
    outside the mask grown by dilate + 3 feather it is the original."""
    from textflux_amd import paste_back as pb
    orig, edit, grey = plref.drift_case(g, o)
    d, r = 9, 3
    od, ed, gd = (torch.from_numpy(x).cuda() for x in (orig, edit, grey))
    alpha = pb.alpha_mask(gd, d, r)
    ring = pb.ring_mask(alpha, pb.RING)
    lut = pb.fit_luts(ops.masked_moments(ed, od, ring))
    want, want_lut, want_ring = plref.paste(orig, edit, grey, d, r)
    assert (ring.cpu().numpy() == want_ring).all() and (lut == want_lut).all()
    on = want_ring[0] != 0
    for c in range(3):
        diff = np.abs(lut[0, c][edit[0, :, :, c][on]].astype(int) - orig[0, :, :, c][on].astype(int))
        print(f"drift ({g}, {o}) channel {c}: max |lut[edit] - orig| on the ring = {diff.max()}")
        assert diff.max() <= 1
    for cm in (True, dict(ring=24, gain=(0.8, 1.25), max_shift=32, min_pixels=256)):
        got = pb.paste(od, ed, gd, d, r, color_match=cm).cpu().numpy()
        assert (got == want).all()
    outside = ref.dilate(grey, d + 3 * r) == 0
    assert outside.any() and (got[outside] == orig[outside]).all()
    if (g, o) != (1.0, 0.0):
        assert (got != pb.paste(od, ed, gd, d, r).cpu().numpy()).any()          # the table is not the identity: the plain paste differs
    # another colour reference moves the fit; too few ring pixels leave the identity table: the plain paste
    ref2 = torch.from_numpy(np.clip(orig.astype(int) + 10, 0, 255).astype(np.uint8)).cuda()
    assert (pb.paste(od, ed, gd, d, r, color_match=True, color_ref=ref2).cpu().numpy() ==
            plref.paste(orig, edit, grey, d, r, color_ref=ref2.cpu().numpy())[0]).all()
    few = pb.paste(od, ed, gd, d, r, color_match=dict(min_pixels=10 ** 6)).cpu().numpy()
    assert (few == ref.paste(orig, edit, grey, d, r)).all()
    with pytest.raises(ValueError):
        pb.paste(od, ed, gd, d, r, color_ref=ref2)


# ---------------------------------------------------------------------------------------------- end to end, through run_items
@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_per_line"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


def test_end_to_end_two_lines(pipe):
    from textflux_amd import batch_driver, glyph
    from textflux_amd import per_line as pl
    scene, mask, words = glyph.synthetic_case(384, 256, multiline=True)
    assert words == ["HELLO", "WORLD"]
    item = dict(image=scene, mask=mask, text="\n".join(words))
    sc, grey = np.array(scene), np.array(mask.convert("L"))
    lines = pl.split_lines(mask, words)
    assert len(lines) == 2
    d, r = 8, 2
    grown = np.zeros(grey.shape, bool)
    for _, _, lm in lines:
        grown |= ref.dilate(np.where(lm[:, :, 0] >= 128, 255, 0).astype(np.uint8), d + 3 * r) > 0
    assert grown.any() and not grown.all()
    outs = {}
    for name, cm in (("plain", None), ("matched", True)):
        saved, pastes = {}, []
        real = pipe.paste_back
        pipe.paste_back = lambda o_, e, m, **k: (pastes.append(k), real(o_, e, m, **k))[1]
        try:
            pb_cfg = dict(per_line=True, dilate=d, feather=r, region=dict(pad=0.0, min_side=96), **({} if cm is None else dict(color_match=cm)))
            res = batch_driver.run_items([item], pipe, None, batch_size=2, num_inference_steps=2, guidance_scale=30.0, seed=42,
                                         loader=lambda x: x, save=lambda i, im: saved.__setitem__(i, np.array(im)), paste_back=pb_cfg)
        finally:
            del pipe.paste_back
        assert res["all_done"] == [0] and not res["failed"] and len(pastes) == 2
        assert all(("color_ref" in k) == (cm is not None) for k in pastes)
        out = outs[name] = saved[0]
        assert out.shape == sc.shape                                            # the scene's size
        assert (out[~grown] == sc[~grown]).all()                                # it differs from the scene only inside the grown line masks
        for _, _, lm in lines:
            core = lm[:, :, 0] >= 128
            assert (out[core] != sc[core]).any()                                # ... and inside each of them it does
