"""Candidates on the device (DESIGN.md section 4 "Candidates"): tfx_warp_affine_gather_u8 and tfx_x0_predict bit for bit against their
restatements (tests/helpers/candidates_ref.py), TextRecognizer.read_device against read, step_window against the unwindowed call and
against a Python-issued loop, and batch_driver.run_items(candidates=...) without and with pruning on the tiny synthetic checkpoint:
every score is read_device's on the plain call with that seed, the choice is the restated rule's, and the saved image is the plain
run's with the chosen seed, byte for byte."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import candidates_ref as ref
from tests.helpers import ocr_ref as X
from tests.helpers import rectify_ref as rref
from tests.test_candidates_cpu import _planted, _rot

BF = torch.bfloat16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EN_DICT = os.path.join(REPO, "tests", "golden", "en_dict.txt")


@contextlib.contextmanager
def batch_independent():
    """the two batch-size-dependent forms off, as tests/test_fullsize_gpu.py switches them: no K-sliced GEMM tail, whole attention items"""
    from textflux_amd import ops
    ops.set_option("gemm_splitk", 0)
    ops.set_option("attention_streamk", 0)
    try:
        yield
    finally:
        ops.set_option("gemm_splitk", 2)
        ops.set_option("attention_streamk", 1)


# ------------------------------------------------------------------------------------------------------------------------ the gather
_gather = {}


def gather_case(C):
    """two 37 x 53 images and three crops -- 1 x 1, 48 x 320 reaching over the image's edges, 7 x 33 at 25 degrees -- packed with 64 guard
    bytes before, between and after them, which leaves every crop but the first at an odd byte; the restatement's result, computed once"""
    if C not in _gather:
        g = np.random.default_rng(11)
        img = g.integers(0, 256, (2, 37, 53, C), dtype=np.uint8)
        crops = [(1, _rot(0, 5, 5, 1, 1), 1, 1), (1, _rot(-8, 40, 30, 48, 320), 48, 320), (0, _rot(25, 26, 18, 7, 33), 7, 33)]
        assert all(m[1] != 0 for _, m, _, _ in crops[1:])
        table, nbytes = ref.pack_table(crops, C, guard=64)
        assert all(int(r[9]) % 2 == 1 for r in table[1:])
        before = g.integers(0, 256, nbytes, dtype=np.uint8)
        want, refused = ref.gather(img, table, before)
        assert refused == 0 and (want != before).any()
        _gather[C] = dict(img=img, crops=crops, table=table, before=before, want=want)
    return _gather[C]


@pytest.mark.parametrize("C", [3, 1])
def test_gather_equals_the_single_warp_and_the_restatement(C):
    from textflux_amd import ops
    c = gather_case(C)
    img = torch.from_numpy(c["img"]).cuda()
    for blocks, table in ((64, c["table"]), (1, torch.from_numpy(c["table"]).cuda()), (7, c["table"])):
        out, refused = ops.warp_affine_gather_u8(img, table, out=torch.from_numpy(c["before"]).cuda(), blocks_per_crop=blocks)
        torch.cuda.synchronize()
        assert int(refused.item()) == 0
        assert (out.cpu().numpy() == c["want"]).all()                  # every crop and every guard byte: before, between and after
    for (b, m, h, w), row in zip(c["crops"], c["table"]):
        off = int(row[9])
        single = ops.warp_affine_u8(img[b:b + 1], m, (h, w))[0]
        assert torch.equal(out[off:off + h * w * C].view(h, w, C), single)
        assert (single.cpu().numpy() == rref.warp_affine(c["img"][b], m, (h, w))[0]).all()
    assert torch.equal(img.cpu(), torch.from_numpy(c["img"]))
    # out=None: a buffer as long as the furthest crop end
    fresh, _ = ops.warp_affine_gather_u8(img, c["table"])
    last = c["table"][2]
    assert fresh.numel() == int(last[9]) + 7 * 33 * C and torch.equal(fresh[int(last[9]):], out[int(last[9]):int(last[9]) + 7 * 33 * C])


@pytest.mark.parametrize("C", [3, 1])
def test_gather_refuses_rows_it_cannot_serve_and_serves_the_rest(C):
    from textflux_amd import ops
    c = gather_case(C)
    img = torch.from_numpy(c["img"]).cuda()
    bad = c["table"].copy()
    bad[0, 0] = 2                                                      # b = B
    bad[2, 9] = c["before"].size - 10                                  # its last bytes would lie behind the buffer
    want, n = ref.gather(c["img"], bad, c["before"])
    assert n == 2
    out, refused = ops.warp_affine_gather_u8(img, bad, out=torch.from_numpy(c["before"]).cuda())
    assert int(refused.item()) == 2 and (out.cpu().numpy() == want).all()
    off = int(bad[1, 9])
    assert (want[off:off + 48 * 320 * C] == c["want"][off:off + 48 * 320 * C]).all() and (want[:off] == c["before"][:off]).all()
    # every other way a row can be wrong, one at a time; the counter adds up over calls
    for col, v in ((7, 0), (8, -3), (9, -1), (0, -1), (7, (1 << 24) + 1), (9, 1 << 40)):
        t = c["table"].copy()
        t[1, col] = v
        want, n = ref.gather(c["img"], t, c["before"])
        out, refused = ops.warp_affine_gather_u8(img, t, out=torch.from_numpy(c["before"]).cuda(), refused=refused)
        assert n == 1 and (out.cpu().numpy() == want).all()
    assert int(refused.item()) == 2 + 6
    with pytest.raises(ValueError, match="device table needs"):
        ops.warp_affine_gather_u8(img, torch.from_numpy(c["table"]).cuda())
    for bad_call in (lambda: ops.warp_affine_gather_u8(img.float(), c["table"]), lambda: ops.warp_affine_gather_u8(img, c["table"][:, :9]),
                     lambda: ops.warp_affine_gather_u8(img, c["table"].astype(np.int32)), lambda: ops.warp_affine_gather_u8(img, c["table"], blocks_per_crop=0),
                     lambda: ops.warp_affine_gather_u8(img, c["table"], out=torch.zeros(8, 8, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            bad_call()
    empty, refused = ops.warp_affine_gather_u8(img, np.zeros((0, 10), np.int64))
    assert empty.numel() == 0 and int(refused.item()) == 0


# ------------------------------------------------------------------------------------------------------------------------ x0_predict
SIGMA = torch.tensor([1.0, 0.8359375, 0.6171875123, 0.3333333433, 0.1111111119, 0.0], dtype=torch.float32)
_x0 = {}


def x0_case(rows, C):
    """x, v bf16 [rows, C] on the host, drawn once; the planted rows of the CPU test (signed zeros, infinities, NaNs, subnormals) come
    first where they fit"""
    if (rows, C) not in _x0:
        g = torch.Generator().manual_seed(rows * 131 + C)
        x, v = torch.randn(rows, C, generator=g).to(BF), torch.randn(rows, C, generator=g).to(BF)
        px, pv, _ = _planted()
        k = min(rows * C, px.numel()) // C
        if k:
            x[:k], v[:k] = px.reshape(-1)[:k * C].view(k, C), pv.reshape(-1)[:k * C].view(k, C)
        _x0[(rows, C)] = (x, v)
    return _x0[(rows, C)]


@pytest.mark.parametrize("how", ["literal", "device_word"])
@pytest.mark.parametrize("rows,C,ld", [(1, 8, 8), (257, 8, 8), (37, 64, 384), (37, 64, 64)], ids=["one_chunk", "257_chunks", "xin_pitch_384", "296_chunks"])
def test_x0_predict_equals_the_restatement(rows, C, ld, how):
    from textflux_amd import ops
    x, v = x0_case(rows, C)
    wide = torch.full((rows, ld), 55.0, dtype=BF, device="cuda")
    wide[:, :C] = x.cuda()
    dx = wide[:, :C] if ld != C else x.cuda()
    guard = torch.full((rows + 2, C), 77.0, dtype=BF, device="cuda")
    sigma = SIGMA.cuda()
    for step in (1, 2, 4, 5):
        want = ref.x0_predict(x, v, SIGMA, step)
        kw = dict(step=step) if how == "literal" else dict(step=0, step_ptr=torch.tensor([step], dtype=torch.int32, device="cuda"))
        got = ops.x0_predict(dx, v.cuda(), sigma, out=guard[1:rows + 1], **kw)
        torch.cuda.synchronize()
        assert got.data_ptr() == guard[1].data_ptr() and ref.same_bits(got, want), (step, (got.float().cpu() != want.float()).sum())
        assert (guard[0] == 77.0).all() and (guard[-1] == 77.0).all()
        assert ref.same_bits(ops.x0_predict(dx, v.cuda(), sigma, **kw), want)                       # out=None: a new tensor
    if ld != C:
        assert (wide[:, C:] == 55.0).all() and ref.same_bits(wide[:, :C].contiguous(), x)           # x is read, never written
    if rows * C > 512:
        assert not ref.same_bits(ref.x0_predict(x, v, SIGMA, 1), ref.x0_predict(x, v, SIGMA, 2))


def test_x0_predict_wrapper_refusals():
    from textflux_amd import ops
    x, v = (t.cuda() for t in x0_case(37, 64))
    sigma = SIGMA.cuda()
    with pytest.raises(TypeError, match="bf16"):
        ops.x0_predict(x.float(), v.float(), sigma)
    with pytest.raises(TypeError, match="sigma"):
        ops.x0_predict(x, v, sigma.double())
    with pytest.raises(TypeError, match="step_ptr"):
        ops.x0_predict(x, v, sigma, step_ptr=torch.zeros(1, device="cuda"))
    with pytest.raises(ValueError, match="one shape"):
        ops.x0_predict(x, v[:36], sigma)
    with pytest.raises(ValueError, match="contiguous"):
        ops.x0_predict(x[:, :32], v[:, :32], sigma)
    with pytest.raises(ValueError, match="outside the table"):
        ops.x0_predict(x, v, sigma, step=6)
    with pytest.raises(RuntimeError, match="must not overlap"):
        ops.x0_predict(x, v, sigma, out=v)
    assert ops.x0_predict(x[:0], v[:0], sigma).shape == (0, 64)


# ------------------------------------------------------------------------------------------------------------------------ read_device
@pytest.fixture(scope="module")
def reader():
    from textflux_amd import ocr as O
    return O.TextRecognizer(O.RecModel(X.seeded_state(97), 97), EN_DICT, (3, 48, 320), 6)


def test_read_device_equals_read_on_the_fixture_crops(reader):
    """the five fixture crops sit in five scenes on whole pixels under upright line masks, so that the device crop is the fixture crop byte
    for byte; read_device then returns read's records: equal ids, bitwise equal losses"""
    from textflux_amd import ocr as O
    crops = X.fixture_crops()
    g = np.random.default_rng(5)
    scenes = g.integers(0, 256, (5, 100, 310, 3), dtype=np.uint8)
    lines = []
    for i, c in enumerate(crops):
        h, w = c.shape[:2]
        y0, x0 = 3 + i, 2 + 2 * i
        scenes[i, y0:y0 + h, x0:x0 + w] = c
        m = np.zeros((100, 310), np.uint8)
        m[y0:y0 + h + 1, x0:x0 + w + 1] = 255                          # |tl - tr| = w, |tl - bl| = h: the rectangle's own size
        lines.append((i, m))
    dev = torch.from_numpy(scenes).cuda()
    for (i, m), c in zip(lines, crops):
        assert torch.equal(O.crop_line(dev[i], m).cpu(), torch.from_numpy(c))
    order = [3, 0, 4, 1, 2]                                            # lines need not come in image order
    want = reader.read([crops[i] for i in order], [X.TARGETS[i] for i in order])
    got = reader.read_device(dev, [lines[i] for i in order], [X.TARGETS[i] for i in order])
    assert [r["ids"] for r in got] == [r["ids"] for r in want] and [r["text"] for r in got] == [r["text"] for r in want]
    assert np.array([r["ctc_loss"] for r in got]).tobytes() == np.array([r["ctc_loss"] for r in want]).tobytes()
    assert sum(np.isfinite(r["ctc_loss"]) for r in want) >= 4
    noT = reader.read_device(dev, lines)
    assert [r["ids"] for r in noT] == [r["ids"] for r in reader.read(crops)] and all(r["ctc_loss"] is None for r in noT)
    # a slanted polygon: the crop is crop_line's, so the record is read's on it
    poly = np.array([[30.0, 20.0], [250.0, 40.0], [247.0, 72.0], [27.0, 52.0]])
    a = reader.read_device(dev, [(2, poly)], ["to you"])
    b = reader.read([O.crop_line(dev[2], poly)], ["to you"])
    assert a[0]["ids"] == b[0]["ids"] and np.float64(a[0]["ctc_loss"]).tobytes() == np.float64(b[0]["ctc_loss"]).tobytes()
    with pytest.raises(ValueError, match="the batch has 5"):
        reader.read_device(dev, [(5, lines[0][1])])
    with pytest.raises(ValueError, match="targets"):
        reader.read_device(dev, lines, ["a"])
    with pytest.raises(ValueError, match="no lines"):
        reader.read_device(dev, [])


# ------------------------------------------------------------------------------------------------------------------------ the pipeline
N_STEPS = 4
_win = {}


def win_inputs():
    """the step-cache tests' call at 256 x 256 (S = 256) with 4 steps, and a batch of 3 built from two of its draws; drawn once"""
    if not _win:
        from tests.test_step_cache_gpu import inputs
        two, more = inputs("16x16"), inputs("16x16", seed=6)
        _win["two"] = dict(two, num_inference_steps=N_STEPS)
        _win["three"] = {k: (torch.cat((v, more[k][:1])) if isinstance(v, torch.Tensor) else v) for k, v in _win["two"].items()}
    return _win


@pytest.fixture(scope="module")
def tiny():
    from tests.test_step_cache_gpu import make_pipe
    return make_pipe("euler")


def test_two_windows_equal_the_plain_call_and_the_preview_is_the_restatement(tiny):
    from tests.helpers import plain_loop as PL
    pipe, inp = tiny, win_inputs()["two"]
    with batch_independent():
        for graph in (False, True):
            pipe.enable_hip_graph(graph)
            plain = pipe(**inp).images
            if not graph:                                              # the scheduler holds the plain call's schedule: the Python-issued loop
                lats, vs = [], []
                PL.plain_loop(pipe, inp["latents"], inp["masked_image_latents"], inp["prompt_embeds"], inp["pooled_prompt_embeds"], (16, 16),
                              forward=lambda ses, mod, i: (lambda v: (vs.append(v.clone()), v)[1])(ses.run(mod)), per_step=lats)
                assert torch.equal(lats[-1], plain) and len(vs) == N_STEPS
                sigmas = pipe.scheduler.sigmas.float().cpu()
                assert sigmas.numel() == N_STEPS + 1
            assert pipe.x0_preview is None or graph
            first = pipe(**inp, step_window=(0, 2)).images
            preview, cond = pipe.x0_preview, pipe.window_conditioning
            assert torch.equal(first, lats[1]) and cond is not None and torch.equal(cond, inp["masked_image_latents"])
            assert preview.shape == first.shape and preview.dtype == BF
            assert ref.same_bits(preview, ref.x0_predict(lats[1], vs[1], sigmas, 2)), graph
            assert not ref.same_bits(preview, ref.x0_predict(lats[1], vs[1], sigmas, 1))
            second = pipe(**dict(inp, latents=first), step_window=(2, 4)).images
            assert torch.equal(second, plain), graph
            assert torch.equal(pipe(**inp, step_window=(0, 4)).images, plain)          # the whole schedule as one window
            one = pipe(**inp, step_window=(0, 1)).images                               # a window of one step
            assert torch.equal(one, lats[0]) and ref.same_bits(pipe.x0_preview, ref.x0_predict(lats[0], vs[0], sigmas, 1))
            three = pipe(**dict(inp, latents=one), step_window=(1, 3)).images
            assert torch.equal(three, lats[2])
            assert torch.equal(pipe(**dict(inp, latents=three), step_window=(3, 4)).images, plain)
            assert torch.equal(pipe(**inp).images, plain)                              # and the plain call is still the plain call
    pipe.enable_hip_graph(False)


def test_a_sample_finished_alone_equals_its_place_in_the_batch(tiny):
    pipe, inp = tiny, win_inputs()["three"]
    pipe.enable_hip_graph(False)
    with batch_independent():
        plain = pipe(**inp).images
        assert plain.shape[0] == 3 and not torch.equal(plain[1], plain[0])
        lat = pipe(**inp, step_window=(0, 2)).images
        alone = {k: (v[1:2] if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
        alone = pipe(**dict(alone, latents=lat[1:2].clone()), step_window=(2, 4)).images
        assert torch.equal(alone[0], plain[1])
        pair = {k: (v[[2, 0]] if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}       # survivors gathered by index
        pair = pipe(**dict(pair, latents=lat[[2, 0]]), step_window=(2, 4)).images
        assert torch.equal(pair[0], plain[2]) and torch.equal(pair[1], plain[0])


def test_output_type_u8_is_the_pil_output_on_the_device(driver_pipe):
    from textflux_amd import glyph
    scene, mask, words = glyph.synthetic_case(256, 128)
    combined, cmask, meta = glyph.compose(scene, mask, words)
    w, h = (combined.size[0] // 32) * 32, (combined.size[1] // 32) * 32
    kw = dict(prompt=glyph.PROMPT_TEMPLATE2, prompt_2=glyph.generate_prompt(words), image=combined.resize((w, h)), mask_image=cmask.resize((w, h)),
              height=h, width=w, num_inference_steps=2, guidance_scale=30.0)
    gen = lambda: torch.Generator(device="cuda").manual_seed(3)
    pil = driver_pipe(**kw, generator=gen()).images[0]
    u8 = driver_pipe(**kw, generator=gen(), output_type="u8").images
    assert u8.is_cuda and u8.dtype == torch.uint8 and tuple(u8.shape) == (1, h, w, 3) and (u8[0].cpu().numpy() == np.array(pil)).all()
    box = (32, 16, 200, 100)
    crop = driver_pipe(**kw, generator=gen(), output_type="u8", output_crop=box).images
    assert torch.equal(crop[0], u8[0, 16:100, 32:200])


# ------------------------------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def driver_pipe(tmp_path_factory):
    import run_inference as ri
    from tests.helpers import tiny_checkpoint as tc
    root = str(tmp_path_factory.mktemp("flux_fill_dev_candidates"))
    tc.write_pipeline_dir(root)
    saved = ri.BASE, ri.TRANSFORMER, ri.PIPE
    ri.BASE, ri.TRANSFORMER, ri.PIPE = root, os.path.join(root, "transformer"), None
    p = ri.load_flux_pipeline()
    ri.BASE, ri.TRANSFORMER, ri.PIPE = saved
    return p


@pytest.fixture(scope="module")
def ocr(tmp_path_factory):
    from safetensors.torch import save_file
    weights = str(tmp_path_factory.mktemp("rec") / "rec.safetensors")
    save_file(X.seeded_state(97), weights)
    return dict(weights=weights, lang="en", dict_path=EN_DICT)


STEPS, SEED, PASTE = 4, 42, dict(per_line=True, dilate=8, feather=2, region=dict(pad=0.0, min_side=96))


def items():
    from textflux_amd import glyph
    scene, mask, words = glyph.synthetic_case(256, 128)
    plain = dict(image=scene, mask=mask, text=words[0])
    scene2, mask2, words2 = glyph.synthetic_case(384, 256, multiline=True)
    return plain, dict(image=scene2, mask=mask2, text="\n".join(words2))


def run(pipe, its, batch_size=3, seed=SEED, paste=None, record=None, **kw):
    """run_items -> (result, {index: the saved image}); record: a list that receives every edit handed to pipe.paste_back"""
    from textflux_amd import batch_driver as bd
    saved = {}
    real = pipe.paste_back
    if record is not None:
        pipe.paste_back = lambda o_, e, m, **k: (record.append(np.array(e)), real(o_, e, m, **k))[1]
    try:
        res = bd.run_items(its, pipe, None, batch_size=batch_size, num_inference_steps=STEPS, guidance_scale=30.0, seed=seed, loader=lambda x: x,
                           save=lambda i, im: saved.__setitem__(i, np.array(im)), **({} if paste is None else dict(paste_back=paste)), **kw)
    finally:
        if record is not None:
            del pipe.paste_back
    assert not res["failed"] and sorted(res["all_done"]) == list(range(len(its))), res
    return res, saved


def works_of(pipe, item, paste=None):
    """the Works run_items prepares for one item"""
    from textflux_amd import batch_driver as bd
    from textflux_amd import per_line as pl
    compose = bool(getattr(pipe, "supports_device_compose", False))
    if paste is None:
        return [bd.prepare_item(0, item, lambda x: x, device_compose=compose)]
    cfg = bd._paste_back_cfg(paste)
    return pl.prepare_lines(0, item, lambda x: x, compose, None, cfg, **bd.pipeline_warps(pipe, cfg))


def direct(pipe, works, seeds, output_type):
    """the plain pipeline call of one batch as run_items assembles it -> (images, the batch's pipeline masks as host arrays)"""
    from textflux_amd import batch_driver as bd
    from textflux_amd import glyph
    n = len(works)
    _, pooled, _ = pipe.encode_prompt(prompt=glyph.PROMPT_TEMPLATE2, prompt_2=glyph.PROMPT_TEMPLATE2, device="cuda", max_sequence_length=512)
    pe, _, _ = pipe.encode_prompt(prompt=[glyph.PROMPT_TEMPLATE2] * n, prompt_2=[w.prompt for w in works], device="cuda", max_sequence_length=512)
    img_in, mask_in = bd._batch_inputs(works, "cuda")
    masks = [m[..., 0] if m.ndim == 3 else m for m in mask_in.cpu().numpy()] if isinstance(mask_in, torch.Tensor) else [np.array(m.convert("L")) for m in mask_in]
    gens = [torch.Generator(device="cuda").manual_seed(s) for s in seeds]
    images = pipe(height=works[0].size[1], width=works[0].size[0], image=img_in, mask_image=mask_in, num_inference_steps=STEPS, generator=gens,
                  max_sequence_length=512, guidance_scale=30.0, prompt_embeds=pe, pooled_prompt_embeds=pooled.expand(n, -1).contiguous(),
                  output_type=output_type).images
    return images, masks


def direct_scores(pipe, rd, work, seeds):
    """read_device on the plain batch of one work's candidates -> per seed its line records, and the pipeline-size results"""
    from textflux_amd import candidates as cd
    u8, masks = direct(pipe, [work] * len(seeds), seeds, "u8")
    lines = cd.work_lines(work, masks[0])
    recs = rd.read_device(u8, [(j, lm) for j in range(len(seeds)) for _, lm in lines], [t for _ in seeds for t, _ in lines])
    return [recs[j * len(lines):(j + 1) * len(lines)] for j in range(len(seeds))], [t for t, _ in lines], u8


def distinct_finite(entry, stage="final"):
    """the condition the comparisons stand on: per line, the candidates' losses are finite and pairwise distinct"""
    by_line = {}
    for s in entry["scores"]:
        if s["stage"] == stage:
            by_line.setdefault(s["line"], []).append(s["ctc_loss"])
    for losses in by_line.values():
        assert all(np.isfinite(v) for v in losses) and len(set(losses)) == len(losses), losses


def test_driver_without_prune(driver_pipe, ocr):
    from PIL import Image
    from textflux_amd import candidates as cd
    from textflux_amd import glyph
    from textflux_amd import ocr as O
    from textflux_amd import per_line as pl
    from textflux_amd import batch_driver as bd
    pipe = driver_pipe
    rd = O.make_reader(O.ocr_cfg(ocr))
    plain, two = items()
    seeds = [SEED, SEED + 1, SEED + 2]
    # ---- a plain item: one work, three candidates in one batch
    res, saved = run(pipe, [plain], ocr=ocr, candidates=3)
    entry = res["candidates"][0][0]
    assert entry["seeds"] == seeds and entry["line"] == 0 and len(entry["scores"]) == 3 and [s["seed"] for s in entry["scores"]] == seeds
    distinct_finite(entry)
    work = works_of(pipe, plain)[0]
    recs, texts, _ = direct_scores(pipe, rd, work, seeds)
    assert texts == ["TEXTFLUX"]
    for s, r in zip(entry["scores"], recs):
        assert s["pred"] == r[0]["text"] and np.float64(s["ctc_loss"]).tobytes() == np.float64(r[0]["ctc_loss"]).tobytes() and s["stage"] == "final"
        assert s["seq_acc"] == (1.0 if r[0]["ids"] == rd.text_ids("TEXTFLUX") else 0.0) and s["ned"] == O.get_ld(r[0]["ids"], rd.text_ids("TEXTFLUX"))
    k = entry["chosen"]
    assert [k] == ref.choose([[dict(seq_acc=s["seq_acc"], ctc_loss=s["ctc_loss"])] for s in entry["scores"]])
    # the same batch size, the same place in the batch: three copies of the item under the chosen seed, without the key
    off, saved_off = run(pipe, [plain] * 3, seed=seeds[k], ocr=ocr)
    assert "candidates" not in off and saved[0].shape == saved_off[k].shape and (saved[0] == saved_off[k]).all()
    assert res["ocr"][0] == off["ocr"][k]                              # and the final report reads the final image, as without the key
    other = [j for j in range(3) if j != k][0]
    assert (run(pipe, [plain] * 3, seed=seeds[other])[1][other] != saved[0]).any()      # another seed is another image
    # ---- a two-line item edited per line: two works of their own geometry, three candidates each
    edits = []
    res, saved = run(pipe, [two], paste=PASTE, record=edits, ocr=ocr, candidates=3)
    entries = res["candidates"][0]
    assert [e["line"] for e in entries] == [0, 1] and len(edits) == 2
    lines = works_of(pipe, two, PASTE)
    assert len(lines) == 2 and lines[0].size != lines[1].size                          # so every line's candidates are a batch of their own
    winners = []
    for e, w in zip(entries, lines):
        distinct_finite(e)
        recs, texts, _ = direct_scores(pipe, rd, w, seeds)
        assert texts == [w.texts[0]] and len(e["scores"]) == 3
        for s, r in zip(e["scores"], recs):
            assert s["pred"] == r[0]["text"] and np.float64(s["ctc_loss"]).tobytes() == np.float64(r[0]["ctc_loss"]).tobytes()
        assert [e["chosen"]] == ref.choose([[dict(seq_acc=s["seq_acc"], ctc_loss=s["ctc_loss"])] for s in e["scores"]])
        imgs, _ = direct(pipe, [w] * 3, seeds, "pil")
        winners.append(imgs[e["chosen"]].crop(glyph.crop_box(w.size, w.meta)))
    assert all((np.array(wn) == ed).all() for wn, ed in zip(winners, edits))           # only the winners reach the paste ...
    want = pl.compose_lines(pipe, lines, winners, bd._paste_back_cfg(PASTE))
    assert (np.array(want) == saved[0]).all()                                          # ... and the unchanged paste makes the scene of them
    if entries[0]["chosen"] == entries[1]["chosen"]:                                   # one seed for both lines: a run without the key says the same
        k = entries[0]["chosen"]
        assert (run(pipe, [two] * 3, seed=seeds[k], paste=PASTE)[1][k] == saved[0]).all()


def test_driver_pruned(driver_pipe, ocr):
    from textflux_amd import batch_driver as bd
    from textflux_amd import per_line as pl
    pipe = driver_pipe
    plain, two = items()
    seeds = [SEED, SEED + 1, SEED + 2]
    cand = dict(n=3, prune=dict(at=2, keep=1))
    with batch_independent():
        res, saved = run(pipe, [plain], ocr=ocr, candidates=cand)
        e = res["candidates"][0][0]
        assert [(s["seed"], s["stage"]) for s in e["scores"][:3]] == [(s, "preview") for s in seeds] and len(e["scores"]) == 4
        distinct_finite(e, "preview")
        k = ref.choose([[dict(seq_acc=s["seq_acc"], ctc_loss=s["ctc_loss"])] for s in e["scores"][:3]])[0]
        assert e["chosen"] == k and (e["scores"][3]["seed"], e["scores"][3]["stage"]) == (seeds[k], "final")
        off, saved_off = run(pipe, [plain], seed=seeds[k], ocr=ocr)                    # its own plain run
        assert (saved[0] == saved_off[0]).all() and res["ocr"][0] == off["ocr"][0]
        # the two-line item, per line: each line's survivor is finished alone and equals its own plain run's edit
        edits = []
        res, saved = run(pipe, [two], paste=PASTE, record=edits, ocr=ocr, candidates=cand)
        entries = res["candidates"][0]
        assert [x["line"] for x in entries] == [0, 1] and len(edits) == 2
        lines = pl.prepare_lines(0, two, lambda x: x, bool(getattr(pipe, "supports_device_compose", False)), None, bd._paste_back_cfg(PASTE),
                                 **bd.pipeline_warps(pipe, bd._paste_back_cfg(PASTE)))
        plain_edits = {}
        for L, x in enumerate(entries):
            distinct_finite(x, "preview")
            k = ref.choose([[dict(seq_acc=s["seq_acc"], ctc_loss=s["ctc_loss"])] for s in x["scores"][:3]])[0]
            assert x["chosen"] == k and [s["seed"] for s in x["scores"] if s["stage"] == "final"] == [seeds[k]]
            if k not in plain_edits:
                rec = []
                plain_edits[k] = (rec, run(pipe, [two], seed=seeds[k], paste=PASTE, record=rec)[1][0])
            assert (plain_edits[k][0][L] == edits[L]).all()
        if entries[0]["chosen"] == entries[1]["chosen"]:
            assert (plain_edits[entries[0]["chosen"]][1] == saved[0]).all()
        else:
            from PIL import Image
            want = pl.compose_lines(pipe, lines, [Image.fromarray(ed) for ed in edits], bd._paste_back_cfg(PASTE))
            assert (np.array(want) == saved[0]).all()
