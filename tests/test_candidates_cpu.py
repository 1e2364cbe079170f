"""Candidates (DESIGN.md section 4 "Candidates") without a device: the restatements (tests/helpers/candidates_ref.py) against
independent arithmetic, the choice rule, the option's parsing and every refusal, expansion and planning, run_items around a stub pipeline
and a stub reader, the CLI flags, and the host-side refusals of the two C entry points through the library as it loads on a CPU."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import candidates_ref as ref
from tests.helpers import rectify_ref as rref
from tests.test_batch_driver_cpu import J, P, T, _embed, _items, _loader
from textflux_amd import batch_driver as bd
from textflux_amd import candidates as cd
from textflux_amd import ocr as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EN_DICT = os.path.join(REPO, "tests", "golden", "en_dict.txt")
BF = torch.bfloat16
OCR = dict(weights=None, lang="en", dict_path=EN_DICT)


# ------------------------------------------------------------------------------------------------------------------- the restatements
def _rot(deg, cx, cy, h, w):
    """Q16 matrix of an upright h x w frame turned by deg around the scene point (cx, cy)"""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    q = 1 << 16
    x0, y0 = cx - (c * w - s * h) / 2, cy - (s * w + c * h) / 2
    return np.array([round(c * q), round(-s * q), round(x0 * q), round(s * q), round(c * q), round(y0 * q)], dtype=np.int64)


def test_gather_restatement_packs_each_crop_where_its_row_says():
    g = np.random.default_rng(0)
    img = g.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    crops = [(1, _rot(0, 5, 5, 1, 1), 1, 1), (1, _rot(-8, 40, 30, 48, 320), 48, 320), (0, _rot(25, 26, 18, 7, 33), 7, 33)]
    table, nbytes = ref.pack_table(crops, 3, guard=64)
    assert [int(r[9]) for r in table] == [64, 131, 131 + 48 * 320 * 3 + 64] and all(int(r[9]) % 2 for r in table[1:])      # odd starts
    before = g.integers(0, 256, nbytes, dtype=np.uint8)
    out, refused = ref.gather(img, table, before)
    assert refused == 0
    covered = np.zeros(nbytes, bool)
    for b, m, h, w in crops:
        row = next(r for r in table if (r[7], r[8]) == (h, w))
        off = int(row[9])
        assert (out[off:off + h * w * 3].reshape(h, w, 3) == rref.warp_affine(img[b], m, (h, w))[0]).all()
        covered[off:off + h * w * 3] = True
    assert (out[~covered] == before[~covered]).all() and (~covered).sum() == 4 * 64
    # rows that cannot be served write nothing and are counted
    bad = table.copy()
    bad[0, 0] = 2                                            # b = B
    bad[2, 9] = nbytes - 10                                  # overruns the buffer
    out2, refused2 = ref.gather(img, bad, before)
    assert refused2 == 2
    off = int(table[1, 9])
    assert (out2[off:off + 48 * 320 * 3] == out[off:off + 48 * 320 * 3]).all() and (out2[:off] == before[:off]).all()
    assert (out2[off + 48 * 320 * 3:] == before[off + 48 * 320 * 3:]).all()
    for col, v in ((7, 0), (8, -3), (9, -1), (0, -1)):
        t = table.copy()
        t[1, col] = v
        assert ref.gather(img, t, before)[1] == 1


def _planted():
    """x, v bf16 [rows, 8] with +-0, +-inf, NaN, subnormals and ordinary values; sigma fp32 whose products round both ways"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, 8, generator=g).to(BF)
    v = torch.randn(64, 8, generator=g).to(BF)
    sub = torch.tensor([1e-40, -1e-40, 9.2e-41, 1.1e-38], dtype=torch.float32).to(BF)      # bf16 subnormals and the smallest normals
    assert (sub[:3].float().abs() < 1.1754944e-38).all() and (sub.float() != 0).all()
    x[0, :4], v[1, :4], v[2, :4], x[2, :4] = sub, sub, sub, sub
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1.0, -1.0, 0.5]).to(BF)
    x[3], v[4], x[5], v[5] = special, special, special, special.flip(0)
    v[6], x[6] = special, torch.zeros(8).to(BF)
    x[7, :2], v[7, :2] = torch.tensor([float("inf"), -float("inf")]).to(BF), torch.tensor([float("inf"), float("inf")]).to(BF)
    x[8], v[8, :4] = torch.zeros(8).to(BF), sub
    sigma = torch.tensor([1.0, 0.8359375, 0.6171875123, 0.3333333433, 0.1111111119, 0.0], dtype=torch.float32)
    return x, v, sigma


def test_x0_predict_restatement_is_torchs_bf16_arithmetic_op_by_op():
    x, v, sigma = _planted()
    up = down = 0
    for step in range(len(sigma)):
        got = ref.x0_predict(x, v, sigma, step)
        s = np.float32(sigma[step].item())
        with np.errstate(all="ignore"):
            m32 = (s * v.float().numpy()).astype(np.float32)                                   # one fp32 product, no FMA
            m = torch.from_numpy(m32).to(BF)                                                   # rounded to bf16, to nearest even
            want = torch.from_numpy((x.float().numpy() - m.float().numpy()).astype(np.float32)).to(BF)
        assert ref.same_bits(got, want), step
        fin = np.isfinite(m32)
        up += int((m.float().numpy()[fin].astype(np.float64) > m32[fin].astype(np.float64)).sum())
        down += int((m.float().numpy()[fin].astype(np.float64) < m32[fin].astype(np.float64)).sum())
    assert up > 20 and down > 20                                                               # the product rounds both ways
    out = ref.x0_predict(x, v, sigma, 1)
    assert torch.isnan(out[3, 4]) and torch.isnan(out[4, 4]) and torch.isnan(out[7, 0])        # NaN in x, NaN in v, inf - inf
    assert out[7, 1].item() == -float("inf")
    assert out[6, 0].item() == 0 and math.copysign(1, out[6, 1].item()) == 1                   # 0 - (-0) = +0
    assert 0 < out[8, 1].float().item() < 1.1754944e-38 and -1.1754944e-38 < out[8, 0].float().item() < 0   # subnormals are not flushed
    assert not ref.same_bits(out, ref.x0_predict(x, v, sigma, 2))


# ------------------------------------------------------------------------------------------------------------------- the choice rule
def _rec(acc, loss):
    return dict(seq_acc=acc, ctc_loss=loss)


def test_choice_rule_on_planted_records():
    for choose in (cd.choose, ref.choose):
        assert choose([[_rec(0.0, 0.1)], [_rec(1.0, 5.0)], [_rec(0.0, 0.01)]]) == [1]                # exact beats a lower loss
        assert choose([[_rec(0.0, float("nan"))], [_rec(0.0, float("inf"))], [_rec(0.0, 7.0)]]) == [2]  # NaN and inf lose
        assert choose([[_rec(0.0, float("nan"))], [_rec(0.0, float("inf"))]]) == [0]                 # both +inf: the lowest k
        assert choose([[_rec(1.0, 2.0)], [_rec(1.0, 2.0)], [_rec(1.0, 3.0)]]) == [0]                 # a tie goes to the lowest k
        assert choose([[_rec(0.0, None)], [_rec(0.0, 9e9)]]) == [1]                                  # a missing loss is +inf
        # several lines: the number of inexact lines first, then the SUM of the losses
        two = [[_rec(1.0, 0.1), _rec(0.0, 0.1)], [_rec(1.0, 3.0), _rec(1.0, 4.0)], [_rec(1.0, 3.5), _rec(1.0, 3.4)], [_rec(0.0, 0.0), _rec(0.0, 0.0)]]
        assert choose(two) == [2] and choose(two, keep=3) == [2, 1, 0] and choose(two, keep=9) == [2, 1, 0, 3]
        assert choose([[_rec(1.0, 1.0), _rec(1.0, float("nan"))], [_rec(1.0, 50.0), _rec(1.0, 60.0)]]) == [1]
    assert cd.choice_key([_rec(1.0, 1.5), _rec(0.0, 2.0)], 4) == ref.choice_key([_rec(1.0, 1.5), _rec(0.0, 2.0)], 4) == (1, 3.5, 4)
    assert cd.pruned_steps(4, 30, 10, 1) == (4 * 10 + 20) / 120


# ------------------------------------------------------------------------------------------------------------ parsing and refusals
def test_option_parsing():
    assert cd.candidates_cfg(None, 42) is None and cd.candidates_cfg(1, 42) is None and cd.candidates_cfg(dict(n=1), 42) is None
    assert cd.candidates_cfg(3, 42) == dict(n=3, seeds=[42, 43, 44], prune=None)
    assert cd.candidates_cfg(dict(n=2, seeds=[7, 3]), 42) == dict(n=2, seeds=[7, 3], prune=None)
    assert cd.candidates_cfg(dict(n=4, prune=dict(at=10)), 0, 30, 8) == dict(n=4, seeds=[0, 1, 2, 3], prune=dict(at=10, keep=1))
    assert cd.candidates_cfg(dict(n=4, prune=dict(at=1, keep=4)), 0, 30, 4)["prune"] == dict(at=1, keep=4)
    for bad, msg in ((0, "at least 1"), (-2, "at least 1"), (True, "must be None"), ("3", "must be None"), (2.0, "must be None"),
                     (dict(n=2, m=1), "unknown keys"), (dict(seeds=[1]), "at least 1"), (dict(n=2, seeds=[1]), "2 different integers"),
                     (dict(n=2, seeds=[1, 1]), "different integers"), (dict(n=2, seeds=[1, 2.5]), "different integers"),
                     (dict(n=1, seeds=[5]), "give the seed"), (dict(n=2, prune=3), "prune must be"), (dict(n=2, prune=dict(keep=1)), "prune must be"),
                     (dict(n=2, prune=dict(at=1, k=1)), "prune must be"), (dict(n=2, prune=dict(at=0)), "inside the schedule"),
                     (dict(n=2, prune=dict(at=30)), "inside the schedule"), (dict(n=2, prune=dict(at=2, keep=3)), "keep=3"),
                     (dict(n=2, prune=dict(at=2, keep=0)), "keep=0"), (dict(n=2, prune=dict(at=2.0)), "integers"),
                     (dict(n=9, prune=dict(at=2)), "share one batch")):
        with pytest.raises(ValueError, match=msg):
            cd.candidates_cfg(bad, 42, 30, 8)
    assert cd.candidates_cfg(9, 42, 30, 8)["n"] == 9                   # without prune a work's candidates may straddle batches


class Unreachable:
    """a pipeline no refusal may reach"""
    def __init__(self, scheduler=None):
        self.scheduler = scheduler

    def __getattr__(self, name):
        raise AssertionError(f"the pipeline was reached ({name})")


def test_every_refusal_comes_before_the_pipeline():
    from textflux_amd import schedulers as S
    euler = S.FlowMatchEulerDiscreteScheduler()
    run = lambda pipe=Unreachable(euler), **kw: bd.run_items(_items()[:2], pipe, None, batch_size=4, device="cpu", loader=_loader, **kw)
    with pytest.raises(ValueError, match="candidates needs ocr"):
        run(candidates=3)
    with pytest.raises(NotImplementedError, match="mixed-geometry"):
        run(candidates=3, ocr=OCR, mixed_pad=0.25)
    with pytest.raises(ValueError, match="share one batch"):
        run(candidates=dict(n=5, prune=dict(at=2)), ocr=OCR)
    with pytest.raises(ValueError, match="inside the schedule"):
        run(candidates=dict(n=2, prune=dict(at=30)), ocr=OCR)
    prune = dict(n=2, prune=dict(at=2))
    amo = S.StochasticRFOvershotDiscreteScheduler()
    multi = S.FlowMatchMultistepScheduler()
    for kw, msg in ((dict(pipe=Unreachable(amo)), "AMO sampler"), (dict(pipe=Unreachable(multi)), "multistep sampler"),
                    (dict(pipe=Unreachable(object())), "other than FlowMatchEulerDiscreteScheduler"), (dict(strength=0.5), "strength"),
                    (dict(keep_known=True), "keep_known"), (dict(change_map=True), "change_map"),
                    (dict(true_cfg=2.0, negative_prompt="bad"), "true CFG"), (dict(step_cache=dict(threshold=0.1)), "step cache")):
        with pytest.raises(NotImplementedError, match="step_window does not run with .*" + msg):
            run(candidates=prune, ocr=OCR, **kw)
    # the same reasons stand behind the pipeline's own argument, with the step callback on top
    from textflux_amd import step_loop
    with pytest.raises(NotImplementedError, match="a step callback"):
        step_loop.refuse_step_window(euler, callback=True)
    with pytest.raises(NotImplementedError, match="mixed-geometry"):
        step_loop.refuse_step_window(euler, mixed=True)
    step_loop.refuse_step_window(euler)
    assert step_loop.check_step_window((0, 4), 4) == (0, 4) and step_loop.check_step_window([2, 3]) == (2, 3)
    for bad in ((2, 2), (3, 2), (-1, 2), (0, 5), (0.5, 2), "ab", 3, (1, 2, 3)):
        with pytest.raises(ValueError, match="step_window must be"):
            step_loop.check_step_window(bad, 4)


def test_the_pipeline_refuses_a_step_window_before_it_launches():
    import inspect
    from textflux_amd import schedulers as S
    from textflux_amd.pipeline import FluxFillPipeline
    pipe = FluxFillPipeline.__new__(FluxFillPipeline)
    pipe.default_sample_size, pipe.vae_scale_factor, pipe._callback_tensor_inputs, pipe._step_cache = 8, 8, ["latents"], None
    pipe.scheduler = S.FlowMatchEulerDiscreteScheduler()
    assert inspect.signature(FluxFillPipeline.__call__).parameters["step_window"].default is None
    lat = torch.zeros(1, 16, 64)
    with pytest.raises(ValueError, match="step_window must be"):
        pipe(prompt="p", num_inference_steps=4, step_window=(0, 5))
    with pytest.raises(ValueError, match="needs `latents`"):
        pipe(prompt="p", num_inference_steps=4, step_window=(2, 4))
    with pytest.raises(ValueError, match="needs output_type='latent'"):
        pipe(prompt="p", num_inference_steps=4, step_window=(0, 2))
    for kw, msg in ((dict(strength=0.5), "strength"), (dict(keep_known=True), "keep_known"), (dict(change_map=True), "change_map"),
                    (dict(negative_prompt="n", true_cfg=2.0), "true CFG"), (dict(callback_on_step_end=lambda *a: {}), "step callback")):
        with pytest.raises(NotImplementedError, match=msg):
            pipe(prompt="p", num_inference_steps=4, step_window=(2, 4), latents=lat, **kw)
    pipe._step_cache = object()
    with pytest.raises(NotImplementedError, match="step cache"):
        pipe(prompt="p", num_inference_steps=4, step_window=(2, 4), latents=lat)
    pipe._step_cache = None
    for sch, msg in ((S.StochasticRFOvershotDiscreteScheduler(), "AMO"), (S.FlowMatchMultistepScheduler(), "multistep"), (object(), "other than")):
        pipe.scheduler = sch
        with pytest.raises(NotImplementedError, match=msg):
            pipe(prompt="p", num_inference_steps=4, step_window=(0, 4))
    with pytest.raises(ValueError, match="unknown output_type"):
        pipe._decode_to_output(lat, 64, 64, "u9")
    assert '"u8"' in inspect.getsource(FluxFillPipeline._decode_to_output)


# ------------------------------------------------------------------------------------------------------------ expansion and planning
def test_expansion_seeds_and_planning():
    works = [bd.prepare_item(i, it, _loader) for i, it in enumerate(_items())]
    assert works[0].texts == ["WORD0"] and works[2].texts == ["AB2", "CD2"] and works[0].seed is None and works[0].cand is None
    cfg = cd.candidates_cfg(dict(n=3, seeds=[9, 4, 6]), 42)
    ex = cd.expand(works, cfg)
    assert len(ex) == 27 and [(w.index, w.cand, w.seed) for w in ex[:4]] == [(0, 0, 9), (0, 1, 4), (0, 2, 6), (1, 0, 9)]
    assert all(e.size == works[e.index].size and e.prompt == works[e.index].prompt for e in ex) and works[0].seed is None
    groups = lambda b: [(w.index, w.cand) for w in b.items]
    # without prune the plan is today's over more works: adjacent, but a work's candidates may straddle two batches
    plan = bd.plan_batches(ex, 4)
    assert groups(plan[0]) == [(0, 0), (0, 1), (0, 2), (1, 0)] and groups(plan[1])[:2] == [(1, 1), (1, 2)]
    for b in plan:
        assert len({w.size for w in b.items}) == 1
    # with prune no work straddles: batches of whole groups
    plan = bd.plan_batches(ex, 4, group=3)
    assert all(len(b.items) == 3 and len({w.index for w in b.items}) == 1 and [w.cand for w in b.items] == [0, 1, 2] for b in plan) and len(plan) == 9
    plan = bd.plan_batches(ex, 8, group=3)
    assert [len(b.items) for b in plan] == [6, 6, 6, 6, 3] and all([w.cand for w in b.items] == [0, 1, 2] * (len(b.items) // 3) for b in plan)
    with pytest.raises(ValueError, match="group"):
        bd.plan_batches(ex, 2, group=3)
    with pytest.raises(ValueError, match="group"):
        bd.plan_batches(ex, 4, 0.2, group=2)
    assert [groups(b) for b in bd.plan_batches(works, 4, group=1)] == [groups(b) for b in bd.plan_batches(works, 4)]
    # two ranks: every item's candidates live on one rank, whole
    plans = bd.rank_plans(ex, 2, 4, per_line=True, group=3)
    owner = {}
    for k, p in enumerate(plans):
        for b in p:
            assert len(b.items) == 3 and len({w.index for w in b.items}) == 1
            owner.setdefault(b.items[0].index, set()).add(k)
    assert all(len(v) == 1 for v in owner.values()) and sorted(owner) == list(range(9))
    assert {i for i, v in owner.items() if v == {0}} == {0, 2, 4, 6, 8}
    plans = bd.rank_plans(ex, 2, 4, per_line=True)             # no prune: still whole per rank, though not whole per batch
    for k, p in enumerate(plans):
        assert {w.index for b in p for w in b.items} == {i for i in range(9) if i % 2 == k}


# ------------------------------------------------------------------------------------------------ run_items around stubs
class CandPipe:
    """Every sample's result is a flat image whose grey level is the seed of the sample's generator.  With step_window the latents carry
    the seed instead: [n, 4, 2] filled with it, x0_preview alike, window_conditioning [n, 4, 3] filled with seed + 0.5."""

    def __init__(self):
        from textflux_amd import schedulers as S
        self.calls, self.text_encoder_2, self.scheduler = [], object(), S.FlowMatchEulerDiscreteScheduler()
        self.x0_preview = self.window_conditioning = None

    def encode_prompt(self, prompt, prompt_2, device=None, max_sequence_length=512, **kw):
        p2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
        return torch.stack([_embed(p) for p in p2]), torch.full((len(p2), P), 3.0), torch.zeros(T, 3)

    def decode_latents(self, latents, height, width, output_type="u8", output_crop=None):
        assert output_type == "u8" and output_crop is None
        self.calls.append(dict(decode=[int(v) for v in latents[:, 0, 0]]))
        return torch.stack([torch.full((height, width, 3), int(v), dtype=torch.uint8) for v in latents[:, 0, 0]])

    def __call__(self, height, width, num_inference_steps, generator, max_sequence_length, guidance_scale, prompt_embeds, pooled_prompt_embeds,
                 image=None, mask_image=None, output_type="pil", step_window=None, latents=None, masked_image_latents=None):
        n = len(generator)
        assert prompt_embeds.shape == (n, T, J) and pooled_prompt_embeds.shape == (n, P)
        seeds = [g.initial_seed() for g in generator]
        self.calls.append(dict(size=(width, height), seeds=seeds, output_type=output_type, step_window=step_window,
                               latents=None if latents is None else latents.clone(),
                               cond=None if masked_image_latents is None else masked_image_latents.clone(),
                               pe=prompt_embeds.clone(), images=image is not None))
        if step_window is not None and step_window[1] < num_inference_steps:
            assert output_type == "latent" and latents is None and image is not None
            lat = torch.stack([torch.full((4, 2), float(s)) for s in seeds])
            self.x0_preview, self.window_conditioning = lat.clone(), torch.stack([torch.full((4, 3), s + 0.5) for s in seeds])
            return SimpleNamespace(images=lat)
        if step_window is not None:
            assert image is None and mask_image is None and step_window[1] == num_inference_steps
            assert [int(v) for v in latents[:, 0, 0]] == seeds and [float(v) for v in masked_image_latents[:, 0, 0]] == [s + 0.5 for s in seeds]
        if output_type == "u8":
            return SimpleNamespace(images=torch.stack([torch.full((height, width, 3), s % 256, dtype=torch.uint8) for s in seeds]))
        assert output_type == "pil"
        return SimpleNamespace(images=[Image.fromarray(np.full((height, width, 3), s % 256, np.uint8)) for s in seeds])


class CandReader:
    """reads the seed off a sample's first byte: `exact` seeds are read exactly, every seed has its planted loss; previews (samples
    whose seed is in `flip`) are read with the planted preview loss instead"""
    def __init__(self, loss, exact=(), preview_loss=None):
        self.loss, self.exact, self.preview_loss, self.device_reads, self.stage = loss, set(exact), preview_loss, [], []

    def text_ids(self, text):
        return [ord(c) for c in text]

    def read_device(self, images_u8, lines, targets):
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and len(lines) == len(targets)
        self.device_reads.append([(b, int(images_u8[b, 0, 0, 0]), t, tuple(np.asarray(lm).shape), int((np.asarray(lm) > 127).sum())) for (b, lm), t in zip(lines, targets)])
        out = []
        table = self.loss if self.preview_loss is None or len(self.device_reads) % 2 == 0 else self.preview_loss
        for (b, lm), t in zip(lines, targets):
            s = int(images_u8[b, 0, 0, 0])
            ids = self.text_ids(t) if s in self.exact else [1]
            out.append(dict(text="".join(chr(i) for i in ids), ids=ids, ctc_loss=table[s]))
        return out

    def read(self, crops, targets):
        return [dict(text="AB", ids=[65, 66], ctc_loss=1.5) for _ in crops]


def _run(monkeypatch, reader, items, **kw):
    monkeypatch.setattr(O, "make_reader", lambda cfg, device="cuda": reader)
    monkeypatch.setattr(O, "crop_line", lambda img, shape, ops=None: torch.zeros(4, 9, 3, dtype=torch.uint8))
    pipe, saved = CandPipe(), {}
    res = bd.run_items(items, pipe, None, device="cpu", loader=_loader, save=lambda i, im: saved.__setitem__(i, np.array(im)), ocr=OCR, **kw)
    return pipe, saved, res


def test_the_planted_winner_is_saved(monkeypatch):
    items = _items()[:3]                                        # two strip edits and one two-line canvas
    loss = {10: 3.0, 11: 1.0, 12: 2.0}
    reader = CandReader(loss)
    pipe, saved, res = _run(monkeypatch, reader, items, batch_size=4, seed=10, candidates=3)
    assert sorted(saved) == [0, 1, 2] and all((saved[i] == 11).all() for i in saved)               # the lowest loss, everywhere
    assert res["done"] == [0, 1, 2] or sorted(res["done"]) == [0, 1, 2]
    assert all(c["output_type"] == "u8" and c["step_window"] is None for c in pipe.calls)
    assert [c["seeds"] for c in pipe.calls] == [[10, 11, 12, 10], [11, 12], [10, 11, 12]]          # adjacent; item 1 straddles two batches
    c = res["candidates"]
    assert sorted(c) == [0, 1, 2] and all(len(c[i]) == 1 and c[i][0]["chosen"] == 1 and c[i][0]["seeds"] == [10, 11, 12] and c[i][0]["line"] == 0 for i in c)
    assert [(s["seed"], s["ctc_loss"], s["stage"]) for s in c[0][0]["scores"]] == [(10, 3.0, "final"), (11, 1.0, "final"), (12, 2.0, "final")]
    assert set(c[0][0]["scores"][0]) == {"seed", "line", "text", "pred", "seq_acc", "ned", "ctc_loss", "stage"}
    # the two-line canvas is read as two lines per candidate, located by the work's own mask (black over the glyph part)
    two = [s for s in c[2][0]["scores"]]
    assert [(s["seed"], s["line"], s["text"]) for s in two] == [(k, l, t) for k in (10, 11, 12) for l, t in ((0, "AB2"), (1, "CD2"))]
    assert len(reader.device_reads) == 3 and [len(r) for r in reader.device_reads] == [4, 2, 6]     # one read_device call per batch
    assert all(shape == (512, 256) and 0 < area < 256 * 256 // 2 for _, _, _, shape, area in reader.device_reads[2])
    assert sorted(res["ocr"]) == [0, 1, 2]                                                          # the final report still reads the final image
    # exact beats loss; given seeds are used as they are
    reader = CandReader({5: 0.1, 99: 9.0, 7: 0.2}, exact=(99,))
    pipe, saved, res = _run(monkeypatch, reader, items[:1], batch_size=8, candidates=dict(n=3, seeds=[5, 99, 7]))
    assert (saved[0] == 99).all() and res["candidates"][0][0]["chosen"] == 1 and pipe.calls[0]["seeds"] == [5, 99, 7]
    # a NaN loss loses, a tie goes to the first
    reader = CandReader({42: float("nan"), 43: 4.0, 44: 4.0})
    pipe, saved, res = _run(monkeypatch, reader, items[:1], batch_size=8, candidates=3)
    assert (saved[0] == 43).all()


def test_one_candidate_issues_exactly_the_calls_of_a_run_without_the_key(monkeypatch):
    from tests.test_batch_driver_cpu import StubPipe
    monkeypatch.setattr(O, "make_reader", lambda cfg, device="cuda": CandReader({}))
    monkeypatch.setattr(O, "crop_line", lambda img, shape, ops=None: torch.zeros(4, 9, 3, dtype=torch.uint8))
    runs = []
    for kw in ({}, dict(candidates=1), dict(candidates=None), dict(candidates=dict(n=1))):
        pipe, saved = StubPipe(0), []                           # its __call__ takes today's keywords only and asserts seed 42
        res = bd.run_items(_items(), pipe, None, batch_size=4, device="cpu", loader=_loader, save=lambda i, im: saved.append((i, np.array(im))),
                           ocr=OCR, **kw)
        assert "candidates" not in res
        runs.append((pipe.calls, pipe.encodes, [(i, a.tobytes()) for i, a in saved], res["done"], res["batches"]))
    assert all(r == runs[0] for r in runs[1:]) and len(runs[0][0]) == 3


def test_prune_finishes_exactly_the_survivors(monkeypatch):
    items = _items()[:2]
    final = {20: 5.0, 21: 1.0, 22: 2.0, 23: 0.5}
    preview = {20: 1.0, 21: 9.0, 22: 0.5, 23: 0.7}              # the previews rank 22, 23, 20, 21: keep=2 finishes 22 and 23
    reader = CandReader(final, preview_loss=preview)
    pipe, saved, res = _run(monkeypatch, reader, items, batch_size=8, seed=20, num_inference_steps=6,
                            candidates=dict(n=4, prune=dict(at=2, keep=2)))
    calls = [c for c in pipe.calls if "decode" not in c]
    assert len(calls) == 2 and [c for c in pipe.calls if "decode" in c] == [dict(decode=[20, 21, 22, 23] * 2)]
    first, second = calls
    assert first["step_window"] == (0, 2) and first["output_type"] == "latent" and first["seeds"] == [20, 21, 22, 23] * 2 and first["images"]
    assert second["step_window"] == (2, 6) and second["output_type"] == "u8" and second["seeds"] == [22, 23, 22, 23] and not second["images"]
    assert [int(v) for v in second["latents"][:, 0, 0]] == [22, 23, 22, 23] and tuple(second["latents"].shape) == (4, 4, 2)
    assert [float(v) for v in second["cond"][:, 0, 0]] == [22.5, 23.5, 22.5, 23.5]
    assert torch.equal(second["pe"], first["pe"][[2, 3, 6, 7]])
    assert all((saved[i] == 23).all() for i in (0, 1))           # among the survivors the final scores decide
    e = res["candidates"][0][0]
    assert e["chosen"] == 3 and [(s["seed"], s["stage"]) for s in e["scores"]] == [(20, "preview"), (21, "preview"), (22, "preview"), (23, "preview"),
                                                                                   (22, "final"), (23, "final")]
    assert [s["ctc_loss"] for s in e["scores"]] == [1.0, 9.0, 0.5, 0.7, 2.0, 0.5]
    # keep = 1: the survivor is the candidate the rule picks from the previews, whatever its final score
    reader = CandReader(final, preview_loss=preview)
    pipe, saved, res = _run(monkeypatch, reader, items[:1], batch_size=4, seed=20, num_inference_steps=6, candidates=dict(n=4, prune=dict(at=3)))
    calls = [c for c in pipe.calls if "decode" not in c]
    assert calls[1]["seeds"] == [22] and calls[1]["step_window"] == (3, 6) and (saved[0] == 22).all() and res["candidates"][0][0]["chosen"] == 2


# ------------------------------------------------------------------------------------------------------------------------- the CLIs
def test_cli_flags(tmp_path):
    import importlib
    import json
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import run_inference as ri
    import run_inference_lora as ril
    re_ = importlib.import_module("run_eval")
    base = ["--image", "i", "--mask", "m", "--words", "w"]
    on = ["--ocr_weights", "p", "--ocr_dict", "d"]
    for parser in (ri.build_parser(), ril.build_parser()):
        a = parser.parse_args(base)
        assert (a.candidates, a.candidates_prune_at, a.candidates_keep) == (None, None, None) and ri.candidates_from_args(a) is None
        assert ri.candidates_from_args(parser.parse_args(base + on + ["--candidates", "4"])) == dict(n=4, prune=None)
        assert ri.candidates_from_args(parser.parse_args(base + on + ["--candidates", "4", "--candidates_prune_at", "10"])) == dict(n=4, prune=dict(at=10, keep=1))
        got = ri.candidates_from_args(parser.parse_args(base + on + ["--candidates", "4", "--candidates_prune_at", "10", "--candidates_keep", "2"]))
        assert got == dict(n=4, prune=dict(at=10, keep=2))
        for bad in (["--candidates", "4"], on + ["--candidates_prune_at", "3"], on + ["--candidates_keep", "2"], on + ["--candidates", "0"],
                    on + ["--candidates", "3", "--candidates_keep", "2"], on + ["--candidates", "3", "--candidates_prune_at", "2", "--step_cache", "0.1"],
                    on + ["--candidates", "3", "--candidates_prune_at", "2", "--multistep"]):
            with pytest.raises(SystemExit):
                ri.candidates_from_args(parser.parse_args(base + bad))
    for lora in (False, True):
        a = re_.build_parser(lora).parse_args(["--candidates", "3", "--candidates_prune_at", "5", "--candidates_keep", "2"])
        assert (a.candidates, a.candidates_prune_at, a.candidates_keep) == (3, 5, 2)
        assert re_.build_parser(lora).parse_args([]).candidates is None
    chosen = {4: [dict(line=0, seeds=[1, 2], chosen=1, scores=[])], 2: [dict(line=0, seeds=[1, 2], chosen=0, scores=[]), dict(line=1, seeds=[1, 2], chosen=1, scores=[])]}
    line = re_.write_candidates_report(chosen, str(tmp_path))
    rep = json.load(open(tmp_path / "candidates_report.json"))
    assert rep["work_count"] == 3 and [(w["item"], w["line"]) for w in rep["works"]] == [(2, 0), (2, 1), (4, 0)] and "2 kept another seed" in line
    re_.write_candidates_report(chosen, str(tmp_path), rank=1, world=2)
    assert json.load(open(tmp_path / "candidates_report.rank1.json"))["work_count"] == 3


# ------------------------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


def test_symbols_are_declared_bound_exported_and_the_abi_version_stays(lib):
    from textflux_amd import _lib as L
    from textflux_amd import ops
    for name, nargs in (("tfx_warp_affine_gather_u8", 13), ("tfx_x0_predict", 10)):
        assert name in L.SIGNATURES and hasattr(lib, name) and len(L.SIGNATURES[name][1]) == nargs
    assert L.ABI_VERSION == 11 == L.header_abi_version()
    hdr = open(os.path.join(REPO, "include", "textflux_hip.h")).read()
    assert "int tfx_warp_affine_gather_u8(const void* images, void* out, int64_t out_bytes" in hdr and "int tfx_x0_predict(const void* x, int64_t ldx" in hdr
    assert "(b, m0, m1, m2, m3, m4, m5, out_h, out_w, offset)" in hdr and "m = bf16(s f32(v))   out = bf16(f32(x) - f32(m))" in hdr
    assert callable(ops.warp_affine_gather_u8) and callable(ops.x0_predict) and ops.GATHER_COLS == 10
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.x0_predict(torch.zeros(2, 8, dtype=BF), torch.zeros(2, 8, dtype=BF), torch.zeros(3))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.warp_affine_gather_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), np.zeros((1, 10), np.int64))
    assert hasattr(O.TextRecognizer, "read_device")


def test_gather_entry_point_checks_its_arguments(lib):
    p = [k << 24 for k in range(1, 6)]                                 # images, out, table, refused, taps: never dereferenced
    def call(ptrs=p, out_bytes=1 << 16, n=3, dims=(2, 8, 8, 3), blocks=4):
        return lib.tfx_warp_affine_gather_u8(ptrs[0], ptrs[1], out_bytes, ptrs[2], n, ptrs[3], *dims, blocks, ptrs[4], None)
    for k in range(5):
        assert call(p[:k] + [None] + p[k + 1:]) != 0 and b"tfx_warp_affine_gather_u8: null pointer" in lib.tfx_last_error()
    assert call(n=-1) != 0 and b"negative crop count" in lib.tfx_last_error()
    assert call(n=65536) != 0 and b"65535" in lib.tfx_last_error()
    for c in (0, 5):
        assert call(dims=(2, 8, 8, c)) != 0 and b"1..4 channels" in lib.tfx_last_error()
    for k in range(3):
        dims = [2, 8, 8, 3]
        dims[k] = 0
        assert call(dims=tuple(dims)) != 0 and b"at least 1" in lib.tfx_last_error()
    assert call(out_bytes=-1) != 0 and b"negative out_bytes" in lib.tfx_last_error()
    for b in (0, 65536):
        assert call(blocks=b) != 0 and b"blocks_per_crop" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2] + 4, p[3], p[4]]) != 0 and b"8-byte aligned" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2], p[3], p[4] + 2]) != 0 and b"8-byte aligned" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2], p[3] + 2, p[4]]) != 0 and b"4-byte aligned" in lib.tfx_last_error()
    for ptrs in ([p[0], p[0], p[2], p[3], p[4]], [p[0], p[0] + 2 * 8 * 8 * 3 - 1, p[2], p[3], p[4]], [p[0], p[1], p[1] + 8, p[3], p[4]],
                 [p[0], p[1], p[2], p[1] + 4, p[4]], [p[0], p[1], p[2], p[0] + 4, p[4]], [p[0], p[1], p[2], p[2] + 8, p[4]]):
        assert call(ptrs) != 0 and b"must not overlap" in lib.tfx_last_error()
    assert call(n=0) == 0 and call([p[0], p[0] + 2 * 8 * 8 * 3, p[2], p[3], p[4]], n=0) == 0         # no crop launches nothing; adjacent is no overlap


def test_x0_predict_entry_point_checks_its_arguments(lib):
    p = [k << 24 for k in range(1, 6)]                                 # x, v, out, sigma, step_ptr: never dereferenced
    def call(ptrs=p, ldx=64, Cc=64, rows=4, step=0):
        return lib.tfx_x0_predict(ptrs[0], ldx, ptrs[1], ptrs[2], Cc, rows, ptrs[3], ptrs[4], step, None)
    for c in (0, -8, 12):
        assert call(Cc=c) != 0 and b"positive multiple of 8" in lib.tfx_last_error()
    assert call(rows=-1) != 0 and b"negative row count" in lib.tfx_last_error()
    for ld in (60, 56, 68):
        assert call(ldx=ld) != 0 and b"ldx must be a multiple of 8 and >= C" in lib.tfx_last_error()
    for k in range(4):
        assert call(p[:k] + [None] + p[k + 1:]) != 0 and b"x0_predict: null pointer" in lib.tfx_last_error()
    for k in range(3):
        assert call(p[:k] + [p[k] + 8] + p[k + 1:]) != 0 and b"16-byte aligned" in lib.tfx_last_error()
    for k in (3, 4):
        assert call(p[:k] + [p[k] + 2] + p[k + 1:]) != 0 and b"4-byte aligned" in lib.tfx_last_error()
    assert call([p[0], p[1], p[0], p[3], p[4]]) != 0 and b"must not overlap x or v" in lib.tfx_last_error()
    assert call([p[0], p[1], p[1] + 16, p[3], p[4]]) != 0 and b"must not overlap x or v" in lib.tfx_last_error()
    # the xin form: x rows of pitch 384 reach further than the contiguous extent
    assert call([p[0], p[1], p[0] + 3 * 384 * 2 + 32, p[3], p[4]], ldx=384) != 0 and b"must not overlap x or v" in lib.tfx_last_error()
    assert call([p[0], p[1], p[2], p[3], None], step=-1) != 0 and b"negative step" in lib.tfx_last_error()
    assert call(rows=0) == 0 and call([None] * 5, rows=0) == 0         # nothing to do: nothing is launched, the pointers mean nothing
