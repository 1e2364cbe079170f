"""Read-back on the host: the fp64 restatement of the recogniser against the reference's recorded outputs (tests/golden/g19_ocr.safetensors,
written by tests/golden/make_ocr_goldens.py), every trap of the reference as a rejected wrong variant, the BatchNorm fold, textflux_amd.ocr
run unchanged over the fp64 engine of tests/helpers/ocr_ref.py, and the host-side pieces (decode, dictionary, metrics, report, plumbing).

The tolerance against the fixture is 2^-40 of each node's largest magnitude: fp64 rounding (2^-53) over a depth below 2^13 operations."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import ocr_ref as X
from textflux_amd import ocr as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EN_DICT = os.path.join(REPO, "tests", "golden", "en_dict.txt")
TOL = 2.0 ** -40
KEEP = 2048


def strided(t):
    flat = t.reshape(-1)
    return flat[::max(1, flat.numel() // KEEP)][:KEEP]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("g19_ocr")


@pytest.fixture(scope="module")
def sd():
    return X.seeded_state(97)


@pytest.fixture(scope="module")
def nodes(sd):
    return X.forward64(sd, X.node_input())


def node_ok(fx, name, t):
    return float((strided(t) - fx["node." + name]).abs().max()) <= TOL * float(fx["node_max." + name])


def test_restatement_matches_the_reference_at_every_node(fx, nodes):
    assert nodes["ctc"].shape == (2, 8, 97) and nodes["pool"].shape == (2, 512, 1, 8)
    for n in X.NODES + ["ctc_neck"]:
        assert node_ok(fx, n, nodes[n]), n


@pytest.mark.parametrize("variant", X.VARIANTS)
def test_each_trap_is_rejected_at_its_own_node(fx, sd, variant):
    got = X.forward64(sd, X.node_input(), variant=variant)
    first = X.NODES.index(X.VARIANT_NODE[variant])
    for n in X.NODES[:first]:
        assert node_ok(fx, n, got[n]), f"{variant}: {n} should not have moved"
    assert not node_ok(fx, X.NODES[first], got[X.NODES[first]]), f"{variant} passes at {X.NODES[first]}"
    assert not node_ok(fx, "ctc", got["ctc"])


def test_hard_swish_divides_and_does_not_multiply_by_a_sixth():
    """(x * relu6(x + 3)) / 6 with a true division: in fp32 the product with the rounded reciprocal gives other bits on ordinary inputs,
    and agrees on neither side of the knees at -3 and 3 by accident."""
    x = torch.cat([torch.arange(-64, 65, dtype=torch.float32) / 8, torch.tensor([-3.0, 3.0, -3.0000002, 2.9999998, 3.0000002])])
    ref = x * F.relu6(x + 3.0) / 6.0                                  # the reference's expression, evaluated left to right
    assert torch.equal(X.hswish(x), ref)
    wrong = x * F.relu6(x + 3.0) * torch.tensor(1.0 / 6.0, dtype=torch.float32)
    assert not torch.equal(wrong, ref)
    assert torch.equal(X.hsigmoid(x), F.relu6(x + 3.0) / 6.0) and not torch.equal(X.hsigmoid(x), F.relu6(1.2 * x + 3.0) / 6.0)


def test_batchnorm_fold_against_the_unfolded_form(sd):
    p = "backbone.block_list.3._pointwise_conv"
    w, bn = sd[p + "._conv.weight"], [sd[f"{p}._batch_norm.{n}"] for n in ("weight", "bias", "running_mean", "running_var")]
    assert float(bn[3].min()) < 0.6 and float(bn[3].max()) > 1.4 and float(bn[2].abs().max()) > 0.05      # the statistics are not trivial
    x = torch.from_numpy(X._ints("fold", (2, w.shape[1], 5, 7), -100, 101) / 50.0)
    unfolded = F.batch_norm(F.conv2d(x, w.double()), bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5)
    w64, b64 = X.fold64(w, *bn)
    folded = F.conv2d(x, w64, b64)
    assert float((folded - unfolded).abs().max()) <= TOL * float(unfolded.abs().max())
    w32, b32 = O.fold_bn(w, *bn)                                       # the product: the same in fp64, rounded ONCE
    assert w32.dtype == torch.float32 and torch.equal(w32, w64.float()) and torch.equal(b32, b64.float())
    assert not torch.equal(w32, (w * (bn[0] / torch.sqrt(bn[3] + 1e-5)).view(-1, 1, 1, 1)))              # an fp32 fold rounds more often


def test_state_spec_is_the_recipe_and_the_loader_refuses_other_dicts(sd):
    spec = O.state_spec(97)
    assert spec[0][0] == "backbone.conv1._conv.weight" and spec[-1] == ("head.fc.bias", (97,)) and len(spec) == len(sd)
    bad = dict(sd)
    bad.pop("head.fc.bias")
    with pytest.raises(ValueError, match="missing"):
        O.RecModel(bad, 97, device="cpu", ops=X.EmuOps())
    with pytest.raises(ValueError, match="shape"):
        O.RecModel(sd, 6625, device="cpu", ops=X.EmuOps())
    with pytest.raises(ValueError, match="model_lang"):
        O.create_predictor(None, "fr", device="cpu", ops=X.EmuOps())
    with pytest.raises(ValueError, match="not find"):
        O.create_predictor("/nonexistent/ppv3_rec.pth", "en", device="cpu", ops=X.EmuOps())


def test_model_runs_unchanged_over_the_fp64_engine(sd):
    """textflux_amd.ocr.RecModel on EmuOps == the restatement with the folded weights rounded to fp32 (what the loader does)."""
    eng = X.EmuOps()
    model = O.RecModel(sd, 97, device="cpu", ops=eng)
    x = X.node_input()
    got = model(x.permute(0, 2, 3, 1).contiguous().double())
    want = X.forward64(sd, x, round32=True)
    for k in ("ctc", "ctc_neck"):
        assert got[k].shape == want[k].shape
        assert float((got[k] - want[k]).abs().max()) <= TOL * float(want[k].abs().max()), k
    # 1 stem + 13 dw + 13 pw + 2 x 2 squeeze-excite FCs + 5 neck convolutions + 2 x 4 block linears + the head
    assert eng.calls.count("ocr_conv_f32") == 1 + 13 + 4 + 5 + 8 + 1 and eng.calls.count("ocr_conv_dw") == 13
    assert eng.calls.count("ocr_scale_channels") == 2 and eng.calls.count("ocr_attention") == 2 and eng.calls.count("ocr_layernorm") == 5


@pytest.fixture(scope="module")
def rec(sd):
    return O.TextRecognizer(O.RecModel(sd, 97, device="cpu", ops=X.EmuOps()), EN_DICT, (3, 48, 320), 6)


def test_recognizer_over_the_fp64_engine_reproduces_the_fixture(fx, rec):
    """Batching sorted by aspect ratio, the turn of the tall crop, the clamp of the wide one: logits inside four times the reference's
    own fp32 distance of its fp64 logits (the engine's weights are the fp32-rounded fold), the decodes and the losses the fixture's."""
    ctc, neck = rec.pred_imglist(X.fixture_crops())
    margin = 4 * float(fx["crops.ref_fp32_distance"])
    assert ctc.shape == (5, 40, 97) and neck.shape == (5, 40, 64)
    assert float((ctc - fx["crops.ctc"]).abs().max()) <= margin
    for i in range(5):
        ids, tix = rec.decode(ctc[i])
        n = int(fx["crops.count"][i])
        assert list(ids) == fx["crops.ids"][i, :n].tolist() and list(tix) == fx["crops.time_index"][i, :n].tolist()
    loss = rec.get_ctcloss(ctc, X.TARGETS, np.ones(5))
    want = fx["crops.ctcloss"]
    assert torch.isinf(loss[3]) and loss[3] > 0 and torch.isinf(want[3])
    keep = [0, 1, 2, 4]
    assert float((loss[keep] - want[keep]).abs().max()) <= 2 * margin          # -log p moves by at most 2 T delta, then / T
    r = rec.read(X.fixture_crops(), X.TARGETS)
    assert [len(x["ids"]) for x in r] == fx["crops.count"].tolist() and r[1]["text"] == rec.get_text(fx["crops.ids"][1, :int(fx["crops.count"][1])])
    assert rec.read(X.fixture_crops()[:2])[0]["ctc_loss"] is None


def test_dictionary_unknown_character_and_decode(rec):
    assert rec.chars[0] == "sos" and rec.chars[-1] == " " and len(rec.chars) == 97 and rec.chars[1] == "0"
    assert rec.text_ids("a b") == [rec.char2id["a"], 96, rec.char2id["b"]]
    assert rec.text_ids("é") == [96]                                  # an unknown character maps to the last id
    assert rec.get_text([rec.char2id["o"], rec.char2id["k"]]) == "ok"
    mat = torch.full((9, 97), -5.0, dtype=torch.float64)
    for t, c in enumerate([0, 7, 7, 0, 7, 3, 3, 3, 0]):
        mat[t, c] = 1.0
    mat[5, 2] = 1.0                                                    # a tie: the first index wins, as numpy's argmax
    ids, tix = rec.decode(mat)
    assert list(ids) == [7, 7, 2, 3] and list(tix) == [1, 4, 5, 6]
    with pytest.raises(ValueError, match="classes"):
        O.TextRecognizer(O.RecModel(X.seeded_state(97), 97, device="cpu", ops=X.EmuOps()), __file__)
    with pytest.raises(ValueError, match="rec_image_shape"):
        O.TextRecognizer(rec.predictor, EN_DICT, (3, 32, 320))


def test_metrics_and_report_schema():
    assert O.levenshtein("kitten", "sitting") == 3 and O.levenshtein([], [1, 2]) == 2 and O.levenshtein([1, 2], [1, 2]) == 0
    assert O.get_ld([1, 2, 3], [1, 2, 3]) == 1.0
    assert abs(O.get_ld([1, 2, 3, 4], [1, 2]) - (1 - 2 / (4 + 1e-5))) < 1e-15
    assert O.get_ld([], []) == 1.0
    recs = [dict(text="ab", pred="ab", seq_acc=1.0, ned=1.0, ctc_loss=0.5), dict(text="cd", pred="c", seq_acc=0.0, ned=0.5, ctc_loss=2.0)]
    rep = O.report(recs)
    assert set(rep) == {"lines", "line_count", "sen_acc", "ned"} and rep["line_count"] == 2 and rep["sen_acc"] == 0.5 and rep["ned"] == 0.75
    assert O.report([]) == dict(lines=[], line_count=0, sen_acc=0.0, ned=0.0)


def test_score_lines_schema(rec):
    out = O.score_lines(rec, X.fixture_crops()[:2], ["hello", ""])
    assert [set(r) for r in out] == [{"text", "pred", "seq_acc", "ned", "ctc_loss"}] * 2
    assert out[0]["text"] == "hello" and out[0]["seq_acc"] == 0.0 and 0.0 <= out[0]["ned"] < 1.0 and out[0]["ctc_loss"] > 0


def test_line_corners_order():
    """the left two corners by x, each pair by y: tl, tr, br, bl"""
    yy, xx = np.mgrid[10:20, 30:90]
    c = O.line_corners(np.stack([xx.ravel(), yy.ravel()], axis=1))
    assert c.tolist() == [[30, 10], [89, 10], [89, 19], [30, 19]]


# ------------------------------------------------------------------------------------------------------ run_items plumbing, refusals
class StubReader:
    """stands in for the recogniser: reads every crop as 'AB' and remembers the crops' sizes"""
    def __init__(self):
        self.seen = []

    def text_ids(self, text):
        return [ord(c) for c in text]

    def read(self, crops, targets):
        self.seen.append([tuple(c.shape) for c in crops])
        return [dict(text="AB", ids=[65, 66], ctc_loss=1.5) for _ in crops]


def _stub_read_back(monkeypatch):
    made = []
    monkeypatch.setattr(O, "make_reader", lambda cfg, device="cuda": made.append(StubReader()) or made[-1])
    monkeypatch.setattr(O, "crop_line", lambda img, shape, ops=None: torch.zeros(int(np.asarray(shape).shape[0]), 9, 3, dtype=torch.uint8))
    return made


def test_run_items_plumbing_with_a_stubbed_recogniser(monkeypatch, tmp_path):
    from tests.test_batch_driver_cpu import StubPipe, _items, _loader
    from textflux_amd import batch_driver as bd
    made = _stub_read_back(monkeypatch)
    ocr = dict(weights=None, lang="en", dict_path=EN_DICT)
    run = lambda pipe, **kw: bd.run_items(_items()[:3], pipe, None, batch_size=4, device="cpu", loader=_loader, save=lambda i, im: saved.append((i, np.array(im))), **kw)
    saved = []
    off = run(StubPipe(0))
    plain, saved = saved, []
    on = run(StubPipe(0), ocr=ocr)
    assert "ocr" not in off and len(made) == 1                         # one recogniser, made only with the key
    assert all(i == j and (a == b).all() for (i, a), (j, b) in zip(plain, saved))
    assert sorted(on["ocr"]) == [0, 1, 2]
    assert [r["text"] for r in on["ocr"][0]] == ["WORD0"] and [r["text"] for r in on["ocr"][2]] == ["AB2", "CD2"]      # two mask regions, two lines
    r = on["ocr"][2][0]
    assert r == dict(text="AB2", pred="AB", seq_acc=0.0, ned=O.get_ld([65, 66], [65, 66, 50]), ctc_loss=1.5)
    assert len(made[0].seen) == 3 and len(made[0].seen[2]) == 2
    # an eval item: every annotation with a text and a polygon is a line, scaled to the pipeline-size result
    from textflux_amd import glyph
    item = dict(img_name="a.png", annotations=[dict(text="AB", polygon=[[100, 60], [400, 60], [400, 120], [100, 120]]),
                                               dict(text="", polygon=[[0, 0], [5, 5], [9, 0]]), dict(text="second", polygon=[[10, 10], [200, 30], [180, 90]])])
    from PIL import Image
    cfg = dict(original_images_dir="imgs", font=glyph.load_font(None), text_height_ratio=0.1667)
    res = bd.run_items([item], StubPipe(0), None, device="cpu", loader=lambda p: Image.fromarray(np.full((260, 520, 3), 77, np.uint8)), eval_cfg=cfg,
                       save_full=lambda w, f, c: None, ocr=ocr)
    assert [(r["text"], r["seq_acc"]) for r in res["ocr"][0]] == [("AB", 1.0), ("second", 0.0)]


def test_ocr_argument_refusals(tmp_path):
    from textflux_amd import batch_driver as bd
    for bad, msg in ((["x"], "must be a dict"), (dict(dict_path=EN_DICT, model="x"), "unknown keys"), (dict(lang="en"), "dict_path"),
                     (dict(dict_path=EN_DICT, lang="fr"), "lang"), (dict(dict_path=EN_DICT, weights=str(tmp_path / "none.pth")), "does not exist"),
                     (dict(dict_path=EN_DICT, batch=-1), "batch")):
        with pytest.raises(ValueError, match=msg):
            bd.run_items([], object(), None, device="cpu", ocr=bad)
    assert O.ocr_cfg(dict(dict_path=EN_DICT)) == dict(weights=None, lang="ch", dict_path=EN_DICT, image_shape=(3, 48, 320), batch=6)


def test_cli_flags_and_report_file(tmp_path):
    import importlib
    import json
    import sys
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import run_inference as ri
    re_ = importlib.import_module("run_eval")
    a = re_.build_parser().parse_args(["--ocr_weights", "w.pth", "--ocr_lang", "en", "--ocr_dict", "d.txt"])
    assert (a.ocr_weights, a.ocr_lang, a.ocr_dict) == ("w.pth", "en", "d.txt")
    a = re_.build_parser(lora=True).parse_args([])
    assert (a.ocr_weights, a.ocr_lang, a.ocr_dict) == (None, "ch", None)
    a = ri.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w"])
    assert ri.ocr_from_args(a) is None                                 # off by default
    a = ri.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w", "--ocr_weights", "p", "--ocr_dict", "d", "--ocr_lang", "en"])
    assert ri.ocr_from_args(a) == dict(weights="p", lang="en", dict_path="d")
    with pytest.raises(SystemExit):
        ri.ocr_from_args(ri.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w", "--ocr_weights", "p"]))
    with pytest.raises(SystemExit):
        ri.ocr_from_args(ri.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w", "--ocr_dict", "d"]))
    import run_inference_lora as ril
    assert ril.build_parser().parse_args(["--image", "i", "--mask", "m", "--words", "w", "--ocr_lang", "en"]).ocr_lang == "en"
    read = {3: [dict(text="a", pred="a", seq_acc=1.0, ned=1.0, ctc_loss=0.1)], 1: [dict(text="bc", pred="b", seq_acc=0.0, ned=0.5, ctc_loss=2.0)]}
    line = re_.write_ocr_report(read, str(tmp_path))
    rep = json.load(open(tmp_path / "ocr_report.json"))
    assert rep["line_count"] == 2 and rep["sen_acc"] == 0.5 and rep["ned"] == 0.75 and [r["item"] for r in rep["lines"]] == [1, 3] and "0.7500" in line
    re_.write_ocr_report(read, str(tmp_path), rank=1, world=2)
    assert json.load(open(tmp_path / "ocr_report.rank1.json"))["line_count"] == 2
