#!/usr/bin/env python3
"""Single-image TextFlux inference on the MI355X engine -- same CLI and function as the reference's run_inference.py
(flags --image --mask --words [--steps 30 --guidance-scale 30 --seed 42], `run_inference(image, mask, words, num_steps=50,
guidance_scale=30, seed=42)`), own implementation (reference: run_inference.py:44-106, 395-531).

Model locations are LOCAL directories (no hub access in this environment):
    TEXTFLUX_BASE  (default ./models/FLUX.1-Fill-dev)       HF pipeline layout incl. model_index.json
    TEXTFLUX_TRANSFORMER (default ./models/textflux-beta/transformer)
"""
import argparse
import os
import sys

import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from textflux_amd import glyph
from textflux_amd.pipeline import FluxFillPipeline
from textflux_amd.schedulers import FlowMatchMultistepScheduler, StochasticRFOvershotDiscreteScheduler
from textflux_amd.transformer import FluxTransformer2DModel

scheduler_name = "default"  # "overshoot" or "default" (module-level switch, as in the reference :16); "multistep": --multistep
BASE = os.environ.get("TEXTFLUX_BASE", "./models/FLUX.1-Fill-dev")
TRANSFORMER = os.environ.get("TEXTFLUX_TRANSFORMER", "./models/textflux-beta/transformer")

PIPE = None


def load_flux_pipeline(text_encoders: bool = True):
    """run_inference.py:44-57.  text_encoders=False (batch driver, ranks > 0) skips T5 / CLIP: those ranks receive their
    prompt embeddings from rank 0."""
    global PIPE
    if PIPE is None:
        transformer = FluxTransformer2DModel.from_pretrained(TRANSFORMER, torch_dtype=torch.bfloat16)
        skip = {} if text_encoders else dict(text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None)
        PIPE = FluxFillPipeline.from_pretrained(BASE, transformer=transformer, torch_dtype=torch.bfloat16, **skip).to("cuda")
    return PIPE


def use_overshoot_sampler(pipe):
    """Swap in the AMO sampler exactly as the reference does (:79-91): from_config, c = 2, overshot t + dt."""
    sch = StochasticRFOvershotDiscreteScheduler.from_config(pipe.scheduler.config)
    sch.set_c(2.0)
    sch.set_overshot_func(lambda t, dt: t + dt)
    pipe.scheduler = sch


def use_multistep_sampler(pipe):
    """Not in the reference: swap in the second-order multistep sampler (textflux_amd/schedulers.py: FlowMatchMultistepScheduler) on
    the current scheduler's config.  One model evaluation per step, like Euler; meant for fewer steps, with no quality claim."""
    pipe.scheduler = FlowMatchMultistepScheduler.from_config(pipe.scheduler.config)


def apply_scheduler_name(pipe):
    if scheduler_name == "overshoot":
        use_overshoot_sampler(pipe)
    elif scheduler_name == "multistep":
        use_multistep_sampler(pipe)


def run_inference(image_input, mask_input, words_input, num_steps=50, guidance_scale=30, seed=42, pipe=None, paste_back=None, known=None):
    """known (not in the reference): None, or dict(keep_known=..., strength=..., change_map=...) handed to the pipeline call (known-region sampling).
    paste_back (not in the reference): None, or dict(dilate, feather) -- the result is then blended back into the input image under
    the dilated and feathered mask and returned at the INPUT's size (FluxFillPipeline.paste_back) instead of at the pipeline's size.
    seamless (True or dict(smooth, max_shift)), grain (True or dict(ring, max_sigma, strength, min_pixels, seed)) and keyed (True or
    dict(lo, hi, dilate, feather, noise, ring, min_pixels)) in it are handed to that paste.
    With per_line=True in it (batch_driver.run_items' keys: region, color_match, rectify, perspective, curve, seamless, grain, keyed) the input is the plain scene and its mask: every text
    line is edited through its own region with a single-line glyph strip and pasted into the scene (textflux_amd/per_line.py)."""
    image = (Image.open(image_input) if isinstance(image_input, str) else image_input).convert("RGB")
    mask = (Image.open(mask_input) if isinstance(mask_input, str) else mask_input).convert("RGB")
    if paste_back is not None and paste_back.get("per_line"):
        return run_inference_per_line(image, mask, words_input, num_steps, guidance_scale, seed, pipe, paste_back, known)[0]
    image_in, mask_in = image, mask
    new_w, new_h = glyph.pipe_size(image)
    image, mask = image.resize((new_w, new_h)), mask.resize((new_w, new_h))
    words = glyph.read_words_from_text(words_input) if isinstance(words_input, str) else list(words_input)
    prompt = glyph.generate_prompt(words)
    print("Generated prompt:", prompt)
    pipe = pipe or load_flux_pipeline()
    generator = torch.Generator(device="cuda").manual_seed(int(seed))
    apply_scheduler_name(pipe)
    out = pipe(height=new_h, width=new_w, image=image, mask_image=mask, num_inference_steps=num_steps,
               generator=generator, max_sequence_length=512, guidance_scale=guidance_scale,
               prompt=glyph.PROMPT_TEMPLATE2, prompt_2=prompt, **(known or {})).images[0]
    if paste_back is None:
        return out
    pasted = pipe.paste_back(image_in, out, mask_in, **{k: v for k, v in paste_back.items() if k in ("dilate", "feather", "seamless", "grain", "keyed") and v is not None})
    return Image.fromarray(pasted[0].cpu().numpy())


def run_inference_per_line(image, mask, words_input, num_steps, guidance_scale, seed, pipe, paste_back, known=None):
    """-> (the scene with every line pasted in, [each line's raw canvas]): run_inference's per_line path."""
    from textflux_amd import batch_driver, per_line
    cfg = batch_driver._paste_back_cfg(paste_back)
    words = glyph.read_words_from_text(words_input) if isinstance(words_input, str) else list(words_input)
    pipe = pipe or load_flux_pipeline()
    apply_scheduler_name(pipe)
    return per_line.edit_scene(pipe, image, mask, words, cfg, num_inference_steps=num_steps, guidance_scale=guidance_scale, seed=seed,
                               **(dict(call_kw=known) if known else {}))


def add_paste_back_args(ap):
    """Not in the reference: paste-back and region editing (textflux_amd/paste_back.py)."""
    ap.add_argument("--paste_back", action="store_true", help="return the ORIGINAL scene at its original size, changed only under the "
                    "dilated and feathered mask, instead of the pipeline's own pixels at pipeline size")
    ap.add_argument("--paste_dilate", type=int, default=16, metavar="N", help="grow the mask by N pixels before feathering (with --paste_back)")
    ap.add_argument("--paste_feather", type=int, default=4, metavar="N", help="radius of the three box passes that soften the mask's edge (with --paste_back)")
    ap.add_argument("--paste_region", action="store_true", help="edit only a region cut around the mask, not the whole scene (with --paste_back)")
    ap.add_argument("--paste_region_max", type=int, default=1024, metavar="N", help="longer side the region is edited at (with --paste_region)")
    ap.add_argument("--paste_per_line", action="store_true", help="edit every text line through a region of its own, with a single-line glyph "
                    "strip, and paste all of them into the one scene (implies --paste_region; with --paste_back)")
    ap.add_argument("--paste_color_match", action="store_true", help="match each pasted edit's colours to the original's on a ring just "
                    "outside the blend (with --paste_back)")
    ap.add_argument("--paste_color_ring", type=int, default=None, metavar="N", help="width of that ring in pixels, 1..255 (implies "
                    "--paste_color_match; with --paste_back)")
    ap.add_argument("--paste_rectify", action="store_true", help="edit a slanted text line upright: cut it as an oriented rectangle, warp it "
                    "upright, edit it and warp the result back (with --paste_back --paste_per_line)")
    ap.add_argument("--paste_rectify_min_angle", type=float, default=None, metavar="DEG", help="smallest slant that is rectified, default 5 "
                    "(implies --paste_rectify)")
    ap.add_argument("--paste_rectify_max_angle", type=float, default=None, metavar="DEG", help="largest slant that is rectified, default 45 "
                    "(implies --paste_rectify)")
    ap.add_argument("--paste_perspective", action="store_true", help="edit a text line seen in perspective upright: cut it as a quadrilateral, "
                    "warp it upright under a homography, edit it and warp the result back (with --paste_back --paste_per_line)")
    ap.add_argument("--paste_perspective_max_fit", type=float, default=None, metavar="F", help="largest quad area / minimum-area rectangle "
                    "area that still counts as perspective, default 0.9 (implies --paste_perspective)")
    ap.add_argument("--paste_perspective_max_taper", type=float, default=None, metavar="R", help="largest ratio of opposite sides, default 4 "
                    "(implies --paste_perspective)")
    ap.add_argument("--paste_curve", action="store_true", help="edit a text line along a bend upright: cut it as a ribbon around its centre "
                    "line, warp it upright through a control grid, edit it and warp the result back (with --paste_back --paste_per_line)")
    ap.add_argument("--paste_curve_min_bend", type=float, default=None, metavar="F", help="smallest sagitta / thickness that counts as "
                    "curved, default 0.2 (implies --paste_curve)")
    ap.add_argument("--paste_curve_max_squeeze", type=float, default=None, metavar="F", help="largest crop reach / radius of curvature, "
                    "default 0.75 (implies --paste_curve)")
    ap.add_argument("--paste_seamless", action="store_true", help="add a pull-push membrane to each pasted edit before the blend, so that it meets "
                    "the scene at the seam (with --paste_back)")
    ap.add_argument("--paste_seamless_smooth", type=int, default=None, metavar="N", help="Jacobi sweeps after the push, 0..255, default 8 "
                    "(implies --paste_seamless)")
    ap.add_argument("--paste_seamless_max_shift", type=int, default=None, metavar="N", help="largest correction in grey levels, 0..255, "
                    "default 32 (implies --paste_seamless)")
    ap.add_argument("--paste_grain", action="store_true", help="give each pasted edit the noise level of the scene around it: hashed white "
                    "grain under the blend's alpha (with --paste_back)")
    ap.add_argument("--paste_grain_max_sigma", type=float, default=None, metavar="F", help="largest standard deviation that is added, in grey "
                    "levels, 0..64, default 6 (implies --paste_grain)")
    ap.add_argument("--paste_grain_strength", type=float, default=None, metavar="F", help="share of the missing noise that is added, 0..4, "
                    "default 1 (implies --paste_grain)")
    ap.add_argument("--paste_grain_seed", type=int, default=None, metavar="N", help="seed of the grain's hash, default 0 (implies --paste_grain)")
    ap.add_argument("--paste_grain_spectrum", action="store_true", help="also give the grain the shape of the scene's noise: blurred over "
                    "neighbouring pixels and shared between the channels as far as the scene's is (implies --paste_grain)")
    ap.add_argument("--paste_grain_max_blur", type=int, default=None, metavar="N", help="largest side tap of the grain's 3-tap blur in 1/256, "
                    "0..64, default 64 (implies --paste_grain_spectrum)")
    ap.add_argument("--paste_keyed", action="store_true", help="keep the scene's bytes inside each pasted edit wherever the edit did not "
                    "really change them: the blend goes over the scene once more under a key grown from the changed pixels (with --paste_back)")
    ap.add_argument("--paste_keyed_lo", type=int, default=None, metavar="N", help="lower threshold of the change in grey levels, 0..256, "
                    "default 10 (implies --paste_keyed)")
    ap.add_argument("--paste_keyed_hi", type=int, default=None, metavar="N", help="upper threshold: a change is kept where it reaches this, and "
                    "as far around as it stays above the lower one, 0..256, default 28 (implies --paste_keyed)")
    ap.add_argument("--paste_keyed_dilate", type=int, default=None, metavar="N", help="grow the changed pixels by N, at least 3 times the "
                    "feather, default 6 (implies --paste_keyed)")
    ap.add_argument("--paste_keyed_feather", type=int, default=None, metavar="N", help="soften the key's edge over N pixels, default 2 "
                    "(implies --paste_keyed)")
    ap.add_argument("--paste_keyed_noise", type=float, default=None, metavar="F", help="keep the lower threshold F standard deviations of "
                    "the scene's noise above zero, 0..64, default 3 (implies --paste_keyed)")


RECTIFY_FLAGS = ("paste_rectify", "paste_rectify_min_angle", "paste_rectify_max_angle")


def rectify_from_args(a):
    """None, or the `rectify` value of the paste_back dict (True, or a dict of the angles that were given).  The flags are refused
    without --paste_back --paste_per_line."""
    given = [f for f in RECTIFY_FLAGS if getattr(a, f, None) not in (None, False)]
    if not given:
        return None
    if not (a.paste_back and getattr(a, "paste_per_line", False)):
        raise SystemExit(f"--{given[0]} needs --paste_back --paste_per_line")
    angles = {k: getattr(a, "paste_rectify_" + k) for k in ("min_angle", "max_angle") if getattr(a, "paste_rectify_" + k) is not None}
    return angles or True


PERSPECTIVE_FLAGS = ("paste_perspective", "paste_perspective_max_fit", "paste_perspective_max_taper")


def perspective_from_args(a):
    """None, or the `perspective` value of the paste_back dict (True, or a dict of the limits that were given).  The flags are refused
    without --paste_back --paste_per_line."""
    given = [f for f in PERSPECTIVE_FLAGS if getattr(a, f, None) not in (None, False)]
    if not given:
        return None
    if not (a.paste_back and getattr(a, "paste_per_line", False)):
        raise SystemExit(f"--{given[0]} needs --paste_back --paste_per_line")
    limits = {k: getattr(a, "paste_perspective_" + k) for k in ("max_fit", "max_taper") if getattr(a, "paste_perspective_" + k) is not None}
    return limits or True


CURVE_FLAGS = ("paste_curve", "paste_curve_min_bend", "paste_curve_max_squeeze")


def curve_from_args(a):
    """None, or the `curve` value of the paste_back dict (True, or a dict of the limits that were given).  The flags are refused without
    --paste_back --paste_per_line."""
    given = [f for f in CURVE_FLAGS if getattr(a, f, None) not in (None, False)]
    if not given:
        return None
    if not (a.paste_back and getattr(a, "paste_per_line", False)):
        raise SystemExit(f"--{given[0]} needs --paste_back --paste_per_line")
    limits = {k: getattr(a, "paste_curve_" + k) for k in ("min_bend", "max_squeeze") if getattr(a, "paste_curve_" + k) is not None}
    return limits or True


SEAMLESS_FLAGS = ("paste_seamless", "paste_seamless_smooth", "paste_seamless_max_shift")


def seamless_from_args(a):
    """None, or the `seamless` value of the paste_back dict (True, or a dict of the values that were given).  The flags are refused
    without --paste_back."""
    given = [f for f in SEAMLESS_FLAGS if getattr(a, f, None) not in (None, False)]
    if not given:
        return None
    if not a.paste_back:
        raise SystemExit(f"--{given[0]} needs --paste_back")
    values = {k: getattr(a, "paste_seamless_" + k) for k in ("smooth", "max_shift") if getattr(a, "paste_seamless_" + k) is not None}
    return values or True


GRAIN_FLAGS = ("paste_grain", "paste_grain_max_sigma", "paste_grain_strength", "paste_grain_seed", "paste_grain_spectrum",
               "paste_grain_max_blur")


def grain_from_args(a):
    """None, or the `grain` value of the paste_back dict (True, or a dict of the values that were given; its `spectrum` is True or
    dict(max_blur)).  The flags are refused without --paste_back."""
    given = [f for f in GRAIN_FLAGS if getattr(a, f, None) is not None and getattr(a, f) is not False]      # a seed or a strength of 0 is given
    if not given:
        return None
    if not a.paste_back:
        raise SystemExit(f"--{given[0]} needs --paste_back")
    values = {k: getattr(a, "paste_grain_" + k) for k in ("max_sigma", "strength", "seed") if getattr(a, "paste_grain_" + k) is not None}
    if getattr(a, "paste_grain_max_blur", None) is not None:
        values["spectrum"] = dict(max_blur=a.paste_grain_max_blur)
    elif getattr(a, "paste_grain_spectrum", False):
        values["spectrum"] = True
    return values or True


KEYED_FLAGS = ("paste_keyed", "paste_keyed_lo", "paste_keyed_hi", "paste_keyed_dilate", "paste_keyed_feather", "paste_keyed_noise")


def keyed_from_args(a):
    """None, or the `keyed` value of the paste_back dict (True, or a dict of the values that were given).  The flags are refused without
    --paste_back."""
    given = [f for f in KEYED_FLAGS if getattr(a, f, None) is not None and getattr(a, f) is not False]       # a threshold or a noise of 0 is given
    if not given:
        return None
    if not a.paste_back:
        raise SystemExit(f"--{given[0]} needs --paste_back")
    values = {k: getattr(a, "paste_keyed_" + k) for k in ("lo", "hi", "dilate", "feather", "noise") if getattr(a, "paste_keyed_" + k, None) is not None}
    return values or True


def paste_back_from_args(a):
    """None, or the paste_back dict of batch_driver.run_items / process_normal_mode.  The per-line, colour, seamless, grain and keyed keys
    appear only when their flags were given."""
    rectify, perspective, curve, seamless = rectify_from_args(a), perspective_from_args(a), curve_from_args(a), seamless_from_args(a)
    grain, keyed = grain_from_args(a), keyed_from_args(a)
    if not a.paste_back:
        for flag in ("paste_region", "paste_per_line", "paste_color_match", "paste_color_ring"):
            if getattr(a, flag, None) not in (None, False):
                raise SystemExit(f"--{flag} needs --paste_back")
        return None
    pb = dict(dilate=a.paste_dilate, feather=a.paste_feather, region=dict(max_side=a.paste_region_max) if a.paste_region else None)
    if getattr(a, "paste_per_line", False):
        pb["per_line"] = True
    if getattr(a, "paste_color_ring", None) is not None:
        pb["color_match"] = dict(ring=a.paste_color_ring)
    elif getattr(a, "paste_color_match", False):
        pb["color_match"] = True
    if rectify is not None:
        pb["rectify"] = rectify
    if perspective is not None:
        pb["perspective"] = perspective
    if curve is not None:
        pb["curve"] = curve
    if seamless is not None:
        pb["seamless"] = seamless
    if grain is not None:
        pb["grain"] = grain
    if keyed is not None:
        pb["keyed"] = keyed
    return pb


def add_known_region_args(ap):
    """Not in the reference's Fill callers: known-region sampling (FluxFillPipeline.__call__: strength, keep_known)."""
    ap.add_argument("--strength", type=float, default=1.0, metavar="F", help="start the loop from the noised input and run int(steps * F) steps (1.0: from pure noise, all steps)")
    ap.add_argument("--keep_known", action="store_true", help="after every step, replace the latents outside the mask by the input's, noised to the next sigma")
    ap.add_argument("--keep_known_mode", choices=("nearest", "cover"), default="nearest", help="how the pixel mask becomes the latent mask: "
                    "its value at every 8th pixel, or 'cover': masked wherever anything masked touches the latent pixel")
    ap.add_argument("--keep_known_grow", type=int, default=0, metavar="N", help="with cover: also mask the N neighbouring latent pixels (0..8)")
    add_change_map_args(ap)
    add_true_cfg_args(ap)


def add_true_cfg_args(ap):
    """Not in the reference's Fill callers: true CFG (FluxFillPipeline.__call__: true_cfg, negative_prompt)."""
    ap.add_argument("--true_cfg", type=float, default=1.0, metavar="F", help="classifier-free guidance against --negative_prompt: every step runs "
                    "the model on [negative; positive] and steps along neg + F * (pos - neg); > 1 switches it on, at about twice the step cost")
    ap.add_argument("--negative_prompt", type=str, default=None, metavar="STR", help="with --true_cfg > 1: the negative prompt (both text encoders)")


def true_cfg_from_args(a):
    """-> {} (the defaults: today's call), or dict(true_cfg, negative_prompt) for the pipeline call"""
    if a.negative_prompt is None and a.true_cfg == 1.0:
        return {}
    if a.negative_prompt is None:
        raise SystemExit("--true_cfg needs --negative_prompt")
    if not a.true_cfg > 1.0:
        raise SystemExit(f"--negative_prompt needs --true_cfg > 1, got {a.true_cfg}")
    return dict(true_cfg=a.true_cfg, negative_prompt=a.negative_prompt)


def add_change_map_args(ap):
    """Not in the reference's Fill callers: change-map sampling (FluxFillPipeline.__call__: change_map), the map derived from each call's mask."""
    ap.add_argument("--change_map", action="store_true", help="give every latent pixel its own release step: the strokes change fully, a halo "
                    "around them a little, the far field never (the map is the dilated and feathered mask; not with --keep_known)")
    ap.add_argument("--change_dilate", type=int, default=None, metavar="N", help="with --change_map: grow the mask by N pixels (default: the paste-back's)")
    ap.add_argument("--change_feather", type=int, default=None, metavar="N", help="with --change_map: soften the grown mask's edge over N pixels (default: the paste-back's)")
    ap.add_argument("--change_mode", choices=("nearest", "cover"), default="nearest", help="with --change_map: the map's value at every 8th pixel, "
                    "or 'cover': a latent pixel is as free as the freest pixel that touches it")
    ap.add_argument("--change_grow", type=int, default=0, metavar="N", help="with --change_mode cover: also look at the N neighbouring latent pixels (0..8)")
    ap.add_argument("--change_last", choices=("keep", "free"), default="keep", help="with --change_map: held pixels end as the input's latents "
                    "(keep), or the last step belongs to the model (free)")


def change_map_from_args(a):
    """-> None (the defaults: today's call), or the change_map dict of the pipeline call"""
    if not a.change_map:
        if a.change_dilate is not None or a.change_feather is not None or a.change_mode != "nearest" or a.change_grow != 0 or a.change_last != "keep":
            raise SystemExit("--change_dilate / --change_feather / --change_mode / --change_grow / --change_last need --change_map")
        return None
    if a.keep_known:
        raise SystemExit("--change_map and --keep_known exclude each other")
    if a.change_grow < 0 or a.change_grow > 8 or (a.change_mode == "nearest" and a.change_grow):
        raise SystemExit("--change_grow is 0 with --change_mode nearest and 0..8 with cover")
    if (a.change_dilate is not None and a.change_dilate < 0) or (a.change_feather is not None and a.change_feather < 0):
        raise SystemExit("--change_dilate / --change_feather must be >= 0")
    cm = dict(mode=a.change_mode, grow=a.change_grow, last=a.change_last)
    if a.change_dilate is not None:
        cm["dilate"] = a.change_dilate
    if a.change_feather is not None:
        cm["feather"] = a.change_feather
    return cm


def known_region_from_args(a):
    """-> None (the defaults: today's call), or the keyword arguments of the pipeline call"""
    if not a.keep_known and (a.keep_known_mode != "nearest" or a.keep_known_grow != 0):
        raise SystemExit("--keep_known_mode / --keep_known_grow need --keep_known")
    if not 0.0 <= a.strength <= 1.0:
        raise SystemExit(f"--strength must lie in [0, 1], got {a.strength}")
    if a.keep_known and (a.keep_known_grow < 0 or a.keep_known_grow > 8 or (a.keep_known_mode == "nearest" and a.keep_known_grow)):
        raise SystemExit("--keep_known_grow is 0 with --keep_known_mode nearest and 0..8 with cover")
    known = {}
    if a.keep_known:
        known["keep_known"] = dict(mode=a.keep_known_mode, grow=a.keep_known_grow)
    if a.strength != 1.0:
        known["strength"] = a.strength
    cm = change_map_from_args(a)
    if cm is not None:
        known["change_map"] = cm
    known.update(true_cfg_from_args(a))
    return known or None


def add_ocr_args(ap):
    """Not in the reference's Fill callers: read-back (textflux_amd/ocr.py) -- every edited line is cropped from the final image, read by the
    recogniser of the reference's eval/ and scored against its text."""
    ap.add_argument("--ocr_weights", type=str, default=None, metavar="P", help="read the result back: the recogniser's state dict (.pth or "
                    ".safetensors, the reference's ppv3_rec.pth); every line's prediction, sentence accuracy, NED and CTC loss are reported")
    ap.add_argument("--ocr_lang", choices=("ch", "en"), default="ch", help="with --ocr_weights: 'ch' = 6625 classes, 'en' = 97")
    ap.add_argument("--ocr_dict", type=str, default=None, metavar="D", help="with --ocr_weights: the model's character list (ppocr_keys_v1.txt / en_dict.txt)")


def ocr_from_args(a):
    """-> None (the defaults: nothing is constructed or launched), or run_items' ocr dict"""
    if a.ocr_weights is None:
        if a.ocr_dict is not None or a.ocr_lang != "ch":
            raise SystemExit("--ocr_lang / --ocr_dict need --ocr_weights")
        return None
    if a.ocr_dict is None:
        raise SystemExit("--ocr_weights needs --ocr_dict (the character list the model was trained with)")
    return dict(weights=a.ocr_weights, lang=a.ocr_lang, dict_path=a.ocr_dict)


def add_candidates_args(ap):
    """Not in the reference: candidates (textflux_amd/candidates.py) -- every edit is run with N seeds and the one that reads best is kept."""
    ap.add_argument("--candidates", type=int, default=None, metavar="N", help="run every edit with the N seeds seed .. seed + N - 1 and keep the "
                    "one the recogniser reads best (needs --ocr_weights; no default: no quality claim is made)")
    ap.add_argument("--candidates_prune_at", type=int, default=None, metavar="P", help="with --candidates: rank the candidates on their "
                    "clean-image estimates after P steps and finish only the best --candidates_keep of every edit (Euler sampler only)")
    ap.add_argument("--candidates_keep", type=int, default=None, metavar="K", help="with --candidates_prune_at: how many candidates of an "
                    "edit are finished (default 1)")


def candidates_from_args(a):
    """-> None (the defaults: the run without the key), or run_items' candidates dict"""
    if a.candidates is None:
        if a.candidates_prune_at is not None or a.candidates_keep is not None:
            raise SystemExit("--candidates_prune_at / --candidates_keep need --candidates N")
        return None
    if a.candidates < 1:
        raise SystemExit(f"--candidates must be at least 1, got {a.candidates}")
    if a.ocr_weights is None:
        raise SystemExit("--candidates needs --ocr_weights / --ocr_dict: the recogniser chooses among them")
    if a.candidates_keep is not None and a.candidates_prune_at is None:
        raise SystemExit("--candidates_keep needs --candidates_prune_at P")
    prune = None
    if a.candidates_prune_at is not None:
        if getattr(a, "step_cache", None) is not None or getattr(a, "multistep", False) or getattr(a, "scheduler", None) in ("overshoot", "multistep"):
            raise SystemExit("--candidates_prune_at needs the Euler sampler without --step_cache (step windows carry the latents alone)")
        prune = dict(at=a.candidates_prune_at, keep=1 if a.candidates_keep is None else a.candidates_keep)
    return dict(n=a.candidates, prune=prune)


def report_candidates(chosen):
    """prints run_items' "candidates" result: per item and line the seeds, the winner and every candidate's score"""
    for item in sorted(chosen):
        for e in chosen[item]:
            print(f"candidates: item {item} line {e['line']}: seed {e['seeds'][e['chosen']]} of {e['seeds']} kept")
            for s in e["scores"]:
                print(f"candidates:   seed {s['seed']} ({s['stage']}): read {s['pred']!r}, NED {s['ned']:.3f}, CTC loss {s['ctc_loss']:.3f}")


def process_candidates(image_path, mask_path, words_path, steps, guidance_scale, seed, pipe, candidates, ocr, out_dir="outputs_my",
                       paste_back=None, known=None):
    """process_normal_mode with candidates: the one item goes through batch_driver.run_items, which runs, reads and chooses; the winner's
    crop (the pasted scene with paste_back) is saved under crop/ as usual."""
    from textflux_amd import batch_driver
    pipe = pipe or load_flux_pipeline()
    saved = []
    res = batch_driver.run_items([dict(image=image_path, mask=mask_path, text=words_path)], pipe, None, batch_size=max(8, candidates["n"]),
                                 num_inference_steps=steps, guidance_scale=guidance_scale, seed=seed, save=lambda i, img: saved.append(img),
                                 paste_back=paste_back, ocr=ocr, candidates=candidates, **(known or {}))
    if not saved:
        raise SystemExit(f"candidates: the item failed ({res['failed']})")
    os.makedirs(os.path.join(out_dir, "crop"), exist_ok=True)
    n = 1
    while os.path.exists(os.path.join(out_dir, "crop", f"crop_{n:04d}.png")):
        n += 1
    saved[0].save(os.path.join(out_dir, "crop", f"crop_{n:04d}.png"))
    report_candidates(res.get("candidates", {}))
    for r in res["ocr"].get(0, []):
        print(f"read-back: wanted {r['text']!r}, read {r['pred']!r}, NED {r['ned']:.3f}, CTC loss {r['ctc_loss']:.3f}")
    print(f"\nProcessing mode: candidates\nCrop: {out_dir}/crop/crop_{n:04d}.png")
    return saved[0]


def report_read_back(ocr, final, mask, words):
    """Reads every line of `final` (the saved crop) back and prints the records; mask = the scene's mask as loaded."""
    from textflux_amd import ocr as rb
    from textflux_amd import per_line
    cfg = rb.ocr_cfg(ocr)
    lines = [(text, lm) for _, text, lm in per_line.split_lines(mask.convert("L"), words)]
    rep = rb.report(rb.read_lines(rb.make_reader(cfg), final, mask.size, lines))
    for r in rep["lines"]:
        print(f"read-back: wanted {r['text']!r}, read {r['pred']!r}, NED {r['ned']:.3f}, CTC loss {r['ctc_loss']:.3f}")
    print(f"read-back: sentence accuracy {rep['sen_acc']:.3f}, NED {rep['ned']:.3f} over {rep['line_count']} lines")
    return rep


def add_step_cache_args(ap):
    """Not in the reference: the first-block step cache (FluxFillPipeline.enable_step_cache)."""
    ap.add_argument("--step_cache", type=float, default=None, metavar="THR", help="skip the block stack on steps whose first-block residual "
                    "moved by less than THR relative to the last computed step (no default: the value is a property of the checkpoint; 0 never skips)")
    ap.add_argument("--step_cache_max_consecutive", type=int, default=None, metavar="K", help="at most K skipped steps in a row (with --step_cache)")


def apply_step_cache_args(a, pipe):
    if a.step_cache is None:
        if a.step_cache_max_consecutive is not None:
            raise SystemExit("--step_cache_max_consecutive needs --step_cache THR")
        return pipe
    return pipe.enable_step_cache(a.step_cache, max_consecutive=a.step_cache_max_consecutive)


def report_step_cache(pipe):
    rep = getattr(pipe, "step_cache_report", None)
    if getattr(pipe, "_step_cache", None) is not None and rep:
        print(f"Step cache: {sum(1 for r in rep if r['skipped'])} of {len(rep)} steps skipped")


def process_normal_mode(image_path, mask_path, words_path, steps, guidance_scale, seed, pipe=None, out_dir="outputs_my", paste_back=None,
                        known=None, ocr=None):
    """ocr: None, or ocr_from_args' dict: the saved crop is read back line by line (report_read_back).  known: None, or dict(keep_known, strength) for every pipeline call (known_region_from_args).  paste_back: None, or dict(dilate, feather, region) as in batch_driver.run_items -- the saved crop is then the original scene at
    its original size with the edit pasted in; with a region only that part of the scene goes through the pipeline."""
    scene, mask = Image.open(image_path).convert("RGB"), Image.open(mask_path).convert("RGB")
    mask_loaded = mask
    words = glyph.read_words_from_text(words_path)
    work = None
    if paste_back is not None and paste_back.get("per_line"):
        print(f"Using per-line region editing ({len(words)} text lines)")
        pipe = pipe or load_flux_pipeline()
        cropped, fulls = run_inference_per_line(scene, mask, words, steps, guidance_scale, seed, pipe, paste_back, known)
        os.makedirs(os.path.join(out_dir, "crop"), exist_ok=True)
        n = 1
        while os.path.exists(os.path.join(out_dir, f"result_{n:04d}.png")):
            n += 1
        for k, full in enumerate(fulls):     # the raw canvases: line 0 under the usual name, line k after it as _line<k>
            full.save(os.path.join(out_dir, f"result_{n:04d}.png" if k == 0 else f"result_{n:04d}_line{k}.png"))
        cropped.save(os.path.join(out_dir, "crop", f"crop_{n:04d}.png"))
        print(f"\nProcessing mode: per-line\nFull Result: {out_dir}/result_{n:04d}.png")
        if ocr is not None:
            report_read_back(ocr, cropped, mask_loaded, words)
        return cropped
    if paste_back is not None:
        from textflux_amd import batch_driver
        cfg = batch_driver._paste_back_cfg(paste_back)
        scene, mask, so, mo, reg = batch_driver._paste_back_inputs(scene, mask, cfg)
        work = batch_driver.Work(0, None, None, "", {}, scene.size, orig_scene=so, orig_mask=mo, region=reg)
    print("Using multi-line text rendering mode" if len(words) > 1 else "Using single-line text rendering mode")
    combined, cmask, meta = glyph.compose(scene, mask, words)
    print("Starting inference...")
    full = run_inference(combined, cmask, words_path, num_steps=steps, guidance_scale=guidance_scale, seed=seed, pipe=pipe,
                         **(dict(known=known) if known else {}))
    cropped = full.crop(glyph.crop_box(full.size, meta))
    if work is not None:
        cropped = batch_driver._paste_into_original(pipe or load_flux_pipeline(), work, cropped, cfg)
    os.makedirs(os.path.join(out_dir, "crop"), exist_ok=True)
    n = 1
    while os.path.exists(os.path.join(out_dir, f"result_{n:04d}.png")):
        n += 1
    full.save(os.path.join(out_dir, f"result_{n:04d}.png"))
    cropped.save(os.path.join(out_dir, "crop", f"crop_{n:04d}.png"))
    print(f"\nProcessing mode: {meta['mode']}\nFull Result: {out_dir}/result_{n:04d}.png")
    if ocr is not None:
        report_read_back(ocr, cropped, mask_loaded, words)
    return cropped


def build_parser():
    ap = argparse.ArgumentParser(description="Flux Text Generation CLI")
    ap.add_argument("--image", type=str, required=True, help="Path to input image")
    ap.add_argument("--mask", type=str, required=True, help="Path to mask image")
    ap.add_argument("--words", type=str, required=True, help="Path to text file containing words")
    ap.add_argument("--steps", type=int, default=30, help="Number of inference steps")
    ap.add_argument("--guidance-scale", type=float, default=30, help="Guidance scale value")
    ap.add_argument("--seed", type=int, default=42, help="Random seed")
    ap.add_argument("--multistep", action="store_true", help="sample with the second-order multistep sampler instead of Euler (not in "
                    "the reference; one model evaluation per step, meant for fewer --steps)")
    add_known_region_args(ap)
    add_step_cache_args(ap)
    add_paste_back_args(ap)
    add_ocr_args(ap)
    add_candidates_args(ap)
    return ap


def main(argv=None):
    global scheduler_name
    a = build_parser().parse_args(argv)
    paste_back = paste_back_from_args(a)
    known = known_region_from_args(a)
    ocr = ocr_from_args(a)
    candidates = candidates_from_args(a)
    if a.multistep:
        scheduler_name = "multistep"
    pipe = apply_step_cache_args(a, load_flux_pipeline()) if a.step_cache is not None or a.step_cache_max_consecutive is not None else None
    if candidates is not None:
        process_candidates(a.image, a.mask, a.words, a.steps, a.guidance_scale, a.seed, pipe, candidates, ocr, paste_back=paste_back, known=known)
        report_step_cache(pipe)
        print("\nProcessing completed successfully!")
        return
    process_normal_mode(a.image, a.mask, a.words, a.steps, a.guidance_scale, a.seed, pipe=pipe, paste_back=paste_back,
                        **(dict(known=known) if known else {}), **(dict(ocr=ocr) if ocr else {}))
    report_step_cache(pipe)
    print("\nProcessing completed successfully!")


if __name__ == "__main__":
    main()
