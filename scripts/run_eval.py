#!/usr/bin/env python3
"""Batch evaluation driver with the reference's own interface (scripts/run_eval.py:201-213 flags, :76-140 per-item rule,
:168-190 outputs), on the MI355X engine:

    python scripts/run_eval.py --json_path annos.json --original_images_dir imgs/ --weights_path models/textflux/transformer \
        [--output_dir visualization_results --font_path resource/font/Arial-Unicode-Regular.ttf --text_height_ratio 0.1667
         --steps 30 --guidance_scale 30 --seed 42 --num_gpus 4 --scheduler "" | overshoot | multistep
         --strength 1.0 --keep_known --keep_known_mode nearest | cover --keep_known_grow 0
         --change_map --change_dilate N --change_feather N --change_mode nearest | cover --change_grow 0 --change_last keep | free
         --true_cfg F --negative_prompt STR
         --ocr_weights ppv3_rec.pth --ocr_lang ch | en --ocr_dict ppocr_keys_v1.txt]

`annos.json` = {"data_list": [{"img_name": ..., "annotations": [{"text": ..., "polygon": [[x, y], ...]}, ...]}, ...]}; per item
the first annotation is used: polygon -> white-on-black mask, glyph strip of height int(width * text_height_ratio) stacked on
top, resize to multiples of 32, prompt = template / generate_prompt([text]); outputs <output_dir>/full_images/<name> and
<output_dir>/cropped_images/<name> (crop top = int(res_h * strip / (orig_h + strip))).  Items with incomplete annotations
are skipped, per-item failures do not stop the run.  With --ocr_weights every annotation's line is cropped from the item's final image,
read by the recogniser of the reference's eval/ and scored (textflux_amd/ocr.py); <output_dir>/ocr_report.json holds the records.

Where the reference starts --num_gpus worker processes that each pull ONE item at a time from a queue, this script re-executes
itself as --num_gpus ranks under torch.distributed.run (one process per GPU, RCCL) and hands the list to
textflux_amd/batch_driver.py: same-geometry batches of --batch_size (an extra flag, default 8) per pipeline call, dealt
round-robin, every rank encoding its own prompts, the fixed CLIP template broadcast once.  The pre-round-3 {image, mask, text}
list interface is still there behind --items / --out.
Model locations are local directories: --weights_path (transformer) and $TEXTFLUX_BASE (the FLUX.1-Fill-dev pipeline layout).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_data_from_json(json_path):
    """`data_list` of an annos.json; [] (with a message) when the file is missing, malformed or empty (reference :44-58)."""
    try:
        with open(json_path, "r", encoding="utf-8") as f:
            data = json.load(f)
    except FileNotFoundError:
        print(f"Error: JSON file not found at '{json_path}'.")
        return []
    except json.JSONDecodeError:
        print(f"Error: JSON file '{json_path}' has an invalid format.")
        return []
    lst = data.get("data_list", []) if isinstance(data, dict) else []
    if not lst:
        print(f"Warning: The 'data_list' in JSON file '{json_path}' is empty.")
    return lst


def build_parser(lora: bool = False):
    """lora=True: the interface of scripts/run_eval_lora.py (reference :219-232) -- --lora_weights_path instead of --weights_path,
    --scheduler defaults to "overshoot"."""
    ap = argparse.ArgumentParser(description="Batched multi-GPU stitching and FLUX-Fill inference (TextFlux evaluation driver)")
    ap.add_argument("--json_path", type=str, help="Path to the annos.json file containing annotation information")
    ap.add_argument("--original_images_dir", type=str, help="Path to the folder containing original images")
    ap.add_argument("--output_dir", type=str, default="visualization_results", help="Main output folder for results")
    if lora:
        ap.add_argument("--lora_weights_path", type=str, help="Path to lora weights")
        # not in the reference: the LoRA as an unmerged runtime adapter, and its strength (defaults = merged at load, strength 1)
        ap.add_argument("--lora_runtime", action="store_true", help="keep the LoRA unmerged (runtime adapter) instead of merging it at load")
        ap.add_argument("--lora_scale", type=float, default=1.0, help="strength of the LoRA (1.0 = as trained)")
    else:
        ap.add_argument("--weights_path", type=str, help="Path to transformer weights")
    ap.add_argument("--font_path", type=str, default="./resource/font/Arial-Unicode-Regular.ttf", help="Path to the font file (.ttf or .ttc)")
    ap.add_argument("--text_height_ratio", type=float, default=0.1667, help="Ratio of top text line height to image width (default: 1/6)")
    ap.add_argument("--steps", type=int, default=30, help="Inference steps")
    ap.add_argument("--guidance_scale", type=float, default=30, help="Guidance scale")
    ap.add_argument("--seed", type=int, default=42, help="Random seed")
    ap.add_argument("--num_gpus", type=int, default=4, help="Number of GPUs to use")
    ap.add_argument("--scheduler", type=str, default="overshoot" if lora else "", help='Sampler, None, "overshoot" or "multistep" (second order, not in the reference)')
    # not in the reference: batching, and the {image, mask, text} list interface of the earlier rounds
    ap.add_argument("--batch_size", type=int, default=8, help="same-geometry images per pipeline call")
    ap.add_argument("--mixed_pad", type=float, default=0.0, help="let images of different sizes share a batch while at most this share of "
                    "its transformer rows is padding (Euler sampler only; 0 = same-geometry batches only)")
    ap.add_argument("--strength", type=float, default=1.0, metavar="F", help="known-region sampling: start from the noised canvas and run int(steps * F) steps")
    ap.add_argument("--keep_known", action="store_true", help="known-region sampling: after every step, replace the latents outside the mask "
                    "by the canvas's, noised to the next sigma")
    ap.add_argument("--keep_known_mode", choices=("nearest", "cover"), default="nearest", help="latent mask from the pixel mask: its value at "
                    "every 8th pixel, or masked wherever anything masked touches the latent pixel (with --keep_known)")
    ap.add_argument("--keep_known_grow", type=int, default=0, metavar="N", help="with cover: also mask the N neighbouring latent pixels, 0..8")
    ap.add_argument("--true_cfg", type=float, default=1.0, metavar="F", help="true CFG against --negative_prompt: every step runs the model on "
                    "[negative; positive] and steps along neg + F * (pos - neg); > 1 switches it on (not with --mixed_pad, not with --step_cache)")
    ap.add_argument("--negative_prompt", type=str, default=None, metavar="STR", help="with --true_cfg > 1: one negative prompt for all items")
    ap.add_argument("--change_map", action="store_true", help="change-map sampling: every latent pixel gets its own release step from the "
                    "dilated and feathered mask of its call (not with --keep_known)")
    ap.add_argument("--change_dilate", type=int, default=None, metavar="N", help="with --change_map: grow the mask by N pixels (default: the paste-back's)")
    ap.add_argument("--change_feather", type=int, default=None, metavar="N", help="with --change_map: soften the grown mask's edge over N pixels (default: the paste-back's)")
    ap.add_argument("--change_mode", choices=("nearest", "cover"), default="nearest", help="with --change_map: the map at every 8th pixel, or "
                    "'cover': a latent pixel is as free as the freest pixel that touches it")
    ap.add_argument("--change_grow", type=int, default=0, metavar="N", help="with --change_mode cover: also look at the N neighbouring latent pixels, 0..8")
    ap.add_argument("--change_last", choices=("keep", "free"), default="keep", help="with --change_map: held pixels end as the canvas's latents "
                    "(keep), or the last step belongs to the model (free)")
    ap.add_argument("--ocr_weights", type=str, default=None, metavar="P", help="read-back: score every edited line with the recogniser of the "
                    "reference's eval/ (its state dict, .pth or .safetensors) and write ocr_report.json (ocr_report.rank<k>.json per rank "
                    "with more than one) into the output folder")
    ap.add_argument("--ocr_lang", choices=("ch", "en"), default="ch", help="with --ocr_weights: 'ch' = 6625 classes, 'en' = 97")
    ap.add_argument("--ocr_dict", type=str, default=None, metavar="D", help="with --ocr_weights: the model's character list (ppocr_keys_v1.txt / en_dict.txt)")
    import run_inference as ri
    ri.add_candidates_args(ap)       # --candidates N --candidates_prune_at P --candidates_keep K: best of N seeds per edit, chosen by read-back
    ap.add_argument("--step_cache", type=float, default=None, metavar="THR", help="first-block step cache: skip the block stack on steps whose "
                    "first-block residual moved by less than THR relative to the last computed step (no default: the value is a property "
                    "of the checkpoint; 0 never skips)")
    ap.add_argument("--step_cache_max_consecutive", type=int, default=None, metavar="K", help="at most K skipped steps in a row (with --step_cache)")
    ap.add_argument("--paste_back", action="store_true", help="cropped_images/ (and --items outputs) are the ORIGINAL scenes at their original "
                    "size, changed only under the dilated and feathered mask, instead of the pipeline's own pixels at pipeline size")
    ap.add_argument("--paste_dilate", type=int, default=16, metavar="N", help="grow the mask by N pixels before feathering (with --paste_back)")
    ap.add_argument("--paste_feather", type=int, default=4, metavar="N", help="radius of the three box passes that soften the mask's edge (with --paste_back)")
    ap.add_argument("--paste_region", action="store_true", help="edit only a region cut around the mask, not the whole scene (with --paste_back)")
    ap.add_argument("--paste_region_max", type=int, default=1024, metavar="N", help="longer side the region is edited at (with --paste_region)")
    ap.add_argument("--paste_per_line", action="store_true", help="edit every text line (every entry of `annotations`; every mask region of "
                    "an --items entry) through a region of its own and paste all of them into the one scene (implies --paste_region; with --paste_back)")
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
    ap.add_argument("--items", type=str, default=None, help="JSON list of {image, mask, text} instead of --json_path")
    ap.add_argument("--out", type=str, default=None, help="output folder of --items mode")
    ap.add_argument("--num_inference_steps", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--gpus", type=int, default=None, help=argparse.SUPPRESS)
    return ap


def select_tasks(data_list):
    """(tasks, skipped names): the reference queues only items whose first annotation has text and polygon (:229-231)."""
    from textflux_amd import batch_driver
    tasks, skipped = [], []
    for it in data_list:
        if batch_driver.eval_item_complete(it):
            tasks.append(it)
        else:
            skipped.append(it.get("img_name"))
            print(f"Skipping {it.get('img_name')}: Incomplete annotation information.")
    return tasks, skipped


def load_lora_transformer(lora_weights_path, base_transformer=None, lora_runtime: bool = False, lora_scale: float = 1.0):
    """The reference worker's load sequence (scripts/run_eval_lora.py:148-167): the BASE FLUX.1-Fill-dev transformer, the LoRA file
    through FluxFillPipeline.lora_state_dict(return_alphas=True), the format check (every key names a LoRA / DoRA tensor, else
    ValueError("Invalid LoRA checkpoint.")), then load_lora_into_transformer -- which here MERGES the update into the fused weights
    once (textflux_amd/lora.py) instead of wrapping every Linear in a PEFT layer.  `base_transformer`: an already loaded
    transformer (tests); default = $TEXTFLUX_BASE/transformer, the local copy of black-forest-labs/FLUX.1-Fill-dev/transformer."""
    import torch
    import run_inference as ri
    from textflux_amd.pipeline import FluxFillPipeline
    from textflux_amd.transformer import FluxTransformer2DModel
    transformer = base_transformer if base_transformer is not None else FluxTransformer2DModel.from_pretrained(
        ri.BASE, subfolder="transformer", torch_dtype=torch.bfloat16)
    state_dict, network_alphas = FluxFillPipeline.lora_state_dict(lora_weights_path, return_alphas=True)
    if not all("lora" in key or "dora_scale" in key for key in state_dict.keys()):
        raise ValueError("Invalid LoRA checkpoint.")
    if lora_runtime:      # --lora_runtime: attached, not merged (FluxTransformer2DModel.attach_lora)
        FluxFillPipeline.load_lora_into_transformer(state_dict=state_dict, network_alphas=network_alphas, transformer=transformer,
                                                    adapter_name="textflux", runtime=True)
        transformer.set_adapters(["textflux"], [lora_scale])
    elif lora_scale != 1.0:
        from textflux_amd import lora
        lora.merge_lora_into_transformer(state_dict, network_alphas, transformer, scale=lora_scale)
    else:
        FluxFillPipeline.load_lora_into_transformer(state_dict=state_dict, network_alphas=network_alphas, transformer=transformer)
    return transformer


def write_ocr_report(read, out_dir, rank: int = 0, world: int = 1) -> str:
    """ocr_report.json (ocr_report.rank<k>.json with more than one rank, each over its own items): the per-line records in item
    order, each with its item index, and the mean sentence accuracy, the mean NED and the line count, as the reference's
    eval/eval_dgocr.py prints them.  Returns the summary line."""
    from textflux_amd import ocr as rb
    rep = rb.report([dict(r, item=i) for i in sorted(read) for r in read[i]])
    path = os.path.join(out_dir, "ocr_report.json" if world == 1 else f"ocr_report.rank{rank}.json")
    with open(path, "w") as f:
        json.dump(rep, f, ensure_ascii=False, indent=1)
    return f"sentence accuracy {rep['sen_acc']:.4f}, NED {rep['ned']:.4f} over {rep['line_count']} lines -> {path}"


def write_candidates_report(chosen, out_dir, rank: int = 0, world: int = 1) -> str:
    """candidates_report.json next to ocr_report.json (candidates_report.rank<k>.json with more than one rank): run_items' "candidates"
    result in item order -- per edited line the seeds, the winner's position and every candidate's score.  Returns the summary line."""
    path = os.path.join(out_dir, "candidates_report.json" if world == 1 else f"candidates_report.rank{rank}.json")
    works = [dict(e, item=i) for i in sorted(chosen) for e in chosen[i]]
    with open(path, "w") as f:
        json.dump(dict(works=works, work_count=len(works)), f, ensure_ascii=False, indent=1)
    moved = sum(1 for e in works if e["chosen"] != 0)
    return f"{len(works)} edits, {moved} kept another seed than the first -> {path}"


def main(argv=None, lora: bool = False, script: str = __file__):
    a = build_parser(lora).parse_args(argv)
    if a.mixed_pad > 0 and a.scheduler in ("overshoot", "multistep"):
        raise SystemExit("--mixed_pad needs the Euler sampler: mixed-geometry batches carry per-sample coefficients only in the fused Euler step")
    if not a.keep_known and (a.keep_known_mode != "nearest" or a.keep_known_grow != 0):
        raise SystemExit("--keep_known_mode / --keep_known_grow need --keep_known")
    if not 0.0 <= a.strength <= 1.0:
        raise SystemExit(f"--strength must lie in [0, 1], got {a.strength}")
    if a.keep_known and (a.keep_known_grow < 0 or a.keep_known_grow > 8 or (a.keep_known_mode == "nearest" and a.keep_known_grow)):
        raise SystemExit("--keep_known_grow is 0 with --keep_known_mode nearest and 0..8 with cover")
    if (a.keep_known or a.strength != 1.0) and a.mixed_pad > 0:
        raise SystemExit("--keep_known / --strength do not serve mixed-geometry batches (--mixed_pad)")
    known = {}
    if a.keep_known:
        known["keep_known"] = dict(mode=a.keep_known_mode, grow=a.keep_known_grow)
    if a.strength != 1.0:
        known["strength"] = a.strength
    if not a.change_map and (a.change_dilate is not None or a.change_feather is not None or a.change_mode != "nearest" or a.change_grow != 0
                             or a.change_last != "keep"):
        raise SystemExit("--change_dilate / --change_feather / --change_mode / --change_grow / --change_last need --change_map")
    if a.change_map:
        if a.keep_known:
            raise SystemExit("--change_map and --keep_known exclude each other")
        if a.mixed_pad > 0:
            raise SystemExit("--change_map does not serve mixed-geometry batches (--mixed_pad)")
        if a.change_grow < 0 or a.change_grow > 8 or (a.change_mode == "nearest" and a.change_grow):
            raise SystemExit("--change_grow is 0 with --change_mode nearest and 0..8 with cover")
        if (a.change_dilate is not None and a.change_dilate < 0) or (a.change_feather is not None and a.change_feather < 0):
            raise SystemExit("--change_dilate / --change_feather must be >= 0")
        known["change_map"] = dict(mode=a.change_mode, grow=a.change_grow, last=a.change_last,
                                   **{k: v for k, v in (("dilate", a.change_dilate), ("feather", a.change_feather)) if v is not None})
    if a.negative_prompt is not None or a.true_cfg != 1.0:
        if a.negative_prompt is None:
            raise SystemExit("--true_cfg needs --negative_prompt")
        if not a.true_cfg > 1.0:
            raise SystemExit(f"--negative_prompt needs --true_cfg > 1, got {a.true_cfg}")
        if a.mixed_pad > 0:
            raise SystemExit("--true_cfg does not serve mixed-geometry batches (--mixed_pad)")
        if a.step_cache is not None:
            raise SystemExit("--true_cfg does not run with --step_cache")
        known["true_cfg"], known["negative_prompt"] = a.true_cfg, a.negative_prompt
    if a.ocr_weights is None and (a.ocr_dict is not None or a.ocr_lang != "ch"):
        raise SystemExit("--ocr_lang / --ocr_dict need --ocr_weights")
    if a.ocr_weights is not None and a.ocr_dict is None:
        raise SystemExit("--ocr_weights needs --ocr_dict (the character list the model was trained with)")
    ocr = dict(weights=a.ocr_weights, lang=a.ocr_lang, dict_path=a.ocr_dict) if a.ocr_weights is not None else None
    import run_inference as ri
    candidates = ri.candidates_from_args(a)
    if candidates is not None and a.mixed_pad > 0:
        raise SystemExit("--candidates does not serve mixed-geometry batches (--mixed_pad)")
    if candidates is not None and candidates["prune"] is not None and (known or candidates["n"] > a.batch_size):
        raise SystemExit("--candidates_prune_at runs without --keep_known / --strength / --change_map / --true_cfg, and --candidates N must "
                         "not exceed --batch_size")
    if a.step_cache is None and a.step_cache_max_consecutive is not None:
        raise SystemExit("--step_cache_max_consecutive needs --step_cache THR")
    if a.step_cache is not None and a.mixed_pad > 0:
        raise SystemExit("--step_cache does not serve mixed-geometry batches (--mixed_pad)")
    for flag in ("paste_region", "paste_per_line", "paste_color_match", "paste_color_ring"):
        if getattr(a, flag) not in (None, False) and not a.paste_back:
            raise SystemExit(f"--{flag} needs --paste_back")
    if a.paste_back and a.mixed_pad > 0:
        raise SystemExit("--paste_back does not serve mixed-geometry batches (--mixed_pad)")
    paste_back = (dict(dilate=a.paste_dilate, feather=a.paste_feather, region=dict(max_side=a.paste_region_max) if a.paste_region else None)
                  if a.paste_back else None)
    if a.paste_back and a.paste_per_line:
        paste_back["per_line"] = True
    if a.paste_back and (a.paste_color_match or a.paste_color_ring is not None):
        paste_back["color_match"] = True if a.paste_color_ring is None else dict(ring=a.paste_color_ring)
    rectify_given = [f for f in ("paste_rectify", "paste_rectify_min_angle", "paste_rectify_max_angle") if getattr(a, f) not in (None, False)]
    if rectify_given:
        if not (a.paste_back and a.paste_per_line):
            raise SystemExit(f"--{rectify_given[0]} needs --paste_back --paste_per_line")
        angles = {k: getattr(a, "paste_rectify_" + k) for k in ("min_angle", "max_angle") if getattr(a, "paste_rectify_" + k) is not None}
        paste_back["rectify"] = angles or True
    perspective_given = [f for f in ("paste_perspective", "paste_perspective_max_fit", "paste_perspective_max_taper")
                         if getattr(a, f) not in (None, False)]
    if perspective_given:
        if not (a.paste_back and a.paste_per_line):
            raise SystemExit(f"--{perspective_given[0]} needs --paste_back --paste_per_line")
        limits = {k: getattr(a, "paste_perspective_" + k) for k in ("max_fit", "max_taper") if getattr(a, "paste_perspective_" + k) is not None}
        paste_back["perspective"] = limits or True
    curve_given = [f for f in ("paste_curve", "paste_curve_min_bend", "paste_curve_max_squeeze") if getattr(a, f) not in (None, False)]
    if curve_given:
        if not (a.paste_back and a.paste_per_line):
            raise SystemExit(f"--{curve_given[0]} needs --paste_back --paste_per_line")
        limits = {k: getattr(a, "paste_curve_" + k) for k in ("min_bend", "max_squeeze") if getattr(a, "paste_curve_" + k) is not None}
        paste_back["curve"] = limits or True
    seamless_given = [f for f in ("paste_seamless", "paste_seamless_smooth", "paste_seamless_max_shift") if getattr(a, f) not in (None, False)]
    if seamless_given:
        if not a.paste_back:
            raise SystemExit(f"--{seamless_given[0]} needs --paste_back")
        values = {k: getattr(a, "paste_seamless_" + k) for k in ("smooth", "max_shift") if getattr(a, "paste_seamless_" + k) is not None}
        paste_back["seamless"] = values or True
    grain_given = [f for f in ("paste_grain", "paste_grain_max_sigma", "paste_grain_strength", "paste_grain_seed", "paste_grain_spectrum",
                               "paste_grain_max_blur")
                   if getattr(a, f) is not None and getattr(a, f) is not False]             # a seed, a strength or a blur of 0 is given
    if grain_given:
        if not a.paste_back:
            raise SystemExit(f"--{grain_given[0]} needs --paste_back")
        values = {k: getattr(a, "paste_grain_" + k) for k in ("max_sigma", "strength", "seed") if getattr(a, "paste_grain_" + k) is not None}
        if a.paste_grain_max_blur is not None:
            values["spectrum"] = dict(max_blur=a.paste_grain_max_blur)
        elif a.paste_grain_spectrum:
            values["spectrum"] = True
        paste_back["grain"] = values or True
    keyed_given = [f for f in ("paste_keyed", "paste_keyed_lo", "paste_keyed_hi", "paste_keyed_dilate", "paste_keyed_feather", "paste_keyed_noise")
                   if getattr(a, f) is not None and getattr(a, f) is not False]             # a threshold or a noise of 0 is given
    if keyed_given:
        if not a.paste_back:
            raise SystemExit(f"--{keyed_given[0]} needs --paste_back")
        values = {k: getattr(a, "paste_keyed_" + k) for k in ("lo", "hi", "dilate", "feather", "noise") if getattr(a, "paste_keyed_" + k) is not None}
        paste_back["keyed"] = values or True
    legacy = a.items is not None
    weights = a.lora_weights_path if lora else a.weights_path
    if not legacy and not (a.json_path and a.original_images_dir and weights):
        raise SystemExit(f"--json_path, --original_images_dir and --{'lora_' if lora else ''}weights_path are required")
    from textflux_amd import distributed as tdist
    # --items (legacy) mode: --gpus only, no respawn without it (as before the reference CLI was added); the reference interface
    # defaults to --num_gpus 4 like the reference, clamped to the GPUs this host has
    if legacy:
        n_gpus = a.gpus
    else:
        n_gpus = a.gpus or a.num_gpus
        try:
            import torch
            have = torch.cuda.device_count()
        except Exception:
            have = 0
        if have and n_gpus > have:
            print(f"--num_gpus {n_gpus} > {have} visible GPUs: using {have}")
            n_gpus = have
    tdist.respawn_under_torchrun(n_gpus, script, sys.argv[1:] if argv is None else list(argv))
    rank, world, local = tdist.init_from_env()
    import run_inference as ri
    from textflux_amd import batch_driver, glyph
    steps = a.num_inference_steps or a.steps
    if legacy:
        with open(a.items) as f:
            items = json.load(f)
        out_dir, eval_cfg = a.out or a.output_dir, None
        os.makedirs(out_dir, exist_ok=True)
    else:
        data_list = load_data_from_json(a.json_path)
        if not data_list:
            print("Data list is empty, exiting program.")
            tdist.shutdown()
            return
        items, _ = select_tasks(data_list)
        out_dir = a.output_dir
        for d in (out_dir, os.path.join(out_dir, "full_images"), os.path.join(out_dir, "cropped_images")):
            os.makedirs(d, exist_ok=True)
        try:
            from PIL import ImageFont
            font = ImageFont.truetype(a.font_path, size=60)
        except (IOError, OSError):
            font = glyph.load_font(None)
            print(f"Font '{a.font_path}' not found, using default font.")
        eval_cfg = dict(original_images_dir=a.original_images_dir, font=font, text_height_ratio=a.text_height_ratio)
        if not lora:
            ri.TRANSFORMER = a.weights_path
    if lora and weights:      # every rank (the reference: every worker) loads the base transformer and merges the LoRA into it
        import torch
        from textflux_amd.pipeline import FluxFillPipeline
        pipe = FluxFillPipeline.from_pretrained(ri.BASE, transformer=load_lora_transformer(weights, lora_runtime=a.lora_runtime, lora_scale=a.lora_scale), torch_dtype=torch.bfloat16).to("cuda")
    else:
        pipe = ri.load_flux_pipeline(text_encoders=True)     # every rank encodes its own prompts: no rank-0 straggler
    if a.scheduler == "overshoot":
        ri.use_overshoot_sampler(pipe)
    elif a.scheduler == "multistep":
        ri.use_multistep_sampler(pipe)
    pipe.enable_hip_graph(True)
    res = batch_driver.run_items(items, pipe, out_dir, batch_size=a.batch_size, num_inference_steps=steps,
                                 guidance_scale=a.guidance_scale, seed=a.seed, device=f"cuda:{local}", eval_cfg=eval_cfg,
                                 mixed_pad=a.mixed_pad, paste_back=paste_back, **known, **(dict(ocr=ocr) if ocr else {}),
                                 **(dict(candidates=candidates) if candidates else {}),
                                 step_cache=None if a.step_cache is None else dict(threshold=a.step_cache, max_consecutive=a.step_cache_max_consecutive))
    if ocr:
        print(f"[rank {rank}] read-back: " + write_ocr_report(res["ocr"], out_dir, rank, world))
    if "candidates" in res:
        print(f"[rank {rank}] candidates: " + write_candidates_report(res["candidates"], out_dir, rank, world))
    if "steps_total" in res:
        print(f"[rank {rank}] step cache: {res['steps_skipped']} of {res['steps_total']} steps skipped")
    print(f"[rank {rank}] {len(res['done'])} images written" + (f"; {len(res['all_done'])}/{len(items)} in total, "
          f"{res['batches']} batches in {res['rounds']} rounds, prompts encoded {res['encode']}" if rank == 0 else ""))
    if rank == 0:
        print("[rank 0] process group: " + json.dumps(tdist.group_info()))
        print("All tasks processed.")
    tdist.shutdown()


if __name__ == "__main__":
    os.environ.setdefault("TOKENIZERS_PARALLELISM", "false")
    main()
