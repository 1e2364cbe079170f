"""FluxFillPipeline on the MI355X engine -- same `__call__` keyword surface, return types and helper names as the
reference class (diffusers/src/diffusers/pipelines/flux/pipeline_flux_fill.py:1321-2137, "P:" below), so that
`run_inference.py`-style callers can switch by changing one import.

What is different underneath:
* the denoising loop (step_loop.py) never re-enters Python-level model code: per step it is ONE `tfx_dit_step_run_ex3`, or the
  replay of the graph captured from it -- the forward and a scheduler update that also writes the new latents into the next
  x_embedder input (no torch.cat per step, P:2085);
* context projection, RoPE tables and the time/guidance/pooled embedding -> AdaLN modulation of ALL steps are computed
  once before the loop (the reference recomputes them every step);
* the AMO sampler's per-step host syncs are gone (coefficients tabulated on the host).
"""
from __future__ import annotations

import inspect
import json
import os
import warnings
from types import SimpleNamespace
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops, step_loop
from .image_processor import VaeImageProcessor
from .schedulers import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler, StochasticRFOvershotDiscreteScheduler, change_cut_table
from .transformer import EULER_PAD, FluxTransformer2DModel

BF16 = torch.bfloat16


def randn_tensor(shape, generator=None, device=None, dtype=None):
    """randn_tensor (D/utils/torch_utils.py:38-83): a CPU generator draws on the CPU and the result is moved, a list of
    generators seeds each batch row separately."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    batch = shape[0]
    rand_device = device
    if generator is not None:
        gen_dev = (generator[0] if isinstance(generator, list) else generator).device.type
        if gen_dev != device.type and gen_dev == "cpu":
            rand_device = torch.device("cpu")
        elif gen_dev != device.type and gen_dev == "cuda":
            raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gen_dev}.")
    if isinstance(generator, list) and len(generator) == 1:
        generator = generator[0]
    if isinstance(generator, list):
        shape1 = (1,) + tuple(shape[1:])
        lat = [torch.randn(shape1, generator=generator[i], device=rand_device, dtype=dtype) for i in range(batch)]
        return torch.cat(lat, dim=0).to(device)
    return torch.randn(shape, generator=generator, device=rand_device, dtype=dtype).to(device)


def calculate_shift(image_seq_len, base_seq_len: int = 256, max_seq_len: int = 4096, base_shift: float = 0.5,
                    max_shift: float = 1.16):
    """P:1248-1258."""
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    b = base_shift - m * base_seq_len
    return image_seq_len * m + b


def per_sample_schedules(scheduler, image_seq_lens, num_inference_steps: int, sigmas=None, device="cpu"):
    """The sigma schedule of every sample of a mixed-geometry batch: calculate_shift makes mu, and with it every sigma, a function of
    the sample's own image token count (P:1980-1990), so sample b gets set_timesteps(sigmas=..., mu=calculate_shift(S_b)) of
    `scheduler` -- what its single-image call would set.  Returns {"timesteps": [B][n] f32, "sigmas": [B][n + 1] f32 (host),
    "dsigma": [B][n] f32, the bf16-exact Euler coefficients of coef_table}.  Host arithmetic; leaves `scheduler` set for the last
    distinct length."""
    sc = scheduler.config
    base = np.linspace(1.0, 1 / num_inference_steps, num_inference_steps) if sigmas is None else sigmas
    cache = {}
    for S in image_seq_lens:
        if S in cache:
            continue
        mu = calculate_shift(S, sc.base_image_seq_len, sc.max_image_seq_len, sc.base_shift, sc.max_shift)
        ts, n = retrieve_timesteps(scheduler, num_inference_steps, "cpu", sigmas=base, mu=mu)
        cache[S] = (ts.detach().float().cpu().clone(), scheduler._sigmas_host.clone(), scheduler.coef_table("cpu", BF16)[:n].clone())
    pick = lambda k: torch.stack([cache[S][k] for S in image_seq_lens]).to(device)
    return dict(timesteps=pick(0), sigmas=pick(1), dsigma=pick(2))


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, timesteps=None, sigmas=None, **kwargs):
    """P:1262-1318."""
    if timesteps is not None and sigmas is not None:
        raise ValueError("Only one of `timesteps` or `sigmas` can be passed. Please choose one to set custom values")
    params = set(inspect.signature(scheduler.set_timesteps).parameters.keys())
    if timesteps is not None:
        if "timesteps" not in params:
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom timestep schedules.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
    elif sigmas is not None:
        if "sigmas" not in params:
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom sigmas schedules.")
        scheduler.set_timesteps(sigmas=sigmas, device=device, **kwargs)
    else:
        scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
        return scheduler.timesteps, num_inference_steps
    return scheduler.timesteps, len(scheduler.timesteps)


class FluxPipelineOutput(SimpleNamespace):
    """`.images` (P:2137, D/pipelines/flux/pipeline_output.py)."""


class _NullBar:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def update(self, n=1):
        pass


def _check_mode_grow(who, mode, grow):
    """the latent packers' mode / grow, as `keep_known` and `change_map` both take them"""
    if mode not in ("nearest", "cover"):
        raise ValueError(f"{who}: mode must be 'nearest' or 'cover', got {mode!r}")
    if grow < 0 or grow > 8 or (mode == "nearest" and grow != 0):
        raise ValueError(f"{who}: grow is 0 for mode 'nearest' and 0..8 for mode 'cover'")


def _repeat_to_batch(t, total, message):
    """t [b, ...] -> [total, ...] by whole repeats; ValueError(message, with {have} and {total} filled in) where b does not divide total"""
    have = t.shape[0]
    if have < total:
        if total % have:
            raise ValueError(message.format(have=have, total=total))
        t = t.repeat(total // have, *([1] * (t.dim() - 1)))
    return t


def _keep_known_cfg(keep_known):
    """keep_known = None / False | True | dict(mode="nearest" | "cover", grow=int) -> None | (mode, grow)"""
    if keep_known is None or keep_known is False:
        return None
    cfg = {} if keep_known is True else dict(keep_known)
    mode, grow = cfg.pop("mode", "nearest"), int(cfg.pop("grow", 0))
    if cfg:
        raise ValueError(f"keep_known: unknown keys {sorted(cfg)}")
    _check_mode_grow("keep_known", mode, grow)
    return mode, grow


CHANGE_MAP_KEYS = ("map", "dilate", "feather", "mode", "grow", "last")


def _change_map_cfg(change_map):
    """change_map = None / False | True | a grey image / uint8 array / uint8 tensor | dict(map=..., dilate=D, feather=F,
    mode="nearest" | "cover", grow=N, last="keep" | "free") -> None | dict(map, dilate, feather, mode, grow, last).  map None: the map
    is derived from the call's mask_image as feather(dilate(mask >= 128)), the paste-back's alpha (dilate / feather default to the
    paste-back's: starting points, not tuned values)."""
    if change_map is None or change_map is False:
        return None
    from .paste_back import DILATE, FEATHER
    cfg = {} if change_map is True else dict(change_map) if isinstance(change_map, dict) else dict(map=change_map)
    unknown = sorted(k for k in cfg if k not in CHANGE_MAP_KEYS)
    if unknown:
        raise ValueError(f"change_map: unknown keys {unknown}")
    given = cfg.get("map")
    if given is not None and ("dilate" in cfg or "feather" in cfg):
        raise ValueError("change_map: dilate / feather derive the map from mask_image and do not go with an explicit map")
    out = dict(map=given, dilate=int(cfg.get("dilate", DILATE)), feather=int(cfg.get("feather", FEATHER)), mode=cfg.get("mode", "nearest"),
               grow=int(cfg.get("grow", 0)), last=cfg.get("last", "keep"))
    _check_mode_grow("change_map", out["mode"], out["grow"])
    if out["last"] not in ("keep", "free"):
        raise ValueError(f"change_map: last must be 'keep' or 'free', got {out['last']!r}")
    if out["dilate"] < 0 or out["feather"] < 0:
        raise ValueError("change_map: dilate and feather must be >= 0")
    return out


def _true_cfg_on(true_cfg, negative_prompt, negative_prompt_embeds) -> bool:
    """True CFG runs when true_cfg > 1 and a negative prompt OR negative embeds are given.  The reference looks at the string alone
    (pipeline_flux_with_cfg.py:714), so negative embeds without a string silently switch it off there; here both count."""
    return true_cfg > 1 and (negative_prompt is not None or negative_prompt_embeds is not None)


class FluxFillPipeline:
    _callback_tensor_inputs = ["latents", "prompt_embeds"]
    supports_output_crop = True
    supports_device_compose = True   # image / mask_image may be uint8 device tensors [B, H, W, 3] / [B, H, W] (ops.compose_canvas)
    supports_paste_back = True       # paste_back(): the result goes back into the original image under a feathered mask
    model_index_name = "model_index.json"

    def __init__(self, scheduler, vae, text_encoder, tokenizer, text_encoder_2, tokenizer_2,
                 transformer: FluxTransformer2DModel):
        self.scheduler, self.vae, self.transformer = scheduler, vae, transformer
        self.text_encoder, self.tokenizer = text_encoder, tokenizer
        self.text_encoder_2, self.tokenizer_2 = text_encoder_2, tokenizer_2
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1) if self.vae is not None else 8
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor * 2)
        self.mask_processor = VaeImageProcessor(
            vae_scale_factor=self.vae_scale_factor * 2,
            vae_latent_channels=self.vae.config.latent_channels if self.vae is not None else 16,
            do_normalize=False, do_binarize=True, do_convert_grayscale=True)
        self.tokenizer_max_length = self.tokenizer.model_max_length if self.tokenizer is not None else 77
        self.default_sample_size = 128
        self._progress_bar_config: Dict[str, Any] = {}
        self._device = transformer.device if transformer is not None else torch.device("cpu")
        self._guidance_scale, self._joint_attention_kwargs, self._num_timesteps, self._interrupt = None, None, 0, False
        self._use_hip_graph = False
        self.fuse_euler_step = True     # Euler update in proj_out's GEMM epilogue (tfx_dit_desc.euler_gate); False = separate scheduler kernel
        self._step_cache = None         # StepCacheConfig while enable_step_cache() is in force
        self.step_cache_report = None   # per step of the last call with the cache: {"metric": [B floats], "skipped": bool}
        # what a call with step_window=(a, b), b < n, leaves (DESIGN.md section 4 "Candidates"): the packed bf16 [B, S, C] clean-image
        # estimate at sigma_b, and the packed conditioning [B, S, 320] the continuing window takes as masked_image_latents
        self.x0_preview = self.window_conditioning = None

    # ------------------------------------------------------------------ loading / placement
    @classmethod
    def from_pretrained(cls, path: str, transformer: Optional[FluxTransformer2DModel] = None, torch_dtype=BF16,
                        device="cuda", **kwargs):
        """Local HF pipeline directory (model_index.json + one sub-folder per component).  A
        component passed as a keyword overrides the on-disk one (run_inference.py:51-55).  No hub access here."""
        from .vae import AutoencoderKL
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path} is not a local directory (this environment has no hub access)")
        with open(os.path.join(path, cls.model_index_name)) as f:
            json.load(f)
        comp: Dict[str, Any] = dict(kwargs)
        if "scheduler" not in comp:
            with open(os.path.join(path, "scheduler", "scheduler_config.json")) as f:
                comp["scheduler"] = FlowMatchEulerDiscreteScheduler.from_config(json.load(f))
        if "vae" not in comp:
            comp["vae"] = AutoencoderKL.from_pretrained(path, subfolder="vae", torch_dtype=torch_dtype, device=device)
        if transformer is None:
            transformer = FluxTransformer2DModel.from_pretrained(path, subfolder="transformer", torch_dtype=torch_dtype,
                                                                 device=device)
        from . import text_encoders
        for name, enc_cls in (("text_encoder", text_encoders.CLIPTextModel), ("text_encoder_2", text_encoders.T5EncoderModel)):
            if name not in comp:     # the HIP text encoders read the transformers checkpoint layout (config.json + safetensors)
                sub = os.path.join(path, name)
                comp[name] = enc_cls.from_pretrained(sub, torch_dtype=torch_dtype, device=device) if os.path.isdir(sub) else None
        for name, cls_name in (("tokenizer", "CLIPTokenizer"), ("tokenizer_2", "T5TokenizerFast")):
            if name not in comp:
                import transformers
                sub = os.path.join(path, name)
                comp[name] = getattr(transformers, cls_name).from_pretrained(sub) if os.path.isdir(sub) else None
        return cls(transformer=transformer, **{k: comp[k] for k in ("scheduler", "vae", "text_encoder", "tokenizer",
                                                                   "text_encoder_2", "tokenizer_2")})

    def to(self, device=None, dtype=None):
        if device is not None:
            self._device = torch.device(device)
            self.transformer.to(device)
            if self.vae is not None:
                self.vae.to(device)
            for m in (self.text_encoder, self.text_encoder_2):
                if m is not None:
                    m.to(device)
        return self

    @property
    def _execution_device(self):
        return self.transformer.device if self.transformer is not None else self._device

    @property
    def device(self):
        return self._execution_device

    def set_progress_bar_config(self, **kwargs):
        self._progress_bar_config = kwargs

    def progress_bar(self, iterable=None, total=None):
        if self._progress_bar_config.get("disable", False):
            return _NullBar()
        try:
            from tqdm.auto import tqdm
            return tqdm(total=total, **self._progress_bar_config)
        except Exception:
            return _NullBar()

    def maybe_free_model_hooks(self):
        pass                         # nothing is offloaded (reference: D/pipelines/pipeline_utils.py offload hooks)

    def enable_vae_slicing(self):
        """One sample at a time through the VAE (reference: pipeline_flux_fill.py enable_vae_slicing -> AutoencoderKL.enable_slicing);
        bit-identical to the batched result here."""
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        self.vae.disable_slicing()

    def enable_vae_tiling(self):
        """Overlapping VAE tiles blended at the seams (reference: pipeline_flux_fill.py enable_vae_tiling -> AutoencoderKL.enable_tiling,
        autoencoder_kl.py:145-160).  As in the reference this computes a different image from the untiled path; nothing at the
        BASELINE geometries needs it on 288 GB of HBM, it exists so that a caller who sets it gets what the reference gives."""
        self.vae.enable_tiling()

    def disable_vae_tiling(self):
        self.vae.disable_tiling()

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def joint_attention_kwargs(self):
        return self._joint_attention_kwargs

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def interrupt(self):
        return self._interrupt

    # ------------------------------------------------------------------ LoRA (merge at load)
    @classmethod
    def lora_state_dict(cls, path_or_dict, return_alphas: bool = False, weight_name: Optional[str] = None, **_):
        from . import lora
        return lora.lora_state_dict(path_or_dict, return_alphas=return_alphas, weight_name=weight_name)

    @classmethod
    def load_lora_into_transformer(cls, state_dict, network_alphas, transformer, adapter_name=None, _pipeline=None,
                                   low_cpu_mem_usage=False, runtime: bool = False):
        """runtime=False (default): merge into the fused weights.  runtime=True: attach as an unmerged adapter
        (FluxTransformer2DModel.attach_lora) whose strength `joint_attention_kwargs={"scale": s}` / set_adapters() change per call."""
        from . import lora
        if runtime:
            name = adapter_name or f"default_{len(transformer._adapters)}"        # D/loaders/peft.py: get_adapter_name
            transformer.attach_lora(name, state_dict, network_alphas)
            return len({k for k in state_dict if k.endswith(".lora_A.weight")})
        return lora.merge_lora_into_transformer(state_dict, network_alphas, transformer)

    def load_lora_weights(self, path_or_dict, adapter_name=None, runtime: bool = False, **kwargs):
        sd, alphas = self.lora_state_dict(path_or_dict, return_alphas=True, **kwargs)
        self.load_lora_into_transformer(sd, alphas, self.transformer, adapter_name=adapter_name, runtime=runtime)

    # runtime adapters (load_lora_weights(..., runtime=True)): D/loaders/lora_base.py:364-640 forwarded to the transformer
    def set_adapters(self, adapter_names, adapter_weights=None):
        self.transformer.set_adapters(adapter_names, adapter_weights)

    def delete_adapters(self, adapter_names):
        self.transformer.delete_adapters(adapter_names)

    def get_active_adapters(self):
        return self.transformer.get_active_adapters()

    def unload_lora_weights(self):
        self.transformer.unload_lora()

    def fuse_lora(self, lora_scale: float = 1.0, **_):
        self.transformer.fuse_lora(lora_scale)

    # ------------------------------------------------------------------ prompt encoding (HIP text encoders, text_encoders.py;
    # any object with the transformers call signature works -- tokenizers are `transformers` objects)
    def enable_prompt_cache(self, max_entries: int = 256):
        """Keep the encoder outputs of the last `max_entries` distinct prompt strings (0 disables).  TextFlux drives the
        pipeline with ONE fixed CLIP prompt (the template) and T5 prompts that differ only in the quoted words
        (run_inference.py:27-40), so a batch driver re-encodes the same strings over and over.  Results
        are exactly what the encoders return for the string -- the cache only skips the call."""
        self._prompt_cache = {} if max_entries > 0 else None
        self._prompt_cache_max = int(max_entries)
        return self

    def _cached_encode(self, kind, prompts, key_extra, encode):
        """Rows of `encode(list_of_missing_prompts)` ([n, ...] tensor) for every prompt, served from the cache where possible."""
        cache = getattr(self, "_prompt_cache", None)
        if cache is None:
            return encode(prompts)
        rows = {p: cache[(kind, p, key_extra)] for p in dict.fromkeys(prompts) if (kind, p, key_extra) in cache}
        missing = [p for p in dict.fromkeys(prompts) if p not in rows]
        if missing:
            out = encode(missing)
            for p, row in zip(missing, out):
                rows[p] = row.detach().clone()     # this call is served from `rows`, so eviction below cannot hurt it
                if len(cache) >= self._prompt_cache_max:
                    cache.pop(next(iter(cache)))           # oldest entry out
                cache[(kind, p, key_extra)] = rows[p]
        return torch.stack([rows[p] for p in prompts])

    def _get_t5_prompt_embeds(self, prompt=None, num_images_per_prompt: int = 1, max_sequence_length: int = 512,
                              device=None, dtype=None):
        """P:1411-1458."""
        device = device or self._execution_device
        dtype = dtype or self.text_encoder_2.dtype
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)

        def encode(ps):
            ids = self.tokenizer_2(ps, padding="max_length", max_length=max_sequence_length, truncation=True,
                                   return_length=False, return_overflowing_tokens=False, return_tensors="pt").input_ids
            return self.text_encoder_2(ids.to(device), output_hidden_states=False)[0]

        emb = self._cached_encode("t5", prompt, (max_sequence_length, str(device)), encode)
        emb = emb.to(dtype=self.text_encoder_2.dtype, device=device)
        _, seq_len, _ = emb.shape
        emb = emb.repeat(1, num_images_per_prompt, 1)
        return emb.view(batch_size * num_images_per_prompt, seq_len, -1)

    def _get_clip_prompt_embeds(self, prompt, num_images_per_prompt: int = 1, device=None):
        """P:1461-1503."""
        device = device or self._execution_device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)

        def encode(ps):
            ids = self.tokenizer(ps, padding="max_length", max_length=self.tokenizer_max_length, truncation=True,
                                 return_overflowing_tokens=False, return_length=False, return_tensors="pt").input_ids
            return self.text_encoder(ids.to(device), output_hidden_states=False).pooler_output

        emb = self._cached_encode("clip", prompt, (self.tokenizer_max_length, str(device)), encode)
        emb = emb.to(dtype=self.text_encoder.dtype, device=device)
        emb = emb.repeat(1, num_images_per_prompt)
        return emb.view(batch_size * num_images_per_prompt, -1)

    def encode_prompt(self, prompt, prompt_2, device=None, num_images_per_prompt: int = 1, prompt_embeds=None,
                      pooled_prompt_embeds=None, max_sequence_length: int = 512, lora_scale=None):
        """P:1586-1663: CLIP pooled from `prompt`, T5 sequence from `prompt_2` (or `prompt`), text_ids = zeros."""
        device = device or self._execution_device
        if prompt_embeds is None:
            if self.text_encoder is None or self.text_encoder_2 is None:
                raise ValueError("text encoders are not loaded: pass `prompt_embeds` and `pooled_prompt_embeds`")
            prompt = [prompt] if isinstance(prompt, str) else prompt
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            pooled_prompt_embeds = self._get_clip_prompt_embeds(prompt, num_images_per_prompt, device)
            prompt_embeds = self._get_t5_prompt_embeds(prompt_2, num_images_per_prompt, max_sequence_length, device)
        dtype = self.text_encoder.dtype if self.text_encoder is not None else self.transformer.dtype
        text_ids = torch.zeros(prompt_embeds.shape[1], 3).to(device=device, dtype=dtype)
        return prompt_embeds, pooled_prompt_embeds, text_ids

    # ------------------------------------------------------------------ latent helpers (same names as the reference)
    @staticmethod
    def _prepare_latent_image_ids(batch_size, height, width, device, dtype):
        ids = torch.zeros(height, width, 3)
        ids[..., 1] = ids[..., 1] + torch.arange(height)[:, None]
        ids[..., 2] = ids[..., 2] + torch.arange(width)[None, :]
        return ids.reshape(height * width, 3).to(device=device, dtype=dtype)

    @staticmethod
    def _pack_latents(latents, batch_size, num_channels_latents, height, width):
        latents = latents.view(batch_size, num_channels_latents, height // 2, 2, width // 2, 2)
        latents = latents.permute(0, 2, 4, 1, 3, 5)
        return latents.reshape(batch_size, (height // 2) * (width // 2), num_channels_latents * 4)

    @staticmethod
    def _unpack_latents(latents, height, width, vae_scale_factor):
        batch_size, num_patches, channels = latents.shape
        height = 2 * (int(height) // (vae_scale_factor * 2))
        width = 2 * (int(width) // (vae_scale_factor * 2))
        latents = latents.view(batch_size, height // 2, width // 2, channels // 4, 2, 2)
        latents = latents.permute(0, 3, 1, 4, 2, 5)
        return latents.reshape(batch_size, channels // (2 * 2), height, width)

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        """P:1797-1830."""
        height = 2 * (int(height) // (self.vae_scale_factor * 2))
        width = 2 * (int(width) // (self.vae_scale_factor * 2))
        shape = (batch_size, num_channels_latents, height, width)
        ids = self._prepare_latent_image_ids(batch_size, height // 2, width // 2, device, dtype)
        if latents is not None:
            return latents.to(device=device, dtype=dtype), ids
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective "
                             f"batch size of {batch_size}. Make sure the batch size matches the length of the generators.")
        latents = randn_tensor(shape, generator=generator, device=device, dtype=dtype)
        return self._pack_latents(latents, batch_size, num_channels_latents, height, width), ids

    def prepare_mask_latents(self, mask, masked_image, batch_size, num_channels_latents, num_images_per_prompt, height,
                             width, dtype, device, generator):
        """P:1505-1583, same arguments and results ((mask [B,S,256], masked_image_latents [B,S,64])); the arithmetic runs in
        the layout kernels (tfx_prep_image -> VAE encoder -> tfx_vae_sample_pack, tfx_pack_mask)."""
        height = 2 * (int(height) // (self.vae_scale_factor * 2))
        width = 2 * (int(width) // (self.vae_scale_factor * 2))
        dev = self._execution_device
        total = batch_size * num_images_per_prompt
        if masked_image.shape[1] == num_channels_latents:      # already latents: only shift / scale / pack (P:1525-1530)
            mil = (masked_image.to(dev, BF16) - self.vae.config.shift_factor) * self.vae.config.scaling_factor
            mil = self._pack_latents(mil, mil.shape[0], num_channels_latents, height, width)
        else:
            x8 = ops.prep_image(masked_image.to(dev), None, norm_mode=0)
            mil = self._sample_and_pack(self.vae.encode_moments_nhwc(x8), generator, dtype, dev)
        mk = torch.empty(mask.shape[0], mil.shape[1], self.vae_scale_factor ** 2 * 4, dtype=BF16, device=dev)
        ops.pack_mask(mask.to(dev, torch.float32), mk, 0, mask.shape[0], mask.shape[-2], mask.shape[-1], binarize=False)
        if mk.shape[0] < total:
            if not total % mk.shape[0] == 0:
                raise ValueError("The passed mask and the required batch size don't match. Masks are supposed to be duplicated to"
                                 f" a total batch size of {total}, but {mk.shape[0]} masks were passed.")
            mk = mk.repeat(total // mk.shape[0], 1, 1)
        if mil.shape[0] < total:
            if not total % mil.shape[0] == 0:
                raise ValueError("The passed images and the required batch size don't match. Images are supposed to be duplicated"
                                 f" to a total batch size of {total}, but {mil.shape[0]} images were passed.")
            mil = mil.repeat(total // mil.shape[0], 1, 1)
        return mk.to(device=device, dtype=dtype), mil.to(device=device, dtype=dtype)

    def _sample_and_pack(self, moments, generator, dtype, dev, out=None, col0=0):
        """Posterior sample + (z - shift) * scale + 2x2 patchify in one kernel; eps is drawn exactly as the reference's
        `latent_dist.sample(generator)` draws it (randn_tensor of the NCHW latent shape in the pipeline dtype, P:1528)."""
        B, h, w, C2 = moments.shape
        eps = randn_tensor((B, C2 // 2, h, w), generator=generator, device=dev, dtype=dtype)
        if out is None:
            out = torch.empty(B, (h // 2) * (w // 2), 2 * C2, dtype=BF16, device=dev)
        c = self.vae.config
        return ops.vae_sample_pack(moments, eps.to(dev), out, col0, c.shift_factor, c.scaling_factor)

    def _encode_conditioning(self, image, mask_image, height, width, batch_size, num_images_per_prompt, dtype, device, generator):
        """image + mask_image (PIL / numpy / torch, as the reference accepts them) -> masked_image_latents [B, S, 320] =
        [VAE latents of image * (1 - mask) | packed mask] (P:2027-2046).  Host work: decoding / resizing only
        (VaeImageProcessor.to_raw); everything else is device kernels on NHWC tensors."""
        dev = self._execution_device
        raw = self.image_processor.to_raw(image, height=height, width=width)
        rawm = self.mask_processor.to_raw(mask_image, height=height, width=width)
        u8 = raw.dtype == torch.uint8
        H, W = (raw.shape[1], raw.shape[2]) if u8 else (raw.shape[2], raw.shape[3])
        if not u8 and raw.shape[1] == self.vae.config.latent_channels:
            return None, H, W                                     # `image` already holds latents: reference-shaped path
        Hm, Wm = (rawm.shape[1], rawm.shape[2]) if rawm.dtype == torch.uint8 else (rawm.shape[2], rawm.shape[3])
        if (Hm, Wm) != (H, W):
            raise ValueError(f"image ({H}x{W}) and mask ({Hm}x{Wm}) sizes differ after preprocessing")
        raw, rawm = raw.to(dev), rawm.to(dev)
        if u8:
            x8 = ops.prep_image(raw, rawm, norm_mode=1)
        else:
            flag = ops.any_negative(raw) if self.image_processor.do_normalize else None
            x8 = ops.prep_image(raw, rawm, norm_mode=2 if flag is not None else 0, neg_flag=flag)
        B = x8.shape[0]
        total = batch_size * num_images_per_prompt
        moments = self.vae.encode_moments_nhwc(x8)
        S = (H // 16) * (W // 16)
        cond = torch.empty(B, S, 4 * self.vae.config.latent_channels + 256, dtype=BF16, device=dev)
        self._sample_and_pack(moments, generator, dtype, dev, out=cond, col0=0)
        ops.pack_mask(rawm, cond, 4 * self.vae.config.latent_channels, B, H, W, binarize=True)
        if B < total:
            if total % B:
                raise ValueError("The passed images and the required batch size don't match. Images are supposed to be duplicated"
                                 f" to a total batch size of {total}, but {B} images were passed.")
            cond = cond.repeat(total // B, 1, 1)
        return cond, H, W

    def check_inputs(self, prompt, prompt_2, height, width, prompt_embeds=None, pooled_prompt_embeds=None,
                     callback_on_step_end_tensor_inputs=None, max_sequence_length=None, image=None, mask_image=None,
                     masked_image_latents=None, negative_prompt=None, negative_prompt_2=None, negative_prompt_embeds=None,
                     negative_pooled_prompt_embeds=None):
        """P:1665-1724 (same conditions, same exception type); the negative_* conditions are FluxCFGPipeline.check_inputs'
        (D/examples/community/pipeline_flux_with_cfg.py:435-460)."""
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found "
                             f"{[k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to only forward one of the two.")
        elif prompt_2 is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt_2`: {prompt_2} and `prompt_embeds`: {prompt_embeds}. Please make sure to only forward one of the two.")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        elif prompt_2 is not None and (not isinstance(prompt_2, str) and not isinstance(prompt_2, list)):
            raise ValueError(f"`prompt_2` has to be of type `str` or `list` but is {type(prompt_2)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        elif negative_prompt_2 is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt_2`: {negative_prompt_2} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                                 f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds`"
                                 f" {negative_prompt_embeds.shape}.")
        if prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed.")
        if negative_prompt_embeds is not None and negative_pooled_prompt_embeds is None:
            raise ValueError("If `negative_prompt_embeds` are provided, `negative_pooled_prompt_embeds` also have to be passed. Make sure to "
                             "generate `negative_pooled_prompt_embeds` from the same text encoder that was used to generate "
                             "`negative_prompt_embeds`.")
        if max_sequence_length is not None and max_sequence_length > 512:
            raise ValueError(f"`max_sequence_length` cannot be greater than 512 but is {max_sequence_length}")
        if image is not None and masked_image_latents is not None:
            raise ValueError("Please provide either  `image` or `masked_image_latents`, `masked_image_latents` should not be passed.")
        if image is not None and mask_image is None:
            raise ValueError("Please provide `mask_image` when passing `image`.")

    # ------------------------------------------------------------------ the hot loop
    def _timestep_chain(self, t: torch.Tensor, dtype) -> float:
        """Value the sinusoid sees for scheduler timestep t: t.to(dtype) (P:2082) / 1000 (P:2086) -> .to(dtype) * 1000
        (transformer_flux.py:1088); in bf16 890.77 -> 892.0.  Host arithmetic on one scalar."""
        ts = t.detach().reshape(1).to("cpu", torch.float32).to(dtype)
        return float(((ts / 1000).to(dtype) * 1000).float())

    def _modulation_table(self, timesteps, B, pooled, guidance_scale, dsigma=None):
        """AdaLN modulation rows of ALL steps, [n, B, mod_len], rows ordered (step, sample).  timesteps: [n] (every sample on one
        schedule) or [n, B] scheduler timesteps.  dsigma ([n] or [n, B], bf16-exact already: coef_table) -> [n, B, mod_len +
        EULER_PAD]: the step's Euler coefficient travels behind its modulation rows and gates proj_out's epilogue
        (tfx_dit_desc.euler_gate)."""
        tr = self.transformer
        dev = tr.device
        t = timesteps.detach().to("cpu", torch.float32)
        n = t.shape[0]
        t_rows = torch.tensor([self._timestep_chain(x, BF16) for x in t.reshape(-1)], dtype=torch.float32).view(n, -1).expand(n, B)
        g_rows = None
        if tr.config.guidance_embeds:
            g = float((torch.full([1], guidance_scale, dtype=torch.float32).to(BF16) * 1000).float())  # P:2070, :1090
            g_rows = torch.full((n * B,), g, dtype=torch.float32, device=dev)
        mod = tr.modulation(tr.temb(t_rows.reshape(-1).to(dev), g_rows, pooled.to(dev, BF16).repeat(n, 1))).view(n, B, tr.mod_len)
        if dsigma is None:
            return mod
        modx = torch.empty(n, B, tr.mod_len + EULER_PAD, dtype=BF16, device=dev)
        modx[:, :, :tr.mod_len] = mod
        modx[:, :, tr.mod_len:] = dsigma.to(dev, BF16).reshape(n, -1, 1)
        return modx

    def _engine_loop(self, latents, masked_image_latents, prompt_embeds, pooled, text_ids, latent_image_ids, timesteps,
                     guidance_scale, callback_on_step_end, callback_tensor_inputs, amo_noise, progress_bar, keep=None, cfg=None,
                     preview=None):
        """Session, conditioning, modulation table, x_embedder input, then the step loop (step_loop.denoise).  The loop starts at
        step 0 of `timesteps`: _call_body sets the timesteps directly in front of it, which clears the scheduler's begin_index --
        unless the call gave `strength` / `keep_known`: then get_timesteps set it, `timesteps` and the scheduler's tables start at that
        step, and `keep` (dict x0 / noise / mask, or x0 / noise alone for a strength-only call) goes to the loop's blend; with hold
        and last in place of mask (`change_map`) it becomes the loop's `change`, with the cut table of the steps that run.
        cfg: true CFG -- dict(scale, prompt_embeds, pooled), the negative conditioning of the B samples: the
        session then has 2B samples, its conditioning and the pooled rows of the modulation table are [negative; positive] (the
        reference's torch.cat, pipeline_flux_with_cfg.py:739-740), both halves of its xin hold the same [latents |
        masked_image_latents] rows, and Euler runs unfused; the loop state (latents, keep, amo_noise) keeps B samples.
        preview: a step_window that ends early (DESIGN.md section 4 "Candidates") -- dict(sigma, step) for step_loop.denoise; Euler
        then runs unfused too, so that the last step's model output exists in the session's `out`."""
        tr, sch = self.transformer, self.scheduler
        dev = tr.device
        B, S, C = latents.shape
        n = len(timesteps)
        both = lambda neg, pos: pos if cfg is None else torch.cat((neg.to(pos.device, pos.dtype), pos), dim=0)
        cond = lambda pe: both(cfg["prompt_embeds"], pe) if cfg is not None else pe
        Bs = B if cfg is None else 2 * B
        ses = tr.session(Bs, S, prompt_embeds.shape[1])
        ses.set_conditioning(cond(prompt_embeds).to(dev, BF16), text_ids, latent_image_ids)
        halves = (ses.xin,) if cfg is None else (ses.xin[:B], ses.xin[B:])      # sample B + b mirrors sample b
        is_amo = isinstance(sch, StochasticRFOvershotDiscreteScheduler)
        multistep = isinstance(sch, FlowMatchMultistepScheduler)    # unfused: its [n, 2] table, the history in the session
        coef = sch.coef_table(dev, BF16)
        # Euler update in proj_out's epilogue (north_star: "flow-matching Euler step fused into the residual add"); the latents then
        # live in xin[:, :, :C].  Not with a step callback (it wants the latents as a tensor every step) and not for AMO.
        fuse = (self.fuse_euler_step and not is_amo and not multistep and callback_on_step_end is None and C == EULER_PAD
                and tr.out_channels == C and cfg is None         # the fused epilogue would update each half of a CFG batch on its own
                and preview is None)                             # ... and leaves no model output behind for the estimate
        mod = self._modulation_table(timesteps, Bs, pooled if cfg is None else both(cfg["pooled"], pooled), guidance_scale,
                                     coef[:n] if fuse else None)
        # x_embedder input [latents | masked_image_latents]; the step keeps columns 0..C-1 up to date
        latents = latents.to(dev, BF16).contiguous()
        mil = masked_image_latents.to(dev, BF16).contiguous()
        for xin in halves:
            ops.scatter_cols_(latents, xin, 0)
            ops.scatter_cols_(mil, xin, C)
        on_step = None
        if callback_on_step_end is not None:
            def on_step(i, lat):     # lat: the live latents; what the callback returns goes back into the loop's state
                nonlocal prompt_embeds
                kw = {k: {"latents": lat, "prompt_embeds": prompt_embeds}[k] for k in callback_tensor_inputs}
                out = callback_on_step_end(self, i, timesteps[i], kw) or {}
                new_lat = out.pop("latents", lat)
                if new_lat is not lat:
                    lat.copy_(new_lat.to(dev, BF16))
                    for xin in halves:
                        ops.scatter_cols_(lat, xin, 0)
                new_pe = out.pop("prompt_embeds", prompt_embeds)
                if new_pe is not prompt_embeds:
                    prompt_embeds = new_pe
                    ses.set_conditioning(cond(prompt_embeds).to(dev, BF16), text_ids, latent_image_ids)
        sch._step_index = sch.begin_index or 0
        change = None
        if keep is not None and "hold" in keep:
            change = dict(x0=keep["x0"], noise=keep["noise"], hold=keep["hold"], sigma=sch.keep_sigma_table(dev, BF16),
                          cut=change_cut_table(n, keep["last"]).to(dev))
            keep = None
        elif keep is not None and "mask" in keep:
            keep = dict(keep, sigma=sch.keep_sigma_table(dev, BF16))
        else:
            keep = None
        return step_loop.denoise(self, ses, mod, latents, coef, n, progress_bar, is_amo, fuse, amo_noise, on_step, multistep,
                                 cfg=None if cfg is None else cfg["scale"], keep=keep, change=change, preview=preview)

    # ------------------------------------------------------------------ known-region sampling
    def get_timesteps(self, num_inference_steps, strength, device):
        """FluxInpaintPipeline.get_timesteps (D/pipelines/flux/pipeline_flux_inpaint.py:420-429), set_begin_index included."""
        init_timestep = min(num_inference_steps * strength, num_inference_steps)
        t_start = int(max(num_inference_steps - init_timestep, 0))
        timesteps = self.scheduler.timesteps[t_start * self.scheduler.order:]
        if hasattr(self.scheduler, "set_begin_index"):
            self.scheduler.set_begin_index(t_start * self.scheduler.order)
        return timesteps, num_inference_steps - t_start

    def _prepare_known_region(self, noise, given_latents, image_latents, image, mask_image, keep_cfg, strength, height, width, dtype,
                              device, generator, change_cfg=None):
        """The original's latents x0, the start of a strength < 1 call and the loop's keep buffers.  x0: `image_latents`, or the VAE
        latents of the UNMASKED preprocessed image (posterior sample, shift / scale, pack) -- drawn here, after every draw the plain
        call makes.  noise: the initial noise (caller-given latents are both noise and start: the reference's quirk, :586-588).
        Returns (start latents, dict(x0, noise[, mask])); with change_cfg (`change_map`) the dict carries hold and last instead of mask."""
        dev = self._execution_device
        total = noise.shape[0]
        if image_latents is not None:
            x0 = image_latents.to(dev, BF16)
        else:
            if image is None:
                raise ValueError("strength / keep_known need `image` (or `image_latents`): the known region is the original's latents")
            raw = self.image_processor.to_raw(image, height=height, width=width)
            if raw.dtype != torch.uint8 and raw.shape[1] == self.vae.config.latent_channels:
                raise ValueError("strength / keep_known with `image` given as VAE latents: pass them packed as `image_latents`")
            raw = raw.to(dev)
            if raw.dtype == torch.uint8:
                x8 = ops.prep_image(raw, None, norm_mode=1)
            else:
                flag = ops.any_negative(raw) if self.image_processor.do_normalize else None
                x8 = ops.prep_image(raw, None, norm_mode=2 if flag is not None else 0, neg_flag=flag)
            x0 = self._sample_and_pack(self.vae.encode_moments_nhwc(x8), generator, dtype, dev)
        x0 = _repeat_to_batch(x0, total, "Cannot duplicate `image` of batch size {have} to {total} text prompts.")
        noise = noise.to(dev, BF16).contiguous()
        x0 = x0.contiguous()
        if x0.shape != noise.shape:
            raise ValueError(f"image latents {tuple(x0.shape)} do not match the latents {tuple(noise.shape)}")
        keep = dict(x0=x0, noise=noise)
        start = noise
        if strength < 1.0 and not given_latents:
            # scale_noise(x0, sigma[t_start], noise) as the blend with an all-zero mask: 0 * (-0) = -0 leaves every value, -0 included
            start = torch.full_like(noise, -0.0)
            sigma = self.scheduler._run_sigmas()[:1].to(BF16).float().to(dev)
            ops.known_region_blend(start, x0, noise, torch.zeros_like(noise), sigma)
        if keep_cfg is not None:
            if mask_image is None:
                raise ValueError("keep_known needs `mask_image`: the known region is what lies outside it")
            mk = ops.keep_mask_pack(self._mask_image_u8(mask_image, height, width, dev), x0.shape[-1], keep_cfg[0], keep_cfg[1])
            mk = _repeat_to_batch(mk, total, "The passed mask and the required batch size don't match. Masks are supposed to be duplicated to"
                                             " a total batch size of {total}, but {have} masks were passed.")
            if mk.shape != x0.shape:
                raise ValueError(f"mask_image packs to {tuple(mk.shape)}, the latents are {tuple(x0.shape)}")
            keep["mask"] = mk
        if change_cfg is not None:
            keep["hold"] = self._change_hold(change_cfg, mask_image, height, width, total, x0.shape[1], dev)
            keep["last"] = change_cfg["last"]
        return start, keep

    def _mask_image_u8(self, mask_image, height, width, device):
        """-> the call's mask as uint8 [B, height, width] on the device, a float mask cut at 0.5 (>= 128 is inside the mask)"""
        rawm = self.mask_processor.to_raw(mask_image, height=height, width=width).to(device)
        if rawm.dtype != torch.uint8:
            rawm = (rawm.reshape(rawm.shape[0], rawm.shape[-2], rawm.shape[-1]) >= 0.5).to(torch.uint8) * 255
        return rawm

    # ------------------------------------------------------------------ change-map sampling
    def change_map_u8(self, change_cfg, mask_image, height, width, device):
        """The call's change map, uint8 [B, height, width] on the device (255 = free from the first step, 0 = never changes): the
        explicit map of the configuration, or feather(dilate(mask_image >= 128)) -- the paste-back's alpha of the same mask."""
        given = change_cfg["map"]
        if given is None:
            if mask_image is None:
                raise ValueError("change_map needs `mask_image` (the map is derived from it) or an explicit map")
            from .paste_back import alpha_mask
            return alpha_mask(self._mask_image_u8(mask_image, height, width, device).contiguous(), change_cfg["dilate"], change_cfg["feather"])
        if isinstance(given, np.ndarray):
            given = torch.from_numpy(np.ascontiguousarray(given))
        if isinstance(given, torch.Tensor):
            if given.dtype != torch.uint8 or given.dim() not in (2, 3):
                raise ValueError(f"change_map: an array / tensor map must be uint8 [H, W] or [B, H, W], got {given.dtype} {tuple(given.shape)}")
            m = given if given.dim() == 3 else given[None]
        else:
            m = self.mask_processor.to_raw(given, height=height, width=width)
            if m.dtype != torch.uint8 or m.dim() != 3:
                raise ValueError("change_map: the map must be an 8-bit grey image, a uint8 array or a uint8 tensor")
        if tuple(m.shape[1:]) != (height, width):
            raise ValueError(f"change_map: the map is {tuple(m.shape[1:])}, the call asks for {(height, width)}")
        return m.to(device).contiguous()

    def _change_hold(self, change_cfg, mask_image, height, width, total, S, device):
        """-> the hold bytes uint8 [total, S, 4] of the call (ops.change_map_pack of its change map), duplicated like a mask"""
        hold = ops.change_map_pack(self.change_map_u8(change_cfg, mask_image, height, width, device), change_cfg["mode"], change_cfg["grow"])
        hold = _repeat_to_batch(hold, total, "The passed change_map and the required batch size don't match. Maps are supposed to be duplicated"
                                             " to a total batch size of {total}, but {have} maps were passed.")
        if tuple(hold.shape) != (total, S, 4):
            raise ValueError(f"change_map packs to {tuple(hold.shape)}, the latents have {(total, S)} tokens")
        return hold.contiguous()

    def enable_hip_graph(self, on: bool = True):
        """Replay ONE captured hipGraph per denoising step (device-side step cursor: modulation rows and scheduler
        coefficients are selected by an int32 on the device, so the same graph serves every step).  Used when no
        `callback_on_step_end` is given and there is more than one step; the graph is captured from the step the eager form
        runs (step_loop.run_steps), so the results are bit-identical."""
        self._use_hip_graph = bool(on)
        return self

    # ------------------------------------------------------------------ first-block step cache (DESIGN.md section 4 "Step cache")
    def enable_step_cache(self, threshold, skip_steps=None, max_consecutive=None):
        """Opt-in and approximate, like enable_fp8() (no reference counterpart: the reference runs every block on every step).  Every
        step runs the embedders and block 0 and measures, per sample, how far the first block's residual moved since the last fully
        computed step: metric = sum |f - f_prev| / sum |f_prev|.  When the largest metric of the batch is below `threshold`, blocks
        1 ... n are not run: the last computed step's residual of those blocks is added instead, then norm_out / proj_out and the
        sampler update as usual.  Step 0 is always computed; cache state never outlives a call.

        threshold has NO default: a useful value is a property of the checkpoint.  To choose one, run with threshold=0 (which never
        skips and is bit-equal to the plain loop) and read `pipe.step_cache_report`: per step {"metric": [B floats], "skipped": bool}.
        skip_steps: an explicit set of steps to skip whatever their metric.  max_consecutive: at most this many threshold skips in a
        row.  The batch's largest metric decides, so a sample's result depends on its batch-mates while the cache is on.  Not for
        call_mixed (raises); a foreign scheduler object's loop ignores it with a warning; every rank of a multi-GPU run decides alone."""
        from .step_cache import StepCacheConfig
        self._step_cache = StepCacheConfig.make(threshold, skip_steps, max_consecutive)
        return self

    def disable_step_cache(self):
        self._step_cache = None
        return self

    # ------------------------------------------------------------------ paste-back (DESIGN.md section 4 "Paste-back")
    def paste_back(self, original, edited, mask, dilate: int = 16, feather: int = 4, color_match=None, color_ref=None, rect=None,
                   origin=(0, 0), seamless=None, grain=None, keyed=None) -> torch.Tensor:
        """The edited image blended into the ORIGINAL one, at the original's size, under the dilated and feathered mask
        (textflux_amd/paste_back.py::paste): pixels outside the mask grown by dilate + 3 feather keep their bytes.  Opt-in, no reference
        counterpart.  original / edited: a PIL image, a uint8 array or tensor [H, W, 3] / [B, H, W, 3], or a list of PIL images (edited
        may have another size: it is resampled with Pillow's bicubic on the device); mask: the same forms, grey [H, W] or RGB (PIL's
        "L" of it is taken).  color_match: None, or True / dict(ring, gain, max_shift, min_pixels): the edit's colours are matched to
        those of color_ref (the forms of `original`, at its size; None: `original`) on a ring just outside the blend before the blend
        (paste_back.paste).  rect (a rectify.Rect, a perspective.Quad or a curve.Ribbon) with origin: `edited` is the upright result of a rectified line and `original` the scene
        window at `origin`; the edit is warped into the window before the blend (paste_back.paste).  seamless: None, or True /
        dict(smooth, max_shift): a pull-push membrane of the difference to color_ref (None: `original`), known just outside the blend,
        is added to the edit before the blend (paste_back.paste; DESIGN.md section 4 "Seamless paste"); color_ref may then be given
        without color_match.  grain: None, or True / dict(ring, max_sigma, strength, min_pixels, seed): after the blend the pasted pixels
        get the noise level of color_ref (None: `original`) just outside the blend, as hashed white grain anchored at the scene position
        `origin` + the pixel's place in `original` (paste_back.paste; DESIGN.md section 4 "Grain match"); color_ref may then be given
        without color_match.  keyed: None, or True / dict(lo, hi, dilate, feather, noise, ring, min_pixels): behind the blend and in
        front of the grain, a pixel keeps `original`'s byte unless the blend really differs there (paste_back.paste; DESIGN.md section 4
        "Keyed paste"); color_ref may then be given without color_match.  Returns uint8 [B, H, W, 3] on the device."""
        from . import paste_back as pb
        dev = self._execution_device

        def rgb(x):
            if isinstance(x, torch.Tensor):
                t = x
            else:
                xs = x if isinstance(x, (list, tuple)) else [x]
                if all(hasattr(i, "convert") for i in xs):
                    t = torch.from_numpy(np.stack([np.array(i.convert("RGB")) for i in xs]))
                else:
                    t = torch.from_numpy(np.ascontiguousarray(x))
            t = t[None] if t.dim() == 3 else t
            if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
                raise ValueError(f"paste_back: images must be uint8 [H, W, 3] or [B, H, W, 3], got {t.dtype} {tuple(t.shape)}")
            return t.to(dev).contiguous()

        def grey(x, hw):
            if isinstance(x, torch.Tensor):
                t = x
            else:
                xs = x if isinstance(x, (list, tuple)) else [x]
                if all(hasattr(i, "convert") for i in xs):
                    t = torch.from_numpy(np.stack([pb.grey_of(i) for i in xs]))
                else:
                    t = torch.from_numpy(np.ascontiguousarray(x))
            if t.dtype != torch.uint8:
                raise ValueError(f"paste_back: the mask must be uint8, got {t.dtype}")
            t = t.to(dev)
            if t.dim() == 4 or (t.dim() == 3 and t.shape[-1] == 3 and tuple(t.shape[:2]) == hw):   # RGB mask: PIL's "L" on the device
                t = ops.rgb_to_grey(t.contiguous())
            return (t[None] if t.dim() == 2 else t).contiguous()

        original = rgb(original)
        kw = {} if rect is None else dict(rect=rect, origin=origin)
        if seamless is not None:
            kw["seamless"] = seamless
        if grain is not None:
            kw.update(grain=grain, origin=origin)
        if keyed is not None:
            kw["keyed"] = keyed
        if color_match is None and color_ref is None:
            return pb.paste(original, rgb(edited), grey(mask, tuple(original.shape[1:3])), dilate, feather, **kw)
        return pb.paste(original, rgb(edited), grey(mask, tuple(original.shape[1:3])), dilate, feather, color_match=color_match,
                        color_ref=None if color_ref is None else rgb(color_ref), **kw)

    # ------------------------------------------------------------------ line warps (DESIGN.md section 4 "Rectified lines" and after)
    def _warp_image(self, name: str, image) -> torch.Tensor:
        """A uint8 image (array or tensor, [H, W, C] or [B, H, W, C]) as a contiguous uint8 [B, H, W, C] tensor on the device; others
        are refused under the caller's `name`."""
        t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
        t = t[None] if t.dim() == 3 else t
        if t.dtype != torch.uint8 or t.dim() != 4:
            raise ValueError(f"{name}: the image must be uint8 [H, W, C] or [B, H, W, C], got {t.dtype} {tuple(t.shape)}")
        return t.to(self._execution_device).contiguous()

    def warp_affine(self, image, m, out_size, coverage: bool = False):
        """A uint8 image (array or tensor, [H, W, C] or [B, H, W, C], C in 1..4) sampled under the Q16 affine matrix m (int64 [6] or
        [B, 6]; rectify.matrices) into out_size = (out_h, out_w) on the device (ops.warp_affine_u8): the resampler of the rectified
        per-line path.  Returns uint8 [B, out_h, out_w, C] on the device, with coverage=True also the coverage [B, out_h, out_w]."""
        return ops.warp_affine_u8(self._warp_image("warp_affine", image), m, out_size, coverage=coverage)

    def warp_perspective(self, image, m, out_size, coverage: bool = False):
        """warp_affine under a homography: m is int64 [9] or [B, 9] (perspective.matrices; ops.warp_perspective_u8), the resampler of
        the perspective per-line path.  Returns uint8 [B, out_h, out_w, C] on the device, with coverage=True also the coverage
        [B, out_h, out_w]."""
        return ops.warp_perspective_u8(self._warp_image("warp_perspective", image), m, out_size, coverage=coverage)

    def warp_grid(self, image, grid, shift, out_size, coverage: bool = False):
        """warp_affine under a control grid: grid is int64 [gh, gw, 2] or [B, gh, gw, 2] of Q16 source positions, one node per
        (1 << shift) destination pixels (curve.grids; ops.warp_grid_u8), the resampler of the curved per-line path and, at shift = 0, a
        per-pixel remap.  Returns uint8 [B, out_h, out_w, C] on the device, with coverage=True also the coverage [B, out_h, out_w]."""
        return ops.warp_grid_u8(self._warp_image("warp_grid", image), grid, shift, out_size, coverage=coverage)

    def _generic_loop(self, latents, masked_image_latents, prompt_embeds, pooled, text_ids, latent_image_ids, timesteps,
                      guidance, callback_on_step_end, callback_tensor_inputs, progress_bar):
        """Reference-shaped loop (P:2077-2116) for foreign scheduler objects: transformer.forward + scheduler.step."""
        if self._step_cache is not None:
            warnings.warn("the step cache lives in the engine's step loop; the loop for a foreign scheduler object ignores it")
        for i, t in enumerate(timesteps):
            if self._interrupt:
                continue
            timestep = t.expand(latents.shape[0]).to(latents.dtype)
            noise_pred = self.transformer(hidden_states=torch.cat((latents, masked_image_latents), dim=2),
                                          timestep=timestep / 1000, guidance=guidance, pooled_projections=pooled,
                                          encoder_hidden_states=prompt_embeds, txt_ids=text_ids, img_ids=latent_image_ids,
                                          joint_attention_kwargs=self.joint_attention_kwargs, return_dict=False)[0]
            latents = self.scheduler.step(noise_pred, t, latents, return_dict=False)[0]
            if callback_on_step_end is not None:
                kw = {k: {"latents": latents, "prompt_embeds": prompt_embeds}[k] for k in callback_tensor_inputs}
                out = callback_on_step_end(self, i, t, kw) or {}
                latents = out.pop("latents", latents)
                prompt_embeds = out.pop("prompt_embeds", prompt_embeds)
            progress_bar.update()
        return latents

    def _decode_to_output(self, latents, height, width, output_type, crop=None):
        """P:2126-2129 + VaeImageProcessor.postprocess: un-patchify, z / scale + shift, VAE decode, denormalise, and the
        output layout, all on NHWC device tensors; only the finished uint8 / float32 image crosses to the host."""
        if output_type not in ("pt", "np", "pil", "u8"):
            raise ValueError(f"unknown output_type {output_type}")
        c = self.vae.config
        h = 2 * (int(height) // (self.vae_scale_factor * 2))
        w = 2 * (int(width) // (self.vae_scale_factor * 2))
        z = ops.unpack_latents(latents.to(self._execution_device, BF16).contiguous(), h, w, c.shift_factor, c.scaling_factor)
        img = self.vae.decode_nhwc(z)
        denorm = self.image_processor.do_normalize
        if output_type == "pt":
            return ops.postprocess(img, c.out_channels, "pt", denorm, crop)
        if output_type == "np":
            return ops.postprocess(img, c.out_channels, "np", denorm, crop).cpu().numpy()
        if output_type == "u8":        # the "pil" output's bytes as a device uint8 [B, H, W, C] tensor: nothing crosses to the host
            return ops.postprocess(img, c.out_channels, "u8", denorm, crop)
        import PIL.Image
        u8 = ops.postprocess(img, c.out_channels, "u8", denorm, crop).cpu().numpy()
        if u8.shape[-1] == 1:
            return [PIL.Image.fromarray(a.squeeze(), mode="L") for a in u8]
        return [PIL.Image.fromarray(a) for a in u8]

    @torch.no_grad()
    def decode_latents(self, latents, height, width, output_type: str = "u8", output_crop=None):
        """Packed latents [B, S, C] (a call's output_type="latent" result, or `x0_preview`) -> what the call itself would have
        returned for them under output_type / output_crop: the same decode, nothing else."""
        return self._decode_to_output(latents, height, width, output_type, output_crop)

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str]] = None, prompt_2: Optional[Union[str, List[str]]] = None,
                 image=None, mask_image=None, masked_image_latents: Optional[torch.Tensor] = None,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 sigmas: Optional[List[float]] = None, guidance_scale: float = 30.0,
                 num_images_per_prompt: Optional[int] = 1, generator=None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, pooled_prompt_embeds: Optional[torch.Tensor] = None,
                 output_type: Optional[str] = "pil", return_dict: bool = True,
                 joint_attention_kwargs: Optional[Dict[str, Any]] = None,
                 callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 512,
                 amo_noise: Optional[List[torch.Tensor]] = None, output_crop=None, strength: float = 1.0, keep_known=None,
                 image_latents: Optional[torch.Tensor] = None, change_map=None,
                 negative_prompt: Optional[Union[str, List[str]]] = None, negative_prompt_2: Optional[Union[str, List[str]]] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, negative_pooled_prompt_embeds: Optional[torch.Tensor] = None,
                 true_cfg: float = 1.0, step_window: Optional[Tuple[int, int]] = None):
        """Same arguments / defaults / return as the reference `__call__` (P:1850-1873, 2122-2137).  Additions:
        `output_type="u8"`: the "pil" output's bytes as a device uint8 [B, H, W, 3] tensor (with `output_crop`: of that window), no
        host copy.
        `step_window` = (a, b), 0 <= a < b <= n (DESIGN.md section 4 "Candidates"; Euler sampler only): run steps a <= i < b of this
        call's n-step schedule, with the tables of the full schedule sliced by absolute step index.  a > 0 needs `latents`, the
        packed state after step a - 1, used as it is (no noise is drawn); a caller who wants the bits of the unwindowed call also
        passes the first window's `pipe.window_conditioning` as `masked_image_latents`, because the conditioning's VAE sample is
        drawn behind the noise from the same generator.  b < n needs output_type="latent", returns the latents at sigma_b, runs the
        unfused Euler step (bit-equal to the fused one) and leaves `pipe.x0_preview`, the packed bf16 [B, S, C] estimate
        x_b - sigma_b v_{b-1} (tfx_x0_predict), and `pipe.window_conditioning`.  NotImplementedError, before anything is launched,
        with the AMO and multistep samplers, a foreign scheduler, `strength`, `keep_known`, `change_map`, true CFG, the step cache
        and a step callback.  None (default) is the call without the key.
        `amo_noise`, a list of pre-drawn eps tensors for the AMO sampler (replay across devices), and
        `output_crop` = (left, top, right, bottom), the callers' result crop (run_inference.py:460-465) applied on the
        device so that only the kept pixels are converted and copied to the host.
        Known-region sampling (FluxInpaintPipeline's loop on the Fill model, opt-in, no quality claim):
        `strength` in [0, 1] starts the loop part-way down the sigma grid from the noised original and runs int(n * strength)
        steps; `keep_known` = True or dict(mode="nearest" | "cover", grow=int) replaces, after every step, the latents outside
        `mask_image` by the original's latents noised to the next sigma (the original itself on the last step); `image_latents`,
        packed [B, S, 64], stands in for the VAE latents of `image` (needed when `image` is not given).
        Change-map sampling (FluxDifferentialImg2ImgPipeline's loop on the Fill model, opt-in, no quality
        claim): `change_map` gives every latent pixel its own release step -- a grey image / uint8 array / uint8 tensor at call size
        (255 = the model's from the first step, 0 = never changes), or dict(map=..., dilate, feather, mode, grow, last); without
        `map` it is feather(dilate(mask_image >= 128)), the paste-back's alpha.  A pixel is held to the noised original while its
        map value lies below the loop's progress; last="keep" (default) ends held pixels as the original's latents, "free" is the
        reference, whose last step belongs to the model.  Not with `keep_known`; with `strength` / `image_latents` as `keep_known`.
        The Fill model's own conditioning still comes from the binary `mask_image`.
        True CFG (FluxCFGPipeline's loop, D/examples/community/pipeline_flux_with_cfg.py:714-812, on the Fill
        model, opt-in, no quality claim): `negative_prompt` / `negative_prompt_2` or `negative_prompt_embeds` +
        `negative_pooled_prompt_embeds`, with the reference's checks, and `true_cfg`.  It is on when true_cfg > 1 and a negative
        prompt OR negative embeds are given -- the reference looks at the string alone, so embeds without a string silently switch
        it off there; here both count.  One negative string serves every sample of the batch.  Every step is then one forward over
        [negative; positive] and noise_pred = neg + true_cfg * (pos - neg) in front of the sampler update, at about twice the cost
        of a plain step.  Works with fp8 linears, runtime LoRA, `strength`, `keep_known`, `change_map`, all three engine
        schedulers, eager and graphs; refused (NotImplementedError) with the step cache and with a foreign scheduler object.  Off,
        the call is today's call."""
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        if _change_map_cfg(change_map) is not None and _keep_known_cfg(keep_known) is not None:
            raise ValueError("change_map and keep_known exclude each other: one blend stands behind the sampler update")
        if step_window is not None:    # refused before anything is encoded or launched
            n_steps = num_inference_steps if sigmas is None else len(sigmas)
            a, b = step_window = step_loop.check_step_window(step_window, n_steps)
            step_loop.refuse_step_window(self.scheduler, strength, keep_known, change_map,
                                         _true_cfg_on(true_cfg, negative_prompt, negative_prompt_embeds), self._step_cache is not None,
                                         callback_on_step_end is not None)
            if a > 0 and latents is None:
                raise ValueError(f"step_window=({a}, {b}) starts behind step 0 and needs `latents`, the packed state after step {a - 1}")
            if b < n_steps and output_type != "latent":
                raise ValueError(f"step_window=({a}, {b}) ends before step {n_steps} and needs output_type='latent' "
                                 "(pipe.x0_preview holds the clean-image estimate)")
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        self.check_inputs(prompt, prompt_2, height, width, prompt_embeds=prompt_embeds,
                          pooled_prompt_embeds=pooled_prompt_embeds,
                          callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs,
                          max_sequence_length=max_sequence_length, image=image, mask_image=mask_image,
                          masked_image_latents=masked_image_latents, negative_prompt=negative_prompt,
                          negative_prompt_2=negative_prompt_2, negative_prompt_embeds=negative_prompt_embeds,
                          negative_pooled_prompt_embeds=negative_pooled_prompt_embeds)
        negative = None
        if _true_cfg_on(true_cfg, negative_prompt, negative_prompt_embeds):
            if self._step_cache is not None:
                raise NotImplementedError("true CFG does not run with the step cache (its metric would mix the two conditionings); "
                                          "call disable_step_cache() or leave negative_prompt / true_cfg out")
            negative = dict(scale=float(true_cfg), prompt=negative_prompt, prompt_2=negative_prompt_2, prompt_embeds=negative_prompt_embeds,
                            pooled_prompt_embeds=negative_pooled_prompt_embeds)
        self._guidance_scale, self._joint_attention_kwargs, self._interrupt = guidance_scale, joint_attention_kwargs, False
        runtime_lora = bool(getattr(self.transformer, "_adapters", None))
        if joint_attention_kwargs is not None and joint_attention_kwargs.get("scale", 1.0) != 1.0 and not runtime_lora:
            raise NotImplementedError("LoRA is merged at load time in this engine; a runtime `scale` is not supported")
        # runtime adapters: the call's scale goes into the adapters' factor vector now and the previous one comes back afterwards
        # (scale_lora_layers / unscale_lora_layers, transformer_flux.py:1073-1079, 1205-1207)
        lora_scale = joint_attention_kwargs.get("scale") if (runtime_lora and joint_attention_kwargs) else None
        prev_lora_scale = self.transformer._lora_call_scale if runtime_lora else None
        if lora_scale is not None:
            self.transformer._write_scales(lora_scale)
        try:
            return self._call_body(prompt, prompt_2, image, mask_image, masked_image_latents, height, width, num_inference_steps,
                                   sigmas, guidance_scale, num_images_per_prompt, generator, latents, prompt_embeds,
                                   pooled_prompt_embeds, output_type, return_dict, callback_on_step_end,
                                   callback_on_step_end_tensor_inputs, max_sequence_length, amo_noise, output_crop, strength,
                                   keep_known, image_latents, change_map, negative, step_window)
        finally:
            if lora_scale is not None:
                self.transformer._write_scales(prev_lora_scale)

    @torch.no_grad()
    def call_mixed(self, prompt: Union[str, List[str]] = None, image=None, mask_image=None, sizes=None,
                   prompt_2: Optional[Union[str, List[str]]] = None, num_inference_steps: int = 50,
                   sigmas: Optional[List[float]] = None, guidance_scale: float = 30.0, generator=None,
                   prompt_embeds: Optional[torch.Tensor] = None, pooled_prompt_embeds: Optional[torch.Tensor] = None,
                   output_type: Optional[str] = "pil", return_dict: bool = True, callback_on_step_end: Optional[Callable] = None,
                   max_sequence_length: int = 512, latents: Optional[List[torch.Tensor]] = None,
                   masked_image_latents: Optional[List[torch.Tensor]] = None, strength: float = 1.0, keep_known=None,
                   change_map=None):
        """One denoising run over samples of DIFFERENT sizes (no reference counterpart: the reference, like `__call__`, runs one
        geometry per call).  image / mask_image: one entry per sample, sizes[b] = (width, height) of sample b (multiples of 16).
        Every sample computes what its own single-image `__call__` computes -- its own latent noise and VAE posterior sample from
        generator[b] (a list, or one generator used for every sample in turn), its own sigma schedule from calculate_shift(S_b)
        (per_sample_schedules), its own rotary table -- but the transformer runs ONCE per step for all of them: rows are padded to
        the longest sample (T + S a multiple of 256), tfx_dit_desc.seq_len keeps every sample's attention on its own rows, and one
        session + captured step graph serves every mix of sizes up to its own.  The VAE runs per group of equal size.  Returns one
        image per sample at its own size (a list; output_type "latent": the packed latents [S_b, C] per sample).  latents /
        masked_image_latents: as in `__call__`, but one tensor [1, S_b, 64] / [1, S_b, 320] per sample (instead of image / mask_image).
        Needs the flow-matching Euler scheduler with fuse_euler_step (only the fused Euler step carries per-sample coefficients) and
        no step callback."""
        sch, tr = self.scheduler, self.transformer
        if change_map is not None and change_map is not False:
            raise NotImplementedError("call_mixed: change_map (change-map sampling) is not supported in mixed-geometry batches (the "
                                      "blend's buffers carry no padding rows); use __call__")
        if strength != 1.0 or keep_known:
            raise NotImplementedError("call_mixed: strength / keep_known (known-region sampling) are not supported in mixed-geometry "
                                      "batches (the blend's buffers carry no padding rows); use __call__")
        if self._step_cache is not None:
            raise NotImplementedError("call_mixed: the step cache does not serve mixed-geometry batches (padded rows would enter the "
                                      "metric's sums); disable_step_cache() or use __call__")
        if isinstance(sch, StochasticRFOvershotDiscreteScheduler):
            raise NotImplementedError("call_mixed: the AMO sampler is not supported in mixed-geometry batches (its coefficients and "
                                      "noise are per step, not per sample); use the Euler scheduler or __call__")
        if isinstance(sch, FlowMatchMultistepScheduler):
            raise NotImplementedError("call_mixed: the multistep sampler is not supported in mixed-geometry batches (its coefficients "
                                      "are per step, not per sample, and its update is not fused into proj_out); use the Euler "
                                      "scheduler or __call__")
        if not isinstance(sch, FlowMatchEulerDiscreteScheduler) or not self.fuse_euler_step:
            raise NotImplementedError("call_mixed needs FlowMatchEulerDiscreteScheduler with fuse_euler_step: only the Euler update "
                                      "fused into proj_out carries per-sample coefficients")
        if callback_on_step_end is not None:
            raise NotImplementedError("call_mixed: a step callback wants the latents as one tensor every step, which the fused Euler "
                                      "step of a mixed-geometry batch does not keep; use __call__")
        if sizes is None or len(sizes) == 0:
            raise ValueError("call_mixed: `sizes` = [(width, height), ...], one per sample")
        B = len(sizes)
        if masked_image_latents is None:
            image, mask_image = list(image), list(mask_image)
            if len(image) != B or len(mask_image) != B:
                raise ValueError(f"call_mixed: {B} sizes but {len(image)} images / {len(mask_image)} masks")
        elif len(masked_image_latents) != B or image is not None:
            raise ValueError("call_mixed: pass either image + mask_image or one masked_image_latents tensor per sample")
        if latents is not None and len(latents) != B:
            raise ValueError(f"call_mixed: {B} sizes but {len(latents)} latents")
        if isinstance(prompt, str):
            prompt = [prompt] * B
        if isinstance(prompt_2, str):
            prompt_2 = [prompt_2] * B
        self.check_inputs(prompt, prompt_2, None, None, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                          max_sequence_length=max_sequence_length, image=image, mask_image=mask_image, masked_image_latents=None)
        self._guidance_scale, self._joint_attention_kwargs, self._interrupt = guidance_scale, None, False
        device = self._execution_device
        dev = tr.device
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds, device=device,
            max_sequence_length=max_sequence_length)
        if prompt_embeds.shape[0] != B:
            raise ValueError(f"call_mixed: {B} sizes but {prompt_embeds.shape[0]} prompts")
        dtype = prompt_embeds.dtype
        gens = list(generator) if isinstance(generator, (list, tuple)) else [generator] * B
        if len(gens) != B:
            raise ValueError(f"You have passed a list of generators of length {len(gens)}, but requested an effective batch size of {B}.")
        C = self.vae.config.latent_channels * 4
        if C != EULER_PAD or tr.out_channels != C:
            raise NotImplementedError("call_mixed: the fused Euler step needs 64 packed latent channels")
        # per sample, in the order of its single-image call: the latent noise first, then (per group) the VAE posterior sample
        lats, ids = [], []
        for b, ((w, h), g) in enumerate(zip(sizes, gens)):
            l, i = self.prepare_latents(1, self.vae.config.latent_channels, h, w, dtype, device, g, None if latents is None else latents[b])
            if l.shape[1] != i.shape[0]:
                raise ValueError(f"call_mixed: latents of sample {b} have {l.shape[1]} rows, its size {(w, h)} has {i.shape[0]} tokens")
            lats.append(l), ids.append(i)
        groups: Dict[Tuple[int, int], List[int]] = {}
        for b, wh in enumerate(sizes):
            groups.setdefault(tuple(wh), []).append(b)
        conds: List[Optional[torch.Tensor]] = [None] * B
        for (w, h), members in groups.items():
            if masked_image_latents is not None:
                for b in members:
                    conds[b] = masked_image_latents[b].reshape(-1, masked_image_latents[b].shape[-1])
                    if conds[b].shape[0] != lats[b].shape[1]:
                        raise ValueError(f"call_mixed: masked_image_latents of sample {b} have {conds[b].shape[0]} rows, expected {lats[b].shape[1]}")
                continue
            gg = [gens[b] for b in members]
            cond, H, W = self._encode_conditioning([image[b] for b in members], [mask_image[b] for b in members], h, w, len(members), 1,
                                                   dtype, device, None if gg[0] is None else gg)
            if cond is None:
                raise NotImplementedError("call_mixed: `image` must hold images, not VAE latents")
            if cond.shape[1] != lats[members[0]].shape[1]:
                raise ValueError(f"call_mixed: sample size {(w, h)} became {W}x{H} in preprocessing; pass images at their pipeline size")
            for k, b in enumerate(members):
                conds[b] = cond[k]
        S_b = [l.shape[1] for l in lats]
        T = prompt_embeds.shape[1]
        N = (T + max(S_b) + 255) // 256 * 256        # whole GEMM tiles: the rounding costs no GEMM time and makes sessions reusable
        S = N - T
        ses = tr.session(B, S, T, mixed=True)
        ses.set_conditioning(prompt_embeds.to(dev, BF16), text_ids, ids)
        n = num_inference_steps if sigmas is None else len(sigmas)
        tabs = per_sample_schedules(sch, S_b, n, sigmas)
        self._num_timesteps = n
        mod = self._modulation_table(tabs["timesteps"].t(), B, pooled_prompt_embeds, guidance_scale, tabs["dsigma"].t())
        for b in range(B):          # x_embedder input [latents | masked_image_latents] of the valid rows; padding rows stay unspecified
            ses.xin[b, :S_b[b], :C].copy_(lats[b][0].to(dev, BF16))
            ses.xin[b, :S_b[b], C:].copy_(conds[b].to(dev, BF16))
        sch._step_index = 0
        with self.progress_bar(total=n) as bar:
            out = step_loop.denoise(self, ses, mod, None, None, n, bar, fuse=True)
        results: List[Any] = [None] * B
        for (w, h), members in groups.items():
            lat = torch.stack([out[b, :S_b[b]] for b in members])
            if output_type == "latent":
                imgs = list(lat)
            else:
                imgs = self._decode_to_output(lat, h, w, output_type)
            for k, b in enumerate(members):
                results[b] = imgs[k]
        self.maybe_free_model_hooks()
        if not return_dict:
            return (results,)
        return FluxPipelineOutput(images=results)

    def _call_body(self, prompt, prompt_2, image, mask_image, masked_image_latents, height, width, num_inference_steps, sigmas,
                   guidance_scale, num_images_per_prompt, generator, latents, prompt_embeds, pooled_prompt_embeds, output_type,
                   return_dict, callback_on_step_end, callback_on_step_end_tensor_inputs, max_sequence_length, amo_noise, output_crop,
                   strength=1.0, keep_known=None, image_latents=None, change_map=None, negative=None, step_window=None):
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        device = self._execution_device
        prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            device=device, num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length)
        cfg = None
        if negative is not None:      # the negatives go through the same encode_prompt (the prompt cache serves them)
            total = batch_size * num_images_per_prompt
            neg = negative["prompt"]
            if isinstance(neg, list) and len(neg) not in (1, batch_size):
                raise ValueError(f"Negative prompt batch size ({len(neg)}) does not match prompt batch size ({batch_size})")
            neg_pe, neg_pooled, _ = self.encode_prompt(
                prompt=neg, prompt_2=negative["prompt_2"], prompt_embeds=negative["prompt_embeds"],
                pooled_prompt_embeds=negative["pooled_prompt_embeds"], device=device, num_images_per_prompt=num_images_per_prompt,
                max_sequence_length=max_sequence_length)
            if neg_pe.shape[0] != total:        # one negative prompt for the whole batch
                neg_pe = _repeat_to_batch(neg_pe, total, "negative prompt embeds")
                neg_pooled = _repeat_to_batch(neg_pooled, total, "negative pooled prompt embeds")
            if neg_pe.shape != prompt_embeds.shape or neg_pooled.shape != pooled_prompt_embeds.shape:
                raise ValueError(f"true CFG: the negative embeddings {tuple(neg_pe.shape)} / {tuple(neg_pooled.shape)} must have the shapes of "
                                 f"the positive ones {tuple(prompt_embeds.shape)} / {tuple(pooled_prompt_embeds.shape)}")
            cfg = dict(scale=negative["scale"], prompt_embeds=neg_pe, pooled=neg_pooled)
        num_channels_latents = self.vae.config.latent_channels
        keep_cfg = _keep_known_cfg(keep_known)
        change_cfg = _change_map_cfg(change_map)
        known = keep_cfg is not None or change_cfg is not None or strength < 1.0
        given_latents = latents is not None
        src_image = image
        latents, latent_image_ids = self.prepare_latents(batch_size * num_images_per_prompt, num_channels_latents, height,
                                                         width, prompt_embeds.dtype, device, generator, latents)
        if masked_image_latents is not None:
            masked_image_latents = masked_image_latents.to(latents.device)
        else:
            masked_image_latents, height, width = self._encode_conditioning(
                image, mask_image, height, width, batch_size, num_images_per_prompt, prompt_embeds.dtype, device, generator)
            if masked_image_latents is None:    # `image` was given as VAE latents (P:1525): the reference-shaped sequence
                image = self.image_processor.preprocess(image, height=height, width=width)
                mask_image = self.mask_processor.preprocess(mask_image, height=height, width=width)
                masked_image = (image * (1 - mask_image)).to(device=device, dtype=prompt_embeds.dtype)
                mask, masked_image_latents = self.prepare_mask_latents(
                    mask_image, masked_image, batch_size, num_channels_latents, num_images_per_prompt, height, width,
                    prompt_embeds.dtype, device, generator)
                masked_image_latents = torch.cat((masked_image_latents, mask), dim=-1)
        sigmas = np.linspace(1.0, 1 / num_inference_steps, num_inference_steps) if sigmas is None else sigmas
        image_seq_len = latents.shape[1]
        sc = self.scheduler.config
        mu = calculate_shift(image_seq_len, sc.base_image_seq_len, sc.max_image_seq_len, sc.base_shift, sc.max_shift)
        timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, sigmas=sigmas, mu=mu)
        engine = isinstance(self.scheduler, (FlowMatchEulerDiscreteScheduler, StochasticRFOvershotDiscreteScheduler, FlowMatchMultistepScheduler))
        keep = None
        if cfg is not None and not engine:
            raise NotImplementedError("true CFG needs one of the engine's schedulers (their step loop holds the combine)")
        if known:
            if not engine:
                raise NotImplementedError("strength / keep_known / change_map need one of the engine's schedulers (their step loop holds the blend)")
            timesteps, num_inference_steps = self.get_timesteps(num_inference_steps, strength, device)
            if num_inference_steps < 1:
                raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline"
                                 f"steps is {num_inference_steps} which is < 1 and not appropriate for this pipeline.")
            latents, keep = self._prepare_known_region(latents, given_latents, image_latents, src_image, mask_image, keep_cfg, strength,
                                                       height, width, prompt_embeds.dtype, device, generator, change_cfg=change_cfg)
        preview = None
        if step_window is not None:    # the schedule's own tables from step a on (set_begin_index), its timesteps a..b-1
            a, b = step_window
            if b < num_inference_steps:
                preview = dict(sigma=self.scheduler.sigmas.to(self.transformer.device, torch.float32).contiguous(), step=b)
                self.x0_preview, self.window_conditioning = None, masked_image_latents
            timesteps = timesteps[a:b]
            self.scheduler.set_begin_index(a)
            num_inference_steps = b - a
        self._num_timesteps = len(timesteps)
        with self.progress_bar(total=num_inference_steps) as bar:
            if engine:
                try:
                    latents = self._engine_loop(latents, masked_image_latents, prompt_embeds, pooled_prompt_embeds, text_ids,
                                                latent_image_ids, timesteps, guidance_scale, callback_on_step_end,
                                                callback_on_step_end_tensor_inputs, amo_noise, bar, keep, cfg, preview)
                except RuntimeError as e:
                    if cfg is None or isinstance(e, NotImplementedError):
                        raise
                    raise RuntimeError(f"{e}\n(true CFG runs every step on a session of {2 * latents.shape[0]} samples, [negative; positive]: "
                                       f"where that is larger than the engine takes, halve the batch)") from e
            else:
                guidance = None
                if self.transformer.config.guidance_embeds:
                    guidance = torch.full([1], guidance_scale, device=device, dtype=torch.float32).expand(latents.shape[0])
                latents = self._generic_loop(latents, masked_image_latents, prompt_embeds, pooled_prompt_embeds, text_ids,
                                             latent_image_ids, timesteps, guidance, callback_on_step_end,
                                             callback_on_step_end_tensor_inputs, bar)
        if output_type == "latent":
            image = latents
        else:
            image = self._decode_to_output(latents, height, width, output_type, output_crop)
        self.maybe_free_model_hooks()
        if not return_dict:
            return (image,)
        return FluxPipelineOutput(images=image)
