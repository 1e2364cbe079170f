"""The two samplers of the TextFlux hot path, same protocol as the reference classes
(`set_timesteps(num_inference_steps, device, sigmas=, mu=)`, `step(model_output, timestep, sample, return_dict=False)[0]`,
`.timesteps`, `.sigmas`, `.config`, `.order`, plus AMO's `set_c` / `set_overshot_func`).

* FlowMatchEulerDiscreteScheduler         <- D/schedulers/scheduling_flow_match_euler_discrete.py
* StochasticRFOvershotDiscreteScheduler   <- D/schedulers/scheduling_stochastic_rf_discrete_overshot.py  (AMO sampler)

Host side (this file): the sigma / timestep tables and the per-step scalar coefficients, evaluated in the same
precision and order as the reference.  Device side: the state update itself runs in libtextflux_hip.so
(`tfx_euler_step` / `tfx_amo_step`); the AMO sampler's per-step `min(tensor, 1)` host syncs (reference :313, :342)
disappear because the coefficient table is built once from the host copy of the sigmas.

* FlowMatchMultistepScheduler             no reference counterpart: second-order multistep on the Euler class's grid (`tfx_multistep_step`)

Known-region sampling: all three carry `scale_noise` (the Euler class's, scheduling_flow_match_euler_discrete.py:
130-176) and `keep_sigma_table` for `tfx_known_region_blend`, and their tables start at `begin_index` (`set_begin_index`).
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch

from . import ops


class _Config(SimpleNamespace):
    def get(self, k, default=None):
        return getattr(self, k, default)

    def to_dict(self):
        return dict(self.__dict__)


def _cfg_dict(config) -> dict:
    if isinstance(config, dict):
        return dict(config)
    if hasattr(config, "to_dict"):
        return config.to_dict()
    return dict(vars(config))


def change_cut_table(n: int, last: str = "keep") -> torch.Tensor:
    """int32 [n] for tfx_change_map_blend (DESIGN.md section 4 "Change-map sampling"): at step i a latent pixel with hold byte q is
    held to the noised original exactly when q > cut[i].  The reference (FluxDifferentialImg2ImgPipeline, pipeline_flux_differential_
    img2img.py:936-938) compares bf16(q / 255) with `torch.arange(n, dtype=bf16) / n`; both sides are evaluated here with the same
    torch expressions on the host, and cut[i] is read off the 256 comparisons -- no integer formula: bf16 ties (n = 3: byte 85 is not
    held at step 1) and the bf16 arange itself (n > 256) decide entries.  n: the number of steps that run, after `strength` (:892).
    last="free": the reference, whose last step leaves the latents to the model (:977): cut[n - 1] = 255.  last="keep": the schedule
    goes on to the last step, where keep_sigma's negative entry makes the held pixels the original's latents themselves."""
    if last not in ("keep", "free"):
        raise ValueError(f"change_map: last must be 'keep' or 'free', got {last!r}")
    n = int(n)
    if n < 1:
        raise ValueError(f"change_cut_table: n must be >= 1, got {n}")
    thresholds = torch.arange(n, dtype=torch.bfloat16) / n
    levels = (torch.arange(256, dtype=torch.float32) / 255).to(torch.bfloat16)
    held = levels[None, :] > thresholds[:, None]                     # [n, 256]
    count = held.sum(dim=1)
    if not bool((held == (torch.arange(256)[None, :] >= (256 - count)[:, None])).all()):
        raise AssertionError("change_cut_table: the held bytes are not an upper set")      # both sides are monotone: cannot happen
    cut = (255 - count).to(torch.int32)
    if last == "free":
        cut[-1] = 255
    return cut


class _FlowMatchBase:
    order = 1
    _keys: Sequence[str] = ()

    def _init_tables(self):
        c = self.config
        ts = np.linspace(1, c.num_train_timesteps, c.num_train_timesteps, dtype=np.float32)[::-1].copy()
        sigmas = torch.from_numpy(ts).to(torch.float32) / c.num_train_timesteps
        if not c.use_dynamic_shifting:
            sigmas = c.shift * sigmas / (1 + (c.shift - 1) * sigmas)
        self.timesteps = sigmas * c.num_train_timesteps
        self.sigmas = sigmas.to("cpu")
        self.sigma_min, self.sigma_max = self.sigmas[-1].item(), self.sigmas[0].item()
        self._step_index = self._begin_index = None
        self._sigmas_host: Optional[torch.Tensor] = None
        self._coef: Optional[torch.Tensor] = None
        self.num_inference_steps = None

    @classmethod
    def from_config(cls, config, **kwargs):
        """Accepts another scheduler's config (dict or namespace) and ignores keys it lacks, as ConfigMixin does
        (used at run_inference.py:81-82 to swap the sampler)."""
        d = _cfg_dict(config)
        d.update(kwargs)
        return cls(**{k: d[k] for k in cls._keys if k in d})

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index
        self._coef = None              # the coefficient tables start at the first executed step

    def _run_sigmas(self) -> torch.Tensor:
        """host fp32 sigmas of the steps that run, from begin_index on, and the closing 0"""
        return self._sigmas_host[self._begin_index or 0:]

    def _table_row(self) -> int:
        """row of coef_table / keep_sigma_table of the current step: the tables start at begin_index, step_index counts the whole grid"""
        return self._step_index - (self._begin_index or 0)

    def scale_noise(self, sample: torch.Tensor, timestep, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward process sigma * noise + (1 - sigma) * sample with the reference's index rule and op order
        (scheduling_flow_match_euler_discrete.py:130-176): begin_index None -> the timestep's own index; step_index set -> that
        (inpainting, after a step); else begin_index (img2img, before the first step).  Protocol method on the caller's tensors; the
        engine's loop runs the same arithmetic in tfx_known_region_blend."""
        sigmas = self.sigmas.to(device=sample.device, dtype=sample.dtype)
        schedule_timesteps = self.timesteps.to(sample.device)
        timestep = torch.as_tensor(timestep).reshape(-1).to(sample.device)
        if self.begin_index is None:
            step_indices = [self.index_for_timestep(t, schedule_timesteps) for t in timestep]
        elif self.step_index is not None:
            step_indices = [self.step_index] * timestep.shape[0]
        else:
            step_indices = [self.begin_index] * timestep.shape[0]
        sigma = sigmas[step_indices].flatten()
        while len(sigma.shape) < len(sample.shape):
            sigma = sigma.unsqueeze(-1)
        return sigma * noise + (1.0 - sigma) * sample

    def keep_sigma_table(self, device, state_dtype=torch.bfloat16) -> torch.Tensor:
        """fp32 [n_run] for tfx_known_region_blend: entry i = sigma_{i+1} of the steps from begin_index on, rounded to the state dtype
        as the reference's scale_noise rounds it (`sigmas.to(dtype=sample.dtype)`); the last entry is -1, "the original itself" (the
        reference's `i == len(timesteps) - 1`, which is not the same as sigma = 0 for signed zeros)."""
        s = self._run_sigmas()
        tab = s[1:].to(state_dtype).float()
        tab[-1] = -1.0
        return tab.to(device)

    def _sigma_to_t(self, sigma):
        return sigma * self.config.num_train_timesteps

    def time_shift(self, mu: float, sigma: float, t):
        return math.exp(mu) / (math.exp(mu) + (1 / t - 1) ** sigma)

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        st = self.timesteps if schedule_timesteps is None else schedule_timesteps
        idx = (st == timestep).nonzero()
        pos = 1 if len(idx) > 1 else 0
        return idx[pos].item()

    def _init_step_index(self, timestep):
        if self.begin_index is None:
            if isinstance(timestep, torch.Tensor):
                timestep = timestep.to(self.timesteps.device)
            self._step_index = self.index_for_timestep(timestep)
        else:
            self._step_index = self._begin_index

    def _finish_set_timesteps(self, sigmas_np, device):
        sig = torch.from_numpy(np.asarray(sigmas_np)).to(dtype=torch.float32)
        self._sigmas_host = torch.cat([sig, torch.zeros(1)])          # host copy: coefficient tables, no syncs later
        sig_dev = sig.to(device=device)
        self.timesteps = (sig_dev * self.config.num_train_timesteps).to(device=device)
        self.sigmas = torch.cat([sig_dev, torch.zeros(1, device=sig_dev.device)])
        self._step_index = self._begin_index = None
        self._coef = None

    @staticmethod
    def _check_timestep(timestep):
        if isinstance(timestep, int) or isinstance(timestep, (torch.IntTensor, torch.LongTensor)):
            raise ValueError("Passing integer indices (e.g. from `enumerate(timesteps)`) as timesteps to `step()` is "
                             "not supported. Make sure to pass one of the `scheduler.timesteps` as a timestep.")

    def __len__(self):
        return self.config.num_train_timesteps


class FlowMatchEulerDiscreteScheduler(_FlowMatchBase):
    _keys = ("num_train_timesteps", "shift", "use_dynamic_shifting", "base_shift", "max_shift", "base_image_seq_len",
             "max_image_seq_len", "invert_sigmas", "use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas")

    def __init__(self, num_train_timesteps: int = 1000, shift: float = 1.0, use_dynamic_shifting=False,
                 base_shift: Optional[float] = 0.5, max_shift: Optional[float] = 1.15,
                 base_image_seq_len: Optional[int] = 256, max_image_seq_len: Optional[int] = 4096,
                 invert_sigmas: bool = False, use_karras_sigmas: Optional[bool] = False,
                 use_exponential_sigmas: Optional[bool] = False, use_beta_sigmas: Optional[bool] = False):
        if invert_sigmas or use_karras_sigmas or use_exponential_sigmas or use_beta_sigmas:
            raise NotImplementedError("sigma re-parameterisations are not used by FLUX.1-Fill / TextFlux (SURVEY Appendix C)")
        self.config = _Config(num_train_timesteps=num_train_timesteps, shift=shift,
                              use_dynamic_shifting=use_dynamic_shifting, base_shift=base_shift, max_shift=max_shift,
                              base_image_seq_len=base_image_seq_len, max_image_seq_len=max_image_seq_len,
                              invert_sigmas=invert_sigmas, use_karras_sigmas=use_karras_sigmas,
                              use_exponential_sigmas=use_exponential_sigmas, use_beta_sigmas=use_beta_sigmas)
        self._init_tables()

    def set_timesteps(self, num_inference_steps: int = None, device: Union[str, torch.device] = None,
                      sigmas: Optional[List[float]] = None, mu: Optional[float] = None):
        """scheduling_flow_match_euler_discrete.py:184-241 -- note the cast to f32 BEFORE the shift."""
        c = self.config
        if c.use_dynamic_shifting and mu is None:
            raise ValueError(" you have a pass a value for `mu` when `use_dynamic_shifting` is set to be `True`")
        if sigmas is None:
            timesteps = np.linspace(self._sigma_to_t(self.sigma_max), self._sigma_to_t(self.sigma_min), num_inference_steps)
            sigmas = timesteps / c.num_train_timesteps
        else:
            sigmas = np.array(sigmas).astype(np.float32)
            num_inference_steps = len(sigmas)
        self.num_inference_steps = num_inference_steps
        sigmas = self.time_shift(mu, 1.0, sigmas) if c.use_dynamic_shifting else c.shift * sigmas / (1 + (c.shift - 1) * sigmas)
        self._finish_set_timesteps(sigmas, device)

    def coef_table(self, device, state_dtype=torch.bfloat16) -> torch.Tensor:
        """dsigma_i = sigma_{i+1} - sigma_i (f32) of the steps from begin_index on, rounded to the model-output dtype exactly where the reference's
        `(sigma_next - sigma) * model_output` rounds it (0-dim f32 tensor cast to the common dtype, :327)."""
        if self._coef is None or self._coef.device != torch.device(device):
            s = self._run_sigmas()
            self._coef = (s[1:] - s[:-1]).to(state_dtype).float().to(device)
        return self._coef

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, return_dict: bool = True):
        self._check_timestep(timestep)
        if self.step_index is None:
            self._init_step_index(timestep)
        prev = sample.to(model_output.dtype).clone().contiguous()
        ops.euler_step_(model_output.contiguous(), prev, self.coef_table(sample.device, model_output.dtype),
                        step=self._table_row())
        self._step_index += 1
        if not return_dict:
            return (prev,)
        return SimpleNamespace(prev_sample=prev)


class StochasticRFOvershotDiscreteScheduler(_FlowMatchBase):
    _keys = ("num_train_timesteps", "shift", "use_dynamic_shifting", "base_shift", "max_shift", "base_image_seq_len",
             "max_image_seq_len")

    def __init__(self, num_train_timesteps: int = 1000, shift: float = 1.0, use_dynamic_shifting=False,
                 base_shift: Optional[float] = 0.5, max_shift: Optional[float] = 1.15,
                 base_image_seq_len: Optional[int] = 256, max_image_seq_len: Optional[int] = 4096):
        self.config = _Config(num_train_timesteps=num_train_timesteps, shift=shift,
                              use_dynamic_shifting=use_dynamic_shifting, base_shift=base_shift, max_shift=max_shift,
                              base_image_seq_len=base_image_seq_len, max_image_seq_len=max_image_seq_len)
        self._init_tables()
        self.attn_map = None
        self.c: Optional[float] = None
        self.overshot_func: Optional[Callable] = None

    def set_c(self, c: float):
        self.c = c
        self._coef = None

    def set_overshot_func(self, overshot_func):
        self.overshot_func = overshot_func
        self._coef = None

    def set_attn_map(self, attn_map):
        if attn_map is not None:
            raise NotImplementedError("attn_map is a dead experiment in the reference: no live caller sets it (SURVEY §0.3)")
        self.attn_map = None

    def set_timesteps(self, num_inference_steps: int = None, device: Union[str, torch.device] = None,
                      sigmas: Optional[List[float]] = None, mu: Optional[float] = None):
        """scheduling_stochastic_rf_discrete_overshot.py:182-224 -- NO f32 cast before the shift (differs from Euler
        in the last ulp)."""
        c = self.config
        if c.use_dynamic_shifting and mu is None:
            raise ValueError(" you have a pass a value for `mu` when `use_dynamic_shifting` is set to be `True`")
        if sigmas is None:
            self.num_inference_steps = num_inference_steps
            timesteps = np.linspace(self._sigma_to_t(self.sigma_max), self._sigma_to_t(self.sigma_min), num_inference_steps)
            sigmas = timesteps / c.num_train_timesteps
        else:
            sigmas = np.asarray(sigmas)
            self.num_inference_steps = len(sigmas)
        sigmas = self.time_shift(mu, 1.0, sigmas) if c.use_dynamic_shifting else c.shift * sigmas / (1 + (c.shift - 1) * sigmas)
        self._finish_set_timesteps(sigmas, device)

    def coef_table(self, device, state_dtype=torch.bfloat16) -> torch.Tensor:
        """Per step {t_over - t, a, b} (:306-349), evaluated on 0-dim f32 host tensors in the reference's order;
        (t_over - t) is rounded to the model-output dtype where `(t_overshoot - t) * (-model_output)` rounds it."""
        if self.c is None or self.overshot_func is None:
            raise RuntimeError("call set_c(...) and set_overshot_func(...) before stepping the AMO sampler")
        if self._coef is None or self._coef.device != torch.device(device):
            s = self._run_sigmas()
            rows = []
            for i in range(len(s) - 1):
                sigma, sigma_next = s[i], s[i + 1]
                t = 1 - sigma
                step_size = sigma - sigma_next
                t_next = min(t + step_size, 1)
                t_over = min(self.overshot_func(t_next, step_size * self.c), 1)
                a = t_next / t_over
                b = ((1 - t_next) ** 2 - (a - t_next) ** 2) ** 0.5
                dt = torch.as_tensor(t_over - t, dtype=torch.float32).to(state_dtype).float()
                rows.append([float(dt), float(a), float(b)])
            self._coef = torch.tensor(rows, dtype=torch.float32).to(device)
        return self._coef

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, return_dict: bool = True,
             noise: Optional[torch.Tensor] = None):
        """`noise=` (extra, optional) injects the eps the reference would have drawn from the global RNG
        (randn_tensor(..., generator=generator), :351-355) so trajectories can be replayed across devices."""
        self._check_timestep(timestep)
        if self.step_index is None:
            self._init_step_index(timestep)
        if noise is None:
            noise = torch.randn(sample.shape, generator=generator, device=sample.device, dtype=torch.float32)
        prev = sample.to(model_output.dtype).clone().contiguous()
        ops.amo_step_(model_output.contiguous(), prev, self.coef_table(sample.device, model_output.dtype),
                      noise.to(sample.device, torch.float32).contiguous(), step=self._table_row())
        sigma = self._sigmas_host[self._step_index].to(sample.device)
        predicted_x1 = sample.to(torch.float32) - sigma * model_output
        self._step_index += 1
        if not return_dict:
            return (prev, predicted_x1)
        return SimpleNamespace(prev_sample=prev, predicted_x1=predicted_x1)


class FlowMatchMultistepScheduler(_FlowMatchBase):
    """Second-order multistep (Adams-Bashforth) sampler on the flow-matching sigma grid: one model evaluation per step, like Euler,
    plus the previous step's model output.  No reference counterpart and opt-in (DESIGN.md section 4 "Multistep sampler"): with
    h_i = sigma_{i+1} - sigma_i,

        x_1     = x_0 + h_0 v_0
        x_{i+1} = x_i + h_i (1 + h_i / (2 h_{i-1})) v_i - h_i^2 / (2 h_{i-1}) v_{i-1}

    -- no division by sigma, so the last step onto sigma = 0 is like any other.  Same config keys, `set_timesteps` (with the f32
    cast before the shift) and `step` protocol as FlowMatchEulerDiscreteScheduler; `order` counts model evaluations per step.  The
    scheduler owns the history: it is reset by `set_timesteps`, and a caller that replaces `sample` between steps leaves it as it is."""
    _keys = FlowMatchEulerDiscreteScheduler._keys
    order = 1

    def __init__(self, *args, **kwargs):
        euler = FlowMatchEulerDiscreteScheduler(*args, **kwargs)       # the same keys, defaults and refusals
        self.config = _Config(**euler.config.to_dict())
        self._init_tables()
        self._v_prev: Optional[torch.Tensor] = None

    def set_timesteps(self, num_inference_steps: int = None, device: Union[str, torch.device] = None,
                      sigmas: Optional[List[float]] = None, mu: Optional[float] = None):
        FlowMatchEulerDiscreteScheduler.set_timesteps(self, num_inference_steps, device, sigmas=sigmas, mu=mu)
        self._v_prev = None

    def coef_table(self, device, state_dtype=torch.bfloat16) -> torch.Tensor:
        """fp32 [n, 2] of the steps from begin_index on (the first executed step is the history-free one): row 0 = (h_0, 0), row i = (h_i (1 + h_i / (2 h_{i-1})), -h_i^2 / (2 h_{i-1})), evaluated in float64 from the
        host copy of the fp32 sigmas and rounded to fp32 once.  (state_dtype: the siblings' signature; the coefficients stay fp32.)"""
        if self._coef is None or self._coef.device != torch.device(device):
            h = np.diff(self._run_sigmas().numpy().astype(np.float64))
            c = np.zeros((len(h), 2), dtype=np.float64)
            c[0, 0] = h[0]
            c[1:, 0] = h[1:] * (1.0 + h[1:] / (2.0 * h[:-1]))
            c[1:, 1] = -h[1:] * h[1:] / (2.0 * h[:-1])
            self._coef = torch.from_numpy(c.astype(np.float32)).to(device)
        return self._coef

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True):
        self._check_timestep(timestep)
        if model_output.dtype != torch.bfloat16 or sample.dtype != torch.bfloat16:
            raise TypeError("multistep_step_: the HIP scheduler kernels operate on bf16 latents / model outputs")
        if self.step_index is None:
            self._init_step_index(timestep)
        v = model_output.contiguous()
        hist = self._v_prev
        if hist is None or hist.shape != v.shape or hist.dtype != v.dtype or hist.device != v.device:
            hist = self._v_prev = torch.empty_like(v)
        prev = sample.clone().contiguous()
        ops.multistep_step_(v, prev, self.coef_table(sample.device), hist, step=self._table_row())
        self._step_index += 1
        if not return_dict:
            return (prev,)
        return SimpleNamespace(prev_sample=prev)
