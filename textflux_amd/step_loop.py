"""The engine's denoising loop, once: n steps of tfx_dit_step_run -- or of the replay of the graph captured
from it -- for the plain loop (phase 0) and the step cache (phases 1, 2 / 3), the Euler, AMO, fused-Euler and multistep samplers (the
last through tfx_dit_step_run_multistep), with or without a step callback, on uniform and mixed-geometry sessions; with the
known-region blend behind every sampler update (tfx_dit_step_run_ex) when the call keeps the known region, or the change-map blend
(tfx_dit_step_run_ex2) when the call gives every latent pixel its own release step.

`run_steps` is the control flow and touches no device: it drives a `steps` object with
    feed_noise(i)   run(phase)   replay(handle)   capture(phase) -> handle (raises CaptureRefused)   destroy(handle)
    metric() -> the head's B floats   save() -> state   restore(state)
`SessionSteps` binds those to a DitSession and the library; tests/test_step_loop_cpu.py binds them to a recorder.  `denoise` is
what the pipeline calls: buffers, side stream, run_steps, result.
"""
from __future__ import annotations

import ctypes as C
import warnings

import torch

from . import _lib as L
from . import ops
from .step_cache import Decider

BF16 = torch.bfloat16


class CaptureRefused(RuntimeError):
    """tfx_dit_step_capture returned an error (driver / runtime state); the message is the library's."""


def _graph_handles(steps, graphs, keys):
    """{phase: handle} for the phases of `keys`, captured now if the session holds none yet; False = eager (a refusal, now or cached).
    Capture does not execute, the state is kept explicit around it anyway."""
    have = {ph: graphs.get(k) for ph, k in keys.items()}
    if all(g is None for g in have.values()):
        saved = steps.save()
        try:
            for ph in keys:
                have[ph] = steps.capture(ph)
        except CaptureRefused as e:      # same kernels, launched eagerly
            warnings.warn(f"hipGraph capture of the denoising step failed ({e}); running the step loop eagerly")
            for g in have.values():
                if g:
                    steps.destroy(g)
            have = dict.fromkeys(have, False)
        steps.restore(saved)
        for ph, k in keys.items():
            graphs[k] = have[ph]
    return have if all(have.values()) else False


def run_steps(steps, n, pipe, progress_bar, graphs, key, decider=None, use_graph=False, callback=None):
    """n steps.  pipe: `_interrupt` is read and `scheduler._step_index` counted; graphs: the session's handle store, under `key` for
    the plain loop and key + ("step_cache", phase) for the cache; decider: the step cache's Decider (None: plain loop); callback(i):
    after step i.  use_graph, and then only without a callback and for n > 1: capture once the first step has run eagerly (a graph
    may only hold kernels that were launched before) and replay from then on."""
    use_graph = use_graph and callback is None and n > 1
    keys = {0: key} if decider is None else {ph: key + ("step_cache", ph) for ph in (1, 2, 3)}
    handles = None           # {phase: handle} once captured or found; False: eager phases

    def issue(ph):
        if handles:
            steps.replay(handles[ph])
        else:
            steps.run(ph)

    for i in range(n):
        if pipe._interrupt:
            continue
        steps.feed_noise(i)
        if decider is None:
            issue(0)
        else:
            issue(1)
            issue(3 if decider.step(i, steps.metric()) else 2)
        pipe.scheduler._step_index += 1
        if use_graph and handles is None:
            handles = _graph_handles(steps, graphs, keys)
        if callback is not None:
            callback(i)
        progress_bar.update()


class SessionSteps:
    """run_steps' device operations on a DitSession: its persistent step buffers `gb`, one tfx_step_desc per phase, stream `side`."""

    def __init__(self, ses, gb, side, phases, is_amo, fuse, amo_noise, multistep=False, keep=False, change=False):
        self.ses, self.gb, self.side, self.st, self.lib = ses, gb, side, side.cuda_stream, L.lib()
        self.sd = {ph: ses.step_desc(gb, is_amo, fuse, phase=ph) for ph in phases}
        self.is_amo, self.amo_noise = is_amo, amo_noise
        # the multistep sampler: sampler 0's descriptor through the *_multistep entry points, with the session's history buffer
        self.v_prev = gb["v_prev"].data_ptr() if multistep else None
        # known-region sampling: the same descriptors through the *_ex entry points, the blend's buffers beside them
        self.extra = None
        if keep:
            self.extra = L.StepExtra(v_prev=self.v_prev, keep_x0=gb["keep_x0"].data_ptr(), keep_noise=gb["keep_noise"].data_ptr(),
                                     keep_mask=gb["keep_mask"].data_ptr(), keep_sigma=gb["keep_sigma"].data_ptr())
        # change-map sampling: the *_ex2 entry points, keep_mask NULL and the hold bytes / cut table in a tfx_step_change beside
        self.change = None
        if change:
            self.extra = L.StepExtra(v_prev=self.v_prev, keep_x0=gb["change_x0"].data_ptr(), keep_noise=gb["change_noise"].data_ptr(),
                                     keep_mask=None, keep_sigma=gb["change_sigma"].data_ptr())
            self.change = L.StepChange(hold=gb["change_hold"].data_ptr(), cut=gb["change_cut"].data_ptr())

    def feed_noise(self, i):
        if not self.is_amo:
            return
        if self.amo_noise is None:
            self.gb["noise"].normal_()      # global device RNG, as the reference's randn_tensor(generator=None); never captured
        else:
            self.gb["noise"].copy_(self.amo_noise[i].to(self.gb["noise"].device, torch.float32))

    def run(self, ph):
        if self.change is not None:
            L.check(self.lib.tfx_dit_step_run_ex2(C.byref(self.sd[ph]), C.byref(self.extra), C.byref(self.change), self.st), "dit_step_run_ex2")
        elif self.extra is not None:
            L.check(self.lib.tfx_dit_step_run_ex(C.byref(self.sd[ph]), C.byref(self.extra), self.st), "dit_step_run_ex")
        elif self.v_prev is not None:
            L.check(self.lib.tfx_dit_step_run_multistep(C.byref(self.sd[ph]), self.v_prev, self.st), "dit_step_run_multistep")
        else:
            L.check(self.lib.tfx_dit_step_run(C.byref(self.sd[ph]), self.st), "dit_step_run")

    def replay(self, handle):
        L.check(self.lib.tfx_dit_step_replay(handle, self.st), "dit_step_replay")

    def capture(self, ph):
        h = C.c_void_p()
        if self.change is not None:
            rc = self.lib.tfx_dit_step_capture_ex2(C.byref(self.sd[ph]), C.byref(self.extra), C.byref(self.change), self.st, C.byref(h))
        elif self.extra is not None:
            rc = self.lib.tfx_dit_step_capture_ex(C.byref(self.sd[ph]), C.byref(self.extra), self.st, C.byref(h))
        elif self.v_prev is not None:
            rc = self.lib.tfx_dit_step_capture_multistep(C.byref(self.sd[ph]), self.v_prev, self.st, C.byref(h))
        else:
            rc = self.lib.tfx_dit_step_capture(C.byref(self.sd[ph]), self.st, C.byref(h))
        if rc != 0:
            raise CaptureRefused(self.lib.tfx_last_error().decode())
        return h.value

    def destroy(self, handle):
        self.lib.tfx_graph_destroy(handle)

    def metric(self):
        c = self.ses.cache
        c["metric_host"].copy_(c["metric"], non_blocking=True)
        self.side.synchronize()
        return c["metric_host"].tolist()

    def save(self):
        self.side.synchronize()
        return [t.clone() for t in self._state()]

    def restore(self, saved):
        for t, s in zip(self._state(), saved):
            t.copy_(s)

    def _state(self):
        state = (self.gb["lat"], self.gb["step"], self.ses.xin)      # (xin also holds the latents when fused)
        return state + (self.gb["v_prev"],) if self.v_prev is not None else state


def denoise(pipe, ses, mod, latents, coef, n, progress_bar, is_amo=False, fuse=False, amo_noise=None, on_step=None, multistep=False,
            keep=None, change=None):
    """The n steps of one engine call on session `ses`, whose xin holds [latents | masked_image_latents] and whose conditioning is
    set.  mod [n, B, mod_len (+ EULER_PAD when fuse)]: the modulation table.  latents [B, S, C] and coef, the sampler's coefficient
    table, may be None when fuse: the fused step reads the latents from xin and its coefficients from `mod`.  on_step(i, lat): the
    step callback, handed the live latent buffer after step i (it may write to it and to ses.xin).  multistep: the second-order
    multistep sampler -- unfused, coef its [n, 2] table, the history buffer gb["v_prev"] owned by the session; a callback that
    replaces the latents leaves the history (the previous model output) as it is.  keep: known-region sampling --
    dict(x0, noise, mask: bf16 [B, S, C]; sigma: fp32 [n], the scheduler's keep_sigma_table): after every sampler update the latents
    become (1 - mask) scale_noise(x0, sigma_{i+1}, noise) + mask latents (tfx_known_region_blend inside the step); the buffers live in
    the session next to v_prev, because captured graphs bake their addresses.  change: change-map sampling --
    dict(x0, noise: bf16 [B, S, C]; hold: uint8 [B, S, 4]; sigma: fp32 [n]; cut: int32 [n], schedulers.change_cut_table): the same blend
    with the mask decided inside the step, held where hold > cut[step] (tfx_change_map_blend); not together with keep; its buffers
    live in the session too.  Runs on the session's side
    stream (capture needs a non-NULL stream), fenced against the caller's current stream on both sides.  The step cache is on when
    pipe.enable_step_cache() is in force; graphs when pipe.enable_hip_graph(True), no callback and n > 1.  Returns the final
    latents and leaves pipe.step_cache_report set."""
    dev = ses.xin.device
    shape = (ses.B, ses.S, ses.model.out_channels)
    gb = ses.graph_buffers(n, 0 if coef is None else coef.numel(), shape)
    gb["mod_table"][:n, :, :mod.shape[2]].copy_(mod)
    if coef is not None:
        gb["coef"][:coef.numel()].copy_(coef.reshape(-1))
    if latents is not None:
        gb["lat"].copy_(latents)
    gb["step"].zero_()
    if multistep:
        assert not is_amo and not fuse and latents is not None
        if "v_prev" not in gb:           # lives and dies with gb: captured graphs bake its address; step 0 never reads it
            gb["v_prev"] = torch.empty_like(gb["lat"])
    if keep is not None:
        if ses.mixed:
            raise NotImplementedError("known-region sampling does not serve mixed-geometry sessions")
        assert keep["sigma"].numel() == n and keep["sigma"].dtype == torch.float32
        if "keep_x0" not in gb:          # live and die with gb, like v_prev
            gb.update({"keep_" + k: torch.empty_like(gb["lat"]) for k in ("x0", "noise", "mask")})
            gb["keep_sigma"] = torch.zeros(gb["mod_table"].shape[0], dtype=torch.float32, device=dev)
        for k in ("x0", "noise", "mask"):
            gb["keep_" + k].copy_(keep[k])
        gb["keep_sigma"][:n].copy_(keep["sigma"])
    if change is not None:
        if keep is not None:
            raise ValueError("change_map and keep_known exclude each other")
        if ses.mixed:
            raise NotImplementedError("change_map (change-map sampling) does not serve mixed-geometry sessions")
        assert change["sigma"].numel() == n and change["sigma"].dtype == torch.float32
        assert change["cut"].numel() == n and change["cut"].dtype == torch.int32
        if "change_x0" not in gb:        # live and die with gb, like v_prev
            gb.update({"change_" + k: torch.empty_like(gb["lat"]) for k in ("x0", "noise")})
            gb["change_hold"] = torch.empty(shape[0], shape[1], 4, dtype=torch.uint8, device=dev)
            gb["change_sigma"] = torch.zeros(gb["mod_table"].shape[0], dtype=torch.float32, device=dev)
            gb["change_cut"] = torch.zeros(gb["mod_table"].shape[0], dtype=torch.int32, device=dev)
        for k in ("x0", "noise", "hold"):
            gb["change_" + k].copy_(change[k])
        gb["change_sigma"][:n].copy_(change["sigma"])
        gb["change_cut"][:n].copy_(change["cut"])
    decider = None
    if pipe._step_cache is not None:
        ses.step_cache_reset()
        decider = Decider(pipe._step_cache)
    cur = torch.cuda.current_stream(dev)
    side = ses.graph_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        steps = SessionSteps(ses, gb, side, (0,) if decider is None else (1, 2, 3), is_amo, fuse, amo_noise, multistep, keep is not None,
                             change is not None)
        ses._mod_keepalive = gb["mod_cur"]
        key = ("multistep", False) if multistep else (is_amo, fuse)
        if keep is not None:
            key += ("keep",)
        if change is not None:
            key += ("change",)
        run_steps(steps, n, pipe, progress_bar, ses.graphs, key, decider, use_graph=pipe._use_hip_graph,
                  callback=None if on_step is None else lambda i: on_step(i, gb["lat"]))
        out = ops.copy_rows_(ses.xin[:, :, :shape[2]], torch.empty(shape, dtype=BF16, device=dev)) if fuse else gb["lat"].clone()
    out.record_stream(cur)
    cur.wait_stream(side)
    pipe.step_cache_report = decider.report if decider is not None else None
    return out
