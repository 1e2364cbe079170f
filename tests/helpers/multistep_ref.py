"""numpy restatement of the second-order multistep sampler (include/textflux_hip.h: tfx_multistep_step; textflux_amd/schedulers.py:
FlowMatchMultistepScheduler), written from the specification with no code shared with the package; torch serves the bf16 casts only.

    h_i = sigma_{i+1} - sigma_i                                   sigmas fp32 [n + 1], the last one 0
    row 0 = (h_0, 0),  row i = (h_i (1 + h_i / (2 h_{i-1})), -h_i^2 / (2 h_{i-1}))         float64, rounded to fp32 once
    step 0:  x' = bf16( f32(x) + c0 f32(v) )                       the history is not read
    step s:  x' = bf16( f32(x) + (c0 f32(v) + c1 f32(v_prev)) )    every product and sum rounded to fp32 on its own
    then v_prev <- v

and the analytic problem the sampler's order is measured on: a Gaussian target of variance s2 under the flow x(sigma) = (1 - sigma)
x0 + sigma eps, whose exact velocity is v = x (sigma - (1 - sigma) s2) / ((1 - sigma)^2 s2 + sigma^2) and whose exact solution is
x(sigma) = x(1) sqrt((1 - sigma)^2 s2 + sigma^2)."""
import math

import numpy as np
import torch


def bf16_round(a):
    """fp32 array -> the nearest bf16 values (ties to even), as an fp32 array"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def shifted_sigmas(n, mu=None, shift=1.0):
    """The pipeline's grid linspace(1, 1/n, n) in fp32 through the Euler class's shift, and the closing 0: fp32 [n + 1]."""
    s = np.linspace(1.0, 1.0 / n, n).astype(np.float32)
    if mu is not None:
        s = math.exp(mu) / (math.exp(mu) + (1 / s - 1) ** 1.0)
    else:
        s = shift * s / (1 + (shift - 1) * s)
    return np.concatenate([np.asarray(s, dtype=np.float32), np.zeros(1, dtype=np.float32)])


def coef_table(sigmas):
    """sigmas fp32 [n + 1] -> fp32 [n, 2]"""
    h = np.diff(np.asarray(sigmas, dtype=np.float32).astype(np.float64))
    out = np.zeros((len(h), 2), dtype=np.float64)
    for i in range(len(h)):
        if i == 0:
            out[i] = (h[0], 0.0)
        else:
            out[i] = (h[i] * (1.0 + h[i] / (2.0 * h[i - 1])), -h[i] * h[i] / (2.0 * h[i - 1]))
    return out.astype(np.float32)


def step(x, v, v_prev, coef, s):
    """One step on bf16-valued fp32 arrays; v_prev is not looked at when s == 0.  Returns (x', the new history)."""
    x, v = np.asarray(x, dtype=np.float32), np.asarray(v, dtype=np.float32)
    c0, c1 = np.float32(coef[s][0]), np.float32(coef[s][1])
    inc = (c0 * v).astype(np.float32)
    if s > 0:
        inc = (inc + (c1 * np.asarray(v_prev, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    return bf16_round((x + inc).astype(np.float32)), v.copy()


def euler_step(x, v, dsigma):
    """The Euler sibling with the reference's rounding points: x' = bf16( f32(x) + bf16(bf16(dsigma) v) )"""
    ds = bf16_round(np.float32(dsigma).reshape(1))[0]
    return bf16_round(np.asarray(x, dtype=np.float32) + bf16_round(ds * np.asarray(v, dtype=np.float32)))


def velocity(x, sigma, s2):
    """exact velocity in float64"""
    sigma = float(sigma)
    return np.asarray(x, dtype=np.float64) * (sigma - (1.0 - sigma) * s2) / ((1.0 - sigma) ** 2 * s2 + sigma ** 2)


def exact(x1, sigma, s2):
    return np.asarray(x1, dtype=np.float64) * math.sqrt((1.0 - float(sigma)) ** 2 * s2 + float(sigma) ** 2)


def model(x, sigma, s2):
    """what the sampler sees: the exact velocity of the bf16 state, rounded to bf16"""
    return bf16_round(velocity(x, sigma, s2).astype(np.float32))


def run(n, sampler, s2=0.25, mu=1.15, x1=None, sigmas=None, trajectory=None):
    """n steps of `sampler` ("multistep" | "euler") from sigma = 1 to 0 with bf16 state and bf16 model output.  sigmas: fp32 [n + 1]
    (default: shifted_sigmas(n, mu)).  trajectory: a list that receives the state after every step.  Returns (final state, relative
    error ||x - exact(0)|| / ||exact(0)||)."""
    x1 = np.random.default_rng(0).standard_normal(4096) if x1 is None else np.asarray(x1)
    sig = shifted_sigmas(n, mu) if sigmas is None else np.asarray(sigmas, dtype=np.float32)
    assert len(sig) == n + 1
    coef = coef_table(sig)
    x = bf16_round(x1.astype(np.float32))
    hist = None
    for i in range(n):
        v = model(x, sig[i], s2)
        if sampler == "multistep":
            x, hist = step(x, v, hist, coef, i)
        elif sampler == "euler":
            x = euler_step(x, v, sig[i + 1] - sig[i])
        else:
            raise ValueError(sampler)
        if trajectory is not None:
            trajectory.append(x.copy())
    want = exact(bf16_round(x1.astype(np.float32)), 0.0, s2)
    return x, float(np.linalg.norm(x - want) / np.linalg.norm(want))
