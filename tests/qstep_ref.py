"""THE SPECIFICATION of the quantisation step, in plain torch: what clc_gauss_lik_step_fwd / _bwd,
clc_quantize_build_indexes_step and clc_gauss_rate_sweep compute, and what clc_amd.vbr.StepTable returns.

The differentiable part runs in whatever dtype it is handed (the tests hand it float64) and its gradients ARE autograd through it;
the integer path is an f32 restatement of the one expression the encoder and the decoder share.  Tensors are [rows, C] (or anything
whose last dimension is the channel); ``step`` is [C].

    sigma = max(scale, 0.11)          (LowerBound's gradient rule: pass if scale >= 0.11 or the gradient is negative)
    t     = (y - mu) / step
    y_hat = step * ste_round(t) + mu, ste_round(t) = t + (round(t) - t).detach()
    y_in  = y + step * u  (training)  |  step * round(t) + mu  (eval; round() has no gradient, so the step reaches y_in as a factor)
    v     = |y_in - mu|
    lik   = max(Phi((step / 2 - v) / sigma) - Phi((-step / 2 - v) / sigma), 1e-9)      (LowerBound's rule again)
"""
import math

import numpy as np
import torch

SCALE_BOUND = float(np.float32(0.11))   # the kernels' 0.11f and 1e-9f (and the oracle's float32 LowerBound buffers), exactly
LIK_BOUND = float(np.float32(1e-9))
STEP_MIN, STEP_MAX = 1.0 / 16, 16.0


class _LowerBoundFn(torch.autograd.Function):
    """max(x, b); gradient passes where x >= b or the gradient is negative (CompressAI's rule, gauss_lik_bwd_kernel's)"""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x)
        ctx.bound = bound
        return torch.clamp(x, min=bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ((x >= ctx.bound) | (g < 0)).to(g.dtype) * g, None


def lower_bound(x, bound):
    return _LowerBoundFn.apply(x, bound)


def phi(x):
    return 0.5 * torch.erfc(-(2 ** -0.5) * x)


def ste_round(t):
    return t + (torch.round(t) - t).detach()


def y_hat(y, mu, step):
    return step * ste_round((y - mu) / step) + mu


def likelihood_unbounded(y, mu, scale, step, noise=None):
    """Phi(a) - Phi(b) before the likelihood bound; noise: the pre-drawn U(-1/2, 1/2) of training mode, None in eval"""
    sigma = lower_bound(scale, SCALE_BOUND)
    if noise is not None:
        y_in = y + step * noise
    else:
        y_in = step * torch.round((y - mu) / step) + mu
    v = torch.abs(y_in - mu)
    half = step / 2
    return phi((half - v) / sigma) - phi((-half - v) / sigma)


def likelihood(y, mu, scale, step, noise=None):
    return lower_bound(likelihood_unbounded(y, mu, scale, step, noise), LIK_BOUND)


def forward(y, mu, scale, step, noise=None):
    """-> (lik, y_hat), the two outputs of clc_gauss_lik_step_fwd"""
    return likelihood(y, mu, scale, step, noise), y_hat(y, mu, step)


def unit_forward(y, mu, scale, noise=None):
    """the unit-step definition the package had before the step (include/clc_hip.h, clc_gauss_lik_fwd), restated on its own"""
    sigma = lower_bound(scale, SCALE_BOUND)
    rq = torch.round(y - mu)
    y_in = y + noise if noise is not None else rq + mu
    v = torch.abs(y_in - mu)
    lik = lower_bound(phi((0.5 - v) / sigma) - phi((-0.5 - v) / sigma), LIK_BOUND)
    return lik, (y - mu) + (rq - (y - mu)).detach() + mu


def rate_bits(y, mu, scale, steps):
    """clc_gauss_rate_sweep: y, mu, scale [B, n, C], steps [K, C] -> bits [B, K] = - sum log2 lik_eval"""
    out = []
    for k in range(steps.shape[0]):
        lik = likelihood(y, mu, scale, steps[k])
        out.append(-torch.log2(lik).reshape(lik.shape[0], -1).sum(1))
    return torch.stack(out, 1)


# ---- the integer path: f32, one expression, for encoder and decoder ----

def scale_index(sg, table):
    """n - 1 - #{k < n - 1: sg <= table[k]} on f32 numpy arrays; a NaN compares false everywhere and takes the last row"""
    sg = np.asarray(sg, np.float32)
    table = np.asarray(table, np.float32)
    idx = np.full(sg.shape, len(table) - 1, np.int32)
    for s in table[:-1]:
        idx -= (sg <= s).astype(np.int32)
    return idx


def integer_path(y, mu, scale, step, table):
    """f32 numpy [rows, C], step [C] -> (symbols int32, indexes int32, y_hat f32).
    symbol = (int) rint((y - mu) / step);  index = scale_index(max(scale, 0.11) / step);  y_hat = (float) symbol * step + mu, a rounded
    multiply and a rounded add.  IEEE division and round-half-even, as on the device."""
    y, mu, scale, step = (np.asarray(a, np.float32) for a in (y, mu, scale, step))
    q = np.rint((y - mu) / step).astype(np.float32)
    sg = np.fmax(scale, np.float32(SCALE_BOUND))   # C's fmaxf: of a NaN and a number, the number — a NaN SCALE is coded as 0.11
    with np.errstate(invalid="ignore", divide="ignore"):
        idx = scale_index((sg / step).astype(np.float32), table)
    prod = (q * step).astype(np.float32)
    return q.astype(np.int32), idx, (prod + mu).astype(np.float32)


def dequantise(symbols, mu, step):
    """the decoder's half of the same expression"""
    prod = (np.asarray(symbols).astype(np.float32) * np.asarray(step, np.float32)).astype(np.float32)
    return (prod + np.asarray(mu, np.float32)).astype(np.float32)


# ---- the step table ----

def ladder(levels=5, coarsest=2.0, finest=0.5):
    """log steps of the geometric ladder, float64 [levels]: ln coarsest at level 0 down to ln finest at the last"""
    if levels == 1:
        return [math.log(coarsest)]
    a, b = math.log(coarsest), math.log(finest)
    return [a + (b - a) * i / (levels - 1) for i in range(levels)]


def step_of(log_step, q):
    """log_step [levels, C] (any dtype) -> the step vector of quality q, float64 maths, rounded once to f32"""
    levels = log_step.shape[0]
    i = min(int(math.floor(q)), levels - 1)
    f = q - i
    ls = log_step.double()
    lo = ls[i]
    hi = ls[min(i + 1, levels - 1)]
    return torch.clamp(torch.exp((1 - f) * lo + f * hi), STEP_MIN, STEP_MAX).float()
