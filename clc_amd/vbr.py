"""Variable-rate coding: the table of quantisation steps a model looks its quality up in.

A quantisation step per channel scales the quantiser of a Gaussian-conditional latent: the symbol is round((y - mu) / step), the value
step * symbol + mu, and a symbol under N(0, sigma^2) is a unit-step symbol under sigma / step — the coder's tables stay as they are.
The kernels are csrc/qstep.hip (ops.gaussian_likelihood_step, ops.quantize_build_indexes_step, ops.gauss_rate_sweep).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

STEP_MIN, STEP_MAX = 1.0 / 16, 16.0


class StepTable(nn.Module):
    """``levels`` step vectors of ``channels`` steps, as one parameter ``log_step [levels, channels]``: the geometric ladder from
    ``coarsest`` (level 0) to ``finest`` (the last level), equal for every channel — the default ladder's middle level is exactly
    ln 1 = 0, the fixed-rate codec.  ``forward(q)`` interpolates the log steps between the levels around the float quality ``q`` in
    [0, levels - 1] (geometric interpolation of the steps), clamps to [1/16, 16], and rounds ONCE from float64 to f32: encoder and
    decoder get the same bits from the same parameters.  Higher q: finer steps, more bits."""

    def __init__(self, channels, levels=5, coarsest=2.0, finest=0.5):
        super().__init__()
        channels, levels = int(channels), int(levels)
        if channels < 1 or levels < 1:
            raise ValueError(f"StepTable: channels and levels must be positive (got channels={channels}, levels={levels})")
        coarsest, finest = float(coarsest), float(finest)
        if not (STEP_MIN <= finest <= coarsest <= STEP_MAX):
            raise ValueError(f"StepTable: need {STEP_MIN} <= finest <= coarsest <= {STEP_MAX} (got coarsest={coarsest}, finest={finest})")
        self.channels, self.levels = channels, levels
        a, b = math.log(coarsest), math.log(finest)
        rungs = [a + (b - a) * i / (levels - 1) for i in range(levels)] if levels > 1 else [a]
        self.log_step = nn.Parameter(torch.tensor(rungs, dtype=torch.float64).float().reshape(levels, 1).repeat(1, channels))

    def check_q(self, q, who="StepTable.forward"):
        """q as a float in [0, levels - 1]; anything else is refused by name"""
        if isinstance(q, bool) or not isinstance(q, (int, float)):
            raise TypeError(f"{who}: q must be a Python float (got {type(q).__name__})")
        q = float(q)
        if not (0.0 <= q <= self.levels - 1):   # (a NaN fails both comparisons)
            raise ValueError(f"{who}: q must be in [0, {self.levels - 1}] for {self.levels} rate levels (got q={q})")
        return q

    def forward(self, q):
        q = self.check_q(q)
        i = min(int(math.floor(q)), self.levels - 1)
        f = q - i
        ls = self.log_step.double()
        log = (1.0 - f) * ls[i] + f * ls[min(i + 1, self.levels - 1)]
        return torch.clamp(torch.exp(log), STEP_MIN, STEP_MAX).float()

    def candidates(self, n=16):
        """n evenly spaced qualities over [0, levels - 1], ascending (coarsest first)"""
        top = float(self.levels - 1)
        return [top * k / (n - 1) for k in range(n)] if n > 1 else [0.0]


def model_step(model, q, who):
    """The step vector of quality q from ``model.y_step`` (None for q None: the fixed-rate path).  A q the model has no table for, or
    one outside it, is refused by name — before any device work."""
    if q is None:
        return None
    q = check_quality(model, q, who)
    return model.y_step(q)


def check_quality(model, q, who):
    """the host half of model_step: q as a checked float, nothing launched"""
    table = getattr(model, "y_step", None)
    if table is None:
        raise ValueError(f"{who}: q={q!r} needs a step table — build the model with rate_levels > 0")
    return table.check_q(q, who)


def frame_qualities(q, frames, who):
    """q of a video call -> one entry per frame: None (fixed rate), one float for every frame, or a list of one float per frame (the
    usual keyframe-finer-than-P-frames allocation); one q serves both latents of a P-frame"""
    if q is None:
        return [None] * frames
    if isinstance(q, (list, tuple)):
        if len(q) != frames:
            raise ValueError(f"{who}: q lists {len(q)} qualities for {frames} frames (one per frame, or one float for all)")
        return list(q)
    return [q] * frames


def refuse_rate_levels(who, kwargs):
    """the model families without a step table refuse its arguments by name"""
    for name in ("rate_levels", "q", "target_bytes"):
        if name in kwargs and kwargs[name] not in (None, 0):
            raise ValueError(f"{who} has no quantisation-step table: {name} is built for ScaleHyperprior, MeanScaleHyperprior and ScaleSpaceFlow only (got {name}={kwargs[name]!r})")
