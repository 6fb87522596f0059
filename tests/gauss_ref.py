"""Float64 specification of the Gaussian-conditional kernels (csrc/entropy.hip: gauss_lik_fwd / _bwd; csrc/qstep.hip: their step twins
and the rate sweep), a first-order error bound per element and output, the inputs the CPU and GPU tests share, a float32 restatement of
the kernels with planted errors, and the comparison functions.

THE SPECIFICATION is tests/qstep_ref.py (forward, rate_bits; the unit step is step == 1, pinned to unit_forward and to the oracle by
tests/test_gauss_ref_cpu.py) in torch.float64 under autograd, on the float32 values the kernels receive.  Kernel and reference must
agree on the symbol at exact ties, so the reference takes q and y_hat from the float32 expression the integer path shares —
q = rint(fl(fl(y - mu) / s)), y_hat = fl(fl(q s) + mu) — and in eval mode that float32 y_hat enters the float64 graph as the VALUE of
y_in (its derivative with respect to the step is still q: it is handed to qstep_ref.likelihood as y = y_hat - s.detach() q, noise = q).
`analyse` writes the same quantities in closed form (a, b, phi(a), phi(b), dl/dv, dl/dsigma); the CPU test pins it to the autograd
result at 1e-10 of the map's largest value (two float64 routes through Phi(a) - Phi(b), which has lost four digits at sigma = 1e4;
the oracle itself is pinned at 1e-12), and the bounds and the ungated alternatives below come from it.

THE BOUND.  u = 2^-24; every term is first order and names the kernel line (qstep.hip's backward kernel; entropy.hip's is the same
with s = 1) whose rounding it counts:

    e_yin   `yin = yv + s * w`               u (|s noise| + |y_in|)            training only: in eval y_in IS the float32 y_hat
    e_v     `d = yin - m`                    e_yin + u |d|                     the u |y_in| part is what makes a large mu matter
    e_a     `a = (h - v) / sg`               2 u |a| + e_v / sigma             (h = 0.5f s and sg are exact); b likewise
    e_Pa    `std_cum(a)`                     phi(a) (e_a + 2 u |a|) + A_erfc u Phi(a) + 2^-126
                                             (the constant 1/sqrt 2 and its product; erfcf, relative to Phi(a) and Phi(b) separately,
                                             so the cancellation at large sigma is in the bound; the flush of a subnormal)
    e_l     `l = std_cum(a) - std_cum(b)`    e_Pa + e_Pb + u |l|
    e_bit   `bits += log2f(lb)`              e_l / (lik ln 2) + A_log2 u |log2 lik|
    e_pa    `pa = kInvSqrt2Pi * expf(..)`    phi(a) ((A_exp + 2) u + u a^2 / 2 + |a| e_a) + 2^-126
    e_dv    `dl_dv = (pb - pa) / sg`         (e_pa + e_pb) / sigma + 2 u |dl_dv|
    e_ds    `dl_dsg = (pb * b - pa * a)/sg`  (|a| e_pa + phi(a) e_a + u phi(a) |a| + the same in b + u |pb b - pa a|) / sigma + u |dl_dsg|
    dscale  `gs = g * dl_dsg`                |g| e_ds + u |gs| + 2^-126
    dy, dmu `gv = g * dl_dv * sgn`           |g| e_dv + 2 u |gv| + 2^-126, + 2 |gv| where |d| <= e_v (the sign itself is in doubt; gv
                                             vanishes there);  `dy = gy + gh` adds u |dy|
    dstep   `acc += (g * (0.5f * (pa + pb) / sg) + gv * w) + gh * (rq - t)`
                                             |g| (e_pa + e_pb) / (2 sigma) + 3 u |T1|  +  |w| e_gv + u |T2|  +  |gh| (2 u |t| + u |q - t|)
                                             + u |T3|  +  2 u (|T1| + |T2| + |T3|) + 2^-126
    sums    dstep[c], bits_partial[b], the sweep's bits[b][k]: the sum of the terms' bounds + (n terms) u sum |term|

One term is second order.  At |mu| = 1e4 and sigma = 0.11 the rounding of `d = yin - m` puts e_a = e_v / sigma at 5e-3; where v meets
the half width (a = 0) the first-order term |a| e_a of e_pa vanishes while phi(a) still moves by phi(a) e_a^2 / 2.  That is 5.4
first-order bounds on one element of the offset regime's (40, 320) map, for the kernel and the host restatement alike, bit for bit.
So e_pa carries phi(a) (1 + a^2) e_a^2 / 2 and e_Pa carries phi(a) |a| e_a^2 / 2 (the second derivatives of phi and Phi), for that
same line `a = (h - v) / sg`; b likewise.

A_erfc, A_exp, A_log2 are the host libm's float32 errors in units of u, measured against float64 over the arguments the regimes reach
(measure_libm(); the CPU test prints them and holds ALLOW to them):  erfc 1.497 u on [-6, 9.19] (where the result is a normal
float32) -> 1.5;  exp 1.027 u on [-87.3, 0] -> 1.1;  log2 0.999 u, relative to |log2 x|, on [1e-9, 1) -> 1.0.

THE GATES.  `sc >= 0.11f` compares float32 with float32: exact.  An element is undecided
  - for the likelihood gate, if |l - 1e-9| lies within budget x e_l;
  - for the scale gate (scale < 0.11 only), if |g dl/dsigma| lies within budget x its bound of 0.
An undecided element may equal, within bound, the gated value (exactly 0) or the ungated one; in the sums it adds the difference of
the two to the bound.  Every other element is held to the reference's gate: a blocked gradient is exactly 0 (bound 0), a passing one
below the likelihood bound is held to its own per-element bound.
No case may have more than 1 % undecided elements.  One class is left out of that count and reported beside it (`und_flush`): where
both exponentials underflow, |g dl/dsigma| is within the 2^-126 terms of its own bound, so the gated and the ungated value are both
zero to a subnormal and the gate decides nothing.  With a scale below 0.11 and a latent a few steps out, or an upstream gradient of
exactly 0, that is common: 8 of the 15 elements of the edges regime's (3, 5) map, up to 31 % of its large maps, 18 % of the mild
ones.  The CPU test prints both shares for every case and asserts that every uncounted element's ungated dscale is below 1e-30.

THE BUDGETS.  BUDGET[quantity] = 8 x the worst error / bound of the float32 restatement below over every regime, shape of CPU_CASES
and mode (8 x: the project's standing margin for a device libm that differs from the host's by a few ulp); the CPU test recomputes
the table and holds BUDGET to it:

    quantity   worst restatement error / bound    budget   at
    lik        0.819                              6.6      offset 70x192, step, training
    bits       0.231                              1.9      offset 3x5, step, training
    dscale     0.856                              6.9      offset 70x192, step, training
    dy         0.996                              8.0      tails 70x192, step, training
    dmu        0.886                              7.1      offset 70x192, step, training
    dstep      0.811                              6.5      wide 5x65, step, eval
    sweep      0.091                              0.75     wide 9x7

(The restatement sits just under 1: the bound is first order and tight, so a budget of about 8 is eight roundings' worth, no more.)

THE MUTANTS (MUTANTS; `restate32(..., mutant=)`).  Each leaves some budget at least tenfold in some regime, but one: sign(0) = 1 is an
EQUIVALENT mutant of these kernels.  At d = 0, v = 0 and b = -a exactly, so pa == pb bit for bit, dl_dv is exactly 0, and g * 0 * sgn
is zero whatever sgn is (a NaN or infinite g gives NaN either way).  The CPU test asserts that equality instead of a factor.
"""
import functools
import math

import numpy as np
import torch

import qstep_ref as Q

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
SB32, LB32 = np.float32(0.11), np.float32(1e-9)
SB, LB = float(SB32), float(LB32)
ALLOW = {"erfc": 1.5, "exp": 1.1, "log2": 1.0}
BUDGET = {"lik": 6.6, "bits": 1.9, "dscale": 6.9, "dy": 8.0, "dmu": 7.1, "dstep": 6.5, "sweep": 0.75}
MARGIN = 8.0

STEPS = (0.25, 1.0, 3.7)
REGIMES = ("mild", "tails", "wide", "offset", "edges", "nonfinite")
# (rows, C, sliced): tests/test_gauss_kernels_gpu.py says what each reaches
SHAPES = [(1, 1, False), (3, 5, False), (9, 7, False), (257, 4, False), (5, 65, False), (70, 192, False), (130, 192, True), (40, 320, False),
          (33, 32, False), (65, 16, False), (16400, 64, False)]
BIG = (16400, 64)
# the shapes the CPU test runs the restatement and the mutants on: all but the largest, which adds elements, not paths
CPU_SHAPES = [(1, 1), (3, 5), (9, 7), (257, 4), (5, 65), (70, 192), (130, 192), (40, 320), (33, 32), (65, 16)]
# which gates a regime reaches on both sides (likelihood gate, scale gate): the tails regime keeps sigma in [0.11, 0.6] and the wide
# one has sigma >= 4, where no likelihood of a latent within a few sigma falls to 1e-9
GATES = {"mild": (True, True), "tails": (True, False), "wide": (False, False), "offset": (True, True), "edges": (True, True)}

MUTANTS = [
    "lik_gate_without_negative_grad",   # 1  pass only if l >= 1e-9
    "no_lik_gate",                      # 2
    "scale_gate_strict",                # 3  sc > 0.11
    "sign_zero_is_one",                 # 4  (equivalent: see the module docstring)
    "upper_tail_one_minus_phi",         # 5  Phi(x) = 1 - erfc(x / sqrt 2) / 2
    "half_width_unit",                  # 6  h = 0.5
    "noise_unscaled",                   # 7  y_in = y + noise
    "dstep_without_half_width",         # 8
    "dstep_without_y_hat_path",         # 9
    "steps_transposed",                 # 10 the sweep reads steps[c * K + k]
    "bits_without_bound",               # 11
    "dmu_positive",                     # 12
    "y_hat_from_rint_y",                # 13 y_hat = rint(y) - mu
]


def holds(regime, rows, C):
    """whether a (rows, C) map can hold the regime"""
    if (rows, C) == BIG:
        return regime in ("mild", "tails")
    if regime == "nonfinite":
        return rows * C >= 128
    return True


def case_id(regime, rows, C, wide=False):
    return f"{regime}-{rows}x{C}" + ("-sliced" if wide else "")


def steps_for(C, stepped):
    """the step vector of a C-channel map: ones, or {0.25, 1.0, 3.7} in turn with channel 3 at 1/16 and channel 4 at 16"""
    if not stepped:
        return torch.ones(C, dtype=F32)
    s = torch.tensor([STEPS[c % 3] for c in range(C)], dtype=F32)
    if C > 3:
        s[3] = 1.0 / 16
    if C > 4:
        s[4] = 16.0
    return s


# ------------------------------------------------------------------------------------------------------------------------ the inputs

def _mild(g, rows, C, step):
    mu = torch.randn((rows, C), generator=g)
    scale = torch.randn((rows, C), generator=g) + 0.5
    t = torch.randn((rows, C), generator=g) * 3
    return mu, scale, t


EDGE_SCALES = [SB, float(np.nextafter(SB32, np.float32(0))), 0.0, -1.0, 0.5, 2.0]
EDGE_T = [0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -0.0, 1.0]
EDGE_W = [0.0, -1.0, 1.0, -0.25, 0.5, 2.0]
NONFINITE = [(f, v) for f in ("y", "mu", "scale", "noise", "w") for v in (float("nan"), float("inf"), float("-inf"))]


def planted(rows, C):
    """flat positions of the 15 planted values of the non-finite regime, one element each"""
    n = rows * C
    pos = [(3 + 8 * k) % n for k in range(len(NONFINITE))]
    assert len(set(pos)) == len(pos)
    return pos


@functools.lru_cache(maxsize=None)
def inputs(regime, rows, C, stepped, seed=5):
    """float32 y, mu, scale, noise, w (upstream gradient of lik, mixed sign), gh (upstream gradient of y_hat), step [C]"""
    g = torch.Generator().manual_seed(seed + 1000 * rows + C + 7919 * REGIMES.index(regime) + (500 if stepped else 0))
    step = steps_for(C, stepped)
    noise = torch.rand((rows, C), generator=g) - 0.5
    w = torch.rand((rows, C), generator=g) - 0.5      # mixed-sign upstream gradients (both arms of the LowerBound rule)
    gh = torch.randn((rows, C), generator=g)
    mu, scale, t = _mild(g, rows, C, step)
    if regime == "tails":
        # three populations by element: sigma puts (v - h) / sigma in [5, 7] for the eval symbol, for the training value, or is free
        k = torch.arange(rows * C).reshape(rows, C) % 3
        qa = torch.randint(1, 9, (rows, C), generator=g).float()
        sign = torch.where(torch.rand((rows, C), generator=g) < 0.5, -1.0, 1.0)
        t = sign * (qa + (torch.rand((rows, C), generator=g) - 0.5) * 0.8)
        z = 5 + 2 * torch.rand((rows, C), generator=g)
        free = 0.11 + 0.49 * torch.rand((rows, C), generator=g)
        s_eval = (qa - 0.5) * step / z
        s_train = ((t + noise).abs() - 0.5).clamp(min=0.05) * step / z
        scale = torch.where(k == 0, s_eval, torch.where(k == 1, s_train, free)).clamp(0.11, 0.6)
    elif regime == "wide":
        scale = torch.exp(math.log(4.0) + torch.rand((rows, C), generator=g) * math.log(64.0))
        if rows >= 2:
            scale[-1] = 1e4
        far = torch.rand((rows, C), generator=g) < 0.5
        t = torch.where(far, torch.randn((rows, C), generator=g) * scale / step, t)
    elif regime == "offset":
        r = torch.arange(rows).reshape(rows, 1).expand(rows, C)
        c = torch.arange(C).reshape(1, C).expand(rows, C)
        mu = torch.tensor([1e3, -1e3, 1e4, -1e4])[(r + c) % 4] + mu
    elif regime == "edges":
        i = torch.arange(rows * C).reshape(rows, C)
        scale = torch.tensor(EDGE_SCALES, dtype=F32)[i % len(EDGE_SCALES)]
        t = torch.tensor(EDGE_T, dtype=F32)[(i // len(EDGE_SCALES)) % len(EDGE_T)]
        w = torch.tensor(EDGE_W, dtype=F32)[(i // (len(EDGE_SCALES) * len(EDGE_T))) % len(EDGE_W)]
        mu = torch.tensor([0.0, 0.25, -3.5, -0.0], dtype=F32)[(i // 5) % 4]
        noise = torch.tensor([0.25, -0.125, 0.375, -0.375, 0.125], dtype=F32)[(i // 7) % 5]   # (no |t + noise| lands on the half width)
        gh = torch.round(gh * 4) / 4
    y = mu + t * step
    if regime == "edges":
        # every other element with t == 0 has its training value y + s noise at mu exactly (dyadic steps; within a rounding of it on the
        # 3.7 channels); the others have y == mu itself, -0.0 included
        even = torch.arange(rows * C).reshape(rows, C) % 2 == 0
        y = torch.where((t == 0) & even, mu - step * noise, y)
    d = {"y": y, "mu": mu, "scale": scale, "noise": noise, "w": w, "gh": gh, "step": step}
    if regime == "nonfinite":
        for p, (f, v) in zip(planted(rows, C), NONFINITE):
            d[f] = d[f].clone()
            d[f].view(-1)[p] = v
    assert all(v.dtype == F32 for v in d.values())
    return d


def clean_of(rows, C, stepped):
    """the non-finite regime's map without its planted values"""
    d = dict(inputs("nonfinite", rows, C, stepped))
    for p, (f, v) in zip(planted(rows, C), NONFINITE):
        d[f] = d[f].clone()
        d[f].view(-1)[p] = 0.5
    return d


def sweep_steps(C, K, seed=22):
    """K candidates [K, C]: the step vector, random ones in [e^-1.5, e^1.5], two that differ in channel 0's step only, the unit step"""
    g = torch.Generator().manual_seed(seed + C)
    rows = [steps_for(C, True)] + [torch.exp((torch.rand(C, generator=g) - 0.5) * 3.0) for _ in range(max(K - 2, 0))] + [torch.ones(C)]
    s = torch.stack(rows[:K]) if K > 1 else torch.stack(rows[:1])
    if K >= 5:
        s[2] = s[1]
        s[2, 0] = s[1, 0] * 2
    return s.float().contiguous()


# ---------------------------------------------------------------------------------------------------------------- the specification

def quantise32(d, step):
    """the float32 expression of the integer path: q = rint(fl(fl(y - mu) / s)), y_hat = fl(fl(q s) + mu), each operation rounded"""
    q = torch.round((d["y"] - d["mu"]) / step)
    return q, q * step + d["mu"]


def reference(d, step, training, hat=True):
    """qstep_ref under autograd in float64 -> lik, y_hat (float32), dy0 (the likelihood's part), dy (with gh), dmu, dscale, and the
    per-element contributions to dstep (the gradient with respect to a step of the element's own)"""
    y, mu, sc = (d[k].double().requires_grad_() for k in ("y", "mu", "scale"))
    se = step.double().expand_as(y).clone().requires_grad_()
    q, yh32 = quantise32(d, step)
    q = q.double()
    if training:
        lik = Q.likelihood(y, mu, sc, se, d["noise"].double())
    else:
        # y_in: the value y_hat, d/dstep = q, d/dmu = 1 (mu - mu.detach() is an exact zero)
        lik = Q.likelihood(yh32.double() - se.detach() * q + (mu - mu.detach()), mu, sc, se, q)
    t = (y - mu) / se
    yh = se * (t + (q - t).detach()) + mu          # qstep_ref.y_hat with the float32 symbol (its own round(t) may differ at a tie)
    w, gh = d["w"].double(), d["gh"].double()
    zero = lambda x, like: torch.zeros_like(like) if x is None else x
    gl = torch.autograd.grad((lik * w).sum(), [y, mu, sc, se], retain_graph=True, allow_unused=True)
    dy0, dmu, dsc, ds_l = (zero(a, y) for a in gl)
    gy_h, gs_h = torch.autograd.grad((yh * gh).sum(), [y, se], allow_unused=True) if hat else (torch.zeros_like(y), torch.zeros_like(y))
    return {"lik": lik.detach(), "y_hat": yh32, "q": q, "dy0": dy0, "dy": dy0 + gy_h, "dmu": dmu, "dscale": dsc, "terms": ds_l + gs_h,
            "dstep": (ds_l + gs_h).sum(0)}


def _phi(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def _pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def analyse(d, step, training, hat=True, backward=True):
    """the closed form in float64, the bounds, the gates.  Keys: l, lik, bit (log2 lik), e_l, e_bit, below_decided, und_l; with backward:
    dscale, dy0, dy, dmu, terms and their e_*, the ungated alternatives alt_*, und (either gate undecided), blocked (decided zero)"""
    y, mu, sc, noise, w, gh = (d[k].double() for k in ("y", "mu", "scale", "noise", "w", "gh"))
    s = step.double().expand_as(y)
    q, yh32 = quantise32(d, step)
    q = q.double()
    if training:
        yin = y + s * noise
        e_yin = U * ((s * noise).abs() + yin.abs())
        wq = noise
    else:
        yin, e_yin, wq = yh32.double(), torch.zeros_like(y), q
    dd = yin - mu
    v, h, sg = dd.abs(), 0.5 * s, torch.clamp(sc, min=SB)
    e_v = e_yin + U * v
    a, b = (h - v) / sg, (-h - v) / sg
    e_a, e_b = 2 * U * a.abs() + e_v / sg, 2 * U * b.abs() + e_v / sg
    Pa, Pb, pa, pb = _phi(a), _phi(b), _pdf(a), _pdf(b)
    e_Pa = pa * (e_a + 2 * U * a.abs() + a.abs() * e_a * e_a / 2) + ALLOW["erfc"] * U * Pa + TINY
    e_Pb = pb * (e_b + 2 * U * b.abs() + b.abs() * e_b * e_b / 2) + ALLOW["erfc"] * U * Pb + TINY
    l = Pa - Pb
    e_l = e_Pa + e_Pb + U * l.abs()
    lik = torch.clamp(l, min=LB)
    below_decided = l < LB - BUDGET["lik"] * e_l
    und_l = (l - LB).abs() <= BUDGET["lik"] * e_l
    bit = torch.log2(lik)
    e_bit = torch.where(below_decided, torch.zeros_like(l), e_l / (lik * math.log(2.0))) + ALLOW["log2"] * U * bit.abs()
    out = {"l": l, "lik": lik, "bit": bit, "e_l": e_l, "e_bit": e_bit, "below_decided": below_decided, "und_l": und_l, "q": q,
           "y_hat": yh32}
    if not backward:
        return out
    e_pa = pa * ((ALLOW["exp"] + 2) * U + U * a * a / 2 + a.abs() * e_a + (1 + a * a) * e_a * e_a / 2) + TINY
    e_pb = pb * ((ALLOW["exp"] + 2) * U + U * b * b / 2 + b.abs() * e_b + (1 + b * b) * e_b * e_b / 2) + TINY
    dl_dv, dl_ds = (pb - pa) / sg, (pb * b - pa * a) / sg
    e_dv = (e_pa + e_pb) / sg + 2 * U * dl_dv.abs()
    e_ds_a = a.abs() * e_pa + pa * e_a + U * pa * a.abs()          # `pa * a`: pa's error, a's error, the product's rounding
    e_ds_b = b.abs() * e_pb + pb * e_b + U * pb * b.abs()          # `pb * b`
    e_ds = (e_ds_a + e_ds_b + U * (pb * b - pa * a).abs()) / sg + U * dl_ds.abs()
    sgn = torch.sign(dd)
    pass_l = (l >= LB) | (w < 0)
    g = torch.where(pass_l, w, torch.zeros_like(w))
    blocked_l = ~pass_l & ~und_l                                 # decided: every gradient of the element is exactly zero
    # ungated ("alt") values: as if the likelihood gate passed; and for dscale as if the scale gate passed too
    alt_ds = w * dl_ds
    e_gs = w.abs() * e_ds + U * alt_ds.abs() + TINY
    gs = g * dl_ds
    pass_s = (sc >= SB) | (gs < 0)
    dscale = torch.where(pass_s, gs, torch.zeros_like(gs))
    und_s = (sc < SB) & (alt_ds.abs() <= BUDGET["dscale"] * e_gs)
    flush_gs = w.abs() * (a.abs() + b.abs()) * TINY / sg + TINY    # the part of e_gs that the two 2^-126 terms of e_pa, e_pb contribute
    blocked_s = ~pass_s & ~und_s
    alt_gv = w * dl_dv * sgn
    e_gv = w.abs() * e_dv + 2 * U * alt_gv.abs() + TINY + torch.where(v <= e_v, 2 * alt_gv.abs(), torch.zeros_like(v))
    gv = g * dl_dv * sgn
    gy = gv if training else torch.zeros_like(gv)
    ghh = gh if hat else torch.zeros_like(gh)
    t = (y - mu) / s
    T1u, T2u, T3 = w * (pa + pb) / (2 * sg), alt_gv * wq, ghh * (q - t)
    T1, T2 = torch.where(pass_l, T1u, torch.zeros_like(T1u)), gv * wq
    e_T = w.abs() * (e_pa + e_pb) / (2 * sg) + 3 * U * T1u.abs() + wq.abs() * e_gv + U * T2u.abs()
    e_T3 = ghh.abs() * (2 * U * t.abs() + U * (q - t).abs()) + U * T3.abs()
    z = torch.zeros_like(l)
    e_T = torch.where(blocked_l, z, e_T + 2 * U * (T1u.abs() + T2u.abs()))
    e_terms = e_T + e_T3 + 2 * U * T3.abs() + TINY + torch.where(und_l & ~pass_l, (T1u + T2u).abs(), z)
    e_gy = torch.where(blocked_l, z, e_gv) if training else z
    und_flush = und_s & (alt_ds.abs() <= BUDGET["dscale"] * flush_gs)      # undecided only through the 2^-126 terms: both values ~ 0
    out.update({
        "dscale": dscale, "e_dscale": torch.where(blocked_l | blocked_s, z, e_gs), "alt_dscale": alt_ds,
        "dy0": gy, "e_dy0": e_gy, "alt_dy0": alt_gv if training else z,
        "dy": gy + ghh, "e_dy": e_gy + (U * (gy + ghh).abs() if training else z),
        "dmu": -gy, "e_dmu": e_gy, "alt_dmu": -alt_gv if training else z,
        "terms": T1 + T2 + T3, "e_terms": e_terms,
        "und": und_l | und_s, "und_counted": und_l | (und_s & ~und_flush), "und_flush": und_flush & ~und_l, "und_l": und_l, "und_s": und_s,
        "gh32": d["gh"], "blocked_l": blocked_l, "blocked_s": blocked_s, "pass_l": pass_l, "pass_s": pass_s, "gs": gs})
    return out


def block_of(n, nb):
    """gauss_lik_fwd_kernel's element order: flat element i belongs to block (i // 256) % nb"""
    return (torch.arange(n) // 256) % nb


def grid_for(n):
    return min(max((n + 1023) // 1024, 1), 1024)


# ------------------------------------------------------------------------------------------------- the kernels restated in float32

def _bound_below(x, bound):
    return torch.where(x < bound, torch.full_like(x, bound), x)


def g_finite(w):
    return (w - w) == 0


def restate32(d, step, training, hat=True, mutant=None):
    """the kernels' lines in torch.float32, one rounding per operation (host libm for erfc, exp, log2); sums in float64 are the caller's"""
    y, m, sc, noise, w, gh = (d[k] for k in ("y", "mu", "scale", "noise", "w", "gh"))
    s = step.expand_as(y)
    K2, K2P = np.float32(0.70710678118654752440), np.float32(0.39894228040143267794)
    if mutant == "upper_tail_one_minus_phi":
        cum = lambda x: 1.0 - 0.5 * torch.erfc(K2 * x)
    else:
        cum = lambda x: 0.5 * torch.erfc(-K2 * x)
    t = (y - m) / s
    rq = torch.round(t)
    deq = rq * s + m
    wq = noise if training else rq
    if training:
        yin = y + (noise if mutant == "noise_unscaled" else s * noise)
    else:
        yin = deq
    sg = _bound_below(sc, SB32)
    dd = yin - m
    v = dd.abs()
    h = torch.full_like(s, 0.5) if mutant == "half_width_unit" else 0.5 * s
    a, b = (h - v) / sg, (-h - v) / sg
    l = cum(a) - cum(b)
    lb = _bound_below(l, LB32)
    bit = torch.log2(l if mutant == "bits_without_bound" else lb)
    g = torch.where(g_finite(w), w, w - w)
    if mutant == "no_lik_gate":
        blocked = torch.zeros_like(l, dtype=torch.bool)
    elif mutant == "lik_gate_without_negative_grad":
        blocked = ~(l >= LB32)
    else:
        blocked = ~((l >= LB32) | (g < 0))
    g = torch.where(blocked, g - g, g)
    pa, pb = K2P * torch.exp(-0.5 * a * a), K2P * torch.exp(-0.5 * b * b)
    dl_dv = (pb - pa) / sg
    dl_ds = (pb * b - pa * a) / sg
    gs = g * dl_ds
    inside = (sc > SB32) if mutant == "scale_gate_strict" else (sc >= SB32)
    gs = torch.where(~(inside | (gs < 0)), gs - gs, gs)
    zero = torch.zeros_like(dd)
    sgn = torch.where(dd > 0, zero + 1, torch.where(dd < 0, zero - 1, zero + 1 if mutant == "sign_zero_is_one" else zero))
    gv = g * dl_dv * sgn
    gy = gv if training else zero
    ghh = gh if hat else zero
    T1 = zero if mutant == "dstep_without_half_width" else g * (0.5 * (pa + pb) / sg)
    T3 = zero if mutant == "dstep_without_y_hat_path" else ghh * (rq - t)
    terms = (T1 + gv * wq) + T3
    y_hat = (torch.round(y) - m) if mutant == "y_hat_from_rint_y" else deq
    return {"lik": lb, "y_hat": y_hat, "bit": bit, "dscale": gs, "dy0": gy, "dy": gy + ghh if hat else gy, "dmu": gy if mutant == "dmu_positive" else (-gv if training else -(gv - gv)),
            "terms": terms, "dstep": terms.double().sum(0).float(), "bits": bit.double().sum().float()}


def sweep32(d, steps, B, mutant=None):
    """the rate sweep restated: bits [B, K] from the eval forward with each candidate"""
    K, C = steps.shape
    flat = steps.reshape(-1)
    out = []
    for k in range(K):
        sk = flat[torch.arange(C) * K + k] if mutant == "steps_transposed" else steps[k]
        bit = restate32(d, sk, False, mutant=mutant)["bit"]
        out.append(-bit.double().reshape(B, -1).sum(1))
    return torch.stack(out, 1).float()


def sweep_reference(d, steps, B):
    """float64 bits [B, K] (qstep_ref.rate_bits' sum, on the float32 symbol) and their bound"""
    bits, bound = [], []
    for k in range(steps.shape[0]):
        an = analyse(d, steps[k], False, backward=False)
        n = an["bit"].numel() // B
        bits.append(-an["bit"].reshape(B, -1).sum(1))
        bound.append(an["e_bit"].reshape(B, -1).sum(1) + n * U * an["bit"].abs().reshape(B, -1).sum(1))
    return torch.stack(bits, 1), torch.stack(bound, 1)


# ------------------------------------------------------------------------------------------------------------------ the comparisons
# Each returns {name: (figure, bar)}: a figure above its bar fails.  A bar of 0 marks an exact property; its figure counts violations.

def _worst(x):
    x = x.double()
    if x.numel() == 0:
        return 0.0
    return float("inf") if bool(torch.isnan(x).any()) else float(x.max())


def _bits(a):
    return a.contiguous().view(torch.int32)


def _ratio(got, want, bound, alt=None, und=None):
    """per element |got - want| / bound (0 / 0 = 0, x / 0 = inf, NaN stays); an undecided element is measured from the nearest of
    the reference's value, the gated value 0 and the ungated value"""
    got = got.double()
    err = (got - want).abs()
    if und is not None:
        err = torch.where(und, torch.minimum(err, torch.minimum(got.abs(), (got - alt).abs())), err)
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def compare_forward(got, an):
    """got: lik, y_hat [rows, C] float32"""
    out = {"y_hat bits": (float((_bits(got["y_hat"].float()) != _bits(an["y_hat"])).sum()), 0.0),
           "lik": (_worst(_ratio(got["lik"], an["lik"], an["e_l"] + U * an["lik"])), BUDGET["lik"]),
           "lik at the bound": (float((got["lik"].float()[an["below_decided"]] != torch.tensor(LB32)).sum()), 0.0)}
    return out


def compare_backward(got, an, training, hat=True):
    """got: dscale, dy, dmu [rows, C]; hat: whether the call had dy_add / g_hat (an's own analysis must have had it: dy includes gh)"""
    z = torch.zeros_like(an["l"])
    out = {"dscale": (_worst(_ratio(got["dscale"], an["dscale"], an["e_dscale"], an["alt_dscale"], an["und"])), BUDGET["dscale"])}
    ghh = an["gh32"].double() if hat else z
    if training:
        want, e = (an["dy"], an["e_dy"]) if hat else (an["dy0"], an["e_dy0"])
        dy = got["dy"].double()
        err = (dy - want).abs()
        alt = torch.minimum((dy - ghh).abs(), (dy - ghh - an["alt_dy0"]).abs())     # the gated value gh, the ungated one
        err = torch.where(an["und_l"], torch.minimum(err, alt), err)
        out["dy"] = (_worst(torch.where(err == 0, z, err / e)), BUDGET["dy"])
        out["dmu"] = (_worst(_ratio(got["dmu"], an["dmu"], an["e_dmu"], an["alt_dmu"], an["und_l"])), BUDGET["dmu"])
    else:
        want = an["gh32"] if hat else z.float()
        out["dy in eval"] = (float((got["dy"].float() != want).sum()), 0.0)
        out["dmu in eval"] = (float((got["dmu"] != 0).sum()), 0.0)
    return out


def sum_bound(e, terms, dim=0):
    """the bound of a float32 sum of n terms: the terms' own bounds + n u sum |term|"""
    n = terms.shape[dim] if terms.dim() > 1 else terms.numel()
    return e.sum(dim) + n * U * terms.abs().sum(dim)


def compare_dstep(got, an):
    bound = sum_bound(an["e_terms"], an["terms"])
    return {"dstep": (_worst(_ratio(got, an["terms"].sum(0), bound)), BUDGET["dstep"])}


def compare_partials(got, an, nb):
    """bits_partial [nb] against the float64 sum of each block's own elements"""
    n = an["bit"].numel()
    blk = block_of(n, nb)
    bit, e = an["bit"].reshape(-1), an["e_bit"].reshape(-1)
    want = torch.zeros(nb, dtype=F64).index_add_(0, blk, bit)
    cnt = torch.zeros(nb, dtype=F64).index_add_(0, blk, torch.ones(n, dtype=F64))
    bound = torch.zeros(nb, dtype=F64).index_add_(0, blk, e) + cnt * U * torch.zeros(nb, dtype=F64).index_add_(0, blk, bit.abs())
    return {"bits": (_worst(_ratio(got, want, bound)), BUDGET["bits"])}


def compare_sweep(got, want, bound):
    return {"sweep": (_worst(_ratio(got, want, bound)), BUDGET["sweep"])}


def ratio(figure, bar):
    if bar == 0.0:
        return float("inf") if figure > 0 else 0.0
    return figure / bar


def failures(figures):
    return {k: v for k, v in figures.items() if not v[0] <= v[1]}


# ---------------------------------------------------------------------------------------------------------------------------- libm

def measure_libm():
    """the float32 errors of torch's erfc, exp and log2 on the host, in units of u relative to the float64 value, over the arguments the
    regimes reach: erfc where the result is a normal float32 (x in [-6, 9.19]); exp on [-87.3, 0]; log2 on [1e-9, 1)"""
    out = {}
    x = torch.linspace(-6.0, 9.19, 2_000_001, dtype=F64).float()
    out["erfc"] = float(((torch.erfc(x).double() - torch.erfc(x.double())).abs() / torch.erfc(x.double())).max()) / U
    x = torch.linspace(-87.3, 0.0, 2_000_001, dtype=F64).float()
    out["exp"] = float(((torch.exp(x).double() - torch.exp(x.double())).abs() / torch.exp(x.double())).max()) / U
    x = torch.exp(torch.linspace(math.log(1e-9), math.log(1.0 - 2.0 ** -23), 2_000_001, dtype=F64)).float()
    out["log2"] = float(((torch.log2(x).double() - torch.log2(x.double())).abs() / torch.log2(x.double()).abs()).max()) / U
    return out


# ---------------------------------------------------------------------------------------------------------------------- the oracle

def oracle32(d, training, dtype=F32):
    """oracle.leaves.GaussianConditional (unit step) in dtype under autograd, with this module's noise: lik, dy (likelihood part), dmu, dscale"""
    from oracle.leaves import GaussianConditional

    gc = GaussianConditional(None).to(dtype)
    y, mu, sc = (d[k].to(dtype).clone().requires_grad_() for k in ("y", "mu", "scale"))
    if training:
        outputs = y + d["noise"].to(dtype)
    elif dtype == F64:      # on the float32 y_hat cast up, as the specification (the oracle's round(y - mu) + mu: d/dmu = 1, d/dy = 0)
        outputs = quantise32(d, torch.ones(d["y"].shape[1]))[1].double() + (mu - mu.detach())
    else:
        outputs = torch.round(y - mu) + mu
    lik = gc.likelihood_lower_bound(gc._likelihood(outputs, sc, mu))
    g = torch.autograd.grad((lik * d["w"].to(dtype)).sum(), [y, mu, sc], allow_unused=True)
    dy, dmu, dsc = (torch.zeros_like(y) if a is None else a for a in g)
    return {"lik": lik.detach(), "dy0": dy, "dmu": dmu, "dscale": dsc}


def spec32(d, step, training):
    """qstep_ref in float32 under autograd: where the step form is NaN (the oracle has no step; the CPU test pins the unit step's NaN
    pattern to the oracle's)"""
    y, mu, sc = (d[k].clone().requires_grad_() for k in ("y", "mu", "scale"))
    se = step.expand_as(y).clone().requires_grad_()
    lik, yh = Q.forward(y, mu, sc, se, d["noise"] if training else None)
    g = torch.autograd.grad((lik * d["w"]).sum(), [y, mu, sc, se], allow_unused=True, retain_graph=True)
    dy, dmu, dsc, ds = (torch.zeros_like(y) if a is None else a for a in g)
    ds = ds + torch.autograd.grad((yh * d["gh"]).sum(), [se])[0]      # (with g_hat: the kernel's third term)
    return {"lik": lik.detach(), "dy0": dy, "dmu": dmu, "dscale": dsc, "terms": ds}
