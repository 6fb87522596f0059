"""Float64 specification of the factorised-density kernels (csrc/entropy.hip: clc_eb_lik_fwd, clc_eb_lik_bwd, clc_eb_aux), the inputs
the CPU and GPU tests share, and the comparison functions both apply.

The specification is plain torch.float64 under autograd, evaluated on the float32 values the kernels get (cast up, never regenerated):

    logits(x)   five layers softplus(M_k) @ h + b_k per channel, + tanh(f_k) * tanh(.) after the first four
    likelihood  lower = logits(v - 1/2), upper = logits(v + 1/2), s = -sign(lower + upper), raw = |sigmoid(s upper) - sigmoid(s lower)|,
                lik = max(raw, 1e-9) with the LowerBound gradient rule: pass if raw >= bound or grad < 0
    v           training: z + noise;  inference: the float32 value rint(z - med) + med (numpy float32), cast up
    aux         per channel sum_q |logits(quantiles[c, q]) - target[q]|, parameters detached, gradient with respect to the quantiles

Every parameter is expanded to one copy per row before use, so one backward pass gives both the gradient (the sum over rows) and the
sum of the absolute per-row contributions, the scale below which a cancelling float32 sum cannot be held.

Maps are [rows, C]; parameters are the EntropyBottleneck's own tensors (matrices [C, fo, fi], biases and factors [C, fo, 1], quantiles
[C, 1, 3]).  A `mutant` names one planted error (MUTANTS); tests/test_eb_ref_cpu.py shows that the comparison functions reject each.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
BOUND = 1e-9
BOUND_F32 = np.float32(1e-9)

# the bars of tests/test_kernels_gpu.py::test_gaussian_likelihood / test_entropy_bottleneck_likelihood
BARS = {"lik": 1e-5, "log": 2e-3, "grad": 2e-4, "aux": 1e-5, "dq": 1e-4}

GRAD_NAMES = [f"dmatrix{k}" for k in range(5)] + [f"dbias{k}" for k in range(5)] + [f"dfactor{k}" for k in range(4)]

MUTANTS = [
    "factor_grad_without_dtanh",      # 1  d/df without (1 - tanh(f)^2)
    "matrix_grad_without_sigmoid",    # 2  d/dM without sigmoid(M)
    "dpre_without_tanh_term",         # 3  dpre = dh instead of dh (1 + tanh(f) (1 - tanh(pre)^2))
    "bound_always_passes",            # 4
    "bound_never_passes_below",       # 5
    "bound_passes_positive_grad",     # 6  grad > 0 in place of grad < 0
    "median_from_quantile0",          # 7
    "round_half_away",                # 8
    "noise_ignored",                  # 9
    "eval_dz_nonzero",                # 10
    "sums_drop_rows_from_256",        # 11
    "sums_drop_last_row",             # 12
    "channel_slot_shifted",           # 13 channel c's gradients in slot c - 1
    "aux_parameter_grads_leak",       # 14
    "aux_target_reversed",            # 15
]

# (rows, C, sliced): see tests/test_eb_kernels_gpu.py for what each reaches
SHAPES = [(1, 1, False), (3, 5, False), (255, 2, False), (256, 2, False), (257, 3, False), (600, 4, True), (128, 192, False)]
# every shape on set A, every set on (257, 3) and the sliced (600, 4)
CASES = [("A",) + s for s in SHAPES] + [(ps,) + s for ps in ("B", "C") for s in SHAPES if s[:2] in ((257, 3), (600, 4))]
AUX_CS = [1, 63, 64, 65, 192]


def case_id(case):
    ps, rows, C, wide = case
    return f"{ps}-{rows}x{C}" + ("-sliced" if wide else "")


# ---------------------------------------------------------------------------------------------------------------- the specification

class _TanhNoDeriv(torch.autograd.Function):       # mutant 1
    @staticmethod
    def forward(ctx, x):
        return torch.tanh(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _SoftplusNoDeriv(torch.autograd.Function):   # mutant 2
    @staticmethod
    def forward(ctx, x):
        return F.softplus(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _LowerBound(torch.autograd.Function):
    """max(x, bound); backward: grad where x >= bound or grad < 0, else 0 (compressai's LowerBound), written out"""

    @staticmethod
    def forward(ctx, x, bound, rule):
        ctx.save_for_backward(x)
        ctx.bound, ctx.rule = bound, rule
        return torch.clamp(x, min=bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        inside = x >= ctx.bound
        passes = {"spec": inside | (g < 0), "bound_always_passes": torch.ones_like(inside), "bound_never_passes_below": inside,
                  "bound_passes_positive_grad": inside | (g > 0)}[ctx.rule]
        return torch.where(passes, g, torch.zeros_like(g)), None, None


def logits_cumulative(x, mats, biases, factors, mutant=None):
    """x [..., C]; parameters [C, fo, fi] / [C, fo, 1] or with leading dimensions that broadcast against x's -> logits [..., C]"""
    softplus = _SoftplusNoDeriv.apply if mutant == "matrix_grad_without_sigmoid" else F.softplus
    tanh_f = _TanhNoDeriv.apply if mutant == "factor_grad_without_dtanh" else torch.tanh
    h = x[..., None, None]
    for k in range(5):
        h = torch.matmul(softplus(mats[k]), h) + biases[k]
        if k < 4:
            h = h + tanh_f(factors[k]) * torch.tanh(h.detach() if mutant == "dpre_without_tanh_term" else h)
    return h[..., 0, 0]


def likelihood(v, mats, biases, factors, mutant=None):
    """-> (raw, max(raw, 1e-9) under the LowerBound gradient rule)"""
    lower = logits_cumulative(v - 0.5, mats, biases, factors, mutant)
    upper = logits_cumulative(v + 0.5, mats, biases, factors, mutant)
    s = -torch.sign(lower + upper).detach()
    raw = torch.abs(torch.sigmoid(s * upper) - torch.sigmoid(s * lower))
    rule = mutant if mutant in ("bound_always_passes", "bound_never_passes_below", "bound_passes_positive_grad") else "spec"
    return raw, _LowerBound.apply(raw, BOUND, rule)


def z_hat_f32(z, P, mutant=None):
    """the float32 value rint(z - med) + med, in numpy float32 (round half to even)"""
    med = P["q"][:, 0, 0 if mutant == "median_from_quantile0" else 1].numpy().astype(np.float32)[None, :]
    t = z.numpy().astype(np.float32) - med
    r = np.rint(t)
    if mutant == "round_half_away":
        r = np.where(np.abs(t - np.trunc(t)) == np.float32(0.5), np.trunc(t) + np.sign(t), r).astype(np.float32)
    out = r + med
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def param_list(P):
    return list(P["m"]) + list(P["b"]) + list(P["f"])


def reference(P, d, training, mutant=None):
    """float64 results on the float32 inputs d (latents()) and parameters P (params()):
    lik, raw, z_hat (float32), dz, grads[14] and gabs[14] (the sums over rows of the per-row contributions and of their magnitudes)"""
    z = d["z"].double().requires_grad_()
    rows, C = z.shape
    leaf = [t.double().requires_grad_() for t in param_list(P)]
    per_row = [t.unsqueeze(0).expand(rows, *t.shape) for t in leaf]
    for t in per_row:
        t.retain_grad()
    zh = z_hat_f32(d["z"], P, mutant)
    if training:
        v = z if mutant == "noise_ignored" else z + d["noise"].double()
    else:
        v = zh.double()
        if mutant == "eval_dz_nonzero":
            v = v + (z - z.detach())
    raw, lik = likelihood(v, per_row[0:5], per_row[5:10], per_row[10:14], mutant)
    (lik * d["w"].double()).sum().backward()
    G = [t.grad for t in per_row]
    for g, t in zip(G, leaf):
        assert torch.allclose(g.sum(0), t.grad, rtol=1e-10, atol=1e-300)
    if mutant == "sums_drop_rows_from_256":
        grads = [g[:256].sum(0) for g in G]
    elif mutant == "sums_drop_last_row":
        grads = [g[:-1].sum(0) for g in G]
    else:
        grads = [g.sum(0) for g in G]
    if mutant == "channel_slot_shifted":
        grads = [torch.roll(g, -1, 0) for g in grads]
    dz = z.grad if z.grad is not None else torch.zeros_like(z)
    return {"lik": lik.detach(), "raw": raw.detach(), "z_hat": zh, "dz": dz, "grads": grads, "gabs": [g.abs().sum(0) for g in G],
            "w": d["w"]}


def aux(P, mutant=None):
    """float64: per-channel loss [C], dquantiles [C, 3], and the parameters' gradients (all zero: they are detached)"""
    quant = P["q"].double().requires_grad_()
    leaf = [t.double().requires_grad_() for t in param_list(P)]
    use = leaf if mutant == "aux_parameter_grads_leak" else [t.detach() for t in leaf]
    target = P["target"].double()
    if mutant == "aux_target_reversed":
        target = target.flip(0)
    logits = logits_cumulative(quant[:, 0, :].t(), use[0:5], use[5:10], use[10:14])      # [3, C]
    loss = (logits - target[:, None]).abs().sum(0)
    loss.sum().backward()
    return {"loss": loss.detach(), "dq": quant.grad[:, 0, :].clone(), "dparams": [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaf]}


# ------------------------------------------------------------------------------------------------------------------------ the oracle

def oracle_module(P, dtype):
    """oracle.leaves.EntropyBottleneck carrying P's values in dtype"""
    from oracle.leaves import EntropyBottleneck

    eb = EntropyBottleneck(P["q"].shape[0])
    with torch.no_grad():
        for k in range(5):
            getattr(eb, f"_matrix{k}").copy_(P["m"][k])
            getattr(eb, f"_bias{k}").copy_(P["b"][k])
            if k < 4:
                getattr(eb, f"_factor{k}").copy_(P["f"][k])
        eb.quantiles.copy_(P["q"])
    assert torch.equal(eb.target, P["target"])
    return eb.to(dtype)


def oracle_result(P, d, training, dtype):
    """the oracle's own functions in dtype, in the layout of reference().  float32: everything in float32, torch.round included;
    float64: on the float32 z_hat cast up, as the specification."""
    eb = oracle_module(P, dtype)
    z = d["z"].to(dtype).clone().requires_grad_()      # (a copy: the shared inputs stay as they are)
    rows, C = z.shape
    med = eb._get_medians()
    zc = z.t().reshape(C, 1, rows)
    if dtype == F32:
        zh = (torch.round(zc - med) + med).detach()
    else:
        zh = z_hat_f32(d["z"], P).t().reshape(C, 1, rows).to(dtype)
    v = zc + d["noise"].to(dtype).t().reshape(C, 1, rows) if training else zh
    raw = eb._likelihood(v)
    lik = eb.likelihood_lower_bound(raw)
    (lik * d["w"].to(dtype).t().reshape(C, 1, rows)).sum().backward()
    back = lambda t: t.detach().reshape(C, rows).t().contiguous()
    grads = [getattr(eb, f"_matrix{k}").grad for k in range(5)] + [getattr(eb, f"_bias{k}").grad for k in range(5)] + \
            [getattr(eb, f"_factor{k}").grad for k in range(4)]
    return {"lik": back(lik), "raw": back(raw), "z_hat": back(zh), "dz": z.grad if z.grad is not None else torch.zeros_like(z), "grads": grads}


def oracle_aux(P, dtype):
    eb = oracle_module(P, dtype)
    total = eb.loss()
    total.backward()
    per_channel = torch.abs(eb._logits_cumulative(eb.quantiles, True) - eb.target).sum((1, 2)).detach()
    dparams = [getattr(eb, f"_matrix{k}").grad for k in range(5)] + [getattr(eb, f"_bias{k}").grad for k in range(5)] + \
              [getattr(eb, f"_factor{k}").grad for k in range(4)]
    return {"loss": per_channel, "total": total.detach(), "dq": eb.quantiles.grad[:, 0, :].clone(),
            "dparams": [g if g is not None else torch.zeros(1, dtype=dtype) for g in dparams]}


# ------------------------------------------------------------------------------------------------------------------------ the inputs

def _new_module(C, seed):
    from oracle.leaves import EntropyBottleneck

    with torch.random.fork_rng():
        torch.manual_seed(seed)
        return EntropyBottleneck(C)


@functools.lru_cache(maxsize=None)
def params(ps, C):
    """parameter set "A", "B" or "C" for C channels, float32.
    A: the weight recipe with seed 3, heavy tails, the likelihood bound is out of reach.
    B: A with _matrix0 += 2: the density falls through the bound inside the ramp of latents().
    C: the constructor's initialisation (every factor zero) with _matrix1[c, 0, 0] = 21 (softplus takes its x > 20 branch) and
       _matrix1[c, 1, 1] = -30 (softplus and sigmoid vanish); medians and outer quantiles are multiples of 1/8."""
    from oracle.recipe import apply_weight_recipe

    eb = _new_module(C, 1234)
    if ps in ("A", "B"):
        apply_weight_recipe(eb, 3)
    with torch.no_grad():
        if ps == "B":
            eb._matrix0 += 2.0
        if ps == "C":
            assert all(float(getattr(eb, f"_factor{k}").abs().max()) == 0.0 for k in range(4))
            eb._matrix1[:, 0, 0] = 21.0
            eb._matrix1[:, 1, 1] = -30.0
            g = torch.Generator().manual_seed(77)
            med = torch.randint(-8, 9, (C,), generator=g).float() / 8
            lo = 3.0 + torch.randint(0, 33, (C,), generator=g).float() / 8
            hi = 3.0 + torch.randint(0, 33, (C,), generator=g).float() / 8
            eb.quantiles.copy_(torch.stack([med - lo, med, med + hi], -1).reshape(C, 1, 3))
    P = {"m": tuple(getattr(eb, f"_matrix{k}").detach().clone() for k in range(5)),
         "b": tuple(getattr(eb, f"_bias{k}").detach().clone() for k in range(5)),
         "f": tuple(getattr(eb, f"_factor{k}").detach().clone() for k in range(4)),
         "q": eb.quantiles.detach().clone(), "target": eb.target.detach().clone()}
    assert all(t.dtype == F32 for t in param_list(P))
    return P


TIE_KS = (-6, -5, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6)     # t = k + 1/2, k of both parities


def layout(ps, rows):
    """(ramp rows, the +-1e4 row or None, the tie rows) of a map of `rows` rows"""
    n_ramp = min(40, rows // 4)
    huge = n_ramp if rows >= 8 else None
    ties = list(range(n_ramp + 1, n_ramp + 1 + len(TIE_KS))) if ps == "C" and rows >= 64 else []
    return n_ramp, huge, ties


def _raw64(P, z, noise, training):
    with torch.no_grad():
        v = z.double() + noise.double() if training else z_hat_f32(z, P).double()
        return likelihood(v, *[[t.double() for t in ts] for ts in (P["m"], P["b"], P["f"])])[0]


def _near_tie(P, z, ties):
    t = z.double() - P["q"][:, 0, 1].double()[None, :]
    near = ((t - torch.floor(t)) - 0.5).abs() < 1e-3
    near[ties] = False
    return near


def _near_bound(P, z, noise):
    near = torch.zeros(z.shape, dtype=torch.bool)
    for training in (False, True):
        near |= (_raw64(P, z, noise, training) / BOUND - 1.0).abs() < 1e-3
    return near


@functools.lru_cache(maxsize=None)
def latents(ps, rows, C, seed=5):
    """float32 z, noise, w (upstream gradient of the likelihood, mixed sign) and gh (upstream gradient of z_hat) for set ps.
    z = med + t: t ~ N(0, 2^2); the leading rows ramp t from -70 to 70 (jittered per channel); one row has t = +-10000.25; in set C
    twelve rows have t = k + 1/2 exactly.  Two conditions hold for every element, in the float64 arithmetic of the specification:
    outside the tie rows no z - med is within 1e-3 of a half-integer, and no raw likelihood (training or inference) is within a
    relative 1e-3 of the bound."""
    P = params(ps, C)
    g = torch.Generator().manual_seed(seed + 1000 * rows + C)
    med = P["q"][:, 0, 1][None, :]
    t = torch.randn((rows, C), generator=g) * 2
    n_ramp, huge, ties = layout(ps, rows)
    if n_ramp:
        t[:n_ramp] = torch.linspace(-70.0, 70.0, n_ramp)[:, None] + (torch.rand((n_ramp, C), generator=g) * 2 - 1)
    if huge is not None:
        t[huge] = 10000.25 * (1 - 2 * (torch.arange(C) % 2).float())
    for r, k in zip(ties, TIE_KS):
        t[r] = k + 0.5
    z = med + t
    noise = torch.rand((rows, C), generator=g) - 0.5
    w = torch.rand((rows, C), generator=g) - 0.3
    gh = torch.randn((rows, C), generator=g)
    for _ in range(12):
        tie, bound = _near_tie(P, z, ties), _near_bound(P, z, noise)
        if not bool(tie.any() | bound.any()):
            break
        z = torch.where(tie, z + 0.01, z)
        z = torch.where(bound & ~tie, z + 0.25, z)
    check_conditions(P, {"z": z, "noise": noise}, ps)
    if ties:
        assert torch.equal(z[ties] - med, torch.tensor(TIE_KS).float()[:, None].expand(len(ties), C) + 0.5), "the ties are not exact"
    return {"z": z, "noise": noise, "w": w, "gh": gh}


def check_conditions(P, d, ps):
    """both input conditions, every element"""
    rows = d["z"].shape[0]
    ties = layout(ps, rows)[2]
    assert not bool(_near_tie(P, d["z"], ties).any()), "a latent sits within 1e-3 of a rounding tie"
    assert not bool(_near_bound(P, d["z"], d["noise"]).any()), "a float64 likelihood sits within a relative 1e-3 of the bound"


# ------------------------------------------------------------------------------------------------------------------- the comparisons
# Each returns {name: (figure, bar)}: a figure above its bar fails.  A bar of 0 marks an exact property; its figure counts violations.

def _worst(x):
    x = x.double()
    if x.numel() == 0:
        return 0.0
    return float("inf") if not bool(torch.isfinite(x).all()) else float(x.max())


def _bits(a):
    return a.contiguous().view(torch.int32)


def compare_forward(got, ref):
    """got: lik [rows, C], z_hat [rows, C] (float32, or float64 holding float32 values)"""
    lik, lik64 = got["lik"].double(), ref["lik"]
    out = {"z_hat bits": (float((_bits(got["z_hat"].float()) != _bits(ref["z_hat"])).sum()), 0.0),
           "lik": (_worst((lik - lik64).abs()) / float(lik64.max()), BARS["lik"]),
           "log lik": (_worst((torch.log(lik) - torch.log(lik64)).abs()), BARS["log"])}
    below = ref["raw"] < BOUND
    out["lik at the bound"] = (float((got["lik"].float()[below] != torch.tensor(BOUND_F32)).sum()), 0.0)
    return out


def compare_backward(got, ref, training):
    """got: dz [rows, C], grads: 14 tensors shaped like the parameters.  dz on its own maximum; each parameter gradient per channel,
    per element on the larger of the channel's largest magnitude and the element's float64 sum of absolute per-row contributions
    (rows terms, each held to the bar on its own size, cannot be held tighter than the bar on their absolute sum)."""
    out = {}
    dz, dz64 = got["dz"].double(), ref["dz"]
    if training:
        out["dz"] = (_worst((dz - dz64).abs()) / max(float(dz64.abs().max()), 1e-300), BARS["grad"])
        # below the bound the LowerBound rule decides: a positive upstream gradient is blocked (dz is exactly zero), a negative one
        # passes (held to the gradient bar on the largest dz among such elements: they are far too small to show on the map's maximum)
        below = ref["raw"] < BOUND
        blocked, passed = below & (ref["w"] >= 0), below & (ref["w"] < 0)
        out["dz blocked below the bound"] = (float((dz[blocked] != 0).sum()), 0.0)
        assert float(dz64[blocked].abs().sum()) == 0.0
        if bool(passed.any()):
            out["dz passed below the bound"] = (_worst((dz - dz64)[passed].abs()) / max(float(dz64[passed].abs().max()), 1e-300), BARS["grad"])
    else:
        out["dz in inference"] = (float((dz != 0).sum()) + float((~torch.isfinite(dz)).sum()), 0.0)
    bad = 0
    for name, g, g64, gabs in zip(GRAD_NAMES, got["grads"], ref["grads"], ref["gabs"]):
        C = g64.shape[0]
        g = g.double().reshape(C, -1)
        bad += int((~torch.isfinite(g)).sum())
        chan_max = g64.reshape(C, -1).abs().max(1, keepdim=True).values
        scale = torch.maximum(chan_max, gabs.reshape(C, -1)).clamp(min=1e-300)
        out[name] = (_worst((g - g64.reshape(C, -1)).abs() / scale), BARS["grad"])
    out["gradients not finite"] = (float(bad), 0.0)
    return out


def compare_aux(got, ref):
    """got: loss [C], dq [C, 3] or None, dparams: list of tensors (the parameters' gradients; must be absent or zero) or None.
    The loss per channel on its own value, dquantiles per channel on the channel's largest."""
    out = {"aux loss": (_worst((got["loss"].double() - ref["loss"]).abs() / ref["loss"].clamp(min=1e-300)), BARS["aux"])}
    if got.get("dq") is not None:
        scale = ref["dq"].abs().max(1, keepdim=True).values.clamp(min=1e-300)
        out["dquantiles"] = (_worst((got["dq"].double() - ref["dq"]).abs() / scale), BARS["dq"])
    if got.get("dparams") is not None:
        out["aux parameter gradients"] = (float(sum(int((g != 0).sum()) for g in got["dparams"])), 0.0)
    return out


def ratio(figure, bar):
    """how many times over its bar (an exact property violated: infinitely)"""
    if bar == 0.0:
        return float("inf") if figure > 0 else 0.0
    return figure / bar


def failures(figures):
    return {k: v for k, v in figures.items() if not v[0] <= v[1]}
