"""Float64 statements of the operations in csrc/elementwise.hip, and the error bounds their float32 kernels are held to.

Plain torch on the CPU; nothing here imports the package under test.  Every `*_ref` takes float64 tensors (the kernels' float32
operands promoted) and returns float64.  Matrices are [rows, C]; maps are pixel-major [N, H, W, C].

Bounds (u = 2^-24, TINY = 2^-126: below the smallest normal float32 a result may be flushed or lose its last bits):
  elementwise   k u S + TINY      S = the expression's terms in absolute values, k = its roundings + 2
  sums          (n + k) u S + TINY
  LayerNorm     the sum form with n = C, times cond = 1 + |mean| / std of the row (two-pass variance in float32)
Each bound function names the kernel line whose roundings it counts.  A kernel that calls a libm function is held to
BUDGET[name] times its bound instead: 8 x the worst error, in units of the bound, of the same formula evaluated in float32 torch on the
CPU on the test's inputs (measured by test_elementwise_ref_cpu.py, which fails when a budget is no longer 8 x its measurement).
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126
F32, F64 = torch.float32, torch.float64

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_GELU, ACT_HALFTANH, ACT_SIGMOID, ACT_SAVED_DERIV = 0, 1, 2, 3, 4, 5, 6
LN_EPS = 1e-5

# 8 x the measured float32-CPU error / bound (see the docstring of test_elementwise_kernels_gpu.py for the measurements)
BUDGET = {
    "ln_y": 0.86,          # rsqrtf
    "ln_rstd": 1.17,       # rsqrtf
    "log2": 2.62,          # log2f, per term (3 u |log2 x|): the sums that call it carry 3 BUDGET["log2"] more roundings, see sum_log2_ref
    "halftanh_pre": 1.98,  # tanhf
    "gelu": 3.66,          # exp2 / rcp and the Abramowitz-Stegun erf
    "gate_fwd": 2.31,      # expf
    "gate_da": 2.81,       # expf
    "gate_db": 2.26,       # expf
}


def rand(seed, *shape, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=F32) * scale + shift).to(F32)


def uniform(seed, *shape, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=F32) * (hi - lo) + lo).to(F32)


def round32(t):
    return t.to(F32).to(F64)


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def _affine(rows, p1, p2, half_rows):
    """per-row parameters of a paired launch: rows >= half_rows use the second module's"""
    if p2 is None:
        return p1[None, :].expand(rows, -1)
    sec = (torch.arange(rows) >= half_rows)[:, None]
    return torch.where(sec, p2[None, :], p1[None, :])


def ln_stats(x):
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    rs = 1.0 / torch.sqrt(var + LN_EPS)
    return mu, rs


def ln_cond(x):
    """1 + |mean| / std per row, std = sqrt(var + eps)"""
    mu, rs = ln_stats(x)
    return 1.0 + mu.abs() * rs


def ln_fwd_ref(x, gamma, beta, gamma2=None, beta2=None, half_rows=0):
    """-> y, mean, rstd and their bounds.
    layernorm_fwd_vec_kernel: mu = sum / C (C - 1 adds, 1 division); d = v - mu (1); rs = rsqrtf(sum(d d) / C + eps) (C adds and products
    at half weight, division, add, rsqrtf); y = d rs gm + bt (3).  Per element: the error of mu reaches y as (C + 1) u cond |gm|, the error
    of rs and the last roundings as (C / 2 + 8) u |xhat gm|, the final add as u |bt|: (C + 8) u cond (|xhat gm| + |gm| + |bt|)."""
    rows, C = x.shape
    gm, bt = _affine(rows, gamma, gamma2, half_rows), _affine(rows, beta, beta2, half_rows)
    mu, rs = ln_stats(x)
    xh = (x - mu[:, None]) * rs[:, None]
    y = xh * gm + bt
    cond = ln_cond(x)
    by = (C + 8) * U * cond[:, None] * ((xh * gm).abs() + gm.abs() + bt.abs()) + TINY
    bmean = (C + 1) * U * x.abs().mean(1) + TINY                    # mu = group_sum(...) / C
    brstd = (C / 2 + 6) * U * rs * cond + TINY                      # rs = rsqrtf(group_sum(d d) / C + eps)
    return {"y": y, "mean": mu, "rstd": rs, "by": by, "bmean": bmean, "brstd": brstd}


def ln_bwd_ref(x, gamma, dy, dadd=None, gamma2=None, half_rows=0, mean=None, rstd=None):
    """-> dx, [dgamma, dbeta] per module, and bounds; mean / rstd: the (float32-rounded) statistics the kernel is handed.
    layernorm_bwd_vec_kernel: xh = (xv - mu) rs (2, and the rounding of the mu / rs it is handed: 3 u cond (|xh| + 1) in all);
    g = d gm (1); s1, s2 = sums / C (C + 2 each); o = rs (g - s1 - xh s2) (+ dadd) (5).  With M2 = mean_c |g| (|xh| + 1):
    S = rs (|g| + mean|g| + (|xh| + 1) M2) + |dadd| and the bound is (C + 10) u cond S.
    dgamma = sum_r d xh over R rows in any order: (R + 6) u sum_r |d| (|xh| + 1) cond_r;  dbeta = sum_r d: (R + 2) u sum_r |d|."""
    rows, C = x.shape
    mu, rs = ln_stats(x)
    cond = ln_cond(x)
    gm = _affine(rows, gamma, gamma2, half_rows)
    xh = (x - mu[:, None]) * rs[:, None]
    g = dy * gm
    s1, s2 = g.mean(1), (g * xh).mean(1)
    dx = rs[:, None] * (g - s1[:, None] - xh * s2[:, None])
    M2 = (g.abs() * (xh.abs() + 1)).mean(1)
    S = rs[:, None] * (g.abs() + g.abs().mean(1)[:, None] + (xh.abs() + 1) * M2[:, None])
    if dadd is not None:
        dx = dx + dadd
        S = S + dadd.abs()
    out = {"dx": dx, "bdx": (C + 10) * U * cond[:, None] * S + TINY, "params": []}
    halves = [(0, rows)] if gamma2 is None else [(0, half_rows), (half_rows, rows)]
    for a, b in halves:
        R = b - a
        dg, db = (dy[a:b] * xh[a:b]).sum(0), dy[a:b].sum(0)
        Sg = (dy[a:b].abs() * (xh[a:b].abs() + 1) * cond[a:b, None]).sum(0)
        Sb = dy[a:b].abs().sum(0)
        out["params"].append({"dgamma": dg, "dbeta": db, "Sg": Sg, "Sb": Sb, "R": R})
    return out


def ln_param_bound(p, which, init=None):
    """bound of an accumulated parameter gradient: init + sum (one more rounding, |init| one more term)"""
    S, k = (p["Sg"], 6) if which == "dgamma" else (p["Sb"], 2)
    if init is not None:
        S, k = S + init.abs(), k + 1
    return (p["R"] + k) * U * S + TINY


def partial_reduce_ref(partial, init=None):
    """partial [nblocks, n] -> out [n] (+ init) and its bound.  partial_reduce_batched_kernel: nblocks - 1 adds in a fixed tree, 1 for the init."""
    nb = partial.shape[0]
    out, S = partial.sum(0), partial.abs().sum(0)
    if init is not None:
        out, S = out + init, S + init.abs()
    return out, (nb + 2) * U * S + TINY


# ------------------------------------------------------------------------------------------------------------------- activations
SLOPE32 = float(torch.tensor(0.01, dtype=F32).double())   # the kernel's 0.01f


def gelu_parts_ref(s):
    cdf = 0.5 * (1.0 + torch.erf(s / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * s * s) / math.sqrt(2.0 * math.pi)
    return cdf, pdf


def act_deriv_ref(s, act, use_pre):
    """d act(v) / dv from the saved tensor (v when use_pre, else the output), and S: its expression's terms in absolute values"""
    one = torch.ones_like(s)
    if act == ACT_LRELU:
        d = torch.where(s > 0, one, one * SLOPE32)
        return d, d
    if act == ACT_RELU:
        d = torch.where(s > 0, one, 0 * one)
        return d, d
    if act == ACT_GELU:
        assert use_pre
        cdf, pdf = gelu_parts_ref(s)
        erf_abs = torch.erf(s.abs() / math.sqrt(2.0))
        return cdf + s * pdf, 0.5 + 0.5 * erf_abs + (s * pdf).abs()     # cdf = 0.5 + copysign(0.5 erf_abs, x);  cdf + x pdf
    if act == ACT_HALFTANH:
        t = torch.tanh(s) if use_pre else 2.0 * s
        return 0.5 * (1.0 - t * t), 0.5 * (1.0 + t * t)                 # 0.5f * (1.f - t * t)
    if act == ACT_SAVED_DERIV:
        return s, s.abs()
    assert act == ACT_NONE
    return one, one


def act_exact(act, use_pre, has_saved=True):
    """g * d is ONE IEEE multiply by an exactly known d: bit-equal to the float64 product rounded to float32"""
    return (not has_saved) or act in (ACT_NONE, ACT_LRELU, ACT_RELU, ACT_SAVED_DERIV)


def act_budget(act, use_pre):
    if act == ACT_GELU:
        return BUDGET["gelu"]
    if act == ACT_HALFTANH and use_pre:
        return BUDGET["halftanh_pre"]
    return 1.0


def act_bwd_ref(dy, saved, act, use_pre):
    """dz = dy act'(saved) and its bound.  act_bwd_kernel `dz = g * d`: HALFTANH tanhf, t t, 1 - ., 0.5 ., g d: k = 4 + 2;
    GELU (gelu_parts: 14 operations, + cdf + x pdf, + g d): k = 17 + 2."""
    d, S = act_deriv_ref(saved, act, use_pre)
    k = {ACT_GELU: 19, ACT_HALFTANH: 6}.get(act, 3)
    return dy * d, k * U * dy.abs() * S + TINY


def unshuffle_ref(t):
    """[N, 2H, 2W, Q] -> [N, H, W, 4Q] with dz[.., 4q + r] = t[n, 2h + (r >> 1), 2w + (r & 1), q]"""
    N, H2, W2, Q = t.shape
    H, W = H2 // 2, W2 // 2
    out = torch.empty(N, H, W, 4 * Q, dtype=t.dtype)
    for r in range(4):
        out[..., r::4] = t[:, (r >> 1)::2, (r & 1)::2, :]
    return out


# float32 evaluations of the libm formulas (the kernels' expressions, operation for operation, in float32 torch on the CPU)
def halftanh_pre_f32(dy, s):
    t = torch.tanh(s)
    return dy * (0.5 * (1.0 - t * t))


def gelu_grad_f32(dy, x):
    """common.h gelu_parts / gelu_grad_f"""
    z = x.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * z + 1.0)
    eh = torch.exp2(-0.72134752044448170368 * x * x)
    poly = t * (t * (t * (t * (t * 1.061405429 + -1.453152027) + 1.421413741) + -0.284496736) + 0.254829592)
    erf_abs = 1.0 - poly * eh
    cdf = 0.5 + torch.copysign(0.5 * erf_abs, x)
    pdf = 0.39894228040143267794 * eh
    return dy * (cdf + x * pdf)


# ------------------------------------------------------------------------------------------------------------------- gate / axpby
def gate_fwd_ref(a, b, idn):
    """gate_fwd_kernel `a * sigmoidf_(b) + idn`: expf, 1 +, 1 /, a *, + idn: k = 5 + 2"""
    s = torch.sigmoid(b)
    return a * s + idn, 7 * U * ((a * s).abs() + idn.abs()) + TINY


def gate_bwd_ref(g, a, b):
    """gate_bwd_kernel: da = g s (k = 4 + 2); db = g a s (1 - s): 3 for s, 1 - s, three products: k = 7 + 2, the terms of (1 - s) are 1 and s"""
    s = torch.sigmoid(b)
    return g * s, 6 * U * (g * s).abs() + TINY, g * a * s * (1 - s), 9 * U * (g * a * s).abs() * (1 + s) + TINY


def gate_fwd_f32(a, b, idn):
    return a * (1.0 / (1.0 + torch.exp(-b))) + idn


def gate_bwd_f32(g, a, b):
    s = 1.0 / (1.0 + torch.exp(-b))
    return g * s, g * a * s * (1.0 - s)


def axpby_ref(a, alpha, b, beta):
    """axpby_kernel `alpha * a[i] + (b ? beta * b[i] : 0.f)`: k = 3 + 2"""
    out, S = alpha * a, (alpha * a).abs()
    if b is not None:
        out, S = out + beta * b, S + (beta * b).abs()
    return out, 5 * U * S + TINY


def sum_n_f32(srcs):
    """sum_n_kernel: ((s0 + s1) + s2) + ... in float32, which torch's float32 add on the CPU reproduces bit for bit"""
    acc = srcs[0].clone()
    for s in srcs[1:]:
        acc = acc + s
    return acc


# ------------------------------------------------------------------------------------------------------------------- column sums
def colsum_terms(rows):
    """adds on the path of one column: colsum_partial_kernel's rows per block, colsum_final_kernel's blocks, the accumulate"""
    nb = max(1, min(512, (rows + 255) // 256))
    return (rows + nb - 1) // nb + nb + 1


def colsum_ref(x, init=None):
    out, S = x.sum(0), x.abs().sum(0)
    if init is not None:
        out, S = out + init, S + init.abs()
    return out, colsum_terms(x.shape[0]) * U * S + TINY


# ------------------------------------------------------------------------------------------------------------------- loss path
def log2_term_ref(x):
    """one term `log2f(x)`: k = 1 + 2.  The libm budget is measured on the TERM: the error of a float32 sum of thousands of terms against
    its worst-case bound is a matter of cancellation, not of log2f, and 8 x a lucky sample would be no bound at all."""
    t = torch.log2(x)
    return t, 3 * U * t.abs() + TINY


LOG2_K = 3 * BUDGET["log2"]   # roundings a device log2f term may carry: BUDGET["log2"] x 3 u |term|


def sum_log2_ref(x):
    """log2_sum_partials_kernel + sum_partials_kernel: n - 1 adds in any order, each term within its log2f budget: (n + LOG2_K) u sum |log2 x|"""
    t = torch.log2(x)
    return t.sum(), (x.numel() + LOG2_K) * U * t.abs().sum() + TINY


def sqdiff_sum_ref(a, b):
    """sqdiff_partials_kernel `d = a - b; s += d * d`: (n + 3) u sum d d"""
    d2 = (a - b) ** 2
    return d2.sum(), (a.numel() + 3) * U * d2.sum() + TINY


def rd_loss_ref(lik_y, lik_z, x_hat, target, lmbda, num_pixels):
    """The reference's RateDistortionLoss (MSE form) as rd_combine_kernel states it:
    bpp = (sum log2 lik_y + sum log2 lik_z) / (-num_pixels); mse = mean (x_hat - x)^2; loss = float32(lmbda 255^2) mse + bpp"""
    c = float(torch.tensor(lmbda * 255 ** 2, dtype=F32).double())
    bpp = (torch.log2(lik_y).sum() + torch.log2(lik_z).sum()) / (-num_pixels)
    mse = ((x_hat - target) ** 2).mean()
    return bpp, mse, c * mse + bpp


def rd_loss_bounds(lik_y, lik_z, x_hat, target, lmbda, num_pixels):
    """bpp: the two log2 sums, their add and the division: ((n_y + LOG2_K + 2) u S_y + (n_z + LOG2_K + 2) u S_z) / P;  mse: (n + 4) u mse;
    loss = c m + b: 2 more roundings on the sum of the terms"""
    c = float(torch.tensor(lmbda * 255 ** 2, dtype=F32).double())
    Sy, Sz = torch.log2(lik_y).abs().sum(), torch.log2(lik_z).abs().sum()
    bb = ((lik_y.numel() + LOG2_K + 2) * Sy + (lik_z.numel() + LOG2_K + 2) * Sz) * U / num_pixels + TINY
    mse = ((x_hat - target) ** 2).mean()
    bm = (x_hat.numel() + 4) * U * mse + TINY
    bl = c * bm + bb + 2 * U * (c * mse + (Sy + Sz) / num_pixels) + TINY
    return bb, bm, bl


INV_LN2_32 = float(torch.tensor(1.0 / math.log(2.0), dtype=F32).double())   # the float argument clc_scaled_recip receives


def rd_grads_ref(lik_y, lik_z, x_hat, target, lmbda, num_pixels, g_bpp, g_mse, g_loss):
    """Gradients of g_bpp bpp + g_mse mse + g_loss loss (None: no gradient for that output) and their bounds.
    rd_grad_scalars_kernel: gb = gl + g_bpp (1), / -P (1); gm = gl c (1) + g_mse (1), / numel (1).
    scaled_recip_kernel `k / x`, k = g coef (1): 2 + 2 + 2;  scaled_diff_kernel `k * (a - b)`, k = 2 g_sq: 3 + 2 + 2."""
    c = float(torch.tensor(lmbda * 255 ** 2, dtype=F32).double())
    gl = 0.0 if g_loss is None else g_loss
    gb, Sb = gl + (g_bpp or 0.0), abs(gl) + abs(g_bpp or 0.0)
    gm, Sm = gl * c + (g_mse or 0.0), abs(gl * c) + abs(g_mse or 0.0)
    n = x_hat.numel()
    out = {}
    for name, lik in (("dy", lik_y), ("dz", lik_z)):
        out[name] = gb / (-num_pixels) * INV_LN2_32 / lik
        out["b" + name] = 6 * U * Sb / num_pixels * INV_LN2_32 / lik + TINY
    out["dx"] = gm / n * 2.0 * (x_hat - target)
    out["bdx"] = 7 * U * Sm / n * 2.0 * (x_hat - target).abs() + TINY
    return out


def scaled_recip_ref(x, g, coef):
    """scaled_recip_kernel `k / x`, k = g coef: k = 2 + 2"""
    return g * coef / x, 4 * U * (g * coef / x).abs() + TINY


def scaled_diff_ref(a, b, g, coef):
    """scaled_diff_kernel `k * (a - b)`: k = 3 + 2"""
    return g * coef * (a - b), 5 * U * (g * coef * (a - b)).abs() + TINY


# ------------------------------------------------------------------------------------------------------------------- GDN parameters
def gdn_reparam_fwd_ref(gamma, beta, gbound, bbound, ped):
    """gdn_reparam_fwd_kernel `t = fmaxf(x, bound); y = t * t - ped`: k = 2 + 2, S = t t + ped.  -> (g_eff, g_eff_t, b_eff), bounds"""
    tg, tb = torch.clamp(gamma, min=gbound), torch.clamp(beta, min=bbound)
    ge, be = tg * tg - ped, tb * tb - ped
    return (ge, ge.t().contiguous(), be), (4 * U * (tg * tg + ped) + TINY, 4 * U * (tb * tb + ped) + TINY)


def gdn_reparam_bwd_ref(x, bound, dy, init=None):
    """gdn_reparam_bwd_kernel: dt = 2 max(x, bound) dy; dx = (x >= bound || dt < 0) ? dt : 0; out = init + dx.
    k: the product (2 . is exact) and the accumulate: 2 + 2.  -> out, bound, pass mask"""
    dt = 2.0 * torch.clamp(x, min=bound) * dy
    keep = (x >= bound) | (dt < 0)
    dx = torch.where(keep, dt, torch.zeros_like(dt))
    S = dx.abs()
    if init is not None:
        dx, S = dx + init, S + init.abs()
    return dx, 4 * U * S + TINY, keep


# ------------------------------------------------------------------------------------------------------------------- RGB stem
def stem_pack_ref(w3, w1x1):
    """w3 [co, cin, 3, 3], w1x1 [co, cin, 1, 1] -> w1 [co, 32] (the [kh][kw][c] patch order, zero from 9 cin), ws [co, 32] (centre tap)"""
    co, cin = w3.shape[:2]
    w1, ws = torch.zeros(co, 32, dtype=w3.dtype), torch.zeros(co, 32, dtype=w3.dtype)
    for kh in range(3):
        for kw in range(3):
            for c in range(cin):
                w1[:, (kh * 3 + kw) * cin + c] = w3[:, c, kh, kw]
    for c in range(cin):
        ws[:, 4 * cin + c] = w1x1[:, c, 0, 0]
    return w1, ws


def stem_unpack_ref(dw1, dws, cin):
    """the transpose of stem_pack_ref: (d w3 [co, cin, 3, 3], d w1x1 [co, cin, 1, 1])"""
    co = dw1.shape[0]
    g3, g1 = torch.zeros(co, cin, 3, 3, dtype=dw1.dtype), torch.zeros(co, cin, 1, 1, dtype=dw1.dtype)
    for kh in range(3):
        for kw in range(3):
            for c in range(cin):
                g3[:, c, kh, kw] = dw1[:, (kh * 3 + kw) * cin + c]
    for c in range(cin):
        g1[:, c, 0, 0] = dws[:, 4 * cin + c]
    return g3, g1


def out_size(H, ks, stride, pad):
    """PyTorch's output size; None where the window does not fit the padded map (F.max_pool2d / F.unfold refuse)"""
    if H + 2 * pad < ks:
        return None
    return (H + 2 * pad - ks) // stride + 1


def im2col_ref(x, ks, stride, pad, ldc):
    """x [N, H, W, C] -> col [N OH OW, ldc]: col[m][(kh ks + kw) C + c] = x[n, oh s - pad + kh, ow s - pad + kw, c], zero outside / from ks ks C"""
    N, H, W, C = x.shape
    OH, OW = out_size(H, ks, stride, pad), out_size(W, ks, stride, pad)
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    col = torch.zeros(N, OH, OW, ldc, dtype=x.dtype)
    for kh in range(ks):
        for kw in range(ks):
            k0 = (kh * ks + kw) * C
            col[..., k0:k0 + C] = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
    return col.reshape(N * OH * OW, ldc)


# ------------------------------------------------------------------------------------------------------------------- pooling
def maxpool_ref(x, ks, stride, pad):
    """x [N, H, W, C] -> [N, OH, OW, C], padding = -inf"""
    N, H, W, C = x.shape
    OH, OW = out_size(H, ks, stride, pad), out_size(W, ks, stride, pad)
    xp = torch.full((N, H + 2 * pad, W + 2 * pad, C), -math.inf, dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = torch.full((N, OH, OW, C), -math.inf, dtype=x.dtype)
    for kh in range(ks):
        for kw in range(ks):
            out = torch.maximum(out, xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride])
    return out


def adaptive_pool_ref(x, L, is_max):
    """x [N, H, W, C] -> out [N, C, L, L] and its bound: bin i covers floor(i H / L) .. ceil((i + 1) H / L) - 1.
    adaptive_pool_kernel `acc + v` over the bin's m values, `acc / m`: (m + 2) u mean |v| (max: exact)"""
    N, H, W, C = x.shape
    out, bound = torch.empty(N, C, L, L, dtype=x.dtype), torch.zeros(N, C, L, L, dtype=x.dtype)
    for i in range(L):
        y0, y1 = (i * H) // L, -((-(i + 1) * H) // L)
        for j in range(L):
            x0, x1 = (j * W) // L, -((-(j + 1) * W) // L)
            win = x[:, y0:y1, x0:x1, :].reshape(N, -1, C)
            m = win.shape[1]
            if is_max:
                out[:, :, i, j] = win.max(1).values
            else:
                out[:, :, i, j] = win.mean(1)
                bound[:, :, i, j] = (m + 2) * U * win.abs().mean(1) + TINY
    return out, bound


# ------------------------------------------------------------------------------------------------------------------- comparison
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all elements (got: float32 from the device, on the CPU)"""
    g = got.to(F64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    assert not torch.isnan(g).any(), "NaN in the result"
    return float(((g - ref).abs() / bound).max())


def bits_equal(got, ref64):
    """got (float32) equals ref64 rounded to float32, bit for bit (so +0 and -0 differ)"""
    want = ref64.to(F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- shared case inputs
# The GPU cases and the CPU measurement of the libm budgets draw their operands from the same seeded builders.
LN_VEC_C = (64, 128, 256)
LN_FALLBACK_C = (3, 48, 96, 192, 320, 512)
LN_FWD_SHAPES = ([(64, r) for r in (1, 15, 17, 35, 2048 * 16 + 7)] + [(128, r) for r in (1, 9, 35, 2048 * 8 + 5)] +
                 [(256, r) for r in (1, 5, 35, 2048 * 4 + 3)] + [(C, r) for C in LN_FALLBACK_C for r in (1, 5, 35)] + [(192, 2048 * 4 + 3)])
LN_BWD_SHAPES = [(C, r) for C in LN_VEC_C + LN_FALLBACK_C for r in (1, 15, 35, 8192 + 19)]


def ln_inputs(C, rows):
    """x with a mean and a spread of its own per row (|mean| / std up to ~6), affine parameters, upstream and residual gradients"""
    seed = 7919 * C + rows
    shift, scale = uniform(seed + 1, rows, 1, lo=-3.0, hi=3.0), uniform(seed + 2, rows, 1, lo=0.5, hi=2.0)
    x = (rand(seed, rows, C) * scale + shift).to(F32)
    return {"x": x, "gamma": rand(seed + 3, C, scale=0.3, shift=1.0), "beta": rand(seed + 4, C, scale=0.2),
            "gamma2": rand(seed + 5, C, scale=0.3, shift=-1.0), "beta2": rand(seed + 6, C, scale=0.2),
            "dy": rand(seed + 7, rows, C), "dadd": rand(seed + 8, rows, C)}


def ln_fwd_f32(x, gamma, beta):
    """layernorm_fwd_kernel's expression in float32 torch"""
    C = x.shape[1]
    mu = x.sum(1, keepdim=True) / C
    d = x - mu
    rs = torch.rsqrt((d * d).sum(1, keepdim=True) / C + 1e-5)
    return d * rs * gamma + beta, mu[:, 0], rs[:, 0]


ACT_SHAPES = [(1, 1), (35, 3), (35, 22), (1025, 64)]
ACT_SPECIALS = (0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0)
UNSHUFFLE_SHAPES = [(2, 3, 5, 8), (1, 1, 1, 4), (1, 7, 2, 20)]   # N, H, W, C of dz
# (activation, use_pre) pairs clc_act_bwd accepts
ACT_MODES = [(ACT_NONE, 0), (ACT_NONE, 1), (ACT_LRELU, 0), (ACT_LRELU, 1), (ACT_RELU, 0), (ACT_RELU, 1), (ACT_GELU, 1),
             (ACT_HALFTANH, 0), (ACT_HALFTANH, 1), (ACT_SAVED_DERIV, 0), (ACT_SAVED_DERIV, 1)]


def act_inputs(rows, C, seed_base=0):
    seed = seed_base + 104729 + 31 * rows + C
    dy, saved = rand(seed, rows, C), rand(seed + 1, rows, C, scale=1.5)
    flat = saved.view(-1)
    k = min(flat.numel(), len(ACT_SPECIALS))
    flat[flat.numel() - k:] = torch.tensor(ACT_SPECIALS[:k], dtype=F32)
    return dy, saved


GATE_N = (1, 1023)


def gate_inputs(n):
    a, b, idn, g = rand(500 + n, n), rand(501 + n, n, scale=3.0), rand(502 + n, n), rand(503 + n, n)
    b[0] = 100.0
    b[-1] = -100.0 if n > 1 else 100.0
    return a, b, idn, g


def gate_inputs_neg():
    """n = 1 with b = -100"""
    a, b, idn, g = gate_inputs(1)
    return a, -b, idn, g


LIK_SHAPES = {"small": (1, 3, 5, 7), "wide": (2, 192, 4, 4)}   # N, C, H, W
IMG_SHAPE = (1, 3, 17, 19)


def lik_inputs(name):
    """likelihoods in [1e-9, 1] as [N, H, W, C], log-uniform so that the small end is populated; the ends planted"""
    N, C, H, W = LIK_SHAPES[name]
    e = uniform(900 + C, N, H, W, C, lo=-9.0, hi=0.0)
    lik = torch.clamp(torch.pow(torch.tensor(10.0, dtype=F32), e), 1e-9, 1.0).to(F32)
    lik.view(-1)[0], lik.view(-1)[-1] = 1e-9, 1.0
    return lik


def img_inputs():
    N, C, H, W = IMG_SHAPE
    return uniform(950, N, H, W, C), uniform(951, N, H, W, C)


GDN_C = (3, 64, 192)
# (where the parameter sits, sign of its upstream gradient): exactly at the bound, one float32 below it, far below it
_GDN_PLANT = [("at", 1), ("below", 1), ("below", -1), ("far", 1), ("far", -1), ("at", -1), ("at", 0), ("below", 0), ("far", 0)]


def _plant(v, dy, bound):
    b32 = torch.tensor(bound, dtype=F32)
    vals = {"at": b32, "below": torch.nextafter(b32, torch.tensor(0.0, dtype=F32)), "far": torch.tensor(-1.0, dtype=F32)}
    fv, fd = v.view(-1), dy.view(-1)
    for j, (where, sign) in enumerate(_GDN_PLANT[: fv.numel()]):
        fv[j] = vals[where]
        fd[j] = sign * (0.5 + j)


def gdn_inputs(C, gbound, bbound):
    """raw gamma [C, C], beta [C] and upstream gradients of both signs, with the LowerBound edge entries planted"""
    gamma, beta = rand(1300 + C, C, C, scale=0.05), rand(1301 + C, C, scale=0.1, shift=1.0)
    dge, dbe = rand(1302 + C, C, C), rand(1303 + C, C)
    _plant(gamma, dge, gbound)
    _plant(beta, dbe, bbound)
    return gamma, beta, dge, dbe


def ln_bwd_carried(x, gamma, dy):
    """When the backward runs on the FORWARD KERNEL's statistics (ops.layernorm) these differ from the exact ones by up to bmean and
    BUDGET["ln_rstd"] brstd; to first order that reaches xh as dxh = bmean rs + |xh| e (e: the relative error of rs), and from there
        dx      rs (|xh| mean_c(|g| dxh) + dxh |s2|) + 3 e rs (|g| + |s1| + |xh s2|)     (rs enters dx up to three times)
        dgamma  sum_r |dy| dxh
    -> what to add to the bounds of ln_bwd_ref for dx and dgamma (dbeta does not see the statistics)"""
    f = ln_fwd_ref(x, gamma, torch.zeros_like(gamma))
    mu, rs = f["mean"], f["rstd"]
    e = (BUDGET["ln_rstd"] * f["brstd"] / rs)[:, None]
    xh = (x - mu[:, None]) * rs[:, None]
    dxh = (f["bmean"] * rs)[:, None] + xh.abs() * e
    g = dy * gamma
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    cdx = rs[:, None] * (xh.abs() * (g.abs() * dxh).mean(1, keepdim=True) + dxh * s2.abs()) + 3 * e * rs[:, None] * (g.abs() + s1.abs() + (xh * s2).abs())
    return cdx, (dy.abs() * dxh).sum(0)


IM2COL_CASES = [(7, 2, 3, 3, 148), (3, 2, 1, 3, 32), (3, 1, 1, 1, 12)]   # ks, stride, pad, C, ldc
POOL_CASES = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]                            # ks, stride, pad
ADAPTIVE_CASES = [(7, 7, 1), (7, 7, 2), (7, 7, 4), (8, 10, 4), (5, 3, 3), (9, 6, 4), (4, 4, 4)]   # H, W, L
