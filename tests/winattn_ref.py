"""Float64 statement of the window-attention contract of csrc/winattn.hip, its first-order error bounds, a float32 restatement and mutants.

Plain torch on the CPU; nothing here imports the package under test.  Written from the header of csrc/winattn.hip and the reference
model's WMSA.forward (the einsum / softmax / roll / mask / relative-embedding chain); index arithmetic only, no torch.roll.

Layout.  A map is [B * H * W, ld] NHWC rows: qkv has 3C columns (channel = which * C + head * hd + c), out / dout have C, dqkv 3C, lse is
[B * H * W][heads].  Window `w` = (b, wy, wx) in that order; its token t = (ty, tx) is the pixel
    y = (wy * ws + ty + shift * ws / 2) mod H,  x = (wx * ws + tx + shift * ws / 2) mod W
of image b.  With i the query and j the key token of a (window, head),
    s[i][j]   = (q_i * hd^-1/2) . k_j + relbias[head][iy - jy + ws - 1][ix - jx + ws - 1]
    masked    <=> shift and ( (wy == last and (iy < g) != (jy < g)) or (wx == last and (ix < g) != (jx < g)) ),  g = ws - ws / 2
    p = softmax_j(s),  lse_i = log sum_j exp s[i][j],  O = p V
    backward as the kernels do it: P = exp(s - lse), dP = dO V^T, D_i = dO_i . O_i, dS = P o (dP - D), dQ = hd^-1/2 dS K,
    dK = dS^T (q hd^-1/2), dV = P^T dO, drelbias[head][bin] = sum of dS over the windows and the (i, j) of that bin.
The paired form uses the second table from window windows_total / 2 on and returns a drelbias per table.

Bounds (u = 2^-24, T = ws^2, E = 4 roundings for exp2 / log, masked entries contribute 0; |a|.|b| is the dot product of the absolute values).
Each is the first-order propagation of one rounding per float32 operation through the graph above.  A rounding is relative, u |x|, only
while x is a normal number: the matrix instructions and the hardware exp2 return 0 for a result below TINY = 2^-126, an ABSOLUTE error of
up to TINY per operation.  So a probability and a dS carry + TINY each (written "+ t" below), and a sum of n products + (n + 1) TINY: the
relative-bias bins of a peaked softmax are sums of a dozen terms of 1e-38, where the n flushes, not u, are the whole error:
    ds    = (hd + 2) u hd^-1/2 |q|.|k| + u |bias|
            q * scale rounds once, the hd products are exact inside FMAs / MFMAs and their sum rounds hd times: (hd + 1) u on the dot
            product; the bias is an exact operand of ONE addition, whose rounding is u |s| <= u (|q.k| + |bias|) — so |bias|
            carries the factor 1, not hd + 2: with a bias of +-100 the looser form would hide an error of a thousand u.
    eps   = ds + sum_j p ds + (2 |s - m| + T + E) u                 relative error of p[i][j]:
            exp(s - m) moves by ds (the numerator's argument) and by the p-weighted mean of ds (the denominator); s - m rounds once and
            its product with log2(e) once more: 2 |s - m| u; the row sum takes T roundings, exp2 / reciprocal / multiply E.
            The backward's exp(s - lse) has the same form with lse for m + log l.
    dp    = p eps + t
    dO    = dp |V| + (T + 1) u p |V|                                 T products summed, one rounding for the store path's multiply
    dlse  = sum_j p ds + (|lse| + T + E) u                           log of a sum with relative error sum p ds + T u, then m + log l rounds
    ddP   = (hd + 1) u |dO| |V|^T
    dD    = |dO| . dO_bound + (hd + 1) u sum |dO o O|                the backward reads the forward's float32 O
    ddS   = dp |dP - D| + p (ddP + dD) + 2 u |dS| + t                one subtraction, one product
    ddQ   = hd^-1/2 (ddS |K| + (T + 2) u |dS| |K|)                   T products summed, the scale, the store
    ddK   = ddS^T |q| hd^-1/2 + (T + 2) u |dS|^T |q| hd^-1/2
    ddV   = dp^T |dO| + (T + 1) u p^T |dO|
    ddrelbias = sum ddS + (n + 1) (u sum |dS| + TINY) (+ u |pre| when accumulating), n = the number of (window, i, j) terms of the bin
    (dO, dQ, dK, dV, ddP, dD: + (terms + 1) TINY likewise)
A kernel is held to BUDGET[regime][kind] times its bound: 8 x the worst error / bound of the float32 restatement below on the small cases
(test_winattn_ref_cpu.py measures and asserts them; the table is in the docstring of test_winattn_kernels_gpu.py).
"""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
E_LIBM = 4
F32, F64 = torch.float32, torch.float64
LOG2E_F32 = torch.tensor(1.44269504088896340736, dtype=F32)

KINDS = ("O", "lse", "dQ", "dK", "dV", "drelbias")
REGIMES = ("mild", "peaked", "offset", "hostile", "exact")
MUTANTS = ("mask_first", "mask_swapped", "roll_reversed", "bias_transposed", "bias_negated", "scale_1_over_hd", "d_dropped",
           "surplus_slot_added", "last_window_missing", "pair_first_table", "max_after_zero_mask", "mantissa10")
GEOMETRIC = ("mask_first", "mask_swapped", "roll_reversed")   # visible in the exact regime too (bias = 0 there hides the two bias mutants)

# (name, C, heads, ws, H, W, B): the small cases of test_winattn_kernels_gpu.py (its docstring says which kernel each means)
SMALL_CASES = [
    ("ws8-c32h4-b1", 32, 4, 8, 16, 24, 1), ("ws8-c32h4-b3", 32, 4, 8, 16, 24, 3),
    ("ws8-c16h2-b1", 16, 2, 8, 16, 24, 1),
    ("ws8-c32h2-b1", 32, 2, 8, 16, 24, 1), ("ws8-c32h2-b3", 32, 2, 8, 16, 24, 3),
    ("ws8-c48h3-b1", 48, 3, 8, 24, 16, 1),
    ("ws8-c64h2-b1", 64, 2, 8, 16, 24, 1), ("ws8-c64h2-b3", 64, 2, 8, 16, 24, 3),
    ("ws4-c16h2-b1", 16, 2, 4, 8, 12, 1), ("ws4-c16h2-b3", 16, 2, 4, 12, 12, 3),
    ("ws4-c32h2-b1", 32, 2, 4, 8, 12, 1), ("ws4-c32h2-b3", 32, 2, 4, 12, 12, 3),
    ("ws4-c64h2-b1", 64, 2, 4, 8, 12, 1), ("ws4-c64h2-b3", 64, 2, 4, 12, 12, 3),
]
PAIR_CASES = [("pair-ws8-c32h2-b2", 32, 2, 8, 16, 16, 2), ("pair-ws4-c64h2-b2", 64, 2, 4, 8, 16, 2)]

# 8 x the worst float32-CPU error / bound over SMALL_CASES + PAIR_CASES, W and SW, rounded up to two significant digits.
# EXACT: in the exact regime every float32 operation behind O, dK (= 0: q = 0), dV and drelbias is exact (small multiples of 2^-12), so the
# restatement has no error to take 8 x of; the only difference admitted is the float64 reference's own rounding of exp(-log n) (measured:
# <= 3e-11 of the bound).  O and dV are held bit for bit on top of it.
EXACT = 1e-6
BUDGET = {
    "mild": {"O": 0.54, "lse": 1.3, "dQ": 0.29, "dK": 0.26, "dV": 0.7, "drelbias": 0.18},
    "peaked": {"O": 0.98, "lse": 3.5, "dQ": 0.59, "dK": 0.73, "dV": 1.7, "drelbias": 0.69},
    "offset": {"O": 2.1, "lse": 3.2, "dQ": 1.1, "dK": 1.2, "dV": 3.2, "drelbias": 1.7},
    "hostile": {"O": 0.76, "lse": 2.1, "dQ": 0.31, "dK": 0.31, "dV": 0.75, "drelbias": 0.2},
    "exact": {"O": EXACT, "lse": 0.045, "dQ": 0.036, "dK": EXACT, "dV": EXACT, "drelbias": EXACT},
}


class Geom:
    def __init__(self, C, heads, ws, H, W, B, shift):
        self.C, self.heads, self.ws, self.H, self.W, self.B, self.shift = C, heads, ws, H, W, B, int(bool(shift))
        self.hd, self.T, self.nbw = C // heads, ws * ws, 2 * ws - 1
        self.nb = self.nbw * self.nbw
        self.nwy, self.nwx = H // ws, W // ws
        self.nwin = self.nwy * self.nwx
        self.windows = B * self.nwin
        self.tokens = B * H * W

    def all_windows(self):
        return torch.arange(self.windows)

    def coords(self, widx):
        b, wr = widx // self.nwin, widx % self.nwin
        return b, wr // self.nwx, wr % self.nwx

    def pixels(self, widx, mutant=None):
        """[n, T] row index of every token of the windows `widx` in the un-rolled map"""
        ws = self.ws
        b, wy, wx = self.coords(widx)
        t = torch.arange(self.T)
        y = wy[:, None] * ws + (t // ws)[None, :]
        x = wx[:, None] * ws + (t % ws)[None, :]
        if self.shift:
            sh = -(ws // 2) if mutant == "roll_reversed" else ws // 2
            y, x = (y + sh) % self.H, (x + sh) % self.W
        return (b[:, None] * self.H + y) * self.W + x

    def mask(self, widx, mutant=None):
        """[n, T(query), T(key)] bool"""
        ws, gap = self.ws, self.ws - self.ws // 2
        _, wy, wx = self.coords(widx)
        t = torch.arange(self.T)
        lo_y, lo_x = (t // ws) < gap, (t % ws) < gap
        my, mx = lo_y[:, None] != lo_y[None, :], lo_x[:, None] != lo_x[None, :]
        if mutant == "mask_swapped":
            my, mx = mx, my
        ey = (wy == (0 if mutant == "mask_first" else self.nwy - 1)) & bool(self.shift)
        ex = (wx == (0 if mutant == "mask_first" else self.nwx - 1)) & bool(self.shift)
        return (ey[:, None, None] & my[None]) | (ex[:, None, None] & mx[None])

    def bias_index(self, mutant=None):
        """[T, T] flat bin (iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1) of (query i, key j)"""
        ws = self.ws
        t = torch.arange(self.T)
        dy = (t // ws)[:, None] - (t // ws)[None, :]
        dx = (t % ws)[:, None] - (t % ws)[None, :]
        if mutant == "bias_negated":
            dy, dx = -dy, -dx
        if mutant == "bias_transposed":
            dy, dx = dx, dy
        return (dy + ws - 1) * self.nbw + (dx + ws - 1)

    def side(self, widx, paired):
        """which table a window uses: the paired form's second table from windows / 2 on"""
        return (widx >= self.windows // 2).long() if paired else torch.zeros_like(widx)


def trunc10(t):
    """float32 values cut to a 10-bit mantissa (toward zero)"""
    return (t.to(F32).contiguous().view(torch.int32) & ~0x1FFF).view(F32).to(t.dtype)


def _heads(g, z):
    n = z.shape[0]
    return z.reshape(n, g.T, g.heads, g.hd).permute(0, 2, 1, 3)


def tokens(z):
    """[n, heads, T, hd] -> [n, T, C];  [n, heads, T] -> [n, T, heads]"""
    if z.dim() == 4:
        return z.permute(0, 2, 1, 3).reshape(z.shape[0], z.shape[2], -1)
    return z.permute(0, 2, 1)


def attend(g, qkv, relbias, dout=None, widx=None, relbias2=None, dtype=F64, mutant=None, lse_in=None, out_in=None):
    """The graph on the windows `widx` (default: all), in `dtype`.  float64: the reference.  float32: the restatement (exp as
    exp2(x log2 e), as the kernels have it), optionally with one planted error.  Returns the intermediates per (window, head):
    [n, heads, T, ...].  lse_in / out_in ([tokens, heads] / [tokens, C] maps): the backward reads these instead of its own."""
    widx = g.all_windows() if widx is None else widx
    n, C = widx.numel(), g.C
    pix = g.pixels(widx, mutant)
    rows = qkv[pix.reshape(-1)].reshape(n, g.T, 3 * C).to(dtype)
    q, k, v = (_heads(g, rows[..., i * C:(i + 1) * C]) for i in range(3))
    if mutant == "mantissa10":
        q, k = trunc10(q), trunc10(k)
    scale = torch.tensor(float(g.hd), dtype=dtype).rsqrt()
    if mutant == "scale_1_over_hd":
        scale = scale * scale
    qs = q * scale
    paired = relbias2 is not None
    tables = torch.stack([relbias, relbias if (not paired or mutant == "pair_first_table") else relbias2]).to(dtype).reshape(2, g.heads, g.nb)
    bidx = g.bias_index(mutant)
    bias = tables[g.side(widx, paired)][:, :, bidx]                       # [n, heads, T, T]
    mask = g.mask(widx, mutant)[:, None]
    raw = qs @ k.transpose(-1, -2) + bias
    s = raw.masked_fill(mask, -math.inf)

    def ex(x):
        return torch.exp(x) if dtype == F64 else torch.exp2(x * LOG2E_F32)

    if mutant == "max_after_zero_mask":
        m = (raw * (~mask).to(dtype)).max(-1, keepdim=True).values
        e = torch.where(mask, torch.zeros((), dtype=dtype), ex(raw - m))
    else:
        m = s.max(-1, keepdim=True).values
        e = ex(s - m)
    l = e.sum(-1, keepdim=True)
    p = e * (1.0 / l)
    lse = (m + torch.log(l)).squeeze(-1)
    O = p @ v
    r = {"pix": pix, "q": q, "k": k, "v": v, "qs": qs, "bias": bias, "mask": mask, "s": s, "m": m, "p": p, "lse": lse, "O": O, "scale": float(scale)}
    if dout is None:
        return r
    dO = _heads(g, dout[pix.reshape(-1)].reshape(n, g.T, C).to(dtype))
    lse_b = lse if lse_in is None else lse_in[pix.reshape(-1)].reshape(n, g.T, g.heads).permute(0, 2, 1).to(dtype)
    O_b = O if out_in is None else _heads(g, out_in[pix.reshape(-1)].reshape(n, g.T, C).to(dtype))
    P = ex(s - lse_b[..., None])
    dP = dO @ v.transpose(-1, -2)
    D = (dO * O_b).sum(-1, keepdim=True)
    dS = P * (dP if mutant == "d_dropped" else dP - D)
    r.update(dO=dO, P=P, dP=dP, D=D, dS=dS, dQ=(dS @ k) * scale, dK=dS.transpose(-1, -2) @ qs, dV=P.transpose(-1, -2) @ dO)
    return r


def drelbias(g, dS, widx=None, paired=False, mutant=None, pre=None):
    """[1 or 2, heads, nb]: dS summed over the windows of each table and the (i, j) of each bin; pre: accumulated into"""
    widx = g.all_windows() if widx is None else widx
    side = g.side(widx, paired)
    bidx = g.bias_index().reshape(-1)
    outs = []
    for sd in range(2 if paired else 1):
        sel = side == sd
        if mutant == "last_window_missing":
            sel = sel & (widx != g.windows - 1)
        tot = dS[sel].sum(0)
        G = 64 // g.T
        if mutant == "surplus_slot_added" and sd == 0 and g.windows % G:
            tot = tot + (G - g.windows % G) * dS[0]
        o = torch.zeros(g.heads, g.nb, dtype=dS.dtype).index_add_(1, bidx, tot.reshape(g.heads, -1))
        outs.append(o if pre is None else o + pre[sd].reshape(g.heads, g.nb).to(dS.dtype))
    return torch.stack(outs)


def bounds(g, r, paired=False, widx=None, pre=None):
    """first-order bounds (module docstring) from the float64 intermediates `r`; token layouts as tokens(), drelbias [1 or 2, heads, nb]"""
    u, T, hd, sc = U, g.T, g.hd, r["scale"]
    aq, ak, av = r["q"].abs(), r["k"].abs(), r["v"].abs()
    vis = ~r["mask"]
    p = r["p"]
    ds = ((hd + 2) * u * sc * (aq @ ak.transpose(-1, -2)) + u * r["bias"].abs()) * vis
    pds = (p * ds).sum(-1, keepdim=True)
    sm = torch.where(vis, (r["s"] - r["m"]).abs(), torch.zeros((), dtype=F64))
    eps = ds + pds + (2 * sm + T + E_LIBM) * u
    dp = p * eps + TINY * vis
    bO = dp @ av + (T + 1) * u * (p @ av) + (T + 1) * TINY
    b = {"O": tokens(bO), "lse": tokens(pds.squeeze(-1) + (r["lse"].abs() + T + E_LIBM) * u + TINY)}
    if "dS" not in r:
        return b
    adO, adS = r["dO"].abs(), r["dS"].abs()
    ddP = (hd + 1) * u * (adO @ av.transpose(-1, -2)) + (hd + 1) * TINY
    dD = (adO * bO).sum(-1, keepdim=True) + (hd + 1) * u * (adO * r["O"].abs()).sum(-1, keepdim=True) + (hd + 1) * TINY
    ddS = (dp * (r["dP"] - r["D"]).abs() + p * (ddP + dD) + 2 * u * adS + TINY) * vis
    b["dQ"] = tokens(sc * (ddS @ ak + (T + 2) * u * (adS @ ak)) + (T + 2) * TINY)
    b["dK"] = tokens(sc * (ddS.transpose(-1, -2) @ aq + (T + 2) * u * (adS.transpose(-1, -2) @ aq)) + (T + 2) * TINY)
    b["dV"] = tokens(dp.transpose(-1, -2) @ adO + (T + 1) * u * (p.transpose(-1, -2) @ adO) + (T + 1) * TINY)
    widx = g.all_windows() if widx is None else widx
    side = g.side(widx, paired)
    bidx = g.bias_index().reshape(-1)
    per_bin = torch.zeros(g.nb, dtype=F64).index_add_(0, bidx, torch.ones(T * T, dtype=F64))
    outs = []
    for sd in range(2 if paired else 1):
        sel = side == sd
        nterm = per_bin * int(sel.sum())
        e1 = torch.zeros(g.heads, g.nb, dtype=F64).index_add_(1, bidx, ddS[sel].sum(0).reshape(g.heads, -1))
        e2 = torch.zeros(g.heads, g.nb, dtype=F64).index_add_(1, bidx, adS[sel].sum(0).reshape(g.heads, -1))
        o = e1 + (nterm[None, :] + 1) * (u * e2 + TINY)
        outs.append(o if pre is None else o + u * pre[sd].reshape(g.heads, g.nb).abs().to(F64))
    b["drelbias"] = torch.stack(outs)
    return b


def results(g, r, paired=False, widx=None, mutant=None, pre=None):
    """the six outputs of a run in the layouts bounds() uses"""
    o = {"O": tokens(r["O"]), "lse": tokens(r["lse"])}
    if "dS" in r:
        o.update(dQ=tokens(r["dQ"]), dK=tokens(r["dK"]), dV=tokens(r["dV"]), drelbias=drelbias(g, r["dS"], widx, paired, mutant, pre))
    return o


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all elements; a NaN or an infinity in `got` counts as infinite"""
    gt = got.to(F64)
    assert gt.shape == ref.shape == bound.shape, (gt.shape, ref.shape, bound.shape)
    if not torch.isfinite(gt).all():
        return math.inf
    return float(((gt - ref).abs() / bound).max())


def bits_equal(got, ref64):
    want = ref64.to(F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=F32)


def build(regime, g, seed=0):
    """Seeded float32 operands of one case: qkv [tokens, 3C], dout [tokens, C], relbias / relbias2 [heads, 2ws-1, 2ws-1] (relbias2 is the
    paired form's second table), pre [2, heads, 2ws-1, 2ws-1] (what accumulate = 1 adds to).

    mild     randn q, k, v, dO; bias 0.5 randn
    peaked   q and k scaled by 6: score std 36, rows near one-hot
    offset   a mild bias + 100 on even heads, - 100 on odd heads: exp overflows / the softmax is 0/0 without the max subtraction
    hostile  every masked key's raw score is more than 100 above every visible key's of the same query.  The far side depends on the
             query's side, so one common direction cannot do it; instead channels 0 / 1 of each head carry the token's y / x side:
             q = e_y sy (channel 0), e_x sx (channel 1), randn elsewhere; k = - M sy + randn, - M sx + randn, randn elsewhere, with
             sy, sx = +1 on the low side and -1 on the high one, e_y / e_x = 1 only in the windows of the last row / column, and
             M = 120 hd^1/2.  A score is then - 120 (e_y sy_i sy_j + e_x sx_i sx_j) + noise of a few units: - 120 or - 240 for every
             visible key, + 120, 0 or + 240 for every masked one.  (A kernel that masks by multiplying with zero and takes the max
             afterwards has exp(- 120) = 0 for every visible key: 0 / 0.)
    exact    q = 0, bias = 0, k / dO small integers, v[token][c] = pixel index mod 256 + c: p is exactly 1 / (number of visible keys)
    """
    gen = _gen(1000 * seed + 17 * g.C + 5 * g.ws + g.H + 3 * g.W + 7 * g.B + g.shift)
    N, C, hd = g.tokens, g.C, g.hd
    qkv, dout = _randn(gen, N, 3 * C), _randn(gen, N, C)
    rb, rb2 = 0.5 * _randn(gen, g.heads, g.nbw, g.nbw), 0.5 * _randn(gen, g.heads, g.nbw, g.nbw)
    pre = _randn(gen, 2, g.heads, g.nbw, g.nbw)
    if regime == "peaked":
        qkv[:, :2 * C] *= 6.0
    elif regime == "offset":
        sign = torch.where(torch.arange(g.heads) % 2 == 0, 100.0, -100.0)[:, None, None]
        rb, rb2 = rb + sign, rb2 + sign
    elif regime == "hostile":
        w = g.all_windows()
        pix = g.pixels(w).reshape(-1)
        _, wy, wx = g.coords(w)
        t = torch.arange(g.T)
        gap = g.ws - g.ws // 2
        sy = torch.where((t // g.ws) < gap, 1.0, -1.0)[None, :].expand(g.windows, -1).reshape(-1)
        sx = torch.where((t % g.ws) < gap, 1.0, -1.0)[None, :].expand(g.windows, -1).reshape(-1)
        ey = ((wy == g.nwy - 1) & bool(g.shift)).float()[:, None].expand(-1, g.T).reshape(-1)
        exx = ((wx == g.nwx - 1) & bool(g.shift)).float()[:, None].expand(-1, g.T).reshape(-1)
        M = 120.0 * math.sqrt(hd)
        for h in range(g.heads):
            qkv[pix, h * hd] = ey * sy
            qkv[pix, h * hd + 1] = exx * sx
            qkv[pix, C + h * hd] += -M * sy
            qkv[pix, C + h * hd + 1] += -M * sx
    elif regime == "exact":
        qkv[:, :C] = 0.0
        qkv[:, C:2 * C] = torch.randint(-3, 4, (N, C), generator=gen).float()
        qkv[:, 2 * C:] = (torch.arange(N) % (g.H * g.W) % 256)[:, None].float() + torch.arange(C)[None, :].float()
        dout = torch.randint(-3, 4, (N, C), generator=gen).float()
        rb, rb2 = torch.zeros_like(rb), torch.zeros_like(rb2)
    else:
        assert regime == "mild", regime
    return {"qkv": qkv, "dout": dout, "relbias": rb, "relbias2": rb2, "pre": pre}


def exact_expected(g, t):
    """exact regime, integer arithmetic: O = mean of v over the visible keys, dV[j] = sum_i dO[i] / n_i over the queries that see j,
    lse = log n — [windows, T, C] float64, exact (every value a small multiple of 1/64)"""
    w = g.all_windows()
    pix = g.pixels(w)
    vis = (~g.mask(w)).to(F64)                                              # [n, Tq, Tk]
    cnt = vis.sum(-1, keepdim=True)
    v = t["qkv"][pix.reshape(-1), 2 * g.C:].reshape(g.windows, g.T, g.C).to(F64)
    dO = t["dout"][pix.reshape(-1)].reshape(g.windows, g.T, g.C).to(F64)
    pm = vis / cnt
    return {"O": pm @ v, "dV": pm.transpose(-1, -2) @ dO, "lse": torch.log(cnt).expand(-1, -1, g.heads)}
