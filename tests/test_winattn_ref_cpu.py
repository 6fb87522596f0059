"""tests/winattn_ref.py checked on the CPU: the float64 statement against the oracle WMSA under autograd, the budgets against the float32
restatement, and the bounds' eyesight against twelve planted errors."""
import functools
import math

import pytest
import torch

import winattn_ref as R

F32, F64 = torch.float32, torch.float64
ALL_CASES = [(c, False) for c in R.SMALL_CASES] + [(c, True) for c in R.PAIR_CASES]


def _oracle_core(qkv_map, relbias, heads, ws, shift):
    """attention core of the oracle WMSA (roll, rel_bias(), shift_mask(); no projections) on a [B, H, W, 3C] map -> [B, H, W, C]"""
    from oracle.graph import WMSA

    B, H, W, C3 = qkv_map.shape
    C = C3 // 3
    m = WMSA(C, C, C // heads, ws, "SW" if shift else "W")
    del m.relative_position_params
    m.relative_position_params = relbias
    x = qkv_map
    sh = ws // 2
    if shift:
        x = torch.roll(x, shifts=(-sh, -sh), dims=(1, 2))
    hw, ww = H // ws, W // ws
    xw = x.reshape(B, hw, ws, ww, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(B, hw * ww, ws * ws, C3)
    hd = C // heads
    qkv = xw.reshape(B, hw * ww, ws * ws, 3 * heads, hd).permute(3, 0, 1, 2, 4)
    q, k, v = qkv[:heads], qkv[heads:2 * heads], qkv[2 * heads:]
    sim = torch.matmul(q, k.transpose(-1, -2)) * hd ** -0.5 + m.rel_bias()[:, None, None]
    if shift:
        sim = sim.masked_fill(m.shift_mask(hw, ww)[None, None], float("-inf"))
    lse = torch.logsumexp(sim, -1)                                                     # [heads, B, nw, T]
    out = torch.matmul(torch.softmax(sim, -1), v).permute(1, 2, 3, 0, 4).reshape(B, hw * ww, ws * ws, C)
    out = out.reshape(B, hw, ww, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    lse = lse.permute(1, 2, 3, 0).reshape(B, hw, ww, ws, ws, heads).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, heads)
    if shift:
        out = torch.roll(out, shifts=(sh, sh), dims=(1, 2))
        lse = torch.roll(lse, shifts=(sh, sh), dims=(1, 2))
    return out, lse


def scatter(g, pix, tok, width):
    """[n, T, width] token rows of windows -> the [tokens, width] map"""
    out = torch.zeros(g.tokens, width, dtype=tok.dtype)
    out[pix.reshape(-1)] = tok.reshape(-1, width)
    return out


ORACLE_SHAPES = [(8, 16, 24), (8, 24, 24), (8, 24, 40), (4, 8, 12), (4, 12, 12), (4, 16, 24), (4, 24, 40)]   # 2x3 and 3x3 grids, 16x24, 24x40


@pytest.mark.parametrize("shift", [0, 1], ids=["W", "SW"])
@pytest.mark.parametrize("ws,H,W", ORACLE_SHAPES, ids=[f"ws{s[0]}-{s[1]}x{s[2]}" for s in ORACLE_SHAPES])
def test_reference_is_the_oracle_under_float64_autograd(ws, H, W, shift):
    C, heads, B = 32, 2, 2
    g = R.Geom(C, heads, ws, H, W, B, shift)
    t = R.build("mild", g, seed=3)
    qkv = t["qkv"].double().requires_grad_()
    rb = t["relbias"].double().requires_grad_()
    out, lse = _oracle_core(qkv.reshape(B, H, W, 3 * C), rb, heads, ws, shift)
    out.backward(t["dout"].double().reshape(B, H, W, C))
    r = R.attend(g, t["qkv"], t["relbias"], t["dout"])
    o = R.results(g, r)

    def same(name, a, b):
        assert bool(((a - b).abs() <= 1e-12 * (1 + b.abs())).all()), (name, float((a - b).abs().max()))

    same("O", scatter(g, r["pix"], o["O"], C), out.detach().reshape(-1, C))
    same("lse", scatter(g, r["pix"], o["lse"], heads), lse.detach().reshape(-1, heads))
    for i, kind in enumerate(("dQ", "dK", "dV")):
        same(kind, scatter(g, r["pix"], o[kind], C), qkv.grad[:, i * C:(i + 1) * C])
    same("drelbias", o["drelbias"][0].reshape(heads, g.nbw, g.nbw), rb.grad)


@functools.lru_cache(maxsize=None)
def _case(case, paired, shift, regime):
    """(geometry, operands, float64 results, bounds) — computed once, shared, never modified"""
    _, C, heads, ws, H, W, B = case
    g = R.Geom(C, heads, ws, H, W, B, shift)
    t = R.build(regime, g)
    r = R.attend(g, t["qkv"], t["relbias"], t["dout"], relbias2=t["relbias2"] if paired else None)
    return g, t, R.results(g, r, paired), R.bounds(g, r, paired)


def _f32(case, paired, shift, regime, mutant=None):
    g, t, ref, bnd = _case(case, paired, shift, regime)
    r = R.attend(g, t["qkv"], t["relbias"], t["dout"], relbias2=t["relbias2"] if paired else None, dtype=F32, mutant=mutant)
    got = R.results(g, r, paired, mutant=mutant)
    return g, t, got, {k: R.worst_ratio(got[k], ref[k], bnd[k]) for k in R.KINDS}


def _exact_bits(g, t, got):
    want = R.exact_expected(g, t)
    return all(R.bits_equal(got[k], want[k]) for k in ("O", "dV"))


@functools.lru_cache(maxsize=None)
def _measure():
    worst = {rg: dict.fromkeys(R.KINDS, 0.0) for rg in R.REGIMES}
    for case, paired in ALL_CASES:
        for shift in (0, 1):
            for rg in R.REGIMES:
                g, t, got, ratios = _f32(case, paired, shift, rg)
                for k, v in ratios.items():
                    worst[rg][k] = max(worst[rg][k], v)
                if rg == "exact":
                    assert _exact_bits(g, t, got), (case, shift)
    return worst


def test_budgets_are_eight_times_the_float32_cpu_error():
    m = _measure()
    for rg in R.REGIMES:
        for k in R.KINDS:
            v, b = m[rg][k], R.BUDGET[rg][k]
            print(f"budget {rg:8s} {k:9s}: float32 CPU error / bound = {v:.4f}, 8 x = {8 * v:.4f}, BUDGET = {b}")
    for rg in R.REGIMES:
        for k in R.KINDS:
            v, b = m[rg][k], R.BUDGET[rg][k]
            if b == R.EXACT:   # exact float32 arithmetic: what is left is the float64 reference's own rounding
                assert v <= 1e-9, (rg, k, v)
                continue
            assert 8 * v <= b, (rg, k, v, b)
            assert b <= 16 * v, f"{rg} {k}: the budget {b} is more than 16 x the measurement {v}"


def test_exact_regime_is_exact_in_float64_and_names_the_keys_seen():
    """the float64 statement itself meets the integer arithmetic of exact_expected, and the values separate the keys: two queries of one
    window with different visible sets get different outputs"""
    for case, paired in ALL_CASES:
        g, t, ref, _ = _case(case, paired, 1, "exact")
        want = R.exact_expected(g, t)
        for k in ("O", "dV", "lse"):
            assert float((ref[k] - want[k]).abs().max()) <= 1e-12, (case, k)
        corner = g.windows - 1                                  # last row and column: four visible sets
        o = ref["O"][corner, :, 0]
        gap = g.ws - g.ws // 2
        ids = [0, gap, gap * g.ws, gap * g.ws + gap]            # one query per quadrant
        assert len({round(float(o[i]), 6) for i in ids}) == 4, (case, o[ids])


def _hostile_margin(g, r):
    s, raw_mask = r["s"], r["mask"].expand_as(r["s"])
    raw = (r["qs"] @ r["k"].transpose(-1, -2) + r["bias"])
    vis_max = torch.where(raw_mask, torch.full_like(raw, -math.inf), raw).max(-1).values
    msk_min = torch.where(raw_mask, raw, torch.full_like(raw, math.inf)).min(-1).values
    return float((msk_min - vis_max).min())


def test_hostile_regime_puts_every_masked_key_100_above_every_visible_one():
    for case, paired in ALL_CASES:
        _, C, heads, ws, H, W, B = case
        g = R.Geom(C, heads, ws, H, W, B, 1)
        t = R.build("hostile", g)
        r = R.attend(g, t["qkv"], t["relbias"])
        assert _hostile_margin(g, r) > 100.0, case


def _kills(mutant, regimes):
    """first (case, shift, regime, kind) at which the mutant's float32 result leaves budget x bound"""
    for case, paired in ALL_CASES:
        for shift in (1, 0):
            for rg in regimes:
                _, _, _, ratios = _f32(case, paired, shift, rg, mutant)
                for k, v in ratios.items():
                    if v > max(R.BUDGET[rg][k], 1e-30):
                        return case[0], shift, rg, k, v
    return None


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_exceeds_a_budget(mutant):
    # the reduced-precision product must show on ordinary operands, the zero-multiply mask where it matters: under the hostile mask
    only = {"mantissa10": ("mild",), "max_after_zero_mask": ("hostile",)}
    regimes = only.get(mutant, tuple(rg for rg in R.REGIMES if rg != "exact"))
    hit = _kills(mutant, regimes)
    print(mutant, "->", hit)
    assert hit is not None, f"{mutant} stays within every budget on every small case: a case is missing"


@pytest.mark.parametrize("mutant", R.GEOMETRIC)
def test_geometric_mutants_break_the_exact_regime(mutant):
    broken = 0
    for case, paired in ALL_CASES:
        g, t, got, _ = _f32(case, paired, 1, "exact", mutant)
        broken += not _exact_bits(g, t, got)
    assert broken == len(ALL_CASES), f"{mutant}: bit equality survives on {len(ALL_CASES) - broken} shifted cases"
