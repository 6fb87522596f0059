"""The Gaussian-conditional kernels through the C ABI, every element against the float64 specification and the per-element bound of
tests/gauss_ref.py: clc_gauss_lik_fwd / _bwd (csrc/entropy.hip) and clc_gauss_lik_step_fwd / _bwd, clc_gauss_rate_sweep,
clc_quantize_build_indexes[_step] (csrc/qstep.hip), on [rows, C] maps, dense or a channel slice of a buffer of sentinels (ld = C + 8):

    (1, 1)      smallest map                                (70, 192)          nby = 3 row blocks in step_grad_final_kernel
    (3, 5)      smallest multi-element map                  (130, 192) sliced  nby = 5
    (9, 7)      C between powers of two below 64            (40, 320)          the widest latent (CLC / TCM / ELIC: M = 320)
    (257, 4)    crosses a 256-thread block                  (33, 32), (65, 16) ELIC's channel groups, a width no test had
    (5, 65)     a channel tile with one live lane           (16400, 64)        1 049 600 elements: grid_for's 1024-block cap; 513 row
                                                                               blocks cut to kMaxRowBlocks = 512 in the backward; as
                                                                               B = 2 x 8200 rows, 513 sweep blocks per image cut to 512

each in training and eval mode, with the unit step (entropy.hip) and with steps from {0.25, 1.0, 3.7} and one channel each at 1/16
and 16 (qstep.hip), in every regime the shape can hold (gauss_ref.REGIMES; the largest map: mild and tails).  Per element: lik, dy
(with and without dy_add / g_hat), dmu, dscale within budget x bound, y_hat bit for bit; per block: bits_partial against the float64 sum
of the block's own elements in the kernel's element order; per channel: dstep; per image and candidate: the sweep's bits.  Exact:
decided-blocked gradients are zero, eval dy is gh and dmu zero, the NaN the output buffers are filled with is gone, the sentinels
survive, two calls give the same bits, dy = dmu = NULL changes nothing else.

Measured on an MI355X (one run of this module, all 283 cases passing): the worst error / (budget x bound) per quantity and regime,
that is the fraction of its budget the kernels use.  A budget is 8 x the float32 host restatement's worst figure, so 0.125 is "as
good as the host's float32" (gauss_ref's docstring has the budgets).  The wrapper column is the autograd wrappers' tails case.

    quantity             mild    tails     wide   offset    edges  wrapper
    bits                0.090    0.182    0.283    0.122    0.040        -
    dmu                 0.104    0.111    0.077    0.125    0.066    0.096
    dscale              0.117    0.124    0.069    0.124    0.062    0.097
    dstep               0.040    0.048    0.125    0.121    0.016    0.007
    dy                  0.124    0.125    0.124    0.121    0.123    0.125
    dy, no g_hat        0.092    0.098    0.068    0.111    0.059        -
    lik                 0.218    0.115    0.246    0.202    0.085    0.107
    sweep               0.586    0.047    0.149        -        -        -

The gradients sit at the host's figure.  lik and bits use up to twice it in the wide regime, where Phi(a) - Phi(b) cancels and the
device's erfcf counts; the sweep's largest figure is the single-element images of the (1, 1) map, 0.44 of the bound itself.  Nothing
needed a kernel fix on finite inputs.

The same module against a library built from the parent commit's entropy.hip and qstep.hip: 57 of the 283 cases fail, and two more in
tests/test_eb_kernels_gpu.py, and nothing else —
    test_non_finite_values_propagate_as_in_the_float32_oracle, all 28: "lik" (fmaxf turned the NaN into a number);
    test_rate_sweep_against_float64, all 28: "the NaN image's bits are not NaN", the last clause of the test (everything before it,
        the float64 comparison and the identities, passes: the test stops at the NaN image);
    test_c_abi_refuses_bad_arguments_by_message: mode 2 with noise given was accepted;
    test_eb_kernels_gpu.py::test_a_nan_latent_stays_nan, both modes.
"""
import functools

import numpy as np
import pytest
import torch

import gauss_ref as R
import qstep_ref as Q

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 4, -777.25
FINITE = [r for r in R.REGIMES if r != "nonfinite"]
CASES = [(reg, rows, C, wide) for rows, C, wide in R.SHAPES for reg in FINITE if R.holds(reg, rows, C)]
IDS = [R.case_id(*c) for c in CASES]
NF_CASES = [(rows, C, wide) for rows, C, wide in R.SHAPES if R.holds("nonfinite", rows, C)]
NF_IDS = [f"{r}x{c}" + ("-sliced" if w else "") for r, c, w in NF_CASES]
MODES, MODE_IDS = [False, True], ["eval", "train"]
STEPPED, STEPPED_IDS = [False, True], ["unit", "step"]
USED = {}      # (quantity, regime) -> worst figure / budget seen in this session (printed when the module is done)


def _api():
    from clc_amd import lib, ops

    return lib.load(), lib, ops._stream()


class _Map:
    """a [rows, C] device map, dense or a channel slice of a [rows, C + 2 PAD] buffer of sentinels; an output map starts as NaN"""

    def __init__(self, rows, C, wide, dev, src=None, dtype=torch.float32):
        self.wide, self.C = wide, C
        self.buf = torch.full((rows, C + 2 * PAD if wide else C), SENTINEL, device=dev, dtype=dtype)
        self.view = self.buf[:, PAD:PAD + C] if wide else self.buf
        if src is not None:
            self.view.copy_(src.to(dev))
        elif dtype == torch.float32:
            self.view.fill_(float("nan"))
        self.ptr, self.ld = self.view.data_ptr(), self.buf.shape[1]
        assert not wide or (self.ld == C + 8 and self.ld % 32 != 0)

    def get(self):
        if self.wide:
            assert bool((self.buf[:, :PAD] == SENTINEL).all()) and bool((self.buf[:, PAD + self.C:] == SENTINEL).all()), "wrote outside the slice"
        return self.view.cpu().clone()


class _Flat:
    """n floats of NaN on the device followed by 8 sentinels that must survive"""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + 8,), SENTINEL, device=dev, dtype=torch.float32)
        self.buf[:n] = float("nan")
        self.ptr = self.buf.data_ptr()

    def get(self):
        assert bool((self.buf[self.n:] == SENTINEL).all()), "wrote past the buffer"
        return self.buf[:self.n].cpu().clone()


def _fwd(dev, d, rows, C, wide, training, stepped, partials=True, y_hat=True):
    L, lib, st = _api()
    m = {k: _Map(rows, C, wide, dev, d[k]) for k in ("y", "mu", "scale", "noise")}
    lik, yh = _Map(rows, C, wide, dev), _Map(rows, C, wide, dev)
    nb = L.clc_gauss_lik_partials(rows, C)
    part = _Flat(nb, dev)
    npn, ldn = (m["noise"].ptr, m["noise"].ld) if training else (None, 0)
    pp, pn = (part.ptr, nb) if partials else (None, 0)
    yp, ldh = (yh.ptr, yh.ld) if y_hat else (None, 0)
    head = (m["y"].ptr, m["y"].ld, m["mu"].ptr, m["mu"].ld, m["scale"].ptr, m["scale"].ld, npn, ldn)
    tail = (lik.ptr, lik.ld, yp, ldh, rows, C, 0 if training else 1, pp, pn, st)
    if stepped:
        sd = d["step"].to(dev)
        lib.check(L.clc_gauss_lik_step_fwd(*head, sd.data_ptr(), *tail), "clc_gauss_lik_step_fwd")
    else:
        lib.check(L.clc_gauss_lik_fwd(*head, *tail), "clc_gauss_lik_fwd")
    return {"lik": lik.get(), "y_hat": yh.get(), "part": part.get(), "nb": nb}


def _bwd(dev, d, rows, C, wide, training, stepped, hat=True, outputs=True):
    L, lib, st = _api()
    m = {k: _Map(rows, C, wide, dev, d[k]) for k in ("y", "mu", "scale", "noise", "w", "gh")}
    dy, dmu, dsc = (_Map(rows, C, wide, dev) for _ in range(3))
    npn, ldn = (m["noise"].ptr, m["noise"].ld) if training else (None, 0)
    hp, ldh = (m["gh"].ptr, m["gh"].ld) if hat else (None, 0)
    dyp, dmp = (dy.ptr, dmu.ptr) if outputs else (None, None)
    head = (m["w"].ptr, m["w"].ld, m["y"].ptr, m["y"].ld, m["mu"].ptr, m["mu"].ld, m["scale"].ptr, m["scale"].ld, npn, ldn)
    dstep = _Flat(C, dev)
    if stepped:
        sd = d["step"].to(dev)
        nbytes = L.clc_gauss_lik_step_bwd_workspace_bytes(rows, C)
        assert nbytes > 0 and nbytes % 4 == 0
        ws = _Flat(nbytes // 4, dev)
        lib.check(L.clc_gauss_lik_step_bwd(*head, sd.data_ptr(), dyp, dy.ld, dmp, dmu.ld, dsc.ptr, dsc.ld, dstep.ptr, rows, C, 0 if training else 1,
                                           hp, ldh, ws.ptr, nbytes, st), "clc_gauss_lik_step_bwd")
        ws.get()
    else:
        lib.check(L.clc_gauss_lik_bwd(*head, dyp, dy.ld, dmp, dmu.ld, dsc.ptr, dsc.ld, rows, C, 0 if training else 1, hp, ldh, st), "clc_gauss_lik_bwd")
    return {"dy": dy.get(), "dmu": dmu.get(), "dscale": dsc.get(), "dstep": dstep.get()}


def _table(dev):
    from clc_amd.models.clc import get_scale_table

    return torch.tensor([float(s) for s in get_scale_table()], dtype=torch.float32, device=dev)


def _qbi(dev, d, rows, C, wide, stepped):
    L, lib, st = _api()
    table = _table(dev)
    my, mm, ms = (_Map(rows, C, wide, dev, d[k]) for k in ("y", "mu", "scale"))
    yh = _Map(rows, C, wide, dev)
    sym = torch.full((rows * C + 8,), -12345, device=dev, dtype=torch.int32)
    idx = torch.full((rows * C + 8,), -12345, device=dev, dtype=torch.int32)
    head = (my.ptr, my.ld, mm.ptr, mm.ld, ms.ptr, ms.ld)
    tail = (table.data_ptr(), table.numel(), sym.data_ptr(), idx.data_ptr(), yh.ptr, yh.ld, rows, C, st)
    if stepped:
        sd = d["step"].to(dev)
        lib.check(L.clc_quantize_build_indexes_step(*head, sd.data_ptr(), *tail), "clc_quantize_build_indexes_step")
    else:
        lib.check(L.clc_quantize_build_indexes(*head, *tail), "clc_quantize_build_indexes")
    assert bool((sym[rows * C:] == -12345).all()) and bool((idx[rows * C:] == -12345).all())
    return sym[:rows * C].cpu().numpy().reshape(rows, C), idx[:rows * C].cpu().numpy().reshape(rows, C), yh.get().numpy()


def _sweep(dev, d, steps, B, n_rows, C, wide):
    L, lib, st = _api()
    my, mm, ms = (_Map(B * n_rows, C, wide, dev, d[k]) for k in ("y", "mu", "scale"))
    K = steps.shape[0]
    sd = steps.contiguous().to(dev)
    bits = _Flat(B * K, dev)
    nbytes = L.clc_gauss_rate_sweep_workspace_bytes(B, n_rows, C, K)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = _Flat(nbytes // 4, dev)
    lib.check(L.clc_gauss_rate_sweep(my.ptr, my.ld, mm.ptr, mm.ld, ms.ptr, ms.ld, sd.data_ptr(), K, B, n_rows, C, bits.ptr, ws.ptr, nbytes, st),
              "clc_gauss_rate_sweep")
    ws.get()
    return bits.get().reshape(B, K)


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a if isinstance(a[k], torch.Tensor))


@functools.lru_cache(maxsize=2)
def _an(reg, rows, C, stepped, training):
    """float64, computed once per case, shared, never modified (two at a time: the largest map's is 300 MB)"""
    d = R.inputs(reg, rows, C, stepped)
    return R.analyse(d, d["step"], training)


@pytest.fixture(scope="module", autouse=True)
def _budget_used():
    """after the module's last test: the table of the docstring, worst figure / budget per quantity and regime over the cases that ran"""
    yield
    cols = [r for r in FINITE + ["wrapper"] if any(c == r for _, c in USED)]
    print("\n    " + "quantity".ljust(16) + "".join(c.rjust(9) for c in cols))
    for q in sorted({q for q, _ in USED}):
        print("    " + q.ljust(16) + "".join((f"{USED[(q, c)]:.3f}" if (q, c) in USED else "-").rjust(9) for c in cols))


def _report(tag, fig):
    for k, (v, bar) in fig.items():
        print(f"{tag:40s} {k:18s} {v:10.3e}   bar {bar:g}")
        if bar > 0:
            key = (k, tag.split("-")[0].split(" ")[0])
            USED[key] = max(USED.get(key, 0.0), v / bar)
    assert not R.failures(fig), (tag, R.failures(fig))


@pytest.mark.parametrize("stepped", STEPPED, ids=STEPPED_IDS)
@pytest.mark.parametrize("training", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_element_against_float64(dev, case, training, stepped):
    reg, rows, C, wide = case
    d, an = R.inputs(reg, rows, C, stepped), _an(reg, rows, C, stepped, training)
    tag = R.case_id(*case) + ("-step" if stepped else "-unit") + ("-train" if training else "-eval")
    f = _fwd(dev, d, rows, C, wide, training, stepped)
    assert f["nb"] == R.grid_for(rows * C)                           # clc_gauss_lik_partials is the grid
    fig = R.compare_forward(f, an)
    fig.update(R.compare_partials(f["part"], an, f["nb"]))
    b = _bwd(dev, d, rows, C, wide, training, stepped, hat=True)
    fig.update(R.compare_backward(b, an, training, hat=True))
    if stepped:
        fig.update(R.compare_dstep(b["dstep"], an))
    b0 = _bwd(dev, d, rows, C, wide, training, stepped, hat=False)  # without dy_add / g_hat
    fig.update({k + ", no g_hat": v for k, v in R.compare_backward(b0, an, training, hat=False).items() if k.startswith("dy")})
    _report(tag, fig)
    assert torch.equal(_bits(b0["dscale"]), _bits(b["dscale"])) and torch.equal(_bits(b0["dmu"]), _bits(b["dmu"]))
    # the same bits run to run; y_hat, bits_partial, dy and dmu are optional and change nothing else
    assert _same_bits(_fwd(dev, d, rows, C, wide, training, stepped), f), "forward differs run to run"
    assert _same_bits(_bwd(dev, d, rows, C, wide, training, stepped, hat=True), b), "backward differs run to run"
    bare = _fwd(dev, d, rows, C, wide, training, stepped, partials=False, y_hat=False)
    assert torch.equal(_bits(bare["lik"]), _bits(f["lik"])) and bool(torch.isnan(bare["y_hat"]).all()) and bool(torch.isnan(bare["part"]).all())
    nul = _bwd(dev, d, rows, C, wide, training, stepped, hat=True, outputs=False)
    assert torch.equal(_bits(nul["dscale"]), _bits(b["dscale"])) and bool(torch.isnan(nul["dy"]).all()) and bool(torch.isnan(nul["dmu"]).all())
    if stepped:
        assert torch.equal(_bits(nul["dstep"]), _bits(b["dstep"]))


# ---- the rate sweep ----

SWEEP_CASES = [(reg, rows, C, wide, 3) for rows, C, wide in R.SHAPES if (rows, C) != R.BIG for reg in ("mild", "tails", "wide")
               if (reg == "mild" or rows * C >= 60)] + [(reg, 8200, 64, False, 2) for reg in ("mild", "tails")]


@pytest.mark.parametrize("reg,n_rows,C,wide,B", SWEEP_CASES, ids=[R.case_id(c[0], c[1], c[2], c[3]) + f"-B{c[4]}" for c in SWEEP_CASES])
def test_rate_sweep_against_float64(dev, reg, n_rows, C, wide, B):
    """K = 16 (5 on the largest map) against float64 per image and candidate at the derived sum bound; candidates 1 and 2 differ in
    channel 0's step alone; K = 1 and K = 5 are columns of the K = 16 call; an image alone is the image of the batch; a NaN in one
    image leaves the other images' bits as they were"""
    big = n_rows * B * C > 500_000
    d = R.inputs(reg, B * n_rows, C, True)
    steps = R.sweep_steps(C, 5 if big else 16)
    K = steps.shape[0]
    want, bound = R.sweep_reference(d, steps, B)
    bits = _sweep(dev, d, steps, B, n_rows, C, wide)
    _report(R.case_id(reg, n_rows, C, wide) + f"-K{K}", R.compare_sweep(bits, want, bound))
    assert bool((steps[1, 1:] == steps[2, 1:]).all()) and float(steps[1, 0]) != float(steps[2, 0])
    for ks in ([0], [0, 1, 2, 3, 4]):
        assert torch.equal(_bits(_sweep(dev, d, steps[ks], B, n_rows, C, wide)), _bits(bits[:, ks])), ks
    one = _sweep(dev, d, steps[K - 1:K], B, n_rows, C, wide)
    assert torch.equal(_bits(one[:, 0]), _bits(bits[:, K - 1]))
    if not big:
        for b in range(B):
            rows = slice(b * n_rows, (b + 1) * n_rows)
            alone = _sweep(dev, {k: d[k][rows] for k in ("y", "mu", "scale")}, steps, 1, n_rows, C, wide)
            assert torch.equal(_bits(alone[0]), _bits(bits[b])), b
    bad = {k: d[k].clone() for k in ("y", "mu", "scale")}
    bad["y"][n_rows + n_rows // 2, C // 2] = float("nan")          # image 1
    got = _sweep(dev, bad, steps, B, n_rows, C, wide)
    assert bool(torch.isnan(got[1]).all()), "the NaN image's bits are not NaN"
    keep = [b for b in range(B) if b != 1]
    assert torch.equal(_bits(got[keep]), _bits(bits[keep])), "a NaN in one image changed another image's bits"


# ---- the integer path on the new shapes (tests/test_qstep_kernels_gpu.py keeps the others) ----

INT_SHAPES = [(9, 7, False), (5, 65, False), (70, 192, False), (40, 320, False), (33, 32, True), (65, 16, False), (16400, 64, False)]


@pytest.mark.parametrize("stepped", STEPPED, ids=STEPPED_IDS)
@pytest.mark.parametrize("rows,C,wide", INT_SHAPES, ids=[f"{r}x{c}" for r, c, _ in INT_SHAPES])
def test_integer_path_on_the_new_shapes(dev, rows, C, wide, stepped):
    """symbols, indexes and y_hat against qstep_ref.integer_path, every element; exact ties and edge scales from the edges regime (the
    largest map: mild), and a NaN scale, which still codes as 0.11 — on purpose: encoder and decoder share the expression"""
    reg = "mild" if (rows, C) == R.BIG else "edges"
    d = {k: v.clone() for k, v in R.inputs(reg, rows, C, stepped).items()}
    d["scale"] = d["scale"].abs() * 40 if reg == "mild" else d["scale"]
    d["scale"][rows // 2, C // 2] = float("nan")
    table = _table(dev).cpu().numpy()
    sym, idx, yh = _qbi(dev, d, rows, C, wide, stepped)
    w_sym, w_idx, w_yh = Q.integer_path(d["y"].numpy(), d["mu"].numpy(), d["scale"].numpy(), d["step"].numpy(), table)
    assert np.array_equal(sym, w_sym) and np.array_equal(idx, w_idx)
    assert np.array_equal(yh.view(np.uint32), w_yh.view(np.uint32)), "y_hat bits"
    s = float(d["step"][C // 2])
    assert idx[rows // 2, C // 2] == Q.scale_index(np.float32(np.float32(0.11) / np.float32(s)), table)


# ---- the non-finite regime ----

@pytest.mark.parametrize("stepped", STEPPED, ids=STEPPED_IDS)
@pytest.mark.parametrize("training", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("rows,C,wide", NF_CASES, ids=NF_IDS)
def test_non_finite_values_propagate_as_in_the_float32_oracle(dev, rows, C, wide, training, stepped):
    """one element each of NaN, +inf, -inf in y, mu, scale, noise and dlik: lik, bits and the gradients are NaN exactly where the float32
    oracle's are (the step form: where qstep_ref's in float32 are; the CPU test pins the two at the unit step), and every other element
    has the bits of a run without the planted values.  One stated departure (gauss_ref / the kernels' comments): at an infinite dlik the
    oracle's gradients are NaN or an infinity by the signs of autograd's two halves; the kernels' are NaN."""
    d, clean = R.inputs("nonfinite", rows, C, stepped), R.clean_of(rows, C, stepped)
    want = R.spec32(d, d["step"], training) if stepped else R.oracle32(d, training)
    pos = R.planted(rows, C)
    inf_g = [p for p, (f, v) in zip(pos, R.NONFINITE) if f == "w" and v == v]
    keep = torch.ones(rows * C, dtype=torch.bool)
    keep[pos] = False
    f, f0 = _fwd(dev, d, rows, C, wide, training, stepped), _fwd(dev, clean, rows, C, wide, training, stepped)
    b, b0 = _bwd(dev, d, rows, C, wide, training, stepped), _bwd(dev, clean, rows, C, wide, training, stepped)
    flat = lambda t: t.reshape(-1)
    assert torch.equal(torch.isnan(f["lik"]), torch.isnan(want["lik"])), "lik"
    assert torch.equal(_bits(flat(f["lik"])[keep]), _bits(flat(f0["lik"])[keep]))
    blk = R.block_of(rows * C, f["nb"])
    nan_blocks = torch.zeros(f["nb"], dtype=torch.bool)
    nan_blocks[blk[flat(torch.isnan(want["lik"]))]] = True
    assert torch.equal(torch.isnan(f["part"]), nan_blocks), "bits_partial"
    dirty = torch.zeros(f["nb"], dtype=torch.bool)
    dirty[blk[pos]] = True
    assert torch.equal(_bits(f["part"][~dirty]), _bits(f0["part"][~dirty]))
    names = {"dscale": "dscale", "dmu": "dmu"}
    if training:
        names["dy"] = "dy0"                                        # (dy = gy + gh: NaN where gy is)
    for got_k, want_k in names.items():
        g, w = flat(torch.isnan(b[got_k])), flat(torch.isnan(want[want_k]))
        w[inf_g] = True
        assert torch.equal(g, w), (got_k, [(fv, bool(g[p]), bool(w[p])) for p, fv in zip(pos, R.NONFINITE)])
        assert torch.equal(_bits(flat(b[got_k])[keep]), _bits(flat(b0[got_k])[keep])), got_k
    if not training:
        assert torch.equal(_bits(b["dy"]), _bits(d["gh"]))
    if stepped:
        w = torch.isnan(want["terms"])
        flat(w)[inf_g] = True
        assert torch.equal(torch.isnan(b["dstep"]), w.any(0)), "dstep"
        same = ~torch.zeros(rows * C, dtype=torch.bool).index_fill_(0, torch.tensor(pos), True).reshape(rows, C).any(0)
        assert torch.equal(_bits(b["dstep"][same]), _bits(b0["dstep"][same]))


# ---- the autograd wrappers ----

@pytest.mark.parametrize("stepped", STEPPED, ids=STEPPED_IDS)
@pytest.mark.parametrize("training", MODES, ids=MODE_IDS)
def test_autograd_wrappers_against_float64(dev, training, stepped):
    """ops.gaussian_likelihood / ops.gaussian_likelihood_step on the tails regime, against the same reference through the same
    comparison functions"""
    from clc_amd import ops

    reg, rows, C = "tails", 70, 192
    d, an = R.inputs(reg, rows, C, stepped), _an(reg, rows, C, stepped, training)
    to4 = lambda t: t.reshape(1, rows, 1, C).permute(0, 3, 1, 2).to(dev)
    back = lambda t: t.detach().permute(0, 2, 3, 1).reshape(rows, C).cpu()
    y, mu, sc = (to4(d[k]).requires_grad_() for k in ("y", "mu", "scale"))
    noise = to4(d["noise"]) if training else None
    if stepped:
        step = d["step"].to(dev).requires_grad_()
        lik, yh = ops.gaussian_likelihood_step(y, sc, mu, step, noise, training)
    else:
        lik, yh = ops.gaussian_likelihood(y, sc, mu, noise, training)
    ((lik * to4(d["w"])).sum() + (yh * to4(d["gh"])).sum()).backward()
    fig = R.compare_forward({"lik": back(lik), "y_hat": back(yh)}, an)
    zeros = torch.zeros(rows, C)
    got = {"dscale": back(sc.grad), "dy": back(y.grad), "dmu": back(mu.grad) if mu.grad is not None else zeros}
    fig.update(R.compare_backward(got, an, training, hat=True))
    if stepped:
        fig.update(R.compare_dstep(step.grad.cpu(), an))
    _report(f"wrapper {'step' if stepped else 'unit'} {'train' if training else 'eval'}", fig)


# ---- the refusals ----

def test_c_abi_refuses_bad_arguments_by_message(dev):
    """every refusal of the unit-step entries (new: mode outside {0, 1}, ld < C per operand), and those of the step twins and the sweep
    that tests/test_qstep_kernels_gpu.py leaves out; no refused call launches a kernel"""
    L, lib, st = _api()
    rows, C = 4, 4
    t = torch.zeros(64, device=dev)
    i32 = torch.zeros(64, device=dev, dtype=torch.int32)
    p, ip = t.data_ptr(), i32.data_ptr()

    def refused(rc, text):
        assert rc < 0 and text in L.clc_last_error().decode(), (rc, text, L.clc_last_error())

    def swap(args, i, v):
        return args[:i] + (v,) + args[i + 1:]

    fwd = (p, C, p, C, p, C, p, C, p, C, p, C, rows, C, 0, None, 0, st)
    for i in (0, 2, 4, 8):                                          # y, mu, scale, lik
        refused(L.clc_gauss_lik_fwd(*swap(fwd, i, None)), "clc_gauss_lik_fwd: bad args")
    refused(L.clc_gauss_lik_fwd(*swap(fwd, 12, 0)), "clc_gauss_lik_fwd: bad args")
    refused(L.clc_gauss_lik_fwd(*swap(fwd, 13, 0)), "clc_gauss_lik_fwd: bad args")
    refused(L.clc_gauss_lik_fwd(*swap(fwd, 6, None)), "clc_gauss_lik_fwd: training mode needs noise")
    for mode in (2, -1):                                            # (with noise given, mode 2 used to run the eval path)
        refused(L.clc_gauss_lik_fwd(*swap(fwd, 14, mode)), f"clc_gauss_lik_fwd: mode must be 0 (training) or 1 (eval) (got {mode})")
    for i in (1, 3, 5, 7, 9, 11):                                   # ldy, ldmu, ldsc, ldn, ldl, ldh
        refused(L.clc_gauss_lik_fwd(*swap(fwd, i, C - 1)), "clc_gauss_lik_fwd: a leading dimension is below C = 4")
    refused(L.clc_gauss_lik_fwd(*swap(swap(fwd, 15, p), 16, 7)), "clc_gauss_lik_fwd: n_partials must be clc_gauss_lik_partials() = 1")

    bwd = (p, C, p, C, p, C, p, C, p, C, p, C, p, C, p, C, rows, C, 0, p, C, st)
    for i in (0, 2, 4, 6, 14):                                      # dlik, y, mu, scale, dscale
        refused(L.clc_gauss_lik_bwd(*swap(bwd, i, None)), "clc_gauss_lik_bwd: bad args")
    refused(L.clc_gauss_lik_bwd(*swap(bwd, 16, 0)), "clc_gauss_lik_bwd: bad args")
    refused(L.clc_gauss_lik_bwd(*swap(bwd, 17, 0)), "clc_gauss_lik_bwd: bad args")
    refused(L.clc_gauss_lik_bwd(*swap(bwd, 8, None)), "clc_gauss_lik_bwd: training mode needs noise")
    refused(L.clc_gauss_lik_bwd(*swap(bwd, 18, 2)), "clc_gauss_lik_bwd: mode must be 0 (training) or 1 (eval) (got 2)")
    for i in (1, 3, 5, 7, 9, 11, 13, 15, 20):                       # lddl, ldy, ldmu, ldsc, ldn, lddy, lddmu, lddsc, ldadd
        refused(L.clc_gauss_lik_bwd(*swap(bwd, i, C - 1)), "clc_gauss_lik_bwd: a leading dimension is below C = 4")

    qbi = (p, C, p, C, p, C, p, 8, ip, ip, p, C, rows, C, st)
    for i in (0, 2, 4, 6, 8, 9):                                    # y, mu, scale, scale_table, symbols, indexes
        refused(L.clc_quantize_build_indexes(*swap(qbi, i, None)), "clc_quantize_build_indexes: bad args")
    for n in (1, 257):
        refused(L.clc_quantize_build_indexes(*swap(qbi, 7, n)), "clc_quantize_build_indexes: n_scales out of range")
    for i in (1, 3, 5, 11):                                         # ldy, ldmu, ldsc, ldh
        refused(L.clc_quantize_build_indexes(*swap(qbi, i, C - 1)), "clc_quantize_build_indexes: a leading dimension is below C = 4")

    # the step twins and the sweep: what tests/test_qstep_kernels_gpu.py does not reach
    sfwd = (p, C, p, C, p, C, p, C, p, p, C, p, C, rows, C, 0, None, 0, st)
    for i in (0, 2, 4, 9):
        refused(L.clc_gauss_lik_step_fwd(*swap(sfwd, i, None)), "clc_gauss_lik_step_fwd: y, mu, scale or lik is NULL")
    for i in (1, 3, 5, 7, 10, 12):
        refused(L.clc_gauss_lik_step_fwd(*swap(sfwd, i, C - 1)), "clc_gauss_lik_step_fwd: a leading dimension is below C = 4")
    need = L.clc_gauss_lik_step_bwd_workspace_bytes(rows, C)
    sbwd = (p, C, p, C, p, C, p, C, p, C, p, p, C, p, C, p, C, p, rows, C, 0, p, C, p, need, st)
    for i in (0, 2, 4, 6, 15):
        refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, i, None)), "clc_gauss_lik_step_bwd: dlik, y, mu, scale or dscale is NULL")
    for i in (10, 17):
        refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, i, None)), "clc_gauss_lik_step_bwd: step or dstep is NULL")
    refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, 20, 3)), "clc_gauss_lik_step_bwd: mode must be 0 (training) or 1 (eval) (got 3)")
    refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, 8, None)), "clc_gauss_lik_step_bwd: training mode needs noise")
    for i in (1, 3, 5, 7, 9, 12, 14, 16, 22):
        refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, i, C - 1)), "clc_gauss_lik_step_bwd: a leading dimension is below C = 4")
    refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, 23, None)), "clc_gauss_lik_step_bwd: ws must be 4-byte aligned")
    refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, 23, p + 2)), "clc_gauss_lik_step_bwd: ws must be 4-byte aligned")
    refused(L.clc_gauss_lik_step_bwd(*swap(sbwd, 24, need - 4)), f"ws_bytes >= clc_gauss_lik_step_bwd_workspace_bytes() = {need}")
    K, B = 2, 1
    wsn = L.clc_gauss_rate_sweep_workspace_bytes(B, rows, C, K)
    sw = (p, C, p, C, p, C, p, K, B, rows, C, p, p, wsn, st)
    for i in (0, 2, 4, 6, 11):
        refused(L.clc_gauss_rate_sweep(*swap(sw, i, None)), "clc_gauss_rate_sweep: y, mu, scale, steps or bits is NULL")
    for k in (0, 17):
        refused(L.clc_gauss_rate_sweep(*swap(sw, 7, k)), f"clc_gauss_rate_sweep: K must be 1 .. 16 candidates (got {k})")
    refused(L.clc_gauss_rate_sweep(*swap(sw, 8, 0)), "clc_gauss_rate_sweep: B must be 1 .. 65535")
    for i in (1, 3, 5):
        refused(L.clc_gauss_rate_sweep(*swap(sw, i, C - 1)), "clc_gauss_rate_sweep: a leading dimension is below C = 4")
    refused(L.clc_gauss_rate_sweep(*swap(sw, 12, None)), "clc_gauss_rate_sweep: ws must be 4-byte aligned")
    refused(L.clc_gauss_rate_sweep(*swap(sw, 12, p + 2)), "clc_gauss_rate_sweep: ws must be 4-byte aligned")
    refused(L.clc_gauss_rate_sweep(*swap(sw, 13, wsn - 4)), f"ws_bytes >= clc_gauss_rate_sweep_workspace_bytes() = {wsn}")
    torch.cuda.synchronize()
    assert float(i32.abs().max()) == 0 and float(t.abs().max()) == 0.0, "a refused call wrote something"
    # an operand that is absent is not looked at: eval takes no noise (ldn = 0), and y_hat, dy, dmu, dy_add may be NULL with ld = 0
    assert L.clc_gauss_lik_fwd(*swap(swap(swap(fwd, 14, 1), 6, None), 7, 0)) == 0
    assert L.clc_gauss_lik_fwd(*swap(swap(fwd, 10, None), 11, 0)) == 0
    assert L.clc_gauss_lik_bwd(*swap(swap(swap(swap(swap(swap(bwd, 10, None), 11, 0), 12, None), 13, 0), 19, None), 20, 0)) == 0
    torch.cuda.synchronize()
