"""The kernels of csrc/elementwise.hip, one launch per case, against the float64 statements of tests/elementwise_ref.py.

Held directly here: LayerNorm forward / backward (the three vector kernels, the one-wave-per-row kernel, paired launches, the parameter
reduce in line and deferred), clc_partial_reduce_batched, the rate-distortion loss path (clc_log2_sum_partials, clc_sqdiff_partials,
clc_sum_partials, clc_rd_combine, clc_rd_grad_scalars, clc_scaled_recip, clc_scaled_diff), clc_act_bwd, clc_unshuffle_act_bwd, clc_colsum,
clc_sum_n, clc_copy2d, clc_axpby, clc_gate_fwd / _bwd, the GDN re-parametrisation (forward, batched forward, backward), clc_stem_pack /
_unpack_add, clc_im2col_small, clc_maxpool2d and clc_adaptive_pool2d.

Conventions
  * operands are float32 tensors from seeded CPU generators (elementwise_ref's builders); the reference sees exactly those values in float64
  * every operand and result with a leading dimension lives in a Buf: wider than its slice, guard rows in front and behind, everything outside
    the slice holding one NaN bit pattern.  An operand read outside its slice poisons the result; after the launch every element outside a
    result's slice must still hold the pattern and no NaN may be inside
  * operations without arithmetic (copy2d, im2col_small, stem_pack, maxpool2d, adaptive max, the transposed GDN image, a lone IEEE multiply in
    the activation backward, sum_n against sequential float32 adds, LayerNorm of a constant row) are held bit for bit
  * everything else is held to the derived bounds of elementwise_ref (u = 2^-24: k u S elementwise, (n + k) u S for sums, LayerNorm with
    n = C times 1 + |mean| / std), libm callers to BUDGET x the bound.

libm budgets: worst error / bound of the kernel's formula in float32 torch on the CPU over the operands of these cases, measured by
test_elementwise_ref_cpu.py::test_libm_budgets_are_eight_times_the_float32_cpu_error, and the constant chosen (8 x, rounded up):
    ln_y          rsqrtf         0.1069   ->  0.86
    ln_rstd       rsqrtf         0.1453   ->  1.17
    halftanh_pre  tanhf          0.2468   ->  1.98
    gelu          exp2/rcp/erf   0.4566   ->  3.66
    gate_fwd      expf           0.2880   ->  2.31
    gate_da       expf           0.3507   ->  2.81
    gate_db       expf           0.2823   ->  2.26
    log2          log2f          0.3268   ->  2.62   per TERM, in units of 3 u |log2 x|; the sums over log2f terms are then held to the derived
                                                     (n + 3 x 2.62) u sum |log2 x| at factor 1: the error of a float32 sum against its worst-case
                                                     bound is a matter of cancellation (measured: 0.0019 and 0.00001 of it), not of log2f

Which LayerNorm kernel serves a call follows from its arguments alone (ln_fwd_impl / ln_bwd_impl):
    forward   layernorm_fwd_vec_kernel<C / 4> iff C in {64, 128, 256}, ldx % 4 == ldy % 4 == 0 and x, y, gamma, beta (gamma2, beta2) are
              16-byte aligned; else layernorm_fwd_kernel (one wave per row, C <= 512); a pair is refused unless it qualifies for the former
    backward  layernorm_bwd_vec_kernel<C / 4> iff C in {64, 128, 256}, ldx, lddy, lddx (ld_add) % 4 == 0 and x, dy, dx, gamma, the workspace
              (dx_add, gamma2) are 16-byte aligned; else layernorm_bwd_kernel
The case ids name the kernel meant ("vec64", "wave96"); Buf keeps slices 16-byte aligned whenever ld % 4 == 0 and offset == 0.
"""
import ctypes
import functools

import pytest
import torch

import elementwise_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = 0x7FC0BEEF   # a quiet NaN with a payload no arithmetic produces
CL = torch.channels_last


class Buf:
    """[rows, C] float32 at leading dimension ld inside a sentinel-filled device buffer with `guard` rows on either side"""

    def __init__(self, dev, rows, C, ld=None, data=None, offset=0, guard=2):
        self.rows, self.C, self.ld = rows, C, (ld or C)
        self.start = guard * self.ld + offset
        total = (rows + 2 * guard) * self.ld + offset
        self.t = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev).view(F32)
        if data is not None:
            assert tuple(data.shape) == (rows, C) and data.dtype == F32, (data.shape, rows, C)
            self.view().copy_(data.to(dev))
        self.ptr = self.t.data_ptr() + 4 * self.start

    def view(self):
        return torch.as_strided(self.t, (self.rows, self.C), (self.ld, 1), self.start)

    def read(self, what="result", partly=False):
        """the slice on the CPU; everything outside it must be untouched and nothing inside NaN (partly: a workspace, not written in full)"""
        host = self.t.cpu()
        outside = torch.ones(host.numel(), dtype=torch.bool)
        torch.as_strided(outside, (self.rows, self.C), (self.ld, 1), self.start).fill_(False)
        assert bool((host.view(torch.int32)[outside] == SENTINEL).all()), f"{what}: written outside its slice"
        got = torch.as_strided(host, (self.rows, self.C), (self.ld, 1), self.start).clone()
        assert partly or not torch.isnan(got).any(), f"{what}: NaN inside the slice"
        return got

    def untouched(self):
        return bool((self.t.view(torch.int32) == SENTINEL).all())


def vec(dev, data=None, n=None, pad=3):
    """a vector as a one-row Buf"""
    n = n if data is None else data.numel()
    return Buf(dev, 1, n, n + pad, None if data is None else data.reshape(1, n), guard=1)


def _lib():
    from clc_amd import ops

    return ops._L(), ops._stream()


def ok(rc):
    L, _ = _lib()
    assert rc == 0, (rc, L.clc_last_error())


def refused(rc, fragment):
    L, _ = _lib()
    assert rc < 0, "the call was accepted"
    msg = L.clc_last_error().decode()
    assert fragment in msg, msg


def held(name, got, ref, bound, factor=1.0):
    ratio = R.worst_ratio(got.reshape(ref.shape), ref, bound)
    print(f"{name}: worst error / bound {ratio:.4f} (allowed {factor})")
    assert ratio <= factor, f"{name}: error {ratio:.4f} x the bound, {factor} allowed"


def exact(name, got, ref64):
    assert R.bits_equal(got.reshape(ref64.shape), ref64), f"{name}: not bit-equal to the reference rounded to float32"


# =================================================================================================================== LayerNorm forward
def _ln_kernel(C, forced=False):
    return f"{'vec' if C in R.LN_VEC_C and not forced else 'wave'}{C}"


def _ln_lds(C, forced=False):
    """(ldx, ldy): multiples of 4 where the vector kernel is meant, odd ones on the one-wave-per-row kernel"""
    return (C + 4, C + 8) if C in R.LN_VEC_C and not forced else (C + 1, C + 3)


@functools.lru_cache(maxsize=4)
def _ln_case(C, rows):
    t = R.ln_inputs(C, rows)
    return t, {k: v.double() for k, v in t.items()}


LN_FWD = [(f"{_ln_kernel(C)}-r{rows}", C, rows, {}) for C, rows in R.LN_FWD_SHAPES] + [
    ("wave64-ldx66-r35", 64, 35, {"ldx": 66}),
    ("wave64-xoffset1-r35", 64, 35, {"xoff": 1}),
    ("vec64-nostats-r35", 64, 35, {"stats": False}),
    ("wave96-nostats-r35", 96, 35, {"stats": False}),
]


@pytest.mark.parametrize("name,C,rows,opt", LN_FWD, ids=[c[0] for c in LN_FWD])
def test_layernorm_fwd(dev, name, C, rows, opt):
    L, st = _lib()
    t, d = _ln_case(C, rows)
    ldx, ldy = _ln_lds(C)
    ldx = opt.get("ldx", ldx)
    x = Buf(dev, rows, C, ldx, t["x"], offset=opt.get("xoff", 0))
    y = Buf(dev, rows, C, ldy)
    gm, bt = t["gamma"].to(dev), t["beta"].to(dev)
    stats = opt.get("stats", True)
    mean, rstd = (vec(dev, n=rows), vec(dev, n=rows)) if stats else (None, None)
    ok(L.clc_layernorm_fwd(x.ptr, ldx, gm.data_ptr(), bt.data_ptr(), y.ptr, ldy, mean.ptr if stats else None, rstd.ptr if stats else None,
                           rows, C, st))
    f = R.ln_fwd_ref(d["x"], d["gamma"], d["beta"])
    held(f"ln fwd {name} y", y.read("y"), f["y"], f["by"], R.BUDGET["ln_y"])
    if stats:
        held(f"ln fwd {name} mean", mean.read("mean"), f["mean"], f["bmean"])
        held(f"ln fwd {name} rstd", rstd.read("rstd"), f["rstd"], f["brstd"], R.BUDGET["ln_rstd"])


@pytest.mark.parametrize("C", [3, 64, 96, 256])
def test_layernorm_fwd_constant_row_is_beta(dev, C):
    """x == 0.5 everywhere: the mean is exact, d == 0, and y == beta bit for bit — no NaN from the zero variance"""
    L, st = _lib()
    rows = 5
    ldx, ldy = _ln_lds(C)
    t, _ = _ln_case(C, 35)
    x, y = Buf(dev, rows, C, ldx, torch.full((rows, C), 0.5)), Buf(dev, rows, C, ldy)
    gm, bt = t["gamma"].to(dev), t["beta"].to(dev)
    mean, rstd = vec(dev, n=rows), vec(dev, n=rows)
    ok(L.clc_layernorm_fwd(x.ptr, ldx, gm.data_ptr(), bt.data_ptr(), y.ptr, ldy, mean.ptr, rstd.ptr, rows, C, st))
    exact("constant row", y.read("y"), t["beta"].double()[None, :].expand(rows, -1))
    assert torch.equal(mean.read("mean"), torch.full((1, rows), 0.5))


@pytest.mark.parametrize("half", [35, 1, 69])
@pytest.mark.parametrize("C", R.LN_VEC_C)
def test_layernorm_fwd_pair(dev, C, half):
    L, st = _lib()
    rows = 70
    t, d = _ln_case(C, rows)
    ldx, ldy = _ln_lds(C)
    x, y = Buf(dev, rows, C, ldx, t["x"]), Buf(dev, rows, C, ldy)
    p = [t[k].to(dev) for k in ("gamma", "beta", "gamma2", "beta2")]
    mean, rstd = vec(dev, n=rows), vec(dev, n=rows)
    ok(L.clc_layernorm_fwd_pair(x.ptr, ldx, p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(), half, y.ptr, ldy, mean.ptr,
                                rstd.ptr, rows, C, st))
    f = R.ln_fwd_ref(d["x"], d["gamma"], d["beta"], d["gamma2"], d["beta2"], half)
    held(f"ln fwd pair vec{C} half {half} y", y.read("y"), f["y"], f["by"], R.BUDGET["ln_y"])
    held(f"ln fwd pair vec{C} half {half} rstd", rstd.read("rstd"), f["rstd"], f["brstd"], R.BUDGET["ln_rstd"])


def test_layernorm_fwd_refusals(dev):
    L, st = _lib()
    rows = 5
    t, _ = _ln_case(64, 35)
    x, y = Buf(dev, rows, 520, 520), Buf(dev, rows, 520, 520)
    gm = torch.ones(520 + 4, device=dev)
    mean = vec(dev, n=rows)
    g, b = gm.data_ptr(), gm.data_ptr()
    refused(L.clc_layernorm_fwd(x.ptr, 520, g, b, y.ptr, 520, mean.ptr, None, rows, 64, st), "mean/rstd must both be given or both NULL")
    refused(L.clc_layernorm_fwd(x.ptr, 520, g, b, y.ptr, 520, None, mean.ptr, rows, 64, st), "mean/rstd must both be given or both NULL")
    refused(L.clc_layernorm_fwd(x.ptr, 520, g, b, y.ptr, 520, None, None, rows, 513, st), "C=513 too large")
    refused(L.clc_layernorm_fwd_pair(x.ptr, 520, g, b, g, b, 2, y.ptr, 520, None, None, rows, 96, st), "needs C in {64,128,256}")
    refused(L.clc_layernorm_fwd_pair(x.ptr, 520, g, b, g + 4, b, 2, y.ptr, 520, None, None, rows, 64, st), "16-B aligned operands")
    refused(L.clc_layernorm_fwd_pair(x.ptr + 4, 520, g, b, g, b, 2, y.ptr, 520, None, None, rows, 64, st), "16-B aligned operands")
    refused(L.clc_layernorm_fwd_pair(x.ptr, 520, g, b, g, b, rows, y.ptr, 520, None, None, rows, 64, st), "clc_layernorm_fwd_pair: bad args")
    assert y.untouched(), "a refused call wrote"
    x.view().fill_(1.0)
    ok(L.clc_layernorm_fwd(x.ptr, 520, g, b, y.ptr, 520, None, None, rows, 64, st))
    torch.cuda.synchronize()


# =================================================================================================================== LayerNorm backward
def _reduce_entry(partial_ptr, nblocks, n, out0, out1, split, accumulate):
    from clc_amd import lib

    e = lib.ReduceEntry()
    e.partial, e.nblocks, e.n, e.out0, e.out1, e.split, e.accumulate = partial_ptr, nblocks, n, out0, out1, split, accumulate
    return e


def _reduce(entries):
    from clc_amd import lib

    L, st = _lib()
    arr = (lib.ReduceEntry * len(entries))(*entries)
    return L.clc_partial_reduce_batched(arr, len(entries), st)


def _stats32(d):
    mu, rs = R.ln_stats(d["x"])
    return mu.to(F32), rs.to(F32)


def _ln_bwd_run(dev, C, rows, variant, half=None):
    """One backward launch.  variant: plain (no dx_add, gradients written), dadd_acc (dx_add with its own ld, gradients accumulated into
    pre-filled buffers), deferred (dgamma = dbeta = NULL, then clc_partial_reduce_batched over the workspace rows, accumulating)."""
    L, st = _lib()
    t, d = _ln_case(C, rows)
    paired = half is not None
    ldx, _ = _ln_lds(C)
    vecpath = C in R.LN_VEC_C
    lddy, lddx, ldadd = (C + 8, C + 12, C + 16) if vecpath else (C + 2, C + 3, C + 5)
    mu32, rs32 = _stats32(d)
    x, dy, dx = Buf(dev, rows, C, ldx, t["x"]), Buf(dev, rows, C, lddy, t["dy"]), Buf(dev, rows, C, lddx)
    use_add = variant != "plain"
    dadd = Buf(dev, rows, C, ldadd, t["dadd"]) if use_add else None
    mean, rstd = vec(dev, mu32), vec(dev, rs32)
    gm, gm2 = t["gamma"].to(dev), t["gamma2"].to(dev)
    accumulate = int(variant != "plain")
    nmod = 2 if paired else 1
    inits = [(R.rand(77 + k, C), R.rand(78 + k, C)) if accumulate else (None, None) for k in range(nmod)]
    outs = [(vec(dev, ig, n=C), vec(dev, ib, n=C)) for ig, ib in inits]
    nbytes = L.clc_layernorm_bwd_workspace_bytes(rows, C)
    assert nbytes % 4 == 0
    ws = Buf(dev, 1, nbytes // 4, guard=1)
    direct = variant != "deferred"
    ptrs = [(o[0].ptr, o[1].ptr) if direct else (None, None) for o in outs]
    if not paired:
        ok(L.clc_layernorm_bwd(dy.ptr, lddy, x.ptr, ldx, gm.data_ptr(), mean.ptr, rstd.ptr, dx.ptr, lddx, dadd.ptr if use_add else None, ldadd,
                               ptrs[0][0], ptrs[0][1], accumulate, rows, C, ws.ptr, nbytes, st))
    else:
        ok(L.clc_layernorm_bwd_pair(dy.ptr, lddy, x.ptr, ldx, gm.data_ptr(), gm2.data_ptr(), half, mean.ptr, rstd.ptr, dx.ptr, lddx,
                                    dadd.ptr if use_add else None, ldadd, ptrs[0][0], ptrs[0][1], ptrs[1][0], ptrs[1][1], accumulate, rows, C,
                                    ws.ptr, nbytes, st))
    if not direct:   # as ops._LayerNormFn.backward: module k owns the workspace rows [k per, (k + 1) per)
        nb = L.clc_layernorm_bwd_blocks(rows, int(paired))
        per = nb // nmod
        assert (nb + (0 if paired else 1)) * 2 * C * 4 <= nbytes
        ok(_reduce([_reduce_entry(ws.ptr + 4 * k * per * 2 * C, per, 2 * C, outs[k][0].ptr, outs[k][1].ptr, C, 1) for k in range(nmod)]))
    b = R.ln_bwd_ref(d["x"], d["gamma"], d["dy"], d["dadd"] if use_add else None, d["gamma2"] if paired else None, half or 0)
    tag = f"ln bwd {_ln_kernel(C)} r{rows} {variant}" + (f" half {half}" if paired else "")
    held(f"{tag} dx", dx.read("dx"), b["dx"], b["bdx"])
    ws.read("workspace", partly=True)   # (nothing behind the workspace's last byte was written)
    for k, p in enumerate(b["params"]):
        ig, ib = (inits[k][0].double(), inits[k][1].double()) if accumulate else (None, None)
        held(f"{tag} dgamma{k}", outs[k][0].read("dgamma"), p["dgamma"] + (ig if accumulate else 0), R.ln_param_bound(p, "dgamma", ig))
        held(f"{tag} dbeta{k}", outs[k][1].read("dbeta"), p["dbeta"] + (ib if accumulate else 0), R.ln_param_bound(p, "dbeta", ib))


@pytest.mark.parametrize("variant", ["plain", "dadd_acc", "deferred"])
@pytest.mark.parametrize("C,rows", R.LN_BWD_SHAPES, ids=[f"{_ln_kernel(C)}-r{r}" for C, r in R.LN_BWD_SHAPES])
def test_layernorm_bwd(dev, C, rows, variant):
    _ln_bwd_run(dev, C, rows, variant)


@pytest.mark.parametrize("variant", ["plain", "dadd_acc", "deferred"])
@pytest.mark.parametrize("rows,half", [(70, 35), (10, 3)])
@pytest.mark.parametrize("C", R.LN_VEC_C)
def test_layernorm_bwd_pair(dev, C, rows, half, variant):
    """(10, 3): one 16-row block would do, the pair rounds the grid up to two — one per module"""
    _ln_bwd_run(dev, C, rows, variant, half=half)


def test_layernorm_bwd_forced_wave_kernel_and_refusals(dev):
    """C = 64 on operands the vector kernel cannot take (dy one float off 16-byte alignment), then what the entry point refuses"""
    L, st = _lib()
    C, rows = 64, 35
    t, d = _ln_case(C, rows)
    mu32, rs32 = _stats32(d)
    x, dy, dx = Buf(dev, rows, C, 68, t["x"]), Buf(dev, rows, C, 68, t["dy"], offset=1), Buf(dev, rows, C, 72)
    mean, rstd, gm = vec(dev, mu32), vec(dev, rs32), t["gamma"].to(dev)
    dg, db = vec(dev, n=C), vec(dev, n=C)
    need, nbytes = L.clc_layernorm_bwd_workspace_bytes(rows, C), L.clc_layernorm_bwd_workspace_bytes(rows, 96)   # (room for the C = 96 refusal)
    ws = Buf(dev, 1, nbytes // 4, guard=1)
    args = lambda **kw: [kw.get("dy", dy.ptr), 68, x.ptr, 68, gm.data_ptr(), mean.ptr, rstd.ptr, dx.ptr, 72, None, 0, kw.get("dg", dg.ptr), db.ptr, 0,
                         rows, kw.get("C", C), ws.ptr, kw.get("nbytes", nbytes), st]
    ok(L.clc_layernorm_bwd(*args()))
    b = R.ln_bwd_ref(d["x"], d["gamma"], d["dy"])
    held("ln bwd wave64-dyoffset1 dx", dx.read("dx"), b["dx"], b["bdx"])
    held("ln bwd wave64-dyoffset1 dgamma", dg.read("dgamma"), b["params"][0]["dgamma"], R.ln_param_bound(b["params"][0], "dgamma"))
    held("ln bwd wave64-dyoffset1 dbeta", db.read("dbeta"), b["params"][0]["dbeta"], R.ln_param_bound(b["params"][0], "dbeta"))
    refused(L.clc_layernorm_bwd(*args(dg=None)), "clc_layernorm_bwd: bad args")
    refused(L.clc_layernorm_bwd(*args(C=513)), "C=513 too large")
    refused(L.clc_layernorm_bwd(*args(nbytes=need - 1)), "workspace too small")
    pair = lambda **kw: [kw.get("dy", dy.ptr - 4), 68, x.ptr, 68, gm.data_ptr(), gm.data_ptr(), kw.get("half", 3), mean.ptr, rstd.ptr, dx.ptr, 72, None, 0,
                         dg.ptr, db.ptr, dg.ptr, db.ptr, 0, rows, kw.get("C", C), ws.ptr, nbytes, st]
    refused(L.clc_layernorm_bwd_pair(*pair(dy=dy.ptr)), "16-B aligned operands")
    refused(L.clc_layernorm_bwd_pair(*pair(C=96)), "needs C in {64,128,256}")
    refused(L.clc_layernorm_bwd_pair(*pair(half=rows)), "clc_layernorm_bwd_pair: bad args")
    ok(L.clc_layernorm_bwd(*args()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("C,folded", [(96, True), (256, False)], ids=["wave96-fold_in-grad_slot", "vec256"])
def test_layernorm_through_ops(dev, C, folded):
    """ops.layernorm on a 1x5x7 map: its own forward statistics feed the backward; with fold_in the parked residual gradient is added to dx
    and with grad_slot dx lands in channels [16, 16 + C) of a wider gradient buffer (lddx > C)"""
    from clc_amd import ops

    rows = 35
    t, d = _ln_case(C, rows)
    nchw = lambda m: m.reshape(1, 5, 7, C).permute(0, 3, 1, 2)
    x = nchw(t["x"]).to(dev).contiguous(memory_format=CL).requires_grad_()
    gm, bt = t["gamma"].to(dev).requires_grad_(), t["beta"].to(dev).requires_grad_()
    fold, slots = (ops.GradFold(), ops.GradSlots()) if folded else (None, None)
    y = ops.layernorm(x, gm, bt, fold, (slots, C + 32, 16) if folded else None)
    if folded:
        assert fold.park(nchw(t["dadd"]).to(dev).contiguous(memory_format=CL))
    y.backward(nchw(t["dy"]).to(dev).contiguous(memory_format=CL))
    f = R.ln_fwd_ref(d["x"], d["gamma"], d["beta"])
    b = R.ln_bwd_ref(d["x"], d["gamma"], d["dy"], d["dadd"] if folded else None)
    flat = lambda g: g.detach().permute(0, 2, 3, 1).reshape(rows, C).cpu()
    held(f"ops.layernorm C{C} y", flat(y), f["y"], f["by"], R.BUDGET["ln_y"])
    # the statistics are the forward kernel's own here, not the rounded exact ones: their budgeted error, carried through, joins the bounds
    cdx, cdg = R.ln_bwd_carried(d["x"], d["gamma"], d["dy"])
    held(f"ops.layernorm C{C} dx", flat(x.grad), b["dx"], b["bdx"] + cdx)
    p = b["params"][0]
    held(f"ops.layernorm C{C} dgamma", gm.grad.cpu(), p["dgamma"], R.ln_param_bound(p, "dgamma") + cdg)
    held(f"ops.layernorm C{C} dbeta", bt.grad.cpu(), p["dbeta"], R.ln_param_bound(p, "dbeta"))
    if folded:
        assert slots.buf is not None and slots.buf.shape[1] == C + 32 and torch.equal(slots.buf[:, 16:16 + C], x.grad)


# =================================================================================================================== clc_partial_reduce_batched
PR_N, PR_NB = (1, 31, 33, 130), (1, 7, 9, 40)


def _pr_entry(dev, i):
    """entry i of a table: every n x nblocks pair, the three split modes, both accumulate modes and a partial offset come round within 48"""
    n, nb = PR_N[i % 4], PR_NB[(i // 4) % 4]
    mode = (i // 16) % 3 if n > 1 else (i // 16) % 2 * 2      # 0: split 0 (all to out1), 1: inside, 2: >= n with out1 NULL
    split = {0: 0, 1: n // 2, 2: n + (i % 3)}[mode]
    accumulate, offset = (i // 16 + i) % 2, (5 if i % 5 < 2 else 0)
    part = R.rand(4000 + i, nb, n)
    pbuf = Buf(dev, 1, nb * n + offset, guard=1)
    pbuf.view()[0, offset:] = part.reshape(-1).to(dev)
    pbuf.view()[0, :offset] = 0.0
    n0, n1 = min(split, n), n - min(split, n)
    init0, init1 = R.rand(5000 + i, max(n0, 1)), R.rand(6000 + i, max(n1, 1))
    out0 = vec(dev, init0 if accumulate and n0 else None, n=max(n0, 1))     # (out0 must be given even when split == 0 sends it nothing)
    out1 = vec(dev, init1 if accumulate else None, n=max(n1, 1)) if mode != 2 else None
    e = _reduce_entry(pbuf.ptr + 4 * offset, nb, n, out0.ptr, out1.ptr if out1 is not None else None, split, accumulate)
    init = torch.cat((init0[:n0], init1[:n1])).double() if accumulate else None
    ref, bound = R.partial_reduce_ref(part.double(), init)
    return e, (pbuf, out0, out1, n0, n1, accumulate, ref, bound)


@pytest.mark.parametrize("count", [1, 64, 65, 130])
def test_partial_reduce_batched(dev, count):
    made = [_pr_entry(dev, i if count > 1 else 21) for i in range(count)]
    ok(_reduce([m[0] for m in made]))
    worst = 0.0
    for i, (_e, (pbuf, out0, out1, n0, n1, accumulate, ref, bound)) in enumerate(made):
        if n0:
            got0 = out0.read(f"entry {i} out0")[0]
        else:   # nothing of this entry goes to out0: it must be untouched
            assert out0.untouched(), f"entry {i}: split == 0 wrote to out0"
            got0 = torch.empty(0)
        got1 = out1.read(f"entry {i} out1")[0] if n1 else torch.empty(0)
        got = torch.cat((got0[:n0], got1[:n1]))
        worst = max(worst, R.worst_ratio(got, ref, bound))
    print(f"partial reduce, {count} entries: worst error / bound {worst:.4f}")
    assert worst <= 1.0


def test_partial_reduce_refusals_name_the_entry(dev):
    good = lambda i: _pr_entry(dev, i)
    keep = [good(i) for i in range(66)]
    es = [k[0] for k in keep]

    def broken(i, **kw):
        tab = list(es[: i + 1])
        e = _reduce_entry(tab[i].partial, tab[i].nblocks, tab[i].n, tab[i].out0, tab[i].out1, tab[i].split, tab[i].accumulate)
        for k, v in kw.items():
            setattr(e, k, v)
        tab[i] = e
        return tab

    refused(_reduce(broken(0, nblocks=0)), "bad entry 0")
    refused(_reduce(broken(2, n=0)), "bad entry 2")
    refused(_reduce(broken(65, split=0, out1=None, n=33)), "bad entry 65")
    from clc_amd import lib

    L, st = _lib()
    refused(L.clc_partial_reduce_batched((lib.ReduceEntry * 1)(es[0]), 0, st), "clc_partial_reduce_batched: bad args")
    ok(_reduce(es[:3]))
    torch.cuda.synchronize()


# =================================================================================================================== the loss path
LMBDA = 0.0067


def _lik_dev(dev, name, sliced):
    """a likelihood map as a logical-NCHW pixel-major leaf; sliced: channels [4, 4 + C) of a NaN-filled buffer 8 wider (ld = C + 8)"""
    lik = R.lik_inputs(name)                      # [N, H, W, C]
    N, H, W, C = lik.shape
    if not sliced:
        return lik, lik.permute(0, 3, 1, 2).to(dev).contiguous(memory_format=CL).requires_grad_()
    buf = torch.full((N, C + 8, H, W), float("nan"), device=dev).contiguous(memory_format=CL)
    buf[:, 4:4 + C] = lik.permute(0, 3, 1, 2).to(dev)
    leaf = buf[:, 4:4 + C].detach().requires_grad_()
    assert leaf.stride(1) == 1 and leaf.stride(3) == C + 8
    return lik, leaf


def _nhwc_cpu(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu()


GRAD_COMBOS = [(1.0, None, None), (None, 0.5, None), (None, None, 2.0), (1.0, -0.5, None), (0.25, None, 2.0), (None, 0.5, -2.0), (1.0, 0.5, 2.0)]


@pytest.mark.parametrize("grads", GRAD_COMBOS, ids=["bpp", "mse", "loss", "bpp+mse", "bpp+loss", "mse+loss", "all"])
@pytest.mark.parametrize("order", ["small-wide", "wide-small"])
def test_rd_loss_mse(dev, order, grads):
    from clc_amd import ops

    ky, kz = ("small", "wide") if order == "small-wide" else ("wide", "small")
    ly, lyd = _lik_dev(dev, ky, sliced=(ky == "wide"))
    lz, lzd = _lik_dev(dev, kz, sliced=(kz == "wide"))
    xh, tg = R.img_inputs()
    xhd = xh.permute(0, 3, 1, 2).to(dev).contiguous(memory_format=CL).requires_grad_()
    tgd = tg.permute(0, 3, 1, 2).to(dev).contiguous(memory_format=CL)
    P = tg.shape[0] * tg.shape[1] * tg.shape[2]
    outs = ops.rd_loss_mse(lyd, lzd, xhd, tgd, LMBDA, P)
    a = [t.double() for t in (ly, lz, xh, tg)]
    ref, bounds = R.rd_loss_ref(*a, LMBDA, P), R.rd_loss_bounds(*a, LMBDA, P)
    for name, o, r, b in zip(("bpp", "mse", "loss"), outs, ref, bounds):
        held(f"rd_loss {order} {name}", o.detach().cpu().reshape(()), r, b)
    sum(g * o for g, o in zip(grads, outs) if g is not None).backward()
    r = R.rd_grads_ref(*a, LMBDA, P, *grads)
    held(f"rd_loss {order} d lik_y", _nhwc_cpu(lyd.grad), r["dy"], r["bdy"])
    held(f"rd_loss {order} d lik_z", _nhwc_cpu(lzd.grad), r["dz"], r["bdz"])
    held(f"rd_loss {order} d x_hat", _nhwc_cpu(xhd.grad), r["dx"], r["bdx"])


@pytest.mark.parametrize("name", ["small", "wide"])
def test_sum_log2_and_sqdiff_sum(dev, name):
    from clc_amd import ops

    lik, likd = _lik_dev(dev, name, sliced=(name == "wide"))
    out = ops.sum_log2(likd)
    ref, bound = R.sum_log2_ref(lik.double())
    held(f"sum_log2 {name}", out.detach().cpu(), ref, bound)
    (out * 0.75).backward()
    r, b = R.scaled_recip_ref(lik.double(), 0.75, R.INV_LN2_32)
    held(f"sum_log2 {name} backward", _nhwc_cpu(likd.grad), r, b)
    xh, tg = R.img_inputs()
    xhd = xh.permute(0, 3, 1, 2).to(dev).contiguous(memory_format=CL).requires_grad_()
    out = ops.sqdiff_sum(xhd, tg.permute(0, 3, 1, 2).to(dev).contiguous(memory_format=CL))
    ref, bound = R.sqdiff_sum_ref(xh.double(), tg.double())
    held("sqdiff_sum", out.detach().cpu(), ref, bound)
    (out * -1.5).backward()
    r, b = R.scaled_diff_ref(xh.double(), tg.double(), -1.5, 2.0)
    held("sqdiff_sum backward", _nhwc_cpu(xhd.grad), r, b)


@pytest.mark.parametrize("n_partials", [1, 2048, "tail"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_log2_and_sqdiff_partials_raw(dev, name, n_partials):
    """any number of partials up to 2048: blocks that get no element write 0, and the partials add up to the sum"""
    L, st = _lib()
    lik = R.lik_inputs(name)
    N, H, W, C = lik.shape
    rows, ld = N * H * W, C + 3
    used = (rows * C + 255) // 256
    nparts = used + 3 if n_partials == "tail" else n_partials
    x = Buf(dev, rows, C, ld, lik.reshape(rows, C))
    part = vec(dev, n=nparts)
    ok(L.clc_log2_sum_partials(x.ptr, ld, rows, C, part.ptr, nparts, st))
    got = part.read("log2 partials")[0]
    assert float(got[used:].abs().sum()) == 0.0 and bool((got[used:].view(torch.int32) == 0).all()), "an empty block must write +0"
    ref, bound = R.sum_log2_ref(lik.double())
    held(f"log2 partials {name} x{nparts}", got.double().sum(), ref, bound)
    # the same through a strided result of clc_scaled_recip (ldo > C)
    g = torch.tensor([-0.375], device=dev)
    out = Buf(dev, rows, C, C + 5)
    ok(L.clc_scaled_recip(x.ptr, ld, rows, C, g.data_ptr(), 1.25, out.ptr, C + 5, st))
    r, b = R.scaled_recip_ref(lik.double().reshape(rows, C), -0.375, 1.25)
    held(f"scaled_recip {name}", out.read("scaled_recip"), r, b)
    a, b_ = R.img_inputs()
    n = a.numel()
    used = (n + 255) // 256
    nparts = used + 3 if n_partials == "tail" else n_partials
    av, bv, part = vec(dev, a.reshape(-1)), vec(dev, b_.reshape(-1)), vec(dev, n=nparts)
    ok(L.clc_sqdiff_partials(av.ptr, bv.ptr, n, part.ptr, nparts, st))
    got = part.read("sqdiff partials")[0]
    assert bool((got[used:].view(torch.int32) == 0).all()), "an empty block must write +0"
    ref, bound = R.sqdiff_sum_ref(a.double(), b_.double())
    held(f"sqdiff partials x{nparts}", got.double().sum(), ref, bound)
    # clc_sum_partials over them, scaled and accumulated
    out = vec(dev, torch.tensor([3.0]))
    ok(L.clc_sum_partials(part.ptr, nparts, -0.5, out.ptr, 1, st))
    S = got.double().abs().sum()
    held(f"sum_partials x{nparts}", out.read("sum")[0], (3.0 - 0.5 * got.double().sum()).reshape(1), (nparts + 3) * R.U * (3.0 + 0.5 * S) + R.TINY)


def test_loss_path_refusals(dev):
    L, st = _lib()
    x, part = vec(dev, torch.ones(64)), vec(dev, n=2049)
    refused(L.clc_log2_sum_partials(x.ptr, 8, 8, 8, part.ptr, 2049, st), "clc_log2_sum_partials: bad args")
    refused(L.clc_sqdiff_partials(x.ptr, x.ptr, 64, part.ptr, 2049, st), "clc_sqdiff_partials: bad args")
    refused(L.clc_sqdiff_partials(x.ptr, x.ptr, 64, part.ptr, 0, st), "clc_sqdiff_partials: bad args")
    refused(L.clc_sum_partials(x.ptr, 0, 1.0, part.ptr, 0, st), "clc_sum_partials: bad args")
    refused(L.clc_rd_combine(x.ptr, 1, x.ptr, 1, x.ptr, 1, 5.0, 3.0, 1.0, part.ptr, part.ptr, part.ptr, st), "clc_rd_combine: bad args")
    refused(L.clc_rd_grad_scalars(None, None, x.ptr, -5.0, 0.0, 1.0, part.ptr, part.ptr, st), "clc_rd_grad_scalars: bad args")
    assert part.untouched()
    part = vec(dev, n=2048)
    ok(L.clc_sqdiff_partials(x.ptr, x.ptr, 64, part.ptr, 2048, st))
    assert float(part.read("partials").abs().sum()) == 0.0


@pytest.mark.parametrize("grads", GRAD_COMBOS, ids=["bpp", "mse", "loss", "bpp+mse", "bpp+loss", "mse+loss", "all"])
def test_rd_grad_scalars_null_gradients(dev, grads):
    """g_* == NULL is "no gradient arrived": g_logsum = (g_loss + g_bpp) / -P, g_sq = (g_loss c + g_mse) / numel"""
    L, st = _lib()
    c32 = float(torch.tensor(LMBDA * 255 ** 2, dtype=F32))
    gd = [None if g is None else torch.tensor([g], device=dev) for g in grads]
    out = vec(dev, n=2)
    ok(L.clc_rd_grad_scalars(*[None if g is None else g.data_ptr() for g in gd], -323.0, 969.0, c32, out.ptr, out.ptr + 4, st))
    gb, gm, gl = (0.0 if g is None else g for g in grads)
    ref = torch.tensor([(gl + gb) / -323.0, (gl * c32 + gm) / 969.0], dtype=F64)
    bound = torch.tensor([4 * R.U * (abs(gl) + abs(gb)) / 323.0, 5 * R.U * (abs(gl * c32) + abs(gm)) / 969.0], dtype=F64) + R.TINY
    held("rd_grad_scalars", out.read("scalars")[0], ref, bound)


@pytest.mark.parametrize("ns", [(1, 1, 1), (7, 300, 1024), (2048, 255, 257)])
def test_rd_combine_is_three_sum_partials_and_the_reference_expression_bit_for_bit(dev, ns):
    L, st = _lib()
    parts = [vec(dev, R.rand(8000 + n + k, n, scale=40.0, shift=(-300.0 if k < 2 else 200.0))) for k, n in enumerate(ns)]
    sums = []
    for p, n in zip(parts, ns):
        o = vec(dev, n=1)
        ok(L.clc_sum_partials(p.ptr, n, 1.0, o.ptr, 0, st))
        sums.append(o.read("sum")[0, 0])
    neg, numel, c = -323.0, 969.0, float(torch.tensor(LMBDA * 255 ** 2, dtype=F32))
    out = [vec(dev, n=1) for _ in range(3)]
    ok(L.clc_rd_combine(parts[0].ptr, ns[0], parts[1].ptr, ns[1], parts[2].ptr, ns[2], neg, numel, c, out[0].ptr, out[1].ptr, out[2].ptr, st))
    sy, sz, sq = sums
    f = lambda v: torch.tensor(v, dtype=F32)
    bpp = (sy + sz) / f(neg)          # float32 torch on the CPU: every operation rounded once, as the reference's tensor expressions
    mse = sq / f(numel)
    loss = f(c) * mse + bpp
    for name, o, want in zip(("bpp", "mse", "loss"), out, (bpp, mse, loss)):
        got = o.read(name)[0, 0]
        assert got.view(torch.int32) == want.view(torch.int32), (name, float(got), float(want))


# =================================================================================================================== activation backward
def _mode_id(m):
    return "none" if m is None else f"act{m[0]}-pre{m[1]}"


@pytest.mark.parametrize("mode", R.ACT_MODES, ids=_mode_id)
@pytest.mark.parametrize("rows,C", R.ACT_SHAPES)
def test_act_bwd(dev, rows, C, mode):
    L, st = _lib()
    act, use_pre = mode
    dy, saved = R.act_inputs(rows, C)
    lddy, lds, lddz = C + 1, C + 2, C + 3
    d, s, z = Buf(dev, rows, C, lddy, dy), Buf(dev, rows, C, lds, saved), Buf(dev, rows, C, lddz)
    ok(L.clc_act_bwd(d.ptr, lddy, s.ptr, lds, use_pre, act, z.ptr, lddz, rows, C, st))
    ref, bound = R.act_bwd_ref(dy.double(), saved.double(), act, use_pre)
    if R.act_exact(act, use_pre):
        exact(f"act_bwd {_mode_id(mode)} {rows}x{C}", z.read("dz"), ref)
    else:
        held(f"act_bwd {_mode_id(mode)} {rows}x{C}", z.read("dz"), ref, bound, R.act_budget(act, use_pre))


@pytest.mark.parametrize("mode", [None] + R.ACT_MODES, ids=_mode_id)
@pytest.mark.parametrize("shape", R.UNSHUFFLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unshuffle_act_bwd(dev, shape, mode):
    L, st = _lib()
    N, H, W, C = shape
    Q, rows = C // 4, N * 2 * H * 2 * W
    act, use_pre = mode if mode is not None else (R.ACT_RELU, 1)   # (ignored without saved)
    dy, saved = R.act_inputs(rows, Q)
    lddy, lds = Q + 1, Q + 3
    d, s = Buf(dev, rows, Q, lddy, dy), Buf(dev, rows, Q, lds, saved)
    z = Buf(dev, N * H * W, C)
    ok(L.clc_unshuffle_act_bwd(d.ptr, lddy, s.ptr if mode is not None else None, lds, use_pre, act, z.ptr, N, H, W, C, st))
    if mode is None:
        ref, bound = dy.double(), None
    else:
        ref, bound = R.act_bwd_ref(dy.double(), saved.double(), act, use_pre)
    ref = R.unshuffle_ref(ref.reshape(N, 2 * H, 2 * W, Q)).reshape(N * H * W, C)
    name = f"unshuffle_act_bwd {_mode_id(mode)} {shape}"
    if R.act_exact(act, use_pre, has_saved=mode is not None):
        exact(name, z.read("dz"), ref)
    else:
        bound = R.unshuffle_ref(bound.reshape(N, 2 * H, 2 * W, Q)).reshape(N * H * W, C)
        held(name, z.read("dz"), ref, bound, R.act_budget(act, use_pre))


def test_act_bwd_through_ops_and_refusals(dev):
    from clc_amd import ops

    L, st = _lib()
    N, H, W, Q = 2, 6, 10, 2
    dy, saved = R.act_inputs(N * H * W, Q, seed_base=9)
    wide = lambda m: torch.full((N, Q + 6, H, W), float("nan"), device=dev).contiguous(memory_format=CL)
    dyb, svb = wide(dy), wide(saved)
    dyb[:, 1:1 + Q] = dy.reshape(N, H, W, Q).permute(0, 3, 1, 2).to(dev)
    svb[:, 3:3 + Q] = saved.reshape(N, H, W, Q).permute(0, 3, 1, 2).to(dev)
    ref, _ = R.act_bwd_ref(dy.double(), saved.double(), R.ACT_LRELU, 1)
    dz = ops.act_bwd(dyb[:, 1:1 + Q], svb[:, 3:3 + Q], True, R.ACT_LRELU)
    exact("ops.act_bwd", _nhwc_cpu(dz).reshape(-1, Q), ref)
    dz = ops.unshuffle_act_bwd(dyb[:, 1:1 + Q], svb[:, 3:3 + Q], True, R.ACT_LRELU)
    exact("ops.unshuffle_act_bwd", _nhwc_cpu(dz), R.unshuffle_ref(ref.reshape(N, H, W, Q)))
    d, z = Buf(dev, 8, 8, 8, torch.ones(8, 8)), Buf(dev, 8, 8, 8)
    refused(L.clc_act_bwd(d.ptr, 8, d.ptr, 8, 0, R.ACT_GELU, z.ptr, 8, 8, 8, st), "GELU needs the pre-activation")
    refused(L.clc_act_bwd(d.ptr, 8, d.ptr, 8, 1, R.ACT_SIGMOID, z.ptr, 8, 8, 8, st), "unsupported activation 5")
    refused(L.clc_unshuffle_act_bwd(d.ptr, 8, None, 0, 1, R.ACT_NONE, z.ptr, 1, 2, 2, 6, st), "clc_unshuffle_act_bwd: bad args")
    refused(L.clc_unshuffle_act_bwd(d.ptr, 1, None, 0, 1, R.ACT_NONE, z.ptr, 1, 2, 2, 8, st), "bad leading dims")
    refused(L.clc_unshuffle_act_bwd(d.ptr, 8, None, 0, 1, R.ACT_NONE, z.ptr + 4, 1, 1, 1, 8, st), "bad leading dims / alignment")
    assert z.untouched()
    ok(L.clc_act_bwd(d.ptr, 8, d.ptr, 8, 1, R.ACT_GELU, z.ptr, 8, 8, 8, st))
    z.read("dz")


# =================================================================================================================== column sums, sums, copies
COLSUM = [(r, C) for r in (1, 255, 257, 1000) for C in (1, 3, 64, 300)] + [(512 * 256 + 3, 3)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,C", COLSUM)
def test_colsum(dev, rows, C, accumulate):
    L, st = _lib()
    x = R.rand(rows + C, rows, C, shift=0.25)
    init = R.rand(11, C) if accumulate else None
    ld = C + 3
    xb, out = Buf(dev, rows, C, ld, x), vec(dev, init, n=C)
    nbytes = L.clc_colsum_workspace_bytes(rows, C)
    ws = Buf(dev, 1, (nbytes + 3) // 4, guard=1)
    if (rows, C) == (257, 3):
        refused(L.clc_colsum(xb.ptr, ld, rows, C, out.ptr, accumulate, ws.ptr, nbytes - 1, st), "workspace too small")
    ok(L.clc_colsum(xb.ptr, ld, rows, C, out.ptr, accumulate, ws.ptr, nbytes, st))
    ref, bound = R.colsum_ref(x.double(), None if init is None else init.double())
    held(f"colsum {rows}x{C} acc {accumulate}", out.read("colsum")[0], ref, bound)
    ws.read("workspace", partly=True)


def test_colsum_through_ops(dev):
    from clc_amd import ops

    x = R.rand(5, 2 * 5 * 7, 20)
    buf = torch.full((2, 28, 5, 7), float("nan"), device=dev).contiguous(memory_format=CL)
    buf[:, 4:24] = x.reshape(2, 5, 7, 20).permute(0, 3, 1, 2).to(dev)
    ref, bound = R.colsum_ref(x.double())
    held("ops.colsum", ops.colsum(buf[:, 4:24]).cpu(), ref, bound)


@pytest.mark.parametrize("rows", [1, 35])
@pytest.mark.parametrize("C", [4, 20])
@pytest.mark.parametrize("n", [1, 2, 3, 12])
def test_sum_n(dev, n, C, rows):
    from clc_amd import lib

    L, st = _lib()
    srcs = [R.rand(300 + 13 * k + C, rows, C, scale=10.0 ** (k % 4 - 1)) for k in range(n)]
    lds = [C + 4 * (k + 1) for k in range(n)]
    bufs = [Buf(dev, rows, C, ld, s) for s, ld in zip(srcs, lds)]
    ldd = C + 4 * (n + 2)
    dst = Buf(dev, rows, C, ldd)
    ok(L.clc_sum_n(lib.ptr_array([b.ptr for b in bufs]), (ctypes.c_int * n)(*lds), n, dst.ptr, ldd, rows, C, st))
    assert torch.equal(dst.read("sum_n").view(torch.int32), R.sum_n_f32(srcs).view(torch.int32)), "not the sequential float32 sum"


def test_sum_n_through_fanout_and_refusals(dev):
    from clc_amd import lib, ops

    L, st = _lib()
    x = R.rand(1, 1, 20, 5, 7).to(dev).contiguous(memory_format=CL).requires_grad_()
    ws = [R.rand(40 + k, 1, 20, 5, 7, scale=10.0 ** (k - 1)) for k in range(3)]
    outs = ops.fanout(x, 3)
    sum((o * w.to(dev).contiguous(memory_format=CL)).sum() for o, w in zip(outs, ws)).backward()
    assert torch.equal(x.grad.cpu(), R.sum_n_f32(ws)), "fanout's backward is not ((g0 + g1) + g2)"
    bufs = [Buf(dev, 4, 8, 12, torch.ones(4, 8)) for _ in range(13)]
    dst = Buf(dev, 4, 8, 12)
    arr = lambda ps: lib.ptr_array(ps)
    ints = lambda n, v=12: (ctypes.c_int * n)(*([v] * n))
    ps = [b.ptr for b in bufs]
    refused(L.clc_sum_n(arr(ps), ints(13), 13, dst.ptr, 12, 4, 8, st), "clc_sum_n: bad args")
    refused(L.clc_sum_n(arr(ps[:2]), ints(2), 2, dst.ptr, 12, 4, 6, st), "clc_sum_n: bad args")
    refused(L.clc_sum_n(arr([ps[0], ps[1] + 4]), ints(2), 2, dst.ptr, 12, 4, 8, st), "source 1 unaligned")
    refused(L.clc_sum_n(arr(ps[:2]), ints(2, 10), 2, dst.ptr, 12, 4, 8, st), "source 0 unaligned")
    assert dst.untouched()
    ok(L.clc_sum_n(arr(ps[:12]), ints(12), 12, dst.ptr, 12, 4, 8, st))
    assert torch.equal(dst.read("sum_n"), torch.full((4, 8), 12.0))


@pytest.mark.parametrize("C", [1, 7, 64])
def test_copy2d(dev, C):
    L, st = _lib()
    rows = 35
    x = R.rand(60 + C, rows, C)
    x.view(-1)[:2] = torch.tensor([-0.0, float("inf")])[: min(2, x.numel())]
    src, dst = Buf(dev, rows, C, C + 2, x), Buf(dev, rows, C, C + 5)
    ok(L.clc_copy2d(src.ptr, C + 2, dst.ptr, C + 5, rows, C, st))
    exact(f"copy2d C{C}", dst.read("copy"), x.double())
    refused(L.clc_copy2d(src.ptr, C + 2, None, C + 5, rows, C, st), "clc_copy2d: bad args")


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("n", [1, 1023, 4097])
def test_axpby(dev, n, with_b):
    L, st = _lib()
    a, b = R.rand(70 + n, n), R.rand(71 + n, n)
    av, bv, out = vec(dev, a), vec(dev, b), vec(dev, n=n)
    ok(L.clc_axpby(av.ptr, 0.75, bv.ptr if with_b else None, -1.5, out.ptr, n, st))
    ref, bound = R.axpby_ref(a.double(), 0.75, b.double() if with_b else None, -1.5)
    held(f"axpby n{n} b {with_b}", out.read("axpby")[0], ref, bound)


@pytest.mark.parametrize("which", ["n1-b+100", "n1-b-100", "n1023"])
def test_gate(dev, which):
    """a sigmoid(b) + idn and its backward; b = +-100 saturates expf (inf / 0): the result is finite and exact to the bound"""
    L, st = _lib()
    a, b, idn, g = {"n1-b+100": lambda: R.gate_inputs(1), "n1-b-100": R.gate_inputs_neg, "n1023": lambda: R.gate_inputs(1023)}[which]()
    n = a.numel()
    av, bv, iv, gv = (vec(dev, t) for t in (a, b, idn, g))
    out, da, db = vec(dev, n=n), vec(dev, n=n), vec(dev, n=n)
    ok(L.clc_gate_fwd(av.ptr, bv.ptr, iv.ptr, out.ptr, n, st))
    ok(L.clc_gate_bwd(gv.ptr, av.ptr, bv.ptr, da.ptr, db.ptr, n, st))
    y, by = R.gate_fwd_ref(a.double(), b.double(), idn.double())
    rda, bda, rdb, bdb = R.gate_bwd_ref(g.double(), a.double(), b.double())
    got = out.read("gate")[0]
    assert torch.isfinite(got).all()
    held(f"gate_fwd {which}", got, y, by, R.BUDGET["gate_fwd"])
    held(f"gate_bwd {which} da", da.read("da")[0], rda, bda, R.BUDGET["gate_da"])
    held(f"gate_bwd {which} db", db.read("db")[0], rdb, bdb, R.BUDGET["gate_db"])


# =================================================================================================================== GDN re-parametrisation
GDN_PED = 2.0 ** -36
GDN_GB = 2.0 ** -18
GDN_BB = float(torch.tensor((1e-6 + 2.0 ** -36) ** 0.5, dtype=F32))


def _gdn_fwd(dev, C):
    L, st = _lib()
    gamma, beta, dge, dbe = R.gdn_inputs(C, GDN_GB, GDN_BB)
    gv, bv = vec(dev, gamma.reshape(-1)), vec(dev, beta)
    ge, get, be = vec(dev, n=C * C), vec(dev, n=C * C), vec(dev, n=C)
    ok(L.clc_gdn_reparam_fwd(gv.ptr, bv.ptr, C, GDN_GB, GDN_BB, GDN_PED, ge.ptr, get.ptr, be.ptr, st))
    return (gamma, beta, dge, dbe), (gv, bv), (ge.read("gamma_eff")[0].reshape(C, C), get.read("gamma_eff_t")[0].reshape(C, C), be.read("beta_eff")[0])


@pytest.mark.parametrize("C", R.GDN_C)
def test_gdn_reparam_fwd(dev, C):
    (gamma, beta, _g, _b), _, (ge, get, be) = _gdn_fwd(dev, C)
    (rg, rgt, rb), (bg, bb) = R.gdn_reparam_fwd_ref(gamma.double(), beta.double(), GDN_GB, GDN_BB, GDN_PED)
    held(f"gdn reparam C{C} gamma_eff", ge, rg, bg)
    held(f"gdn reparam C{C} beta_eff", be, rb, bb)
    assert torch.equal(get.view(torch.int32), ge.t().contiguous().view(torch.int32)), "the transposed image is not the image transposed"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("C", R.GDN_C)
def test_gdn_reparam_bwd(dev, C, accumulate):
    L, st = _lib()
    gamma, beta, dge, dbe = R.gdn_inputs(C, GDN_GB, GDN_BB)
    ig, ib = (R.rand(91, C * C), R.rand(92, C)) if accumulate else (None, None)
    gv, bv, dgv, dbv = vec(dev, gamma.reshape(-1)), vec(dev, beta), vec(dev, dge.reshape(-1)), vec(dev, dbe)
    og, ob = vec(dev, ig, n=C * C), vec(dev, ib, n=C)
    ok(L.clc_gdn_reparam_bwd(gv.ptr, bv.ptr, C, GDN_GB, GDN_BB, dgv.ptr, dbv.ptr, og.ptr, ob.ptr, accumulate, st))
    for name, x, bound_, dy, init, got in (("dgamma", gamma.reshape(-1), GDN_GB, dge.reshape(-1), ig, og.read("dgamma")[0]),
                                           ("dbeta", beta, GDN_BB, dbe, ib, ob.read("dbeta")[0])):
        ref, bound, keep = R.gdn_reparam_bwd_ref(x.double(), bound_, dy.double(), None if init is None else init.double())
        held(f"gdn reparam bwd C{C} acc {accumulate} {name}", got, ref, bound)
        # a blocked gradient is exactly nothing: 0 written, or the pre-filled value unchanged
        blocked = ~keep
        want = init[blocked] if accumulate else torch.zeros(int(blocked.sum()))
        assert int(blocked.sum()) >= 1 and torch.equal(got[blocked], want), f"{name}: a gradient below the bound leaked"
        assert bool((got[:9][keep[:9]] != (init[:9][keep[:9]] if accumulate else 0)).any())   # the planted entries that pass do arrive


def test_gdn_reparam_fwd_batched_equals_single_launches(dev):
    from clc_amd import lib, ops

    L, st = _lib()
    Cs = (3, 192, 64)
    singles, entries, keep, first = [], [], [], 0
    for C in Cs:
        _in, (gv, bv), got = _gdn_fwd(dev, C)
        singles.append(got)
        ge, get, be = vec(dev, n=C * C), vec(dev, n=C * C), vec(dev, n=C)
        e = lib.GDNEntry()
        e.gamma, e.beta, e.gamma_eff, e.gamma_eff_t, e.beta_eff, e.C, e.first_block = gv.ptr, bv.ptr, ge.ptr, get.ptr, be.ptr, C, first
        e.gamma_bound, e.beta_bound, e.pedestal = GDN_GB, GDN_BB, GDN_PED
        first += (C * C + C + 255) // 256
        entries.append(e)
        keep.append((gv, bv, ge, get, be))
    table = ops._device_table(entries, lib.GDNEntry, dev)
    refused(L.clc_gdn_reparam_fwd_batched(table.data_ptr(), 0, first, st), "clc_gdn_reparam_fwd_batched: bad args")
    ok(L.clc_gdn_reparam_fwd_batched(table.data_ptr(), 3, first, st))
    for C, single, (_gv, _bv, ge, get, be) in zip(Cs, singles, keep):
        for name, one, many in zip(("gamma_eff", "gamma_eff_t", "beta_eff"), single, (ge, get, be)):
            assert torch.equal(many.read(name)[0].view(torch.int32), one.reshape(-1).view(torch.int32)), f"batched {name} C{C}"


# =================================================================================================================== RGB stem
@pytest.mark.parametrize("co,cin", [(22, 3), (128, 3), (5, 1)])
def test_stem_filters(dev, co, cin):
    """ops.stem_filters: the exact layout forward; the backward ADDS both gradients into the parameters' persistent gradient buffers"""
    from clc_amd import ops

    w3, w1x1 = R.rand(1, co, cin, 3, 3), R.rand(2, co, cin, 1, 1)
    p3 = w3.to(dev).contiguous(memory_format=CL).requires_grad_()
    p1 = w1x1.to(dev).requires_grad_()
    assert ops.to_kernel_weight(p3) is p3 and ops.to_kernel_weight(p1) is p1
    i3, i1 = R.rand(3, co, cin, 3, 3), R.rand(4, co, cin, 1, 1)
    for p, init in ((p3, i3), (p1, i1)):
        p.grad = torch.empty_like(p).copy_(init.to(dev))
        p._clc_direct = True
        assert ops._direct_grad(p) is p.grad
    w1, ws = ops.stem_filters(p3, p1)
    r1, rs = R.stem_pack_ref(w3.double(), w1x1.double())
    exact("stem_pack w1", w1.detach().cpu(), r1)
    exact("stem_pack ws", ws.detach().cpu(), rs)
    dw1, dws = R.rand(5, co, 32), R.rand(6, co, 32)
    g3_before = p3.grad
    ((w1 * dw1.to(dev)).sum() + (ws * dws.to(dev)).sum()).backward()
    assert p3.grad is g3_before, "the gradient buffer was replaced, not added into"
    g3, g1 = R.stem_unpack_ref(dw1, dws, cin)   # float32: one IEEE add per element
    assert torch.equal(p3.grad.cpu(), i3 + g3) and torch.equal(p1.grad.cpu(), i1 + g1)


def test_stem_filters_refuse_four_input_channels(dev):
    from clc_amd import lib, ops

    L, st = _lib()
    w3, w1x1 = torch.ones(8, 4, 3, 3, device=dev).contiguous(memory_format=CL), torch.ones(8, 4, 1, 1, device=dev)
    with pytest.raises(lib.ClcError, match="9 \\* cin must fit 32 columns"):
        ops.stem_filters(w3, w1x1)
    out = Buf(dev, 8, 32)
    refused(L.clc_stem_unpack_add(out.ptr, out.ptr, w3.data_ptr(), w1x1.data_ptr(), 8, 4, st), "clc_stem_unpack_add: bad args")
    w1, ws = ops.stem_filters(w3[:, :3].contiguous(memory_format=CL), w1x1[:, :3].contiguous())
    assert float(w1.sum()) == 8 * 27 and float(ws.sum()) == 8 * 3


# =================================================================================================================== patch rows and pooling
@pytest.mark.parametrize("hw", [(9, 11), (1, 1)], ids=["9x11", "1x1"])
@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_im2col_small(dev, case, hw):
    L, st = _lib()
    ks, stride, pad, C, ldc = case
    N, (H, W) = 2, hw
    x = R.rand(100 + ks + H, N, H, W, C)
    OH, OW = R.out_size(H, ks, stride, pad), R.out_size(W, ks, stride, pad)
    ldx = C + 2
    xb, col = Buf(dev, N * H * W, C, ldx, x.reshape(-1, C)), Buf(dev, N * OH * OW, ldc)
    ok(L.clc_im2col_small(xb.ptr, ldx, N, H, W, C, ks, stride, pad, col.ptr, ldc, OH, OW, st))
    ref = R.im2col_ref(x.double(), ks, stride, pad, ldc)
    got = col.read("patch rows")
    exact(f"im2col {case} {hw}", got, ref)
    assert bool((got[:, ks * ks * C:].view(torch.int32) == 0).all()), "the padding columns must be +0"


def test_im2col_small_through_ops_and_refusals(dev):
    from clc_amd import ops

    L, st = _lib()
    x = R.rand(7, 2, 9, 11, 3)
    buf = torch.full((2, 8, 9, 11), float("nan"), device=dev).contiguous(memory_format=CL)
    buf[:, 2:5] = x.permute(0, 3, 1, 2).to(dev)
    col = ops.im2col_small(buf[:, 2:5], 3, 2)
    exact("ops.im2col_small", _nhwc_cpu(col).reshape(-1, 32), R.im2col_ref(x.double(), 3, 2, 1, 32))
    xb, out = Buf(dev, 2 * 9 * 11, 3, 3, x.reshape(-1, 3)), Buf(dev, 2 * 5 * 6, 32)
    call = lambda ldc=32, OH=5, OW=6, ks=3, H=9, W=11, pad=1: L.clc_im2col_small(xb.ptr, 3, 2, H, W, 3, ks, 2, pad, out.ptr, ldc, OH, OW, st)
    refused(call(ldc=24), "ldc must be a multiple of 4 and >= ks*ks*C")
    refused(call(ldc=30), "ldc must be a multiple of 4 and >= ks*ks*C")
    refused(call(OH=6), "clc_im2col_small: output dims")
    refused(call(ks=4, H=1, W=1, pad=1, OH=1, OW=1, ldc=48), "clc_im2col_small: output dims")   # a 4x4 window on a padded 3x3 map: F.unfold refuses
    assert out.untouched()
    ok(call())
    out.read("patch rows")


@pytest.mark.parametrize("C", [4, 20])
@pytest.mark.parametrize("hw", [(7, 9), (1, 1)], ids=["7x9", "1x1"])
@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_maxpool2d(dev, case, hw, C):
    """all-negative maps: a padding of 0 instead of -inf would win every border window.  Where F.max_pool2d refuses the shape (a 2x2 window on
    a 1x1 map) the entry point refuses it too."""
    L, st = _lib()
    ks, stride, pad = case
    N, (H, W) = 2, hw
    x = -R.uniform(200 + ks + H + C, N, H, W, C, lo=0.5, hi=2.0)
    ldx, ldy = C + 4, C + 8
    OH, OW = R.out_size(H, ks, stride, pad), R.out_size(W, ks, stride, pad)
    xb = Buf(dev, N * H * W, C, ldx, x.reshape(-1, C))
    if OH is None:
        y = Buf(dev, N, C, ldy)
        for oh in (0, 1):
            refused(L.clc_maxpool2d(xb.ptr, ldx, y.ptr, ldy, N, H, W, C, ks, stride, pad, oh, oh, st), "clc_maxpool2d: output dims")
        assert y.untouched()
        return
    y = Buf(dev, N * OH * OW, C, ldy)
    ok(L.clc_maxpool2d(xb.ptr, ldx, y.ptr, ldy, N, H, W, C, ks, stride, pad, OH, OW, st))
    exact(f"maxpool {case} {hw} C{C}", y.read("maxpool"), R.maxpool_ref(x.double(), ks, stride, pad).reshape(-1, C))


def test_maxpool2d_refusals(dev):
    L, st = _lib()
    xb, y = Buf(dev, 2 * 7 * 9, 8, 8, -torch.ones(126, 8)), Buf(dev, 2 * 4 * 5, 8, 8)
    call = lambda C=8, OH=4, ldx=8, x=xb.ptr: L.clc_maxpool2d(x, ldx, y.ptr, 8, 2, 7, 9, C, 3, 2, 1, OH, 5, st)
    refused(call(C=6), "clc_maxpool2d: bad args")
    refused(call(ldx=10), "clc_maxpool2d: bad args")
    refused(call(x=xb.ptr + 4), "clc_maxpool2d: bad args")
    refused(call(OH=3), "clc_maxpool2d: output dims")
    refused(call(OH=5), "clc_maxpool2d: output dims")
    assert y.untouched()
    ok(call())
    assert torch.equal(y.read("maxpool"), -torch.ones(40, 8))


@pytest.mark.parametrize("C", [3, 10])
@pytest.mark.parametrize("is_max", [1, 0], ids=["max", "avg"])
@pytest.mark.parametrize("case", R.ADAPTIVE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_adaptive_pool2d(dev, case, is_max, C):
    L, st = _lib()
    H, W, Lb = case
    N, ldx = 2, C + 3
    x = -R.uniform(300 + H + W + Lb + C, N, H, W, C, lo=0.5, hi=2.0)
    xb, out = Buf(dev, N * H * W, C, ldx, x.reshape(-1, C)), vec(dev, n=N * C * Lb * Lb)
    ok(L.clc_adaptive_pool2d(xb.ptr, ldx, out.ptr, N, H, W, C, Lb, is_max, st))
    ref, bound = R.adaptive_pool_ref(x.double(), Lb, bool(is_max))
    got = out.read("pooled")[0].reshape(N, C, Lb, Lb)          # [N][C][L][L]
    if is_max:
        exact(f"adaptive max {case} C{C}", got, ref)
    else:
        held(f"adaptive avg {case} C{C}", got, ref, bound)
    if (case, C) == (R.ADAPTIVE_CASES[0], 3):
        refused(L.clc_adaptive_pool2d(xb.ptr, ldx, out.ptr, N, H, W, C, H + 1, is_max, st), "clc_adaptive_pool2d: bad args")
        refused(L.clc_adaptive_pool2d(xb.ptr, C - 1, out.ptr, N, H, W, C, Lb, is_max, st), "clc_adaptive_pool2d: bad args")
        ok(L.clc_adaptive_pool2d(xb.ptr, ldx, out.ptr, N, H, W, C, Lb, is_max, st))
        torch.cuda.synchronize()
