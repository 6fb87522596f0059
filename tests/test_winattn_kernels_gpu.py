"""The kernels of csrc/winattn.hip through raw clc_winattn_* calls, held per element to the float64 statement of tests/winattn_ref.py.

Conventions
  * operands are float32 tensors from the seeded CPU builders of winattn_ref (regimes mild / peaked / offset / hostile / exact); the reference
    sees exactly those values in float64
  * every operand and result with a leading dimension (qkv, out, dout, dqkv) is a channel slice of a wider buffer: ld = width + 8, the slice
    starts 4 floats into the row — 16-byte aligned, as the ABI demands, and never 128-byte aligned, so the whole-line loads and stores of the
    NH > 1 forward kernel start inside a line.  Everything outside a slice holds one NaN bit pattern (SENTINEL): an operand read outside its
    slice poisons the result; after a launch everything outside a result's slice still holds the pattern and nothing inside does.  lse,
    drelbias and the workspace are dense and have sentinel words in front and behind.  One dense launch per case (ld = width, 128-byte aligned)
    must give the bits of the sliced one
  * the backward reads the forward's own float32 out and lse, as in training
  * all six outputs (O, lse, dQ, dK, dV, drelbias) of every small case are held, every element, to BUDGET[regime][kind] x bound

Which kernel a case means (winattn_fwd_impl / winattn_bwd_impl; B4 = the 4-block 16x16x1 MFMA form, chosen by tuning key 16: bit 1 =
head_dim 16, bit 2 = head_dim-8 backward, bit 4 = head_dim-8 forward; default 3.  Key 16 at 0 and at 7 reaches both forms of every template):
    ws  C / heads (hd)   forward                                      backward                           maps
    8   32 / 4 (8)       winattn_fwd_mfma_kernel<8, B4, 4>            winattn_bwd_mfma_kernel<8, B4>     16x24, B = 1, 3
                         (heads % 4 == 0: four heads per workgroup)
    8   16 / 2 (8)       winattn_fwd_mfma_kernel<8, B4, 1>            winattn_bwd_mfma_kernel<8, B4>     16x24, B = 1
    8   32 / 2 (16)      winattn_fwd_mfma_kernel<16, B4, 2>           winattn_bwd_mfma_kernel<16, B4>    16x24, B = 1, 3
    8   48 / 3 (16)      winattn_fwd_mfma_kernel<16, B4, 1>           winattn_bwd_mfma_kernel<16, B4>    24x16, B = 1
    8   64 / 2 (32)      winattn_fwd_mfma_kernel<32, false, 1>        winattn_bwd_mfma_kernel<32, false> 16x24, B = 1, 3
    4   16 / 2 (8)       winattn_fwd_kernel<16, 8>                    winattn_bwd_kernel<16, 8>          8x12 B = 1 (6 windows: the second
    4   32 / 2 (16)      winattn_fwd_kernel<16, 16>                   winattn_bwd_kernel<16, 16>         group of 4 is partial); 12x12 B = 3
    4   64 / 2 (32)      winattn_fwd_kernel<16, 32>                   winattn_bwd_kernel<16, 32>         (27 windows)
Every ws = 8 backward of these maps has nbx * heads <= 1024, so tuning key 18 (default 1) splits each window group over two workgroups; the
ws = 8 rows also run with key 18 at 0 (one workgroup per group).  Key 18's split and groups_per_block > 1 cannot coincide: the split needs
nbx * heads <= 1024, more than one group per block needs groups * heads > 2048, and nbx = ceil(groups / per) >= groups / per with
per = ceil(groups * heads / 2048) puts nbx * heads above 1024 whenever per > 1 — so there is no such case to hunt for.

Large grids (groups_per_block > 1; the rule is restated in fwd_per() / asserted from clc_winattn_bwd_blocks so that a changed target shows):
    forward T = 16       hd 8, heads 1, B = 1, 732x724: 33 123 windows, 8 281 groups, per = 2; the last group and the last block are short
    forward MFMA NH = 1  hd 32, heads 1, B = 129 of 64x64          forward MFMA NH = 4  hd 8, heads 4, B = 65 of 64x64
    forward MFMA NH = 2  hd 16, heads 2, B = 65 of 64x64
    backward MFMA        hd 8, heads 8, B = 3 of 72x88: 297 groups, per = 2, 149 blocks (the last one short)
    backward VALU        hd 32, heads 2, B = 1 of 260x260: 4 225 windows, 1 057 groups (the last partial), per = 2
The forward cases hold the first and last window, the windows on either side of every 64th block boundary and 64 seeded random windows;
the backward cases are small enough to hold every window and drelbias.

Exact regime: q = 0 and bias = 0, so every score is 0 and p = 1 / (visible keys) = 1/64, 1/32 or 1/16 (1/16, 1/8, 1/4 for ws = 4) exactly;
v[token][c] = pixel index mod 256 + c and dO are small integers, so O (the mean of v over exactly the keys the query saw) and dV are small
multiples of 1/64 in any summation order and are held bit for bit: a wrong roll, partition or mask changes the set and therefore the bits.
dV additionally needs exp2(-(log n) log2 e) == 1 / n from the backward's rebuilt probabilities.

Bounds: the derivation of every term is in the docstring of winattn_ref.py (u = 2^-24, T = ws^2, E = 4):
    ds = (hd + 2) u hd^-1/2 |q|.|k| + u |bias|;  eps = ds + sum_j p ds + (2 |s - m| + T + E) u;  dp = p eps + t;
    dO = dp |V| + (T + 1) u p |V|;  dlse = sum_j p ds + (|lse| + T + E) u;  ddP = (hd + 1) u |dO| |V|^T;
    dD = |dO| . dO_bound + (hd + 1) u sum |dO o O|;  ddS = dp |dP - D| + p (ddP + dD) + 2 u |dS| + t;
    ddQ = hd^-1/2 (ddS |K| + (T + 2) u |dS| |K|);  ddK likewise with |q|;  ddV = dp^T |dO| + (T + 1) u p^T |dO|;
    ddrelbias = sum ddS + (n + 1) (u sum |dS| + TINY) (+ u |pre| when accumulating)
t = TINY = 2^-126: a result below the smallest normal number is returned as 0 by the matrix instructions and the hardware exp2, an absolute
error per operation; every sum of n products carries (n + 1) TINY.  (Seen on the MI355X: a relative-bias bin of the peaked regime whose
twelve terms are all near 1e-38 came back 1.3e-38 off.)

Budgets: worst error / bound of the float32 restatement on the CPU over the small and paired cases (W and SW), measured and asserted by
test_winattn_ref_cpu.py::test_budgets_are_eight_times_the_float32_cpu_error, the budget chosen (8 x, rounded up to two significant
digits), and the worst error / (budget x bound) of the kernels on the MI355X as the tests here print it ("exact": float32 arithmetic is
exact there, see winattn_ref.EXACT):
    regime   kind       float32 CPU   budget   MI355X worst error / (budget x bound)
    mild     O              0.0667     0.54   0.1361
    mild     lse            0.1582      1.3   0.1657
    mild     dQ             0.0352     0.29   0.1189
    mild     dK             0.0316     0.26   0.1278
    mild     dV             0.0868      0.7   0.1568
    mild     drelbias       0.0216     0.18   0.4651
    peaked   O              0.1219     0.98   0.1370
    peaked   lse            0.4272      3.5   0.1220
    peaked   dQ             0.0734     0.59   0.1229
    peaked   dK             0.0908     0.73   0.1317
    peaked   dV             0.2053      1.7   0.1388
    peaked   drelbias       0.0852     0.69   0.0984
    offset   O              0.2552      2.1   0.1229
    offset   lse            0.3949      3.2   0.1273
    offset   dQ             0.1276      1.1   0.1160
    offset   dK             0.1490      1.2   0.1242
    offset   dV             0.3888      3.2   0.1215
    offset   drelbias       0.2096      1.7   0.1233
    hostile  O              0.0938     0.76   0.1230
    hostile  lse            0.2610      2.1   0.1243
    hostile  dQ             0.0387     0.31   0.1251
    hostile  dK             0.0386     0.31   0.1247
    hostile  dV             0.0931     0.75   0.1241
    hostile  drelbias       0.0243      0.2   0.2607
    exact    O             0.0e+00    exact   0.0000
    exact    lse            0.0056    0.045   0.1247
    exact    dQ             0.0044    0.036   0.1217
    exact    dK            0.0e+00    exact   0.0000
    exact    dV            1.6e-10    exact   0.0002
    exact    drelbias      2.7e-11    exact   0.0000
"""
import contextlib
import functools

import pytest
import torch

import winattn_ref as R

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
SENTINEL = 0x7FC0BEEF   # a quiet NaN with a payload no arithmetic produces
GUARD = 64              # sentinel words in front of and behind every buffer (256 bytes: the body stays 128-byte aligned)
KEY_SPLIT = 18


class Buf:
    """[rows, width] float32 inside a sentinel-filled device buffer.  sliced: ld = width + 8 and the slice starts 4 floats into the row"""

    def __init__(self, dev, rows, width, sliced=False, data=None):
        self.rows, self.width = rows, width
        self.ld, self.off = (width + 8, 4) if sliced else (width, 0)
        self.t = torch.full((2 * GUARD + rows * self.ld,), SENTINEL, dtype=I32, device=dev).view(F32)
        self.ptr = self.t.data_ptr() + 4 * (GUARD + self.off)
        assert self.ptr % 16 == 0 and (not sliced or self.ptr % 128 != 0)
        if data is not None:
            assert tuple(data.shape) == (rows, width) and data.dtype == F32, (data.shape, rows, width)
            self.view().copy_(data.to(dev))

    def view(self):
        return torch.as_strided(self.t, (self.rows, self.width), (self.ld, 1), GUARD + self.off)

    def bits(self):
        return self.view().contiguous().view(I32)

    def check(self, what, full=True):
        """everything outside the slice untouched; (full) nothing inside still the pattern"""
        w = self.t.view(I32)
        body = w[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)
        intact = bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + self.rows * self.ld:] == SENTINEL).all())
        intact = intact and bool((body[:, :self.off] == SENTINEL).all()) and bool((body[:, self.off + self.width:] == SENTINEL).all())
        assert intact, f"{what}: written outside its slice"
        if full:
            assert not bool((body[:, self.off:self.off + self.width] == SENTINEL).any()), f"{what}: elements of the slice were not written"
        return self

    def untouched(self):
        return bool((self.t.view(I32) == SENTINEL).all())


def _lib():
    from clc_amd import ops

    return ops._L(), ops._stream()


def ok(rc):
    L, _ = _lib()
    assert rc == 0, (rc, L.clc_last_error())


@contextlib.contextmanager
def tuning(**keys):
    """set tuning keys ("k16" = key 16) for a block and put the old values back"""
    L, _ = _lib()
    old = {}
    try:
        for name, v in keys.items():
            k = int(name[1:])
            old[k] = L.clc_set_tuning(k, v)
            assert old[k] >= 0, L.clc_last_error()
        yield
    finally:
        for k, v in old.items():
            L.clc_set_tuning(k, v)


CONFIGS = {"default": {}, "k16=0": {"k16": 0}, "k16=7": {"k16": 7}, "k18=0": {"k18": 0}}


class Run:
    pass


def launch(dev, g, t, sliced=True, paired=False, accumulate=0, null_drel=False, bwd=True, lse=True):
    """forward (with lse), then backward on the forward's own out and lse"""
    L, st = _lib()
    N, C, heads = g.tokens, g.C, g.heads
    r = Run()
    r.g, r.paired = g, paired
    r.qkv, r.out = Buf(dev, N, 3 * C, sliced, t["qkv"]), Buf(dev, N, C, sliced)
    r.lse = Buf(dev, N, heads) if lse else None
    r.rb, r.rb2 = t["relbias"].to(dev).contiguous(), t["relbias2"].to(dev).contiguous()
    geom = (g.B, g.H, g.W, C, heads, g.ws, g.shift)
    lse_ptr = r.lse.ptr if lse else None
    if paired:
        ok(L.clc_winattn_fwd_pair(r.qkv.ptr, r.qkv.ld, r.rb.data_ptr(), r.rb2.data_ptr(), r.out.ptr, r.out.ld, lse_ptr, *geom, st))
    else:
        ok(L.clc_winattn_fwd(r.qkv.ptr, r.qkv.ld, r.rb.data_ptr(), r.out.ptr, r.out.ld, lse_ptr, *geom, st))
    r.out.check("out")
    if lse:
        r.lse.check("lse")
    if not bwd:
        return r
    r.dout, r.dqkv = Buf(dev, N, C, sliced, t["dout"]), Buf(dev, N, 3 * C, sliced)
    ntab = 2 if paired else 1
    pre = t["pre"].reshape(2, 1, heads * g.nb) if accumulate else (None, None)
    r.drel = [Buf(dev, 1, heads * g.nb, data=pre[k]) for k in range(ntab)]
    nbytes = L.clc_winattn_bwd_workspace_bytes(g.B, g.H, g.W, heads, g.ws)
    assert nbytes > 0 and nbytes % (4 * heads * g.nb) == 0
    r.ws_bytes, r.wsb = nbytes, Buf(dev, 1, nbytes // 4)
    dptr = [None if null_drel else d.ptr for d in r.drel]
    if paired:
        ok(L.clc_winattn_bwd_pair(r.dout.ptr, r.dout.ld, r.qkv.ptr, r.qkv.ld, r.rb.data_ptr(), r.rb2.data_ptr(), r.out.ptr, r.out.ld, r.lse.ptr,
                                  r.dqkv.ptr, r.dqkv.ld, dptr[0], dptr[1], accumulate, *geom, r.wsb.ptr, nbytes, st))
    else:
        ok(L.clc_winattn_bwd(r.dout.ptr, r.dout.ld, r.qkv.ptr, r.qkv.ld, r.rb.data_ptr(), r.out.ptr, r.out.ld, r.lse.ptr, r.dqkv.ptr, r.dqkv.ld,
                             dptr[0], accumulate, *geom, r.wsb.ptr, nbytes, st))
    torch.cuda.synchronize()
    r.dqkv.check("dqkv")
    r.wsb.check("workspace", full=False)
    for d in r.drel:
        if null_drel:
            assert d.untouched(), "drelbias = NULL, yet a drelbias buffer of an earlier argument was written"
        else:
            d.check("drelbias")
    r.out.check("out after the backward"), r.lse.check("lse after the backward"), r.qkv.check("qkv"), r.dout.check("dout")
    return r


def gathered(r, pix, bwd=True):
    """the outputs of a run at the token rows `pix` [n, T], in the layouts of winattn_ref.results()"""
    g = r.g
    n, C = pix.shape[0], g.C
    idx = pix.reshape(-1).to(r.out.t.device)
    got = {"O": r.out.view()[idx].cpu().reshape(n, g.T, C), "lse": r.lse.view()[idx].cpu().reshape(n, g.T, g.heads)}
    if bwd:
        d = r.dqkv.view()[idx].cpu().reshape(n, g.T, 3 * C)
        got.update(dQ=d[..., :C], dK=d[..., C:2 * C], dV=d[..., 2 * C:], drelbias=torch.stack([b.view().cpu().reshape(g.heads, g.nb) for b in r.drel]))
    return got


def same_bits(name, a, b):
    assert torch.equal(a, b), f"{name}: not bit-equal"


def held(name, regime, got, ref, bnd, kinds=R.KINDS):
    bad = []
    for k in kinds:
        budget = R.BUDGET[regime][k]
        ratio = R.worst_ratio(got[k], ref[k], bnd[k]) / budget
        print(f"winattn {regime} {k}: worst error / (budget x bound) = {ratio:.4f} (budget {budget}) [{name}]")
        if not ratio <= 1.0:
            bad.append((k, ratio))
    assert not bad, f"{name}: error / (budget x bound) {bad}"


def held_exact(name, g, t, got):
    want = R.exact_expected(g, t)
    for k in ("O", "dV"):
        if k in got:
            assert R.bits_equal(got[k], want[k]), f"{name}: {k} is not bit-equal to the integer arithmetic of the exact regime"
    if "dK" in got:
        assert bool((got["dK"] == 0).all()), f"{name}: dK != 0 with q = 0"


@functools.lru_cache(maxsize=None)
def case_ref(case, paired, shift, regime, accumulate=False):
    """(geometry, operands, float64 results, bounds): computed once, shared, never modified"""
    _, C, heads, ws, H, W, B = case
    g = R.Geom(C, heads, ws, H, W, B, shift)
    t = R.build(regime, g)
    r = R.attend(g, t["qkv"], t["relbias"], t["dout"], relbias2=t["relbias2"] if paired else None)
    pre = t["pre"] if accumulate else None
    return g, t, r["pix"], R.results(g, r, paired, pre=pre), R.bounds(g, r, paired, pre=pre)


def _cfg_applies(case, cfg):
    _, C, heads, ws, *_ = case
    if cfg == "default":
        return True
    if cfg == "k18=0":
        return ws == 8
    return ws == 8 and C // heads in (8, 16)


SMALL = [(c, cfg) for c in R.SMALL_CASES for cfg in CONFIGS if _cfg_applies(c, cfg)]


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("shift", [0, 1], ids=["W", "SW"])
@pytest.mark.parametrize("case,cfg", SMALL, ids=[f"{c[0]}-{cfg}" for c, cfg in SMALL])
def test_small_cases_against_float64(dev, case, cfg, shift, regime):
    g, t, pix, ref, bnd = case_ref(case, False, shift, regime)
    name = f"{case[0]} {'SW' if shift else 'W'} {cfg}"
    with tuning(**CONFIGS[cfg]):
        r = launch(dev, g, t)
        d = launch(dev, g, t, sliced=False)
    for what in ("out", "lse", "dqkv"):
        same_bits(f"{name}: dense and sliced {what}", getattr(r, what).bits(), getattr(d, what).bits())
    same_bits(f"{name}: dense and sliced drelbias", r.drel[0].bits(), d.drel[0].bits())
    got = gathered(r, pix)
    held(name, regime, got, ref, bnd)
    if regime == "exact":
        held_exact(name, g, t, got)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("shift", [0, 1], ids=["W", "SW"])
@pytest.mark.parametrize("case", R.PAIR_CASES, ids=[c[0] for c in R.PAIR_CASES])
def test_paired_launch_uses_the_second_table_from_the_second_half_on(dev, case, shift, regime):
    g, t, pix, ref, bnd = case_ref(case, True, shift, regime)
    r = launch(dev, g, t, paired=True)
    got = gathered(r, pix)
    held(f"{case[0]} {'SW' if shift else 'W'}", regime, got, ref, bnd)
    if regime == "exact":
        held_exact(case[0], g, t, got)


MODES = [R.SMALL_CASES[1], R.SMALL_CASES[4], R.SMALL_CASES[7], R.SMALL_CASES[8], R.SMALL_CASES[13]]   # one per backward kernel template and head_dim family


@pytest.mark.parametrize("case", MODES, ids=[c[0] for c in MODES])
def test_drelbias_accumulates_into_a_prefilled_buffer(dev, case):
    g, t, pix, ref, bnd = case_ref(case, False, 1, "mild", True)
    r = launch(dev, g, t, accumulate=1)
    held(f"{case[0]} accumulate", "mild", gathered(r, pix), ref, bnd, ("drelbias",))


def test_paired_drelbias_accumulates_into_prefilled_buffers(dev):
    for case in R.PAIR_CASES:
        g, t, pix, ref, bnd = case_ref(case, True, 1, "mild", True)
        r = launch(dev, g, t, paired=True, accumulate=1)
        held(f"{case[0]} accumulate", "mild", gathered(r, pix), ref, bnd, ("drelbias",))


def _partial_rows(r, paired):
    L, _ = _lib()
    g = r.g
    nblocks = L.clc_winattn_bwd_blocks(g.B, g.H, g.W, g.heads, g.ws, int(paired))
    n = g.heads * g.nb
    assert 0 < nblocks * n * 4 <= r.ws_bytes
    rows = r.wsb.view().cpu().reshape(-1)[:nblocks * n].reshape(nblocks, n)
    assert not torch.isnan(rows).any(), "a partial row of the workspace was not written"
    return rows.double()


NULL_MODES = [(c, cfg) for c in MODES for cfg in ("default", "k18=0") if _cfg_applies(c, cfg)]


@pytest.mark.parametrize("case,cfg", NULL_MODES, ids=[f"{c[0]}-{cfg}" for c, cfg in NULL_MODES])
def test_null_drelbias_leaves_the_partial_rows_in_the_workspace(dev, case, cfg):
    g, t, pix, ref, bnd = case_ref(case, False, 1, "mild")
    with tuning(**CONFIGS[cfg]):
        r = launch(dev, g, t, null_drel=True)
        rows = _partial_rows(r, False)
    got = {"drelbias": rows.sum(0).reshape(1, g.heads, g.nb)}
    held(f"{case[0]} {cfg} partial rows", "mild", got, ref, bnd, ("drelbias",))


@pytest.mark.parametrize("case", R.PAIR_CASES, ids=[c[0] for c in R.PAIR_CASES])
def test_null_drelbias_paired_first_half_of_the_rows_is_module_one(dev, case):
    g, t, pix, ref, bnd = case_ref(case, True, 1, "mild")
    r = launch(dev, g, t, paired=True, null_drel=True)
    rows = _partial_rows(r, True)
    assert rows.shape[0] % 2 == 0
    h = rows.shape[0] // 2
    got = {"drelbias": torch.stack([rows[:h].sum(0), rows[h:].sum(0)]).reshape(2, g.heads, g.nb)}
    held(f"{case[0]} partial rows", "mild", got, ref, bnd, ("drelbias",))


@pytest.mark.parametrize("case", MODES, ids=[c[0] for c in MODES])
def test_backward_is_reproducible(dev, case):
    g, t, *_ = case_ref(case, False, 1, "mild")
    a, b = launch(dev, g, t), launch(dev, g, t)
    same_bits("dqkv of two runs", a.dqkv.bits(), b.dqkv.bits())
    same_bits("drelbias of two runs", a.drel[0].bits(), b.drel[0].bits())


@pytest.mark.parametrize("case", MODES + [R.SMALL_CASES[2], R.SMALL_CASES[5]], ids=[c[0] for c in MODES] + [R.SMALL_CASES[2][0], R.SMALL_CASES[5][0]])
def test_forward_without_lse_gives_the_same_output(dev, case):
    g, t, *_ = case_ref(case, False, 1, "mild")
    a, b = launch(dev, g, t, bwd=False), launch(dev, g, t, bwd=False, lse=False)
    same_bits("out with and without lse", a.out.bits(), b.out.bits())


B3 = [c for c in R.SMALL_CASES if c[6] == 3]


@pytest.mark.parametrize("shift", [0, 1], ids=["W", "SW"])
@pytest.mark.parametrize("case", B3, ids=[c[0] for c in B3])
def test_image_0_of_a_batch_of_3_equals_the_batch_of_1(dev, case, shift):
    g, t, *_ = case_ref(case, False, shift, "mild")
    _, C, heads, ws, H, W, _ = case
    g1 = R.Geom(C, heads, ws, H, W, 1, shift)
    t1 = dict(t, qkv=t["qkv"][:H * W].contiguous(), dout=t["dout"][:H * W].contiguous())
    a, b = launch(dev, g, t), launch(dev, g1, t1)
    for what in ("out", "lse", "dqkv"):
        same_bits(f"{what} of image 0", getattr(a, what).bits()[:H * W], getattr(b, what).bits())


NAN_CASES = [R.SMALL_CASES[0], R.SMALL_CASES[3], R.SMALL_CASES[6], R.SMALL_CASES[10]]


@pytest.mark.parametrize("case", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_a_nan_in_one_key_stays_in_its_window_and_head(dev, case):
    g, t, pix, *_ = case_ref(case, False, 1, "mild")
    C, hd = g.C, g.hd
    w0, t0, h0 = 1, 5, 1
    bad = dict(t, qkv=t["qkv"].clone())
    bad["qkv"][pix[w0, t0], C + h0 * hd + 3] = float("nan")
    clean, dirty = launch(dev, g, t), launch(dev, g, bad)
    inside = torch.zeros(g.tokens, C, dtype=torch.bool)
    inside[pix[w0], h0 * hd:(h0 + 1) * hd] = True
    lse_in = torch.zeros(g.tokens, g.heads, dtype=torch.bool)
    lse_in[pix[w0], h0] = True
    masks = {"out": inside, "lse": lse_in, "dqkv": inside.repeat(1, 3)}
    for what, m in masks.items():
        a, b = getattr(clean, what).bits().cpu(), getattr(dirty, what).bits().cpu()
        assert torch.equal(a[~m], b[~m]), f"{what}: the NaN reached another window or head"
    da, db = clean.drel[0].bits().cpu().reshape(g.heads, g.nb), dirty.drel[0].bits().cpu().reshape(g.heads, g.nb)
    others = [h for h in range(g.heads) if h != h0]
    assert torch.equal(da[others], db[others]), "drelbias: the NaN reached another head's bins"
    r = R.attend(g, bad["qkv"], t["relbias"], t["dout"], widx=torch.tensor([w0]))
    ref = R.results(g, r, widx=torch.tensor([w0]))
    got = gathered(dirty, pix[w0:w0 + 1])
    for k in R.KINDS:
        nan_ref = torch.isnan(ref[k])
        assert nan_ref.any(), k
        assert bool(torch.isnan(got[k])[nan_ref].all()), f"{k}: float64 gives NaN where the kernel gives a number"


# ---------------------------------------------------------------------------------------------------------------- large grids
def fwd_per(g, paired=False):
    """groups per workgroup of the forward, as winattn_fwd_impl / fill() state it: target 4096 workgroups when the heads that share a
    128-byte line run as the waves of one workgroup (8x8 windows, head_dim 8 / 16, heads a multiple of 32 / head_dim), else 8192"""
    G = 64 // g.T
    groups = (g.windows + G - 1) // G
    nh = 32 // g.hd if (g.ws == 8 and g.hd in (8, 16) and g.heads % (32 // g.hd) == 0) else 1
    target = 4096 if nh > 1 else 8192
    per = max(1, (groups * (g.heads // nh) + target - 1) // target)
    if paired:
        while ((g.windows // 2) // G) % per:
            per -= 1
    return per, groups


def bwd_per(g):
    L, _ = _lib()
    G = 64 // g.T
    groups = (g.windows + G - 1) // G
    per = max(1, (groups * g.heads + 2047) // 2048)                     # target: 2048 workgroups
    nbx = (groups + per - 1) // per
    split = g.ws == 8 and L.clc_get_tuning(KEY_SPLIT) != 0 and nbx * g.heads <= 1024   # key 18: two workgroups per group on small grids
    blocks = L.clc_winattn_bwd_blocks(g.B, g.H, g.W, g.heads, g.ws, 0)
    assert blocks == nbx * (2 if split else 1), (blocks, groups, per, split)
    return per, groups


def chosen_windows(g, per, groups, seed=5):
    G = 64 // g.T
    w = {0, g.windows - 1}
    nblocks = (groups + per - 1) // per
    for b in range(64, nblocks, 64):
        w.update((b * per * G - 1, b * per * G))
    gen = torch.Generator().manual_seed(seed)
    w.update(torch.randint(0, g.windows, (64,), generator=gen).tolist())
    return torch.tensor(sorted(w))


# (name, C, heads, ws, H, W, B, images per chunk for the per = 1 comparison)
LARGE_FWD = [("valu-t16-732x724", 8, 1, 4, 732, 724, 1, 0), ("mfma-nh1-hd32-b129", 32, 1, 8, 64, 64, 129, 43),
             ("mfma-nh4-hd8-b65", 32, 4, 8, 64, 64, 65, 13), ("mfma-nh2-hd16-b65", 32, 2, 8, 64, 64, 65, 13)]


@pytest.mark.parametrize("shift", [0, 1], ids=["W", "SW"])
@pytest.mark.parametrize("case", LARGE_FWD, ids=[c[0] for c in LARGE_FWD])
def test_forward_with_more_than_one_group_per_workgroup(dev, case, shift):
    name, C, heads, ws, H, W, B, chunk = case
    g = R.Geom(C, heads, ws, H, W, B, shift)
    per, groups = fwd_per(g)
    assert per > 1, (per, groups)
    t = R.build("mild", g)
    r = launch(dev, g, t, bwd=False)
    sel = chosen_windows(g, per, groups)
    ref_r = R.attend(g, t["qkv"], t["relbias"], widx=sel)
    held(name, "mild", gathered(r, ref_r["pix"], bwd=False), R.results(g, ref_r), R.bounds(g, ref_r), ("O", "lse"))
    for b0 in range(0, B, chunk) if chunk else ():
        nb = min(chunk, B - b0)
        gc = R.Geom(C, heads, ws, H, W, nb, shift)
        assert fwd_per(gc)[0] == 1
        rows = slice(b0 * H * W, (b0 + nb) * H * W)
        c = launch(dev, gc, dict(t, qkv=t["qkv"][rows]), bwd=False)
        same_bits(f"{name}: out of images {b0}..", r.out.bits()[rows], c.out.bits())
        same_bits(f"{name}: lse of images {b0}..", r.lse.bits()[rows], c.lse.bits())


LARGE_BWD = [("mfma-hd8-h8-b3-72x88", 64, 8, 8, 72, 88, 3, 1), ("valu-hd32-h2-260x260", 64, 2, 4, 260, 260, 1, 0)]


@pytest.mark.parametrize("shift", [0, 1], ids=["W", "SW"])
@pytest.mark.parametrize("case", LARGE_BWD, ids=[c[0] for c in LARGE_BWD])
def test_backward_with_more_than_one_group_per_workgroup(dev, case, shift):
    name, C, heads, ws, H, W, B, chunk = case
    g = R.Geom(C, heads, ws, H, W, B, shift)
    per, groups = bwd_per(g)
    assert per > 1 and groups % per == 1, (per, groups)      # the last workgroup is short
    t = R.build("mild", g)
    r = launch(dev, g, t)
    ref_r = R.attend(g, t["qkv"], t["relbias"], t["dout"])
    held(name, "mild", gathered(r, ref_r["pix"]), R.results(g, ref_r), R.bounds(g, ref_r))
    for b0 in range(0, B, chunk) if chunk else ():
        gc = R.Geom(C, heads, ws, H, W, chunk, shift)
        assert bwd_per(gc)[0] == 1
        rows = slice(b0 * H * W, (b0 + chunk) * H * W)
        c = launch(dev, gc, dict(t, qkv=t["qkv"][rows], dout=t["dout"][rows]))
        for what in ("out", "lse", "dqkv"):
            same_bits(f"{name}: {what} of image {b0}", getattr(r, what).bits()[rows], getattr(c, what).bits())


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_c_abi_refuses_bad_arguments_by_name(dev):
    L, st = _lib()
    rows, wide = 2 * 32 * 32, 3 * 64 + 16                # room for every geometry below, were a call accepted after all
    qkv, dout = Buf(dev, rows, wide), Buf(dev, rows, wide)
    out, dqkv, lse, drel, drel2 = Buf(dev, rows, wide), Buf(dev, rows, wide), Buf(dev, rows, 8), Buf(dev, 1, 8 * 225), Buf(dev, 1, 8 * 225)
    qkv.view().zero_(), dout.view().zero_()
    rb = torch.zeros(8 * 225, device=dev)
    wsb = Buf(dev, 1, 1 << 16)

    def fwd(B=1, H=16, W=16, C=32, heads=2, ws=8, ldq=96, ldo=32, q=qkv.ptr, o=out.ptr):
        return L.clc_winattn_fwd(q, ldq, rb.data_ptr(), o, ldo, lse.ptr, B, H, W, C, heads, ws, 1, st)

    def bwd(B=1, H=16, W=16, C=32, heads=2, ws=8, lddo=32, ldq=96, ldo=32, lddq=96, do=dout.ptr, q=qkv.ptr, dq=dqkv.ptr, short=0, pair=False):
        need = L.clc_winattn_bwd_workspace_bytes(B, H, W, heads, ws)
        if pair:
            return L.clc_winattn_bwd_pair(do, lddo, q, ldq, rb.data_ptr(), rb.data_ptr(), out.ptr, ldo, lse.ptr, dq, lddq, drel.ptr, drel2.ptr, 0,
                                          B, H, W, C, heads, ws, 1, wsb.ptr, need - short, st)
        return L.clc_winattn_bwd(do, lddo, q, ldq, rb.data_ptr(), out.ptr, ldo, lse.ptr, dq, lddq, drel.ptr, 0, B, H, W, C, heads, ws, 1,
                                 wsb.ptr, need - short, st)

    def pair_fwd(B, H, W, ws):
        return L.clc_winattn_fwd_pair(qkv.ptr, 96, rb.data_ptr(), rb.data_ptr(), out.ptr, 32, lse.ptr, B, H, W, 32, 2, ws, 1, st)

    def refused(rc, text):
        assert rc != 0, f"accepted: {text}"
        msg = L.clc_last_error().decode()
        assert text in msg, (text, msg)

    refused(fwd(ws=6, H=12, W=12), "clc_winattn_fwd: window size must be 8 or 4 (got 6)")
    refused(bwd(ws=6, H=12, W=12), "clc_winattn_bwd: window size must be 8 or 4 (got 6)")
    refused(fwd(H=20), "clc_winattn_fwd: 20x16 tokens not a multiple of / larger than the window 8")
    refused(bwd(H=20), "clc_winattn_bwd: 20x16 tokens not a multiple of / larger than the window 8")
    refused(fwd(H=8), "clc_winattn_fwd: 8x16 tokens not a multiple of / larger than the window 8")
    refused(bwd(H=8), "clc_winattn_bwd: 8x16 tokens not a multiple of / larger than the window 8")
    refused(fwd(C=24, ldq=72), "clc_winattn_fwd: head_dim must be 8/16/32 (got 12)")
    refused(bwd(C=24, ldq=72, lddq=72), "clc_winattn_bwd: head_dim must be 8/16/32 (got 12)")
    refused(fwd(ldq=98), "clc_winattn_fwd: bad leading dims")
    refused(fwd(ldo=34), "clc_winattn_fwd: bad leading dims")
    refused(bwd(lddo=34), "clc_winattn_bwd: bad leading dims")
    refused(bwd(ldo=34), "clc_winattn_bwd: bad out")
    refused(bwd(lddq=98), "clc_winattn_bwd: bad lddq")
    refused(fwd(ldq=92), "clc_winattn_fwd: bad leading dims")
    refused(bwd(ldq=92), "clc_winattn_bwd: bad leading dims")
    refused(bwd(lddq=92), "clc_winattn_bwd: bad lddq")
    refused(fwd(q=qkv.ptr + 4), "clc_winattn_fwd: unaligned")
    refused(fwd(o=out.ptr + 4), "clc_winattn_fwd: unaligned")
    refused(bwd(do=dout.ptr + 4), "clc_winattn_bwd: unaligned")
    refused(bwd(dq=dqkv.ptr + 4), "clc_winattn_bwd: unaligned")
    refused(bwd(short=1), "clc_winattn_bwd: workspace too small")
    refused(pair_fwd(3, 16, 16, 8), "clc_winattn_fwd_pair: the paired form needs an even batch whose half holds whole window groups")
    refused(bwd(B=3, pair=True), "clc_winattn_bwd_pair: the paired form needs an even batch whose half holds whole window groups")
    refused(pair_fwd(2, 12, 12, 4), "clc_winattn_fwd_pair: the paired form needs an even batch whose half holds whole window groups")
    refused(bwd(B=2, H=12, W=12, ws=4, pair=True), "clc_winattn_bwd_pair: the paired form needs an even batch whose half holds whole window groups")
    torch.cuda.synchronize()
    for name, b in (("out", out), ("dqkv", dqkv), ("lse", lse), ("drelbias", drel), ("drelbias2", drel2), ("workspace", wsb)):
        assert b.untouched(), f"a refused call wrote {name}"
    ok(fwd())
    ok(bwd())
    torch.cuda.synchronize()
