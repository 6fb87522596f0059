"""Every convolution family of clc_conv2d against the float64 reference of its contract (tests/conv_epilogue_ref.py).

clc_conv2d (csrc/conv_igemm.hip) routes a launch to one of about a dozen kernel families, and each family applies the per-element epilogue
(bias, residual before / after the activation with a gate, saved pre-activation or its derivative, GDN / IGDN / MUL2, the activation,
the output gate, PixelShuffle / stride-2 class / ld store) and the operand prologues (IN_SQUARE, the fused activation derivative xs) in code
of its own.  Each RECIPE below is a shape + mode that reaches one family; each CASE runs one set of options on it through ops.conv_raw,
asserts the family that ran (ops.PROFILE), and checks every stored element per output channel against float64, that no NaN from the
NaN-filled output buffers is left inside the written slice and that every byte outside it is untouched.

Coverage (family: recipe -> options run; "-> x" = the option makes the family refuse the launch and family x takes it):

  direct small-Cin (id 1)   direct: Cin 3, ragged 20x20 map, Cout 22      all six activations, res after / first, res_gate lrelu / saved,
                                                                          y_pre, pre_deriv gelu / lrelu, out_gate lrelu / relu / halftanh
                                                                          (og_pre both) / saved, MUL2, odd-offset output (general and
                                                                          lean scalar epilogue), stride 2
                            direct_gdn: 1x1 Cin 3 -> 3                    IN_SQUARE + GDN (+ res), IN_SQUARE + IGDN
                            direct_slice: 8 of 12 channels from channel 2 lrelu + res + y_pre, GELU pre_deriv
  split-K <32> (3)          splitk32: 12x12 48 -> 40 (ragged M, Cout)     activations, res / res_first, gates, y_pre, pre_deriv, shuffle
                                                                          (+ res + y_pre), slice / odd views, IN_SQUARE GDN / IGDN (3x3),
                                                                          xs lrelu / relu / saved
  split-K <64> (3)          splitk64: 8 x 16x16 64 -> 160                 the model combinations, odd view, GDN + res
                            splitk_pix: 24x24 64 -> 64 (keys 4/5)         lrelu + res + y_pre, halftanh res_first
                            splitk_t2: data gradient, stride 2 (classes)  res + res_gate + out_gate, xs lrelu / relu / saved, MUL2, odd view
  <128,128> heavy128 (4)    heavy128: 8 x 16x16 384 -> 160, bvo, key 17   lrelu + res + y_pre, gelu pre_deriv, res_first + res_gate,
                                                                          og halftanh; odd view / xs / shuffle -> split-K <64>
  <64,64> K-split (4)       ksplit_t: data gradient 512 -> 128 at 32x32   res + res_gate + out_gate, og halftanh, MUL2, gelu pre_deriv,
                                                                          res_first; odd view -> unsplit <64,64>; xs -> register-staged
  <64,64> unsplit (4 / 5)   d64: 3 x 20x20 64 -> 96 (ragged M, Cout)      activations, res, gates, y_pre, shuffle, views, 1x1 form (5)
                            d64_t2: data gradient s2, 16x16 classes       res + res_gate + out_gate (stride-2 class store), odd view
  <128,128> (4 / 5)         d128_reg: 32x64 64 -> 128, key 10 on / off    every epilogue option on the register epilogue and on the LDS one
                            d128_lds: 40x40 64 -> 128 (ragged M)          LDS epilogue, odd view, shuffle; xs / IN_SQUARE -> register-staged
                            d128_t2: data gradient s2 to 80x80            res + res_gate + out_gate, MUL2
  <128,64> / <256,64> /     d128x64: 48x48 64 -> 48                       activations, gates, views; xs -> register-staged
  <128,32> / <64,32>        d256x64: 2 x 256x256 16 -> 64                 lrelu + res + y_pre, res_first + og, odd view
                            d128x32: 256x256 16 -> 24                     lrelu + res + y_pre, gelu pre_deriv, odd view
                            d64x32: 36x40 32 -> 20                        lrelu + res + y_pre, og, shuffle
  <128,64> 1x1 tile (5)     t1x1: 48x48 96 -> 80, key 7                   activations, gates, IN_SQUARE, views
  p1x1 (8)                  p1x1: 256x256 128 -> 128                      y_pre, gates, res_first, IN_SQUARE + GDN / IGDN (+ res), MUL2;
                                                                          act-less bias / res -> lin; odd view / shuffle -> 1x1 tile; xs -> reg.
  n16 (10)                  n16: 64x64 32 -> 12                           activations, res, gates, y_pre, odd view, shuffle; xs -> <64,32>
  lin (11)                  lin / lin_t: 128x256 128 -> 128 fwd / dgrad   bias, res 0.5, slice view; act / y_pre / gate / odd -> 1x1 tile
  halo (12)                 halo / halo_t: 2 x 64x64 128 -> 256           register-epilogue options, shuffle (lrelu / relu);
                                                                          shuffle + res -> <128,128>; odd view -> <128,128>; xs -> reg.
  Winograd 128 / 64 (13)    wino128 / wino64 / wino64_t                   lean and general epilogues, GDN-free options, shuffle (+ res +
                                                                          y_pre, lean and general), out_gate; odd view -> direct tiles
plus the autograd contract of ops.conv2d (y, dx, dw, db, d(res) against float64 autograd) and the filter-gradient prologue of
wgrad_raw / wgrad_batched (dys with its activation, IN_SQUARE, stride 2, accumulation into pre-filled buffers) on every wgrad family.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_ref as R

pytestmark = pytest.mark.gpu

CL = torch.channels_last
NONE, LRELU, RELU, GELU, HTANH, SIGM, SAVED = R.ACT_NONE, R.ACT_LRELU, R.ACT_RELU, R.ACT_GELU, R.ACT_HALFTANH, R.ACT_SIGMOID, R.ACT_SAVED_DERIV
SQ = R.IN_SQUARE
GDN, IGDN, MUL2 = R.NORM_GDN, R.NORM_IGDN, R.NORM_MUL2


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def route(v):
    """kernel-variant id -> family tag (ids: conv_igemm.hip launch_t / launch_dma2_t / launch_splitk_t / launch_n16 / launch_p1x1, conv_halo.hip,
    conv_wino.hip, fused_mlp.hip)"""
    if v == 1:
        return "direct"
    fam, bm, bn = (v >> 20) & 15, (v >> 3) & 511, (v & 7) << 5
    if fam in (1, 3, 4, 5):
        return f"{fam}:{bm}x{bn}"
    if fam == 12:
        return "12" + ("s" if v & 1 else "")
    if fam == 13:
        return "13:" + ("64" if (v >> 12) & 1 else "128") + ("s" if v & 1 else "")
    return str(fam)


# ---------------------------------------------------------------------------------------------------------------------------- recipes
# name: (N, Cin, H, W, Cout, ks, stride, transposed, pack, batch_variant_ok, {tuning key: value}, family tag)
# (transposed: H x W is dY's map, Cin its channels, Cout the launch's output channels; the output map is H x W (stride 1) or 2H x 2W)
RECIPES = {
    "direct": (2, 3, 20, 20, 22, 3, 1, False, None, False, {}, "direct"),
    "direct_s2": (2, 3, 20, 20, 22, 3, 2, False, None, False, {}, "direct"),
    "direct_gdn": (2, 3, 12, 12, 3, 1, 1, False, None, False, {}, "direct"),
    "direct_slice": (2, 8, 12, 10, 16, 3, 1, False, None, False, {}, "direct"),
    "splitk32": (2, 48, 12, 12, 40, 3, 1, False, None, False, {}, "3:32x32"),
    "splitk64": (8, 64, 16, 16, 160, 3, 1, False, None, False, {}, "3:32x64"),
    "splitk_pix": (2, 64, 24, 24, 64, 3, 1, False, None, False, {4: 1024, 5: 64}, "3:32x32"),
    "splitk_t2": (2, 64, 8, 8, 48, 3, 2, True, None, False, {}, "3:32x32"),
    "heavy128": (8, 384, 16, 16, 160, 3, 1, False, None, True, {17: 1}, "4:128x128"),
    "ksplit_t": (2, 512, 32, 32, 128, 3, 1, True, None, False, {11: 1}, "4:64x64"),
    "d64": (3, 64, 20, 20, 96, 3, 1, False, None, False, {}, "4:64x64"),
    "d64_1x1": (3, 64, 20, 20, 96, 1, 1, False, None, False, {}, "5:64x64"),
    "d64_t2": (4, 256, 16, 16, 128, 3, 2, True, None, False, {}, "4:64x64"),
    "d128_reg": (1, 64, 32, 64, 128, 3, 1, False, None, False, {10: 1}, "4:128x128"),
    "d128_lds": (1, 64, 40, 40, 128, 3, 1, False, None, False, {10: 0}, "4:128x128"),
    "d128_ragged": (1, 64, 40, 40, 128, 3, 1, False, None, False, {10: 1}, "4:128x128"),
    "d128_t2": (1, 128, 40, 40, 128, 3, 2, True, None, False, {}, "4:128x128"),
    "d128x64": (1, 64, 48, 48, 48, 3, 1, False, None, False, {}, "4:128x64"),
    "d256x64": (2, 16, 256, 256, 64, 3, 1, False, None, False, {15: 1}, "4:256x64"),
    "d128x32": (1, 16, 256, 256, 24, 3, 1, False, None, False, {15: 1}, "4:128x32"),
    "d64x32": (1, 32, 36, 40, 20, 3, 1, False, None, False, {}, "4:64x32"),
    "t1x1": (1, 96, 48, 48, 80, 1, 1, False, None, False, {7: 8}, "5:128x64"),
    "p1x1": (1, 128, 256, 256, 128, 1, 1, False, None, False, {13: 1}, "8"),
    "n16": (1, 32, 64, 64, 12, 3, 1, False, None, False, {20: 1}, "10"),
    "lin": (1, 128, 128, 256, 128, 1, 1, False, None, False, {21: 1}, "11"),
    "lin_t": (1, 128, 128, 256, 128, 1, 1, True, None, False, {21: 1}, "11"),
    "halo": (2, 128, 64, 64, 256, 3, 1, False, "wpk", False, {22: 1}, "12"),
    "halo_t": (2, 128, 64, 64, 256, 3, 1, True, "wpk", False, {22: 1}, "12"),
    "wino128": (2, 128, 64, 96, 256, 3, 1, False, "wino", False, {23: 7}, "13:128"),
    "wino64": (2, 64, 64, 64, 128, 3, 1, False, "wino", False, {23: 7}, "13:64"),
    "wino64_t": (2, 64, 64, 64, 128, 3, 1, True, "wino", False, {23: 7}, "13:64"),
}

# options: act, res (scale), first (res_first), rg / og = (act, pre), pre (y_pre), deriv (pre_deriv), norm, sq (IN_SQUARE), xs = (act, pre),
# shuf, view ("dense" | "slice": a 16-B aligned channel slice of a wider buffer, input too | "odd": output at channel offset 1, vec_epi off)
O = {
    "none": dict(),
    "lrelu": dict(act=LRELU),
    "relu": dict(act=RELU, bias=False),
    "gelu": dict(act=GELU),
    "htanh": dict(act=HTANH),
    "sigmoid": dict(act=SIGM),
    "lrelu_res_pre": dict(act=LRELU, res=0.5, pre=True),                      # the model's forward layers
    "relu_first": dict(act=RELU, res=1.0, first=True, pre=True),
    "htanh_first05": dict(act=HTANH, res=0.5, first=True, pre=True),
    "gelu_deriv": dict(act=GELU, pre=True, deriv=True),                       # the model's GELU layers
    "lrelu_deriv": dict(act=LRELU, pre=True, deriv=True),
    "htanh_deriv_res": dict(act=HTANH, res=0.5, pre=True, deriv=True),
    "gelu_res": dict(act=GELU, res=0.5, pre=True),
    "dgrad_gates": dict(res=1.0, rg=(LRELU, False), og=(LRELU, False), bias=False),   # the model's data gradients
    "rg_lrelu_pre": dict(act=LRELU, res=0.5, rg=(LRELU, True), pre=True),
    "rg_saved_first": dict(act=RELU, res=0.5, first=True, rg=(SAVED, False), pre=True),
    "og_relu": dict(og=(RELU, False), res=0.5),
    "og_htanh_pre": dict(act=LRELU, og=(HTANH, True), pre=True),
    "og_htanh_out": dict(og=(HTANH, False), res=0.5, rg=(RELU, True)),
    "og_saved": dict(act=GELU, og=(SAVED, False)),
    "mul2_res": dict(norm=MUL2, res=1.0, bias=False),                         # GDN's data gradient
    "gdn_res": dict(norm=GDN, sq=True, res=1.0, pre=True),                    # the model's GDN layers
    "igdn": dict(norm=IGDN, sq=True, pre=True),
    "gdn_lrelu": dict(norm=GDN, sq=True, act=LRELU, og=(RELU, True)),
    "xs_lrelu": dict(xs=(LRELU, True), res=0.5),
    "xs_relu": dict(xs=(RELU, False), act=LRELU, pre=True),
    "xs_saved": dict(xs=(SAVED, False), og=(LRELU, False)),
    "shuf_res_pre": dict(act=LRELU, res=0.5, pre=True, shuf=True),
    "shuf_first": dict(act=RELU, res=1.0, first=True, pre=True, shuf=True),
    "shuf_gelu": dict(act=GELU, res=0.5, pre=True, deriv=True, shuf=True),
    "shuf_lrelu": dict(act=LRELU, shuf=True),
    "slice": dict(act=LRELU, res=0.5, pre=True, view="slice"),
    "slice_gates": dict(res=0.5, rg=(LRELU, True), og=(LRELU, False), view="slice"),
    "odd": dict(act=LRELU, res=0.5, pre=True, view="odd"),
    "odd_gates": dict(act=GELU, res=0.5, first=True, rg=(LRELU, True), og=(HTANH, True), pre=True, deriv=True, view="odd"),
    "odd_plain": dict(res=0.5, view="odd"),
    "odd_og": dict(act=RELU, res=0.5, og=(LRELU, False), view="odd"),          # the lean form of the scalar epilogue with its LeakyReLU gate
    "res_plain": dict(res=0.5),
    "slice_res": dict(res=0.5, view="slice"),
}

ACTS = ["none", "lrelu", "relu", "gelu", "htanh", "sigmoid"]
EPI = ["lrelu_res_pre", "relu_first", "htanh_first05", "gelu_deriv", "lrelu_deriv", "htanh_deriv_res", "gelu_res", "dgrad_gates", "rg_lrelu_pre",
       "rg_saved_first", "og_relu", "og_htanh_pre", "og_htanh_out", "og_saved", "mul2_res"]
XS = ["xs_lrelu", "xs_relu", "xs_saved"]
GDNS = ["gdn_res", "igdn", "gdn_lrelu"]
DGRAD = ["dgrad_gates", "og_htanh_out", "og_saved", "rg_saved_first", "mul2_res", "lrelu_res_pre", "gelu_deriv", "res_plain"]

# recipe -> [(option, expected family or None = the recipe's)]: the explicit coverage table
_ = None
CASES = {
    "direct": [(o, _) for o in ACTS + EPI + ["odd", "odd_gates", "odd_og"]],
    "direct_s2": [(o, _) for o in ["lrelu_res_pre", "og_htanh_pre", "gelu_deriv"]],
    "direct_gdn": [(o, _) for o in GDNS],
    "direct_slice": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "odd"]],
    "splitk32": [(o, _) for o in ACTS + EPI + GDNS + XS + ["shuf_res_pre", "shuf_first", "shuf_gelu", "slice", "slice_gates", "odd", "odd_gates", "odd_og"]],
    "splitk64": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "dgrad_gates", "odd", "gdn_res", "xs_relu", "shuf_res_pre", "htanh"]],
    "splitk_pix": [(o, _) for o in ["lrelu_res_pre", "htanh_first05", "odd_gates"]],
    "splitk_t2": [(o, _) for o in DGRAD + XS + ["odd", "odd_gates", "odd_og", "slice"]],
    "heavy128": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "rg_saved_first", "og_htanh_out", "sigmoid", "slice"]]
                + [("odd", "3:32x64"), ("xs_lrelu", "3:32x64"), ("shuf_res_pre", "3:32x64")],
    "ksplit_t": [(o, _) for o in DGRAD + ["htanh_first05", "slice_gates"]] + [("odd_gates", _), ("odd_og", _), ("xs_lrelu", "1:64x64"), ("xs_saved", "1:64x64")],
    "d64": [(o, _) for o in ACTS + EPI + ["shuf_res_pre", "shuf_first", "slice", "odd", "odd_gates", "odd_og"]] + [("xs_relu", "1:64x64"), ("gdn_res", "1:64x64")],
    "d64_1x1": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "og_htanh_pre", "gdn_res", "igdn", "odd"]] + [("xs_lrelu", "1:64x64")],
    "d64_t2": [(o, _) for o in DGRAD + ["odd_gates"]] + [("xs_saved", "1:64x64")],
    "d128_reg": [(o, _) for o in ACTS + EPI + ["slice", "slice_gates"]],
    "d128_lds": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "rg_saved_first", "og_htanh_out", "og_saved", "mul2_res", "sigmoid", "shuf_res_pre"]],
    "d128_ragged": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "dgrad_gates", "odd", "odd_gates", "odd_og", "shuf_gelu"]]
                   + [("xs_lrelu", "1:128x128"), ("gdn_res", "1:128x128")],
    "d128_t2": [(o, _) for o in ["dgrad_gates", "mul2_res", "og_saved", "odd_gates"]],
    "d128x64": [(o, _) for o in ["lrelu", "gelu_deriv", "htanh_first05", "dgrad_gates", "og_htanh_pre", "sigmoid", "slice", "odd_gates"]]
               + [("xs_saved", "1:128x64")],
    "d256x64": [(o, _) for o in ["lrelu_res_pre", "og_htanh_out", "odd"]],
    "d128x32": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "odd"]],
    "d64x32": [(o, _) for o in ["lrelu_res_pre", "og_htanh_pre", "shuf_res_pre", "odd_gates"]],
    "t1x1": [(o, _) for o in ["none", "htanh", "lrelu_res_pre", "gelu_deriv", "dgrad_gates", "rg_saved_first", "og_saved", "igdn", "slice", "odd"]],
    "p1x1": [(o, _) for o in ["lrelu_res_pre", "gelu_deriv", "htanh_first05", "rg_lrelu_pre", "og_htanh_out", "og_saved", "gdn_res", "igdn",
                              "mul2_res", "sigmoid", "slice"]]
            + [("res_plain", "11"), ("odd", "5:128x64"), ("shuf_res_pre", "5:128x64"), ("xs_lrelu", "1:128x64")],
    "n16": [(o, _) for o in ["lrelu", "gelu", "htanh", "lrelu_res_pre", "gelu_deriv", "dgrad_gates", "og_htanh_pre", "odd", "odd_og", "shuf_res_pre"]]
           + [("xs_relu", "1:64x32")],
    "lin": [("res_plain", _), ("none", _), ("slice_res", _), ("slice", "5:128x64"), ("lrelu", "5:128x64"), ("og_relu", "5:128x64"), ("odd_plain", "5:128x64")],
    "lin_t": [("res_plain", _), ("slice_res", _), ("dgrad_gates", "5:128x64")],
    "halo": [(o, _) for o in ["none", "lrelu", "gelu", "htanh", "lrelu_res_pre", "gelu_deriv", "relu_first", "rg_saved_first", "og_htanh_pre",
                              "og_saved", "slice"]]
            + [("shuf_lrelu", "12s"), ("shuf_res_pre", "4:128x128"), ("odd", "4:128x128"), ("xs_lrelu", "1:128x128")],
    "halo_t": [(o, _) for o in ["dgrad_gates", "og_htanh_out", "res_plain", "mul2_res"]],
    "wino128": [(o, _) for o in ["none", "lrelu_res_pre", "relu_first", "gelu_deriv", "og_htanh_pre", "rg_saved_first", "dgrad_gates", "sigmoid",
                                 "slice"]]
               + [("shuf_res_pre", "13:128s"), ("shuf_gelu", "13:128s"), ("odd", "4:128x128")],
    "wino64": [(o, _) for o in ["lrelu_res_pre", "htanh_first05", "gelu_deriv", "og_saved", "mul2_res", "slice_gates"]]
              + [("shuf_first", "13:64s"), ("shuf_gelu", "13:64s"), ("xs_lrelu", "1:128x128"), ("odd", "4:128x128")],
    "wino64_t": [(o, _) for o in ["dgrad_gates", "og_htanh_out", "mul2_res", "res_plain"]] + [("xs_relu", "1:128x128")],
}
ALL_CASES = [(r, o, e) for r, lst in CASES.items() for o, e in lst]


@functools.lru_cache(maxsize=None)
def _recipe_data(name):
    """CPU float32 operands of a recipe: x [N, Cin, H, W], the kernel-layout filter, bias, and |filter| / positive bias for GDN."""
    N, Cin, H, W, Cout, ks, stride, tr, pack, bvo, keys, fam = RECIPES[name]
    seed = sum(map(ord, name))
    x = _rand((N, Cin, H, W), seed)
    w = _rand((Cout, ks * ks * Cin), seed + 1, (1.0 / (Cin * ks * ks)) ** 0.5)
    b = _rand((Cout,), seed + 2, 0.1)
    g = torch.Generator().manual_seed(seed + 3)
    w_gdn = torch.rand((Cout, ks * ks * Cin), generator=g) * (0.5 / (Cin * ks * ks))      # gamma >= 0
    b_gdn = 0.5 + torch.rand((Cout,), generator=g)                                      # beta in [0.5, 1.5]
    return x, w, b, w_gdn, b_gdn


def _out_hw(name):
    N, Cin, H, W, Cout, ks, stride, tr, *_r = RECIPES[name]
    if tr:
        return (H * stride, W * stride)
    pad = ks // 2
    return ((H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1)


def _xs_of(name, act, pre):
    x = _recipe_data(name)[0]
    return R.away_from_zero(x.shape, 900 + act * 2 + pre)


@functools.lru_cache(maxsize=None)
def _acc(name, gdn, sq, xs):
    """float64 accumulator of a recipe, once per prologue (cached: the large-map GEMMs are the expensive part of this file)"""
    N, Cin, H, W, Cout, ks, stride, tr, *_r = RECIPES[name]
    x, w, b, w_gdn, b_gdn = _recipe_data(name)
    xsv = _xs_of(name, *xs) if xs else None
    return R.gemm(x, w_gdn if gdn else w, ks=ks, stride=stride, transposed=tr, out_hw=_out_hw(name), in_op=SQ if sq else R.IN_NONE,
                  xs=xsv, xs_act=xs[0] if xs else NONE, xs_pre=bool(xs[1]) if xs else False)


@pytest.fixture
def tuned(request):
    """set tuning keys for one test, restored in a finalizer"""
    from clc_amd import lib as _lib

    L = _lib.load()

    def set_keys(keys):
        for k, v in keys.items():
            old = L.clc_set_tuning(k, v)
            assert old >= 0, f"tuning key {k}"
            request.addfinalizer(lambda k=k, old=old: L.clc_set_tuning(k, old))

    return set_keys


def _buffer(dev, N, C, H, W, view, fill=float("nan")):
    """(buffer, view of it): dense; a 16-B aligned channel slice [4, 4 + C) of C + 8 channels; or channels [1, 1 + C) of C + 3 (vec_epi off)"""
    extra, off = {"dense": (0, 0), "slice": (8, 4), "odd": (3, 1)}[view]
    buf = torch.full((N, C + extra, H, W), fill, device=dev).contiguous(memory_format=CL)
    return buf, buf[:, off:off + C]


def _check_untouched(buf, v, what):
    """no NaN left inside the written view; every channel outside it still NaN"""
    assert not torch.isnan(v).any(), f"{what}: NaN left inside the written slice (element not stored)"
    off = v.data_ptr() - buf.data_ptr()
    c0 = off // 4
    C = v.shape[1]
    outside = torch.cat([buf[:, :c0], buf[:, c0 + C:]], 1)
    if outside.numel():
        assert torch.isnan(outside).all(), f"{what}: a channel outside the written slice was overwritten"


def _check(got, want, tol, what, mask=None):
    """per-output-channel relative error: max |got - want| over a channel / max |want| over that channel (floored at 1e-4 of the global max)"""
    g = got.detach().double().cpu()
    err = (g - want).abs()
    if mask is not None:
        err = err.masked_fill(mask, 0.0)
    gmax = max(want.abs().max().item(), 1e-30)
    chmax = want.abs().amax(dim=(0, 2, 3)).clamp_min(1e-4 * gmax)
    rel = err.amax(dim=(0, 2, 3)) / chmax
    c = int(rel.argmax())
    assert rel[c].item() <= tol, f"{what}: rel err {rel[c].item():.3e} > {tol:.0e} in channel {c} (channel max {chmax[c].item():.3e})"


def _run_case(dev, tuned, rname, oname, expect):
    from clc_amd import ops

    N, Cin, H, W, Cout, ks, stride, tr, pack, bvo, keys, fam = RECIPES[rname]
    opt = dict(O[oname])
    expect = expect or fam
    tuned(keys)
    x, w, b, w_gdn, b_gdn = _recipe_data(rname)
    gdn = opt.get("norm") in (GDN, IGDN)
    sq = bool(opt.get("sq"))
    xs = opt.get("xs")
    shuf = bool(opt.get("shuf"))
    view = opt.get("view", "dense")
    act = opt.get("act", NONE)
    OH, OW = _out_hw(rname)
    Co, OHs, OWs = (Cout // 4, 2 * OH, 2 * OW) if shuf else (Cout, OH, OW)
    seed = sum(map(ord, rname + oname))
    wk, bk = (w_gdn, b_gdn) if gdn else (w, b)
    use_bias = opt.get("bias", True)

    # operands (input as a channel slice of a wider buffer for the "slice" view; its other channels hold a large finite value)
    if rname == "direct_slice":
        xb = torch.full((N, Cin + 4, H, W), 1e3).contiguous(memory_format=CL)
        xb[:, 2:2 + Cin] = x
        xd = xb.to(dev)[:, 2:2 + Cin]
    elif view == "slice":
        xb = torch.full((N, Cin + 8, H, W), 1e3).contiguous(memory_format=CL)
        xb[:, 4:4 + Cin] = x
        xd = xb.to(dev)[:, 4:4 + Cin]
    else:
        xd = x.to(dev).contiguous(memory_format=CL)
    wd = wk.to(dev).contiguous()
    bd = bk.to(dev) if use_bias else None
    res = _rand((N, Co, OHs, OWs), seed + 1) if "res" in opt else None
    mul = None
    if opt.get("norm"):
        mul = x if (gdn and sq and Cin == Cout and not tr) else _rand((N, Co, OHs, OWs), seed + 2)
    rg = (R.away_from_zero((N, Co, OHs, OWs), seed + 3), *opt["rg"]) if "rg" in opt else None
    og = (R.away_from_zero((N, Co, OHs, OWs), seed + 4), *opt["og"]) if "og" in opt else None
    xsv = _xs_of(rname, *xs) if xs else None
    D = lambda t: None if t is None else t.to(dev).contiguous(memory_format=CL)
    ybuf, y = _buffer(dev, N, Co, OHs, OWs, view)
    pbuf, yp = _buffer(dev, N, Co, OHs, OWs, view) if opt.get("pre") else (None, None)
    wpk = wwino = None
    if pack == "wpk":
        wpk = ops.halo_pack(wd, Cout, Cin)
    elif pack == "wino":
        wwino = ops.wino_pack(wd, Cout, Cin, flip=tr)
    ops.PROFILE = []
    try:
        ops.conv_raw(xd, wd, bd, ks=ks, stride=stride, act=act, in_op=SQ if sq else R.IN_NONE, norm=opt.get("norm", R.NORM_NONE), mul=D(mul),
                     res=D(res), res_scale=opt.get("res", 1.0), res_first=bool(opt.get("first")), y_pre=yp, shuffle=shuf, transposed=tr,
                     out=y, out_hw=(OH, OW) if tr else None, xs=D(xsv), xs_act=xs[0] if xs else NONE, xs_pre=bool(xs[1]) if xs else False,
                     pre_deriv=bool(opt.get("deriv")), res_gate=(D(rg[0]), rg[1], rg[2]) if rg else None,
                     out_gate=(D(og[0]), og[1], og[2]) if og else None, batch_variant_ok=bvo, wpk=wpk, wwino=wwino)
        torch.cuda.synchronize()
        variants = [r.variant for r in ops.PROFILE if r.fam in ("conv_igemm", "conv_direct_small")]
    finally:
        ops.PROFILE = None
    assert len(variants) == 1, variants
    assert route(variants[0]) == expect, f"{rname}/{oname}: ran {route(variants[0])} (id {variants[0]:#x}), recipe expects {expect}"

    acc = _acc(rname, gdn, sq, tuple(xs) if xs else None)
    epi = dict(act=act, res=res, res_scale=opt.get("res", 1.0), res_first=bool(opt.get("first")), res_gate=rg, y_pre=True,
               pre_deriv=False, norm=opt.get("norm", R.NORM_NONE), mul=mul, out_gate=og, shuffle=shuf)
    want, v = R.epilogue(acc, bk if use_bias else None, **epi)
    want_pre = R.epilogue(acc, bk if use_bias else None, **dict(epi, pre_deriv=bool(opt.get("deriv"))))[1] if opt.get("pre") else None
    mask = None
    if act in (LRELU, RELU):   # the kink of the activation of v itself: which side a |v| ~ 1e-8 lands on is summation-order noise
        mask = v.abs() < 1e-6 * v.abs().max()
        assert mask.double().mean().item() < 1e-3, f"{mask.double().mean().item():.2e} of the elements sit at the kink"
    tol = 1e-4 if tr else 2e-5
    _check_untouched(ybuf, y, f"{rname}/{oname} y")
    _check(y, want, tol, f"{rname}/{oname} y", mask)
    if yp is not None:
        _check_untouched(pbuf, yp, f"{rname}/{oname} y_pre")
        _check(yp, want_pre, tol, f"{rname}/{oname} y_pre", mask)


@pytest.mark.parametrize("rname,oname,expect", ALL_CASES, ids=[f"{r}-{o}" for r, o, _e in ALL_CASES])
def test_conv_family_epilogue_vs_fp64(dev, tuned, rname, oname, expect):
    _run_case(dev, tuned, rname, oname, expect)


def test_every_family_is_in_the_table():
    """the coverage table names every family clc_conv2d has, and every option is run somewhere"""
    fams = {RECIPES[r][-1] if e is None else e for r, o, e in ALL_CASES}
    for tag in ("direct", "3:32x32", "3:32x64", "4:128x128", "4:64x64", "5:64x64", "4:128x64", "4:256x64", "4:128x32", "4:64x32", "5:128x64", "8", "10",
                "11", "12", "12s", "13:128", "13:64", "13:128s", "13:64s", "1:64x64", "1:128x128"):
        assert tag in fams, tag
    assert {o for _r, o, _e in ALL_CASES} == set(O)


# ------------------------------------------------------------------------------------------------------------ autograd of ops.conv2d
# sizes: a <= 16x16 map (split-K family); a ragged 32x32-class map (<64,64> tiles); a 3x3 large map with >= ops.MATERIALIZE_DZ rows (dz as its own
# pass); 128 channels on a 64x128 map (recorded forward and data gradient on the Winograd / halo kernels)
AG_SIZES = {"s16": (2, 32, 12, 12, 48), "r32": (1, 64, 24, 20, 96), "big": (2, 32, 128, 128, 32), "c128": (2, 128, 64, 128, 64)}
AG_RES = {"none": None, "after": (0.5, False), "first1": (1.0, True), "first05": (0.5, True)}
AG_ACTS = [NONE, LRELU, RELU, GELU, HTANH]


def _ag_cases():
    cases = []
    for size in ("s16", "r32"):
        for i, act in enumerate(AG_ACTS):
            for j, res in enumerate(AG_RES):
                cases.append((size, act, res, (i + j) % 2 == 1, (i + 2 * j) % 3 == 2 and size == "s16", ""))
    for size in ("big", "c128"):
        for act, res, shuf, s2 in ((LRELU, "after", False, False), (GELU, "none", False, False), (RELU, "first1", False, False),
                                   (HTANH, "first05", True, False), (LRELU, "none", True, False), (NONE, "after", False, True)):
            cases.append((size, act, res, shuf, s2, ""))
    cases += [("r32", LRELU, "after", False, False, "out_slice"), ("r32", GELU, "first05", False, True, "in_slice"),
              ("s16", RELU, "after", True, False, "out_slice")]
    return cases


AG_CASES = _ag_cases()


@pytest.mark.parametrize("size,act,res,shuf,s2,views", AG_CASES,
                         ids=[f"{c[0]}-{R.ACT_NAMES[c[1]]}-{c[2]}-{'shuf' if c[3] else 'noshuf'}-s{2 if c[4] else 1}{'-' + c[5] if c[5] else ''}" for c in AG_CASES])
def test_conv2d_autograd_vs_fp64(dev, size, act, res, shuf, s2, views):
    from clc_amd import ops

    N, Cin, H, W, Cout = AG_SIZES[size]
    stride = 2 if s2 else 1
    seed = sum(map(ord, f"{size}{act}{res}{shuf}{s2}{views}"))
    x = _rand((N, Cin, H, W), seed)
    w = _rand((Cout, Cin, 3, 3), seed + 1, (1.0 / (Cin * 9)) ** 0.5)
    b = _rand((Cout,), seed + 2, 0.1)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    oshape = (N, Cout // 4, 2 * OH, 2 * OW) if shuf else (N, Cout, OH, OW)
    rs = AG_RES[res]
    r = _rand(oshape, seed + 3) if rs else None
    gy = _rand(oshape, seed + 4)

    if views == "in_slice":
        xb = _rand((N, Cin + 8, H, W), seed + 5).to(dev).contiguous(memory_format=CL)
        xb[:, 4:4 + Cin] = x.to(dev)
        xb.requires_grad_(True)
        xd = xb[:, 4:4 + Cin]
    else:
        xb = xd = x.to(dev).contiguous(memory_format=CL).requires_grad_(True)
    wd = w.to(dev).contiguous(memory_format=CL).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True)
    rd = r.to(dev).contiguous(memory_format=CL).requires_grad_(True) if rs else None
    out = None
    if views == "out_slice":
        obuf = torch.full((oshape[0], oshape[1] + 8, oshape[2], oshape[3]), float("nan"), device=dev).contiguous(memory_format=CL)
        out = obuf[:, 4:4 + oshape[1]]
    ops.PROFILE = []
    try:
        y = ops.conv2d(xd, wd, bd, stride=stride, act=act, res=rd, res_scale=rs[0] if rs else 1.0, res_first=bool(rs and rs[1]), shuffle=shuf, out=out)
        fwd = [route(r.variant) for r in ops.PROFILE if r.fam in ("conv_igemm", "conv_direct_small")]
    finally:
        ops.PROFILE = None
    if size == "c128" and not s2:
        assert fwd and fwd[-1].startswith("13:"), f"recorded forward ran {fwd}, not the Winograd kernels"
    if out is not None:
        _check_untouched(obuf, out, "conv2d out=")
    saved = y.grad_fn.saved_tensors[2]   # the kernel's own saved pre-activation / output: which side of a LeakyReLU / ReLU kink it took
    y.backward(gy.to(dev).contiguous(memory_format=CL))

    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    rr = r.double().requires_grad_() if rs else None
    z = F.conv2d(xr, wr, br, stride=stride, padding=1)
    if shuf:
        z = F.pixel_shuffle(z, 2)
    if rs and rs[1]:
        z = z + rs[0] * rr
    if act in (LRELU, RELU):
        pos = saved.detach().cpu() > 0
        a = torch.where(pos, z, (0.01 if act == LRELU else 0.0) * z)
    else:
        a = R.act_f(z, act)
    if rs and not rs[1]:
        a = a + rs[0] * rr
    a.backward(gy.double())
    _check(y, a.detach(), 2e-5, "y")
    _check(xb.grad[:, 4:4 + Cin] if views == "in_slice" else xd.grad, xr.grad, 1e-4, "dx")
    if views == "in_slice":
        assert (xb.grad[:, :4] == 0).all() and (xb.grad[:, 4 + Cin:] == 0).all()
    _check(wd.grad, wr.grad, 1e-4, "dw")
    assert (bd.grad.double().cpu() - br.grad).abs().max().item() <= 1e-4 * br.grad.abs().max().item(), "db"
    if rs:
        _check(rd.grad, rr.grad, 1e-4, "dres")


def test_conv2d_sigmoid_has_no_backward(dev):
    """ACT_SIGMOID is a forward-only epilogue: a recording forward refuses it with a ClcError (no silent wrong gradient), inference runs it"""
    from clc_amd import lib as _lib
    from clc_amd import ops

    x = _rand((1, 16, 8, 8), 1).to(dev).contiguous(memory_format=CL)
    w = _rand((8, 16, 3, 3), 2, 0.1).to(dev).contiguous(memory_format=CL).requires_grad_(True)
    with pytest.raises(_lib.ClcError, match="SIGMOID"):
        ops.conv2d(x, w, None, act=SIGM)
    with torch.no_grad():
        y = ops.conv2d(x, w, None, act=SIGM)
    want = torch.sigmoid(F.conv2d(x.double().cpu(), w.detach().double().cpu(), None, padding=1))
    _check(y, want, 2e-5, "sigmoid forward")


# ------------------------------------------------------------------------------------------------------------ filter-gradient prologue
# name: (N, Cin, H, W, Cout, ks, stride, expected variant family: "small" (id 1) | "taps" (649xx) | "tiled" (bm * 1000 + bn))
WG_RECIPES = {
    "small": (2, 3, 32, 32, 24, 3, 2, "small"),
    "taps": (2, 64, 32, 32, 64, 3, 1, "taps"),
    "tiled_s2": (2, 128, 32, 32, 96, 3, 2, "tiled"),
    "tiled_1x1": (2, 128, 24, 20, 128, 1, 1, "tiled"),
}
WG_OPTS = {"plain": {}, "lrelu_pre": dict(dys=(LRELU, True)), "relu_out": dict(dys=(RELU, False)), "saved": dict(dys=(SAVED, False)),
           "square": dict(sq=True), "square_lrelu": dict(sq=True, dys=(LRELU, False))}
WG_CASES = [(r, o, mode) for r in WG_RECIPES for o in WG_OPTS if not (o.startswith("square") and WG_RECIPES[r][5] != 1) for mode in ("single", "acc", "batched")]


def _wg_family(v):
    return "small" if v == 1 else ("taps" if 64900 < v < 65000 else ("tiled" if v in (128128, 128064, 64128, 64064) else str(v)))


@pytest.mark.parametrize("rname,oname,mode", WG_CASES, ids=[f"{r}-{o}-{m}" for r, o, m in WG_CASES])
def test_wgrad_prologue_vs_fp64(dev, rname, oname, mode):
    from torch.nn.grad import conv2d_weight

    from clc_amd import lib as _lib
    from clc_amd import ops

    N, Cin, H, W, Cout, ks, stride, fam = WG_RECIPES[rname]
    opt = WG_OPTS[oname]
    pad = ks // 2
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    seed = sum(map(ord, rname + oname))
    x, dy = _rand((N, Cin, H, W), seed), _rand((N, Cout, OH, OW), seed + 1)
    dys = R.away_from_zero((N, Cout, OH, OW), seed + 2) if "dys" in opt else None
    sq = bool(opt.get("sq"))
    D = lambda t: t.to(dev).contiguous(memory_format=CL)
    kw = dict(x=D(x), dy=D(dy), ks=ks, stride=stride, pad=pad, Cout=Cout, Cin=Cin, want_bias=True, in_op=SQ if sq else R.IN_NONE)
    if dys is not None:
        kw.update(dys=D(dys), dys_act=opt["dys"][0], dys_pre=bool(opt["dys"][1]))
    dw0 = _rand((Cout * ks * ks * Cin,), seed + 3, 0.1) if mode != "single" else torch.zeros(Cout * ks * ks * Cin)
    db0 = _rand((Cout,), seed + 4, 0.1) if mode != "single" else torch.zeros(Cout)
    ops.PROFILE = []
    try:
        if mode == "single":
            dw, db = ops.wgrad_raw(**kw)
        else:
            dw, db = dw0.to(dev), db0.to(dev)
            if mode == "acc":
                ops.wgrad_raw(**kw, dw_out=dw, db_out=db)
            else:
                keep = ops.wgrad_batched([dict(kw, dw_out=dw, db_out=db)])   # stream-K grouped launch (key 1 at its default)
        torch.cuda.synchronize()
        recs = [r.variant for r in ops.PROFILE if r.fam in ("conv_wgrad", "wgrad_small")]
    finally:
        ops.PROFILE = None
    d = _lib.WgradDesc()
    d.N, d.H, d.W, d.Cin, d.ldx, d.OH, d.OW, d.Cout, d.lddy, d.ks, d.stride, d.pad = N, H, W, Cin, Cin, OH, OW, Cout, Cout, ks, stride, pad
    planned = ops._L().clc_conv2d_wgrad_variant(__import__("ctypes").byref(d))
    assert _wg_family(planned) == fam, planned
    if mode != "batched":
        assert recs and recs[-1] == planned, (recs, planned)
    xi = x.double() ** 2 if sq else x.double()
    g = dy.double() * (R.act_d(dys.double(), opt["dys"][0], opt["dys"][1]) if dys is not None else 1.0)
    want_w = conv2d_weight(xi, (Cout, Cin, ks, ks), g, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1)   # kernel layout
    want_b = g.sum((0, 2, 3))
    gw, gb = dw.double().cpu() - dw0.double(), db.double().cpu() - db0.double()
    rows = lambda t: t.view(Cout, -1)
    err_w = ((rows(gw) - rows(want_w)).abs().amax(1) / rows(want_w).abs().amax(1).clamp_min(1e-4 * want_w.abs().max())).max().item()
    assert err_w <= 1e-4, f"dW rel err {err_w:.3e}"
    assert (gb - want_b).abs().max().item() <= 1e-4 * want_b.abs().max().item(), "dbias"
