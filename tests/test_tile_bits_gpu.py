"""The five kernels that hold a copy of the f32 MFMA tile loop (conv5_kernel, conv5_wgrad_kernel of csrc/conv5.hip; ckbd_conv_kernel,
ckbd_wgrad_kernel of csrc/ckbd_context.hip; row_gemm_kernel of csrc/row_gemm.hip) give the BITS of the build that wrote
tests/golden/tile_gemm_bits.npz.  The float64 bounds of the kernel tests allow any summation order and their integer operands are
exact in any order, so only this test sees a changed ORDER RULE (stated in each of the three files) — on which three coders' streams
rest.  A fix to one copy of the loop that forks it from the other two shows here.

The file holds one pool of float32 randn values (stored, never re-drawn; every case cuts its operands from the pool's start) and the
outputs of the three cases.  The cases are the smallest that reach every part of the loop — two K chunks with a tail (36 channels),
several taps / ranges, a partial row tile, rows crossing an image border, a Cout tail below one quad group:
  conv5     Conv2d(36, 8, 5, stride=2) on [2, 36, 6, 10], LeakyReLU: y, dx (the stride-2 transposed launch, four parity classes), dw
  ckbd      ops.ckbd_conv 36 -> 8 on [2, 36, 5, 7], LeakyReLU: y, dx, dw
  row_gemm  the four-range configuration "4" of test_row_gemm_gpu.py (pixel 36, dense 32, pixel 68, dense 4: K = 140), P = 43, B = 3,
            one list entry outside the map, N = 66, ReLU: out, the sentinel rows included

A DELIBERATE change of the summation order must regenerate the file AND raise kGeneration (the kernel generation in
clc_kernel_config_tag) with it: streams written before the change no longer decode.  To regenerate, run this module with
CLC_WRITE_TILE_BITS=1 and CLC_LIB_PATH at the library of the build whose bits are to be kept (_write_golden below).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_gemm_bits.npz")
CL = torch.channels_last
SENTINEL = -777.0
H, W = 3, 5                      # the map of the row_gemm case
P, B, BAD, N = 43, 3, 7, 66      # its list: entry BAD lies outside the map
POOL = 18630                     # the largest case (row_gemm) takes this many values


class _Pool:
    def __init__(self, values):
        self.v, self.at = values, 0

    def take(self, *shape):
        n = int(np.prod(shape))
        out = self.v[self.at:self.at + n].clone().view(*shape)
        assert out.numel() == n, "the pool is too small"
        self.at += n
        return out


def _conv5(pool, dev):
    from clc_amd import layers
    from clc_amd.ops import ACT_LRELU

    x, w, b, dy = pool.take(2, 36, 6, 10), pool.take(8, 36, 5, 5), pool.take(8), pool.take(2, 8, 3, 5)
    layer = layers.Conv2d(36, 8, 5, stride=2).to(dev)
    with torch.no_grad():
        layer.weight.copy_(w.to(dev))
        layer.bias.copy_(b.to(dev))
    xg = x.to(dev).contiguous(memory_format=CL).requires_grad_()
    y = layer(xg, act=ACT_LRELU)
    y.backward(dy.to(dev).contiguous(memory_format=CL))
    return {"y": y.detach(), "dx": xg.grad, "dw": layer.weight.grad}


def _ckbd(pool, dev):
    from clc_amd import ops

    x, w, b, dy = pool.take(2, 36, 5, 7), pool.take(8, 36, 5, 5), pool.take(8), pool.take(2, 8, 5, 7)
    xg = x.to(dev).contiguous(memory_format=CL).requires_grad_()
    wg, bg = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y = ops.ckbd_conv(xg, wg, bg, act=ops.ACT_LRELU)
    y.backward(dy.to(dev).contiguous(memory_format=CL))
    return {"y": y.detach(), "dx": xg.grad, "dw": wg.grad}


def _row_gemm(pool, dev):
    from clc_amd import ops
    from test_row_gemm_gpu import RANGES, _pixels

    rows = B * P
    srcs = []
    for kind, Cc, extra, off in RANGES["4"]:   # the pool holds the channels that are read; the rest of each buffer is zero
        if kind == "pixel":
            t = torch.zeros((B, off + Cc + extra, H, W)).contiguous(memory_format=CL)
            t[:, off:off + Cc] = pool.take(B, Cc, H, W)
            srcs.append((kind, t.to(dev)[:, off:off + Cc]))
        else:
            t = torch.zeros((rows + 3, Cc + extra))
            t[:rows, :Cc] = pool.take(rows, Cc)
            srcs.append((kind, t.to(dev)[:, :Cc]))
    w, bias = pool.take(N, 140), pool.take(N)
    pix = _pixels(P, BAD, torch.Generator().manual_seed(43))
    out = torch.full((rows, N), SENTINEL, device=dev)
    ops.row_gemm(srcs, pix.to(dev), B, H, W, w.to(dev), bias.to(dev), out, act=ops.ACT_RELU)
    assert int((out == SENTINEL).all(1).sum()) == B   # the outside pixel's row of every image
    return {"out": out}


CASES = {"conv5": _conv5, "ckbd": _ckbd, "row_gemm": _row_gemm}


def _write_golden(dev):
    """Writes the fixture from the loaded library: meant for the build BEFORE a change, hence CLC_LIB_PATH is required."""
    assert os.environ.get("CLC_LIB_PATH"), "CLC_WRITE_TILE_BITS=1 needs CLC_LIB_PATH at the library whose bits are to be kept"
    values = torch.randn(POOL, generator=torch.Generator().manual_seed(20221))
    data = {"pool": values.numpy()}
    for name, run in CASES.items():
        for key, t in run(_Pool(values), dev).items():
            data[f"{name}.{key}"] = t.cpu().contiguous().numpy()   # logical NCHW order
    np.savez_compressed(GOLDEN, **data)
    assert os.path.getsize(GOLDEN) < 200 * 1024


@pytest.fixture(scope="module")
def golden():
    if os.environ.get("CLC_WRITE_TILE_BITS") == "1":
        _write_golden(torch.device("cuda:0"))
    with np.load(GOLDEN) as f:
        return {k: torch.from_numpy(f[k]) for k in f.files}


@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_recorded_build(golden, name):
    got = CASES[name](_Pool(golden["pool"]), torch.device("cuda:0"))
    for key, t in got.items():
        want = golden[f"{name}.{key}"]
        same = torch.equal(t.cpu().contiguous(), want)
        print(f"{name}.{key}: {tuple(want.shape)} {'same bits' if same else 'DIFFERENT bits'}")
        assert same, f"{name}.{key}: the summation order changed (see the module docstring before regenerating)"
