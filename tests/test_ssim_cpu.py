"""clc_amd.ssim without a GPU: the pytorch_msssim import surface of compat.install(), the window, and the argument checks
(ValueError before anything reaches the GPU)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compat_exposes_pytorch_msssim_api():
    code = r"""
import clc_amd.compat as c
c.install()
from pytorch_msssim import ssim, ms_ssim, SSIM, MS_SSIM
import clc_amd.ssim, clc_amd.train
assert ms_ssim is clc_amd.train.ms_ssim
assert ssim is clc_amd.ssim.ssim and SSIM is clc_amd.ssim.SSIM and MS_SSIM is clc_amd.ssim.MS_SSIM
m = MS_SSIM(data_range=1.0, channel=1, win_size=7)
assert tuple(m.win.shape) == (1, 1, 1, 7) and m.data_range == 1.0
assert SSIM().data_range == 255
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-2000:]


def test_default_window_is_the_clc_ssim_init_window():
    """ssim_window(11, 1.5) carries the fp32 taps clc_ssim_init uploads (its loop is folded to these constants at compile time)."""
    from clc_amd import ops

    bits = [C.c_uint32.from_buffer(C.c_float(t)).value for t in ops.ssim_window(11, 1.5)]
    half = [0x3a86cab8, 0x3bf8ff02, 0x3d13758c, 0x3ddff880, 0x3e5a1e20, 0x3e8832b1]
    assert bits == half + half[-2::-1]


@pytest.mark.parametrize("ws, sigma", [(3, 1.5), (7, 1.0), (15, 2.0)])
def test_window_is_fspecial_gauss_1d(ws, sigma):
    from clc_amd import ops

    coords = torch.arange(ws, dtype=torch.float) - ws // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    taps = torch.tensor(ops.ssim_window(ws, sigma))
    assert len(taps) == ws and (taps - g).abs().max().item() <= 1e-7


def test_custom_win_taps():
    from clc_amd import ops

    w = torch.tensor([0.1, 0.2, 0.4, 0.2, 0.1])
    assert ops.ssim_window_taps(win=w.view(1, 1, 1, 5).repeat(3, 1, 1, 1)) == tuple(w.tolist())
    bad = w.view(1, 1, 1, 5).repeat(3, 1, 1, 1)
    bad[1, 0, 0, 0] = 0.0
    with pytest.raises(ValueError):
        ops.ssim_window_taps(win=bad)


@pytest.mark.parametrize("case", ["even_window", "window_too_large", "even_custom_win", "ms_ssim_too_small", "ssim_too_small",
                                  "shape_mismatch", "not_4d", "not_fp32", "too_many_scales"])
def test_argument_checks_raise_value_error_on_cpu(case):
    from clc_amd import ssim

    x = torch.rand(1, 3, 200, 210)
    y = torch.rand(1, 3, 200, 210)
    call = {
        "even_window": lambda: ssim.ms_ssim(x, y, win_size=10),
        "window_too_large": lambda: ssim.ssim(x, y, win_size=17),
        "even_custom_win": lambda: ssim.ssim(x, y, win=torch.ones(3, 1, 1, 4) / 4),
        "ms_ssim_too_small": lambda: ssim.ms_ssim(x[..., :160], y[..., :160]),
        "ssim_too_small": lambda: ssim.ssim(x[..., :10, :], y[..., :10, :]),
        "shape_mismatch": lambda: ssim.ms_ssim(x, y[..., :209]),
        "not_4d": lambda: ssim.ssim(x[None], y[None]),
        "not_fp32": lambda: ssim.ssim(x.double(), y.double()),
        "too_many_scales": lambda: ssim.ms_ssim(x, y, weights=[0.1] * 7),
    }[case]
    with pytest.raises(ValueError):
        call()


def test_cpu_tensors_are_refused_without_fallback():
    from clc_amd import lib, ssim

    with pytest.raises(lib.ClcError):
        ssim.ms_ssim(torch.rand(1, 3, 200, 200), torch.rand(1, 3, 200, 200))
