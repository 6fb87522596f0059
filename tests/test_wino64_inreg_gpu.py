"""conv_wino64_kernel (csrc/conv_wino.hip) with the input transform in registers: every lane builds its MFMA A operand (row w of B^T d B for one
tile and four channels) from the LDS-resident halo, no V buffer.  Same entry points and bars as test_kernels_gpu.py::
test_wino_conv_vs_direct_and_fp64, on the smallest shapes the host rule (N * (H / 8) * (W / 16) * (rows / 64) >= 128) still gives to the 64-wide
kernel; every case asserts through the launch record that the 64-wide kernel ran."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _dev(t, dev):
    return t.to(dev).contiguous(memory_format=CL)


CASES = [
    # N, H, W, Cin, Cout, mode
    (2, 64, 128, 64, 64, "lrelu_res"),       # bias, LeakyReLU and residual
    (2, 64, 128, 128, 64, "plain"),          # two 64-channel groups: the halo re-deposited inside an item
    (1, 64, 128, 192, 128, "plain"),         # Cin not a multiple of 128, two n-tiles
    (16, 24, 48, 64, 64, "plain"),           # non-power-of-two map: every border class of tile
    (2, 64, 128, 64, 64, "dgrad_gate"),      # data gradient: flipped taps, gated output
    (1, 32, 128, 64, 256, "shuffle_lrelu"),  # PixelShuffle epilogue: conv_wino64_kernel<true>
    (2, 64, 128, 64, 64, "strided"),         # a channel slice of a wider buffer: ldx > Cin
]


@pytest.mark.parametrize("N,H,W,Cin,Cout,mode", CASES)
def test_wino64_inreg_vs_direct_and_fp64(dev, N, H, W, Cin, Cout, mode):
    """Against an fp64 convolution the 64-wide Winograd kernel's error is no larger than the direct kernel's (and inside the existing
    3e-6 / 1.5 e_d + 2e-7 bars); against the direct kernel it is within 4e-6 of the largest output."""
    from clc_amd import lib, ops
    from clc_amd.ops import ACT_LRELU

    L = lib.load()
    restore = L.clc_set_tuning(23, 7)     # (bit 2: the 64-wide instantiation)
    try:
        g = torch.Generator().manual_seed(N * 1000 + H + Cout)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).to(dev).contiguous(memory_format=CL)
        b = (torch.randn(Cout, generator=g) * 0.1).to(dev)
        wk = ops.to_kernel_weight(w)
        tr = mode == "dgrad_gate"
        rows_out = Cin if tr else Cout          # the launch's output channels
        ptiles = N * (H // 8) * (W // 16)
        assert ptiles * (rows_out // 64) >= 128                                                      # the host rule's floor for the 64-wide kernel ...
        assert not (Cin % 128 == 0 and Cout % 128 == 0 and ptiles * (rows_out // 128) >= 192)        # ... and not the 128-wide one's launch
        kw = dict(ks=3, stride=1)
        if tr:   # "x" is dY [N, Cout, H, W]; the launch's K channels = Cout, its rows = Cin
            x = _dev(torch.randn(N, Cout, H, W, generator=g), dev)
            assert ops.wino_ok(N, H, W, Cout, Cin, 3, 1, transposed=True)
            wt = ops.filter_transpose(wk, Cout, 9, Cin).view(Cin, -1)
            u = ops.wino_pack(wt, Cin, Cout, flip=True)
            gate = _dev(torch.randn(N, Cin, H, W, generator=g), dev)
            res = _dev(torch.randn(N, Cin, H, W, generator=g), dev)
            run = lambda wwino: ops.conv_raw(x, wt, None, ks=3, stride=1, pad=1, transposed=True, out_hw=(H, W), out_gate=(gate, ACT_LRELU, False),
                                             res=res, res_scale=0.25, wwino=wwino)
            ref = F.conv_transpose2d(x.double().cpu(), w.double().cpu(), padding=1)
            ref = (ref + 0.25 * res.double().cpu()) * torch.where(gate.double().cpu() > 0, 1.0, 0.01)
        else:
            wide = _dev(torch.randn(N, 2 * Cin, H, W, generator=g), dev)
            x = wide[:, Cin:] if mode == "strided" else _dev(torch.randn(N, Cin, H, W, generator=g), dev)
            assert ops.wino_ok(N, H, W, Cin, Cout, 3, 1)
            ref = F.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
            if mode in ("plain", "strided"):
                kw.update(bias=b)
            elif mode == "lrelu_res":
                r = _dev(torch.randn(N, Cout, H, W, generator=g), dev)
                kw.update(bias=b, act=ACT_LRELU, res=r, res_scale=0.5)
                ref = F.leaky_relu(ref, 0.01) + 0.5 * r.double().cpu()
            elif mode == "shuffle_lrelu":
                kw.update(bias=b, act=ACT_LRELU, shuffle=True)
                ref = F.pixel_shuffle(F.leaky_relu(ref, 0.01), 2)
            outw = ops.new_act(N, 2 * Cout, H, W, wide) if mode == "strided" else None
            run = lambda wwino: ops.conv_raw(x, wk, kw.get("bias"), **{k: v for k, v in kw.items() if k != "bias"}, wwino=wwino,
                                             out=(outw[:, :Cout] if outw is not None else None))
            u = ops.wino_pack(wk, Cout, Cin)
        ops.PROFILE = []
        try:
            y_w = run(u).clone()
            y_d = run(None).clone()
            torch.cuda.synchronize()
            full = [r.variant for r in ops.PROFILE if r.fam == "conv_igemm"]
        finally:
            ops.PROFILE = None
        assert (full[0] >> 20) == 13 and (full[1] >> 20) != 13, [hex(v) for v in full]       # the Winograd kernel ran, then a direct one
        assert (full[0] >> 12) & 1, hex(full[0])                                              # ... its 64-wide instantiation
        assert (full[0] & 1) == (1 if mode == "shuffle_lrelu" else 0), hex(full[0])          # ... <true> for the PixelShuffle store
        assert ((full[0] >> 4) & 0xFF) == (Cout if tr else Cin) // 64, hex(full[0])          # ... over this many 64-channel groups
        scale = ref.abs().max().item()
        e_w = (y_w.double().cpu() - ref).abs().max().item() / scale
        e_d = (y_d.double().cpu() - ref).abs().max().item() / scale
        d_wd = (y_w - y_d).abs().max().item() / scale
        print(f"wino64 {N}x{H}x{W} {Cin}->{Cout} {mode}: err vs fp64 winograd {e_w:.2e} direct {e_d:.2e}; winograd vs direct {d_wd:.2e}")
        assert e_w <= e_d, (e_w, e_d)
        assert e_w < 3e-6 and e_w < 1.5 * e_d + 2e-7, (e_w, e_d)
        assert d_wd < 4e-6
    finally:
        L.clc_set_tuning(23, restore)
