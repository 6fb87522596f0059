"""MS-SSIM forward + backward (gradient for x only): the previous kernels (clc_ssim_scale_fwd / clc_ssim_scale_bwd + clc_avgpool2,
window in __constant__ memory) against the descriptor kernels behind clc_amd.ops.ms_ssim, interleaved in one process.

Both legs run the same Python shape: an autograd Function over the per-scale C calls and the same product of powers.  Each round
times --iters free-running forward + backward passes of one leg between two device events (the legs alternate which goes first);
the median round is the number.  "eager" rounds include the host's launch cost; "graphed" rounds replay one captured hipGraph of
forward + backward per leg, so they time the kernels alone.  Before timing, the legs' loss and dx are compared bit for bit.

    python tools/bench_msssim.py [--shape 4,3,512,512] [--iters 20] [--rounds 9]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CL = torch.channels_last


class _PreviousMeans(torch.autograd.Function):
    """The previous ops path: clc_ssim_init + clc_ssim_scale_fwd / clc_ssim_scale_bwd + clc_avgpool2 (even sides, dx only)."""

    @staticmethod
    def forward(ctx, x, y, levels, data_range):
        from clc_amd import lib

        L = lib.load()
        st = torch.cuda.current_stream().cuda_stream
        lib.check(L.clc_ssim_init(), "clc_ssim_init")
        B, Cc = x.shape[0], x.shape[1]
        xs, ys = [x], [y]
        means = torch.empty((levels, B * Cc, 2), device=x.device)
        for s in range(levels):
            xc, yc = xs[-1], ys[-1]
            h, w = xc.shape[2], xc.shape[3]
            nbytes = L.clc_ssim_workspace_bytes(B, h, w, Cc)
            ws = torch.empty((nbytes + 3) // 4, device=x.device)
            lib.check(L.clc_ssim_scale_fwd(xc.data_ptr(), Cc, yc.data_ptr(), Cc, B, h, w, Cc, data_range, means[s].data_ptr(), ws.data_ptr(),
                                           nbytes, st), "clc_ssim_scale_fwd")
            if s + 1 < levels:
                xn = torch.empty((B, Cc, h // 2, w // 2), device=x.device, memory_format=CL)
                yn = torch.empty((B, Cc, h // 2, w // 2), device=x.device, memory_format=CL)
                lib.check(L.clc_avgpool2(xc.data_ptr(), Cc, xn.data_ptr(), B, h, w, Cc, st), "clc_avgpool2")
                lib.check(L.clc_avgpool2(yc.data_ptr(), Cc, yn.data_ptr(), B, h, w, Cc, st), "clc_avgpool2")
                xs.append(xn)
                ys.append(yn)
        ctx.data_range = data_range
        ctx.save_for_backward(*xs, *ys)
        return means

    @staticmethod
    def backward(ctx, g):
        from clc_amd import lib

        L = lib.load()
        st = torch.cuda.current_stream().cuda_stream
        saved = ctx.saved_tensors
        levels = len(saved) // 2
        g = g.contiguous()
        dnext = None
        for s in reversed(range(levels)):
            xc, yc = saved[s], saved[levels + s]
            B, Cc, h, w = xc.shape
            nbytes = L.clc_ssim_workspace_bytes(B, h, w, Cc)
            ws = torch.empty((nbytes + 3) // 4, device=xc.device)
            dx = torch.empty((B, Cc, h, w), device=xc.device, memory_format=CL)
            lib.check(L.clc_ssim_scale_bwd(xc.data_ptr(), Cc, yc.data_ptr(), Cc, B, h, w, Cc, ctx.data_range, g[s].data_ptr(),
                                           dnext.data_ptr() if dnext is not None else None, dx.data_ptr(), Cc, ws.data_ptr(), nbytes, st),
                      "clc_ssim_scale_bwd")
            dnext = dx
        return dnext, None, None, None


def previous_ms_ssim(x, y, data_range=1.0):
    from clc_amd import ops

    B, Cc = x.shape[0], x.shape[1]
    W = ops.MS_SSIM_WEIGHTS
    return ops.ms_ssim_combine(_PreviousMeans.apply(x, y, len(W), float(data_range)).view(len(W), B, Cc, 2), W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4,3,512,512")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    from clc_amd import ops
    from clc_amd.recipe import synthetic_image

    B, Cc, H, W = (int(v) for v in a.shape.split(","))
    if Cc != 3:
        raise SystemExit("--shape: synthetic_image makes 3-channel images")
    dev = torch.device("cuda:0")
    y = synthetic_image(B, H, W, 5, smooth=True).to(dev).contiguous(memory_format=CL)
    g = torch.Generator().manual_seed(6)
    x0 = (y.cpu() + 0.05 * torch.randn(y.shape, generator=g)).clamp(0, 1).to(dev).contiguous(memory_format=CL)
    legs = {"previous": previous_ms_ssim, "descriptor": ops.ms_ssim}
    res = {}
    for name, fn in legs.items():
        x = x0.clone().requires_grad_()
        loss = fn(x, y, data_range=1.0)
        loss.backward()
        res[name] = (loss.detach(), x.grad)
    bit_identical = torch.equal(res["previous"][0], res["descriptor"][0]) and torch.equal(res["previous"][1], res["descriptor"][1])

    def run(fn, n):
        x = x0.clone().requires_grad_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            x.grad = None
            fn(x, y, data_range=1.0).backward()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def capture(fn):
        xs = x0.clone()

        def step():
            xl = xs.detach().requires_grad_()
            return torch.autograd.grad(fn(xl, y, data_range=1.0), xl)[0]

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        return graph

    def replay(graph, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    graphs = {k: capture(fn) for k, fn in legs.items()}
    modes = {"eager": lambda k, n: run(legs[k], n), "graphed": lambda k, n: replay(graphs[k], n)}
    out = {"bench": "ms_ssim_fwd_bwd", "shape": [B, Cc, H, W], "iters": a.iters, "rounds": a.rounds, "bit_identical": bit_identical}
    for mode, timed in modes.items():
        for k in legs:
            timed(k, 3)
        times = {k: [] for k in legs}
        for r in range(a.rounds):
            for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                times[k].append(timed(k, a.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        out[mode] = {"ms_per_iter_median": {k: round(v, 4) for k, v in med.items()},
                     "ms_per_iter_rounds": {k: [round(t, 4) for t in v] for k, v in times.items()},
                     "descriptor_over_previous": round(med["descriptor"] / med["previous"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
