"""Micro-benchmark of the scale-space operators (csrc/scale_space.hip) -> profiles/ssf_bench.json.

Legs: scale_space_volume + scale_space_warp, forward alone and forward + backward (gradients to the frame, the flow and the scale, so
the volume gradient's sorted gather and the volume's adjoint chain run), at 256x256 and 512x768, batch 1 and 4, L = 5, sigma0 = 1.5.
Baseline: the same composition through torch's own GPU ops in float32 — the plain-torch restatement of tests/ssf_ref.py (depthwise
conv2d on a replicate-padded frame, avg_pool2d, F.interpolate, torch.stack, F.grid_sample), never the code under test.
Device time by events, every shape warmed up, at least `window-ms` of work per timing, `rounds` timings per leg, the two legs of a
shape alternating in one process; median and range (min .. max).  The expectation is "not slower"; the ratio is recorded whatever it
is, and the exit status is 0 either way.  GB/s = the bytes the operators must move (frame in, volume out and in, flow, scale and
output; backward: the same again for the gradients) over the median time.

Fails without a GPU; there is no fallback.
usage: python tools/bench_ssf.py [--rounds 7] [--window-ms 100] [--out profiles/ssf_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import ssf_ref
from clc_amd.scale_space import scale_space_volume, scale_space_warp

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssf_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ssf.py measures on the GPU: none found")
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
L, SIGMA0 = 5, 1.5


def time_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def measure(legs, nbytes):
    reps = {}
    for k, fn in legs.items():
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2, int(args.window_ms * 1e3 / time_us(fn, 2)) + 1)
    t = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            t[k].append(time_us(fn, reps[k]))
    out = {}
    for k, v in t.items():
        v = sorted(v)
        out[k] = {"us_median": v[len(v) // 2], "us_min": v[0], "us_max": v[-1], "calls_per_timing": reps[k], "gb_per_s": nbytes / v[len(v) // 2] / 1e3}
    return out


report = {"levels": L, "sigma0": SIGMA0, "rounds": args.rounds, "window_ms": args.window_ms, "device": torch.cuda.get_device_name(0), "shapes": []}
for B, H, W in ((1, 256, 256), (4, 256, 256), (1, 512, 768), (4, 512, 768)):
    D = L + 1
    x = torch.rand((B, 3, H, W), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    info = torch.cat((torch.randn((B, 2, H, W), generator=g) * 0.05, torch.randn((B, 1, H, W), generator=g) * 0.5), 1)
    info = info.to(dev).contiguous(memory_format=torch.channels_last)
    dy = torch.rand((B, 3, H, W), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    xn, infon, dyn = x.contiguous(), info.contiguous(), dy.contiguous()   # torch's ops at their native layout

    def hip_fwd():
        with torch.no_grad():
            return scale_space_warp(scale_space_volume(x, SIGMA0, L), info[:, :2], info[:, 2:3])

    def torch_fwd():
        with torch.no_grad():
            return ssf_ref.warp(ssf_ref.volume(xn, SIGMA0, L), infon[:, :2], infon[:, 2:3])

    def hip_both():
        a, b = x.detach().requires_grad_(), info.detach().requires_grad_()
        scale_space_warp(scale_space_volume(a, SIGMA0, L), b[:, :2], b[:, 2:3]).backward(dy)
        return a.grad, b.grad

    def torch_both():
        a, b = xn.detach().requires_grad_(), infon.detach().requires_grad_()
        ssf_ref.warp(ssf_ref.volume(a, SIGMA0, L), b[:, :2], b[:, 2:3]).backward(dyn)
        return a.grad, b.grad

    # the two routes compute the same thing (also the first warm-up)
    ya, yb = hip_fwd(), torch_fwd()
    (ga, fa), (gb, fb) = hip_both(), torch_both()
    diffs = {"y": (ya - yb).abs().max().item(), "dx_of_max": ((ga - gb).abs().max() / gb.abs().max()).item(),
             "dflow_dscale_of_max": ((fa - fb).abs().max() / fb.abs().max()).item()}
    pix = B * H * W
    fwd_bytes = 4.0 * pix * (3 + 2 * 4 * D + 3 + 3)   # frame, the volume written and read (16-byte voxels), flow | scale, output
    case = {"batch": B, "frame": [H, W], "max_diff": diffs, "legs": {}}
    for name, legs, nbytes in (("forward", {"hip": hip_fwd, "torch": torch_fwd}, fwd_bytes),
                               ("forward_backward", {"hip": hip_both, "torch": torch_both}, 2 * fwd_bytes)):
        res = measure(legs, nbytes)
        res["ratio_torch_over_hip"] = res["torch"]["us_median"] / res["hip"]["us_median"]
        res["hip_not_slower"] = bool(res["hip"]["us_median"] <= res["torch"]["us_median"])
        case["legs"][name] = res
        print(f"{B}x{H}x{W} {name:17s} | " + " | ".join(
            f"{k} {res[k]['us_median']:9.1f} us [{res[k]['us_min']:.1f} .. {res[k]['us_max']:.1f}] {res[k]['gb_per_s']:7.1f} GB/s" for k in legs)
            + f" | x{res['ratio_torch_over_hip']:.2f}", flush=True)
    report["shapes"].append(case)
    del x, info, dy, xn, infon, dyn
report["hip_not_slower_everywhere"] = all(leg["hip_not_slower"] for c in report["shapes"] for leg in c["legs"].values())
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("the HIP operators are not slower than torch's composition on every leg:", report["hip_not_slower_everywhere"])
