"""Micro-benchmark of the 5x5 kernels (csrc/conv5.hip) -> profiles/conv5_bench.json.

Shapes: the layers of bmshj2018-hyperprior (N = 128, M = 192) at 256x256, batch 8.  Device time by events, at least `window-ms` of work
per timing, `rounds` timings per leg, the legs of one shape alternating in one process; median and range (min .. max).
TF = algorithmic FLOP / time (a transposed launch counts the live taps only), share of the 157.3 TF f32-MFMA peak.

  BAR      forward 128 -> 128, 5x5 / stride 2 on 128x128 (26.8 GFLOP): the direct kernel against the only route to the same result
           that existed before it — clc_im2col_small patch rows (3200 columns) + the 1x1 kernel.  The direct kernel's median must be
           below that route's and the two ranges must not overlap, else exit status 1.
  no bar   its deconv twin (64x64 -> 128x128), its filter gradient, the 192-channel 16x16 -> 8x8 hyper layer (a latency point), a full
           training step of ScaleHyperprior(128, 192) on the batch (forward + RD loss + backward, plain autograd), and — as context —
           the 128 -> 128 3x3 / stride-2 layer on the same map (the launch tools/bench_conv.py times).
  optional --torch: the plain-torch restatement's training step on the same GPU (off by default: it needs the vendor convolution
           library's kernel search, which may not run everywhere; a failure is recorded, not fatal).
usage: python tools/bench_conv5.py [--rounds 7] [--window-ms 100] [--out profiles/conv5_bench.json] [--no-step] [--torch]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from clc_amd import ops

PEAK_TF = 157.3
CL = torch.channels_last
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv5_bench.json"))
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--torch", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_conv5.py measures on the GPU: none found")
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)


def time_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def measure(legs, flop):
    """legs: {name: fn}; alternating rounds; -> {name: stats}"""
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
        out[k] = {"us_median": v[len(v) // 2], "us_min": v[0], "us_max": v[-1], "calls_per_timing": reps[k]}
        if flop:
            out[k]["tflops"] = flop / out[k]["us_median"] / 1e6
            out[k]["share_of_f32_mfma_peak"] = out[k]["tflops"] / PEAK_TF
    return out


def show(name, flop, res):
    print(f"{name:34s} {flop / 1e9:7.2f} GF | " + " | ".join(
        f"{k} {r['us_median']:9.1f} us [{r['us_min']:.1f} .. {r['us_max']:.1f}]" + (f" {r['tflops']:5.1f} TF {100 * r['share_of_f32_mfma_peak']:4.1f}%" if "tflops" in r else "")
        for k, r in res.items()), flush=True)


def rnd(*shape, scale=1.0):
    t = torch.randn(*shape, generator=g) * scale
    return t.to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.to(dev)


report = {"rounds": args.rounds, "window_ms": args.window_ms, "peak_tf": PEAK_TF, "device": torch.cuda.get_device_name(0)}

# ---- 128 -> 128, 5x5 / stride 2 on 8 x 128 x 128
N, C, H = 8, 128, 128
x, w, b = rnd(N, C, H, H), rnd(C, C, 5, 5, scale=0.02), rnd(C)
dy = rnd(N, C, H // 2, H // 2)
wmat = ops.patch_filter(w, 25 * C).contiguous()
flop = 2.0 * N * (H // 2) ** 2 * 25 * C * C


def direct():
    return ops.conv_raw(x, w, b, ks=5, stride=2, act=1)


def patch_route():
    return ops.conv_raw(ops.im2col_small(x, 5, 2, 25 * C), wmat, b, ks=1, act=1)


d = (direct() - patch_route()).abs().max().item() / direct().abs().max().item()
res = measure({"direct": direct, "patch_rows_1x1": patch_route}, flop)
show("fwd 128->128 5x5 s2 @8x128^2", flop, res)
ok = res["direct"]["us_median"] < res["patch_rows_1x1"]["us_median"] and res["direct"]["us_max"] < res["patch_rows_1x1"]["us_min"]
report["forward_128"] = {"gflop": flop / 1e9, **res, "max_diff_of_largest_output": d, "direct_wins_with_disjoint_ranges": ok}

wt = ops.filter_transpose(w, C, 25, C)
flop_t = 2.0 * N * (H // 2) ** 2 * 25 * C * C   # every (dy pixel, tap) pair lands inside the 2x map: the live taps are the same MACs
res = measure({"deconv": lambda: ops.conv_raw(dy, wt, b, ks=5, stride=2, pad=2, transposed=True, out_hw=(H, H), act=1)}, flop_t)
show("deconv 128->128 5x5 s2 64^2->128^2", flop_t, res)
report["deconv_128"] = {"gflop": flop_t / 1e9, **res}

res = measure({"wgrad": lambda: ops.wgrad_raw(x, dy, ks=5, stride=2, pad=2, Cout=C, Cin=C, want_bias=True)}, flop)
show("wgrad 128->128 5x5 s2 @8x128^2", flop, res)
report["wgrad_128"] = {"gflop": flop / 1e9, **res}

w3 = rnd(C, C, 3, 3, scale=0.03)
flop3 = 2.0 * N * (H // 2) ** 2 * 9 * C * C
res = measure({"conv3x3_s2": lambda: ops.conv_raw(x, w3, b, ks=3, stride=2, act=1)}, flop3)
show("context: fwd 128->128 3x3 s2 @8x128^2", flop3, res)
report["context_3x3_s2_128"] = {"gflop": flop3 / 1e9, **res}
del x, dy, wmat
torch.cuda.empty_cache()

# ---- the 192-channel hyper layer, 16x16 -> 8x8: a latency point
xh, wh, bh = rnd(N, 192, 16, 16), rnd(192, 192, 5, 5, scale=0.02), rnd(192)
floph = 2.0 * N * 64 * 25 * 192 * 192
res = measure({"direct": lambda: ops.conv_raw(xh, wh, bh, ks=5, stride=2, act=2)}, floph)
show("fwd 192->192 5x5 s2 @8x16^2", floph, res)
report["hyper_192"] = {"gflop": floph / 1e9, **res}

# ---- a full training step (plain autograd)
if not args.no_step:
    from clc_amd import models
    from clc_amd.recipe import synthetic_image
    from clc_amd.train import RateDistortionLoss

    img = synthetic_image(8, 256, 256, 100).to(dev)
    net = models.ScaleHyperprior(128, 192).to(dev).train()
    crit = RateDistortionLoss(0.0067)

    def step():
        net.zero_grad(set_to_none=True)
        crit(net(img), img)["loss"].backward()

    res = measure({"fwd_loss_bwd": step}, 0.0)
    show("ScaleHyperprior(128,192) step bs8", 0.0, res)
    report["train_step_scale_hyperprior_128_192_bs8_256"] = res
    if args.torch:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import hyperprior_ref
            from oracle.loss import RateDistortionLoss as ORD

            ref = hyperprior_ref.ScaleHyperprior(128, 192).to(dev).train()
            ref.load_state_dict(net.state_dict())
            oc = ORD(0.0067)

            def tstep():
                ref.zero_grad(set_to_none=True)
                oc(ref(img), img)["loss"].backward()

            res = measure({"fwd_loss_bwd": tstep}, 0.0)
            show("plain-torch restatement step", 0.0, res)
            report["train_step_plain_torch"] = res
        except Exception as e:   # the vendor convolution library may be missing or fail its kernel search
            report["train_step_plain_torch"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            print("plain-torch restatement did not run:", report["train_step_plain_torch"]["error"], flush=True)
    else:
        report["train_step_plain_torch"] = "not run (pass --torch)"

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("direct forward beats the patch-row route with disjoint ranges:", ok)
sys.exit(0 if ok else 1)
