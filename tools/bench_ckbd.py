"""Micro-benchmark of the checkerboard context layer (csrc/ckbd_context.hip) -> profiles/ckbd_bench.json.

Shapes: the 192 -> 384 context layer of JointCheckerboardHierarchicalPriors(192, 192) at latent 16x16 x batch 8 (a 256x256 training
batch), latent 32x48 x batch 1 and x batch 8 (512x768).  Device time by events, every shape warmed up, at least `window-ms` of work per
timing, `rounds` timings per leg, the two legs of a shape alternating in one process; median and range (min .. max).
TF = algorithmic FLOP / time (12 taps at the non-anchor pixels), share of the 157.3 TF f32-MFMA peak.

  BAR      forward, data gradient and filter gradient of the layer on the new kernels against the only earlier route to the same
           result: the 5x5 kernels of csrc/conv5.hip on the mask-multiplied 25-tap filter plus the zeroing that route needs (the
           anchors of the output; the anchors of dy before either gradient; the masked taps of dw).  For EVERY leg the new kernel's
           median must be below the dense route's and the two ranges must not overlap, else exit status 1.  The multiplication
           count predicts about 25 * 2 / 12 = 4.2x; that is a prediction, not a gate.
  no bar   wall-clock compress / decompress of JointCheckerboardHierarchicalPriors(192, 192) beside mbt2018's
           (JointAutoregressiveHierarchicalPriors) at 256x256 and 512x768, batch 1 and 8.  For information only: the models and the
           streams differ.

Fails without a GPU; there is no fallback.
usage: python tools/bench_ckbd.py [--rounds 7] [--window-ms 100] [--out profiles/ckbd_bench.json] [--no-codec]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from clc_amd import ops

PEAK_TF = 157.3
CL = torch.channels_last
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ckbd_bench.json"))
ap.add_argument("--no-codec", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ckbd.py measures on the GPU: none found")
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
        out[k]["tflops"] = flop / out[k]["us_median"] / 1e6   # the algorithmic FLOPs of the layer, whatever the route multiplies
        out[k]["share_of_f32_mfma_peak"] = out[k]["tflops"] / PEAK_TF
    return out


def rnd(*shape, scale=1.0):
    t = torch.randn(*shape, generator=g) * scale
    return t.to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.to(dev)


Cin, Cout = 192, 384
w = rnd(Cout, Cin, 5, 5, scale=0.02)
bias = rnd(Cout)
mask = torch.zeros(5, 5)
for kh, kw in ops.CKBD_TAPS:
    mask[kh, kw] = 1
mask = mask.to(dev)
w25 = (w * mask).contiguous(memory_format=CL)              # the dense route's filter: 13 of 25 taps are zeros
w12 = ops.ckbd_filter(w)                                  # [Cout][12][Cin]
wt25 = ops.filter_transpose(w25, Cout, 25, Cin)
wt12 = ops.filter_transpose(w12, Cout, 12, Cin)
mask_w = mask.view(1, 1, 5, 5)

report = {"layer": f"{Cin} -> {Cout}", "rounds": args.rounds, "window_ms": args.window_ms, "peak_tf": PEAK_TF, "device": torch.cuda.get_device_name(0),
          "predicted_ratio_from_multiplications": 25 * 2 / 12, "shapes": []}
all_ok = True
for B, H, W in ((8, 16, 16), (1, 32, 48), (8, 32, 48)):
    x, dy = rnd(B, Cin, H, W), rnd(B, Cout, H, W)
    other = ops.ckbd_nonanchor_mask(H, W, dev)
    nonanchors = B * sum(1 for h in range(H) for ww in range(W) if not (h + ww) & 1)
    flop = 2.0 * nonanchors * 12 * Cin * Cout

    def fwd_new():
        return ops.ckbd_conv_raw(x, w12, bias, Cout)

    def fwd_dense():
        return ops.conv_raw(x, w25, bias, ks=5, stride=1).mul_(other)

    def dgrad_new():
        return ops.ckbd_conv_raw(dy, wt12, None, Cin, transposed=True)

    def dgrad_dense():
        return ops.conv_raw(dy * other, wt25, None, ks=5, stride=1, pad=2, transposed=True, out_hw=(H, W))

    def wgrad_new():
        return ops.ckbd_wgrad_raw(x, dy, Cout, Cin)

    def wgrad_dense():
        dw, _ = ops.wgrad_raw(x, dy * other, ks=5, stride=1, pad=2, Cout=Cout, Cin=Cin, want_bias=False)
        return dw.view(Cout, 5, 5, Cin).permute(0, 3, 1, 2).mul_(mask_w)

    # the two routes compute the same thing (also the first warm-up)
    diffs = {}
    for name, a, b in (("forward", fwd_new(), fwd_dense()), ("dgrad", dgrad_new(), dgrad_dense()),
                       ("wgrad", wgrad_new(), ops.ckbd_filter(wgrad_dense()))):
        diffs[name] = (a - b).abs().max().item() / b.abs().max().item()
    case = {"batch": B, "latent": [H, W], "gflop": flop / 1e9, "max_diff_of_largest_element": diffs, "legs": {}}
    for name, legs in (("forward", {"ckbd": fwd_new, "dense_conv5": fwd_dense}), ("dgrad", {"ckbd": dgrad_new, "dense_conv5": dgrad_dense}),
                       ("wgrad", {"ckbd": wgrad_new, "dense_conv5": wgrad_dense})):
        res = measure(legs, flop)
        ok = res["ckbd"]["us_median"] < res["dense_conv5"]["us_median"] and res["ckbd"]["us_max"] < res["dense_conv5"]["us_min"]
        all_ok &= ok
        res["ratio_dense_over_ckbd"] = res["dense_conv5"]["us_median"] / res["ckbd"]["us_median"]
        res["ckbd_wins_with_disjoint_ranges"] = ok
        case["legs"][name] = res
        print(f"{B}x{H}x{W} {name:8s} {flop / 1e9:6.2f} GF | " + " | ".join(
            f"{k} {res[k]['us_median']:8.1f} us [{res[k]['us_min']:.1f} .. {res[k]['us_max']:.1f}] {res[k]['tflops']:5.1f} TF {100 * res[k]['share_of_f32_mfma_peak']:4.1f}%"
            for k in legs) + f" | x{res['ratio_dense_over_ckbd']:.2f} | bar {ok}", flush=True)
    report["shapes"].append(case)
    del x, dy
report["ckbd_wins_everywhere"] = bool(all_ok)

# ---- for information: the coders' wall clock
if not args.no_codec:
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe, synthetic_image

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def stats(v):
        v = sorted(v)
        return {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "timings": len(v)}

    report["codec_wall_clock"] = []
    nets = {}
    for name, cls in (("mbt2018-checkerboard", models.JointCheckerboardHierarchicalPriors), ("mbt2018", models.JointAutoregressiveHierarchicalPriors)):
        net = cls(192, 192)
        apply_weight_recipe(net, 0)
        net = net.to(dev).eval()
        net.update(force=True)
        nets[name] = net
    for h, ww in ((256, 256), (512, 768)):
        for B in (1, 8):
            img = synthetic_image(B, h, ww, 100, smooth=True).to(dev)
            case = {"image": [h, ww], "batch": B}
            for name, net in nets.items():
                item = net.compress(img)   # warm-up
                net.decompress(item["strings"], item["shape"])
                tc, td = [], []
                for _ in range(3):
                    ms, item = wall_ms(lambda: net.compress(img))
                    tc.append(ms)
                    ms, _ = wall_ms(lambda: net.decompress(item["strings"], item["shape"]))
                    td.append(ms)
                case[name] = {"compress_wall": stats(tc), "decompress_wall": stats(td), "y_bytes_per_image": [len(s) for s in item["strings"][0]]}
            report["codec_wall_clock"].append(case)
            print(f"{h}x{ww} batch {B}: " + " | ".join(
                f"{name} compress {case[name]['compress_wall']['ms_median']:.1f} ms, decompress {case[name]['decompress_wall']['ms_median']:.1f} ms" for name in nets), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("the checkerboard kernels beat the dense route with disjoint ranges on every leg:", all_ok)
sys.exit(0 if all_ok else 1)
