"""Micro-benchmark of the batch-invariant row GEMM (csrc/row_gemm.hip) and of the space-channel context coder -> profiles/scctx_bench.json.

Device time by events, every shape warmed up, at least `window-ms` of work per timing, `rounds` timings per leg, the two legs of a
shape alternating in one process; median and range (min .. max).  TF = 2 rows K N / time, share of the 157.3 TF f32-MFMA peak.

  BAR      clc_row_gemm against clc_ar_linear, the only earlier route to the same product, on the aggregation layers of the default
           Elic2022: 672 -> 640 (group 0), 704 -> 640 (group 1), 1 408 -> 640 (the last group), 640 -> 512, 512 -> 32 and 512 -> 384, at
           128, 768 and 6 144 rows (the anchors of a 16x16 latent, of the 32x48 latent of one 512x768 image, and of a batch of 8).  The
           first layers read their K ranges from pixel-major maps as the coder does (clc_ar_linear takes two ranges, so its context
           maps are concatenated beforehand; the product is the same), the others from a dense buffer.  On the two wide layers of each
           chain (... -> 640 and 640 -> 512) at 768 and 6 144 rows the new kernel's median must be below clc_ar_linear's and the two
           ranges must not overlap, else exit status 1.  128 rows and the narrow last layers are reported, not gated.
  no bar   wall-clock compress / decompress of Elic2022() beside JointCheckerboardHierarchicalPriors(192, 192) at 256x256 and
           512x768, batch 1 and 8.  For information only: the models and the streams differ.

Fails without a GPU; there is no fallback.
usage: python tools/bench_scctx.py [--rounds 7] [--window-ms 100] [--out profiles/scctx_bench.json] [--no-codec]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from clc_amd import ops
from clc_amd.models import ckbd_pixels

PEAK_TF = 157.3
CL = torch.channels_last
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scctx_bench.json"))
ap.add_argument("--no-codec", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_scctx.py measures on the GPU: none found")
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
        out[k]["tflops"] = flop / out[k]["us_median"] / 1e6
        out[k]["share_of_f32_mfma_peak"] = out[k]["tflops"] / PEAK_TF
    return out


def rnd(*shape, scale=1.0):
    t = torch.randn(*shape, generator=g) * scale
    return t.to(dev).contiguous(memory_format=CL) if t.dim() == 4 else t.to(dev)


# (K ranges of the layer: None = one dense range of K channels, N, gated)
LAYERS = [((640, 32), 640, True), ((640, 32, 32), 640, True), ((640, 384, 384), 640, True), ((640,), 512, True), ((512,), 32, False),
          ((512,), 384, False)]
ROWS = [(128, 1, 16, 16), (768, 1, 32, 48), (6144, 8, 32, 48)]   # (rows, B, latent H, W): the anchors of every image
report = {"rounds": args.rounds, "window_ms": args.window_ms, "peak_tf": PEAK_TF, "device": torch.cuda.get_device_name(0), "cases": []}
all_ok = True
for rows, B, H, W in ROWS:
    anchors, _ = ckbd_pixels(H, W)
    pix = torch.tensor(anchors, dtype=torch.int32).reshape(-1, 2).to(dev)
    assert B * len(anchors) == rows
    for ranges, N, gated in LAYERS:
        K = sum(ranges)
        w, bias = rnd(N, K, scale=K ** -0.5), rnd(N)
        out_new, out_old = torch.empty((rows, N), device=dev), torch.empty((rows, N), device=dev)
        if len(ranges) == 1:
            x = rnd(rows, K)
            new_srcs = old_srcs = [("dense", x)]
        else:
            maps = [rnd(B, c, H, W) for c in ranges]
            new_srcs = [("pixel", m) for m in maps]
            old_srcs = [("pixel", maps[0]), ("pixel", torch.cat(maps[1:], 1).contiguous(memory_format=CL))]

        def new():
            return ops.row_gemm(new_srcs, pix, B, H, W, w, bias, out_new, act=ops.ACT_LRELU)

        def old():
            return ops.ar_linear(old_srcs, pix, B, H, W, w, bias, out_old, act=ops.ACT_LRELU)

        diff = (new() - old()).abs().max().item() / out_old.abs().max().item()   # the two routes compute the same thing (also a warm-up)
        flop = 2.0 * rows * K * N
        res = measure({"row_gemm": new, "ar_linear": old}, flop)
        ok = res["row_gemm"]["us_median"] < res["ar_linear"]["us_median"] and res["row_gemm"]["us_max"] < res["ar_linear"]["us_min"]
        is_gated = gated and rows >= 768
        if is_gated:
            all_ok &= ok
        res.update({"rows": rows, "batch": B, "latent": [H, W], "K_ranges": list(ranges), "N": N, "gflop": flop / 1e9, "gated": is_gated,
                    "row_gemm_wins_with_disjoint_ranges": ok, "ratio_ar_linear_over_row_gemm": res["ar_linear"]["us_median"] / res["row_gemm"]["us_median"],
                    "max_diff_of_largest_element": diff})
        report["cases"].append(res)
        print(f"{rows:5d} rows {K:5d} -> {N:3d} {flop / 1e9:6.2f} GF | " + " | ".join(
            f"{k} {res[k]['us_median']:9.1f} us [{res[k]['us_min']:.1f} .. {res[k]['us_max']:.1f}] {res[k]['tflops']:6.2f} TF {100 * res[k]['share_of_f32_mfma_peak']:5.2f}%"
            for k in ("row_gemm", "ar_linear")) + f" | x{res['ratio_ar_linear_over_row_gemm']:.1f} | {'BAR' if is_gated else 'info'} {ok} | diff {diff:.1e}", flush=True)
report["row_gemm_wins_every_gated_case"] = bool(all_ok)

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
    for name, make in (("elic2022", lambda: models.Elic2022()), ("mbt2018-checkerboard", lambda: models.JointCheckerboardHierarchicalPriors(192, 192))):
        net = make()
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
print("clc_row_gemm beats clc_ar_linear with disjoint ranges on every gated case:", all_ok)
sys.exit(0 if all_ok else 1)
