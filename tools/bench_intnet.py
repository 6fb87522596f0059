"""Measurements for the integer hyper-synthesis net (csrc/int_conv.hip, clc_amd/intnet.py) -> profiles/intnet_bench.json.

One process, every leg warmed up, the two legs interleaved round by round, device time under events over `reps` calls per timing,
median [min .. max] over `rounds` timings.  NOTHING IS GATED: the numbers go into DESIGN 32.

  (a) TIME: IntegerHyperSynthesis.forward (the input quantiser and three clc_int_conv launches) against the float _hyper_synthesis of
      the same model, on the z_hat of 256x256 and 512x768 images at batch 1 and 8, for ScaleHyperprior(128, 192) and
      MeanScaleHyperprior(192, 320).
  (b) RATE: eval-forward bpp with exact=True against exact=False on seeded images, and the share of scale indexes that differ.  The
      weights are the rescaled recipe's, UNTRAINED, and the conversion is post-training without any fine-tuning: the column shows what
      the approximation costs on this net, not what a trained and calibrated model would pay.

Fails without a GPU; there is no fallback.
usage: python tools/bench_intnet.py [--rounds 15] [--reps 20] [--out profiles/intnet_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intnet_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_intnet.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import models
from clc_amd.recipe import apply_weight_recipe, synthetic_image


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.reps   # us per call


def stats(v):
    v = sorted(v)
    return {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1], "timings": len(v)}


def race(legs):
    for fn in legs.values():   # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    acc = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            acc[k].append(timed(fn))
    return {k: stats(v) for k, v in acc.items()}


def build(cls, N, M):
    m = cls(N, M, integer_hyper=True)
    apply_weight_recipe(m, 3)
    with torch.no_grad():   # as the tests: the bare recipe gives a flat latent and parameters near zero
        m.g_a[6].weight.mul_(20.0)
        m.h_s[4].weight.mul_(4.0)
        m.h_s[4].bias.add_(0.6)
    m = m.to(dev).eval()
    m.update(force=True)
    m.integerize(synthetic_image(2, 256, 256, 11, smooth=True).to(dev))
    return m


report = {"rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0), "time": [], "rate": [],
          "weights": "rescaled recipe weights, untrained; post-training conversion, calibrated on two seeded 256x256 images"}
for name, cls, N, M in (("bmshj2018-hyperprior", models.ScaleHyperprior, 128, 192), ("mbt2018-mean", models.MeanScaleHyperprior, 192, 320)):
    m = build(cls, N, M)
    shifts = torch.cat([getattr(m.h_s_int, f"shift{i}") for i in range(3)])
    print(f"{name} N={N} M={M}: spec_hash 0x{m.h_s_int.spec_hash():08x}, f0 = {int(m.h_s_int.fixed_point[0])}, shifts {int(shifts.min())} .. {int(shifts.max())}",
          flush=True)
    for (h, w) in ((256, 256), (512, 768)):
        for B in (1, 8):
            x = synthetic_image(B, h, w, 31 + B, smooth=True).to(dev)
            with torch.no_grad():
                y = m._analysis(m._prep(x))
                z_hat = m.entropy_bottleneck(m._hyper_analysis(y), training=False)[0]
                res = race({"integer": lambda: m.h_s_int(z_hat), "float": lambda: m._hyper_synthesis(z_hat)})
            res["integer_over_float"] = res["integer"]["median_us"] / res["float"]["median_us"]
            print(f"(a) {name} {B}x{h}x{w}: " + " | ".join(f"{k} {v['median_us']:.1f} [{v['min_us']:.1f} .. {v['max_us']:.1f}] us"
                                                          for k, v in res.items() if isinstance(v, dict)) + f" | ratio {res['integer_over_float']:.2f}", flush=True)
            report["time"].append({"model": name, "N": N, "M": M, "image": [B, h, w], "z": list(z_hat.shape), **res})
    # ---- (b)
    x = synthetic_image(4, 256, 256, 77, smooth=True).to(dev)
    with torch.no_grad():
        a, b = m(x, exact=True), m(x)
        y = m._analysis(m._prep(x))
        z_hat = m.entropy_bottleneck(m._hyper_analysis(y), training=False)[0]
        si, mi = m.h_s_int(z_hat)
        sf, mf = m._params(z_hat)
        gc = m.gaussian_conditional
        differ = float((gc.build_indexes(si) != gc.build_indexes(sf)).float().mean())
    px = x.shape[0] * x.shape[2] * x.shape[3]
    bpp = lambda o: float(sum(-torch.log2(v).sum() for v in o["likelihoods"].values())) / px
    row = {"model": name, "N": N, "M": M, "images": list(x.shape), "bpp_exact": bpp(a), "bpp_float": bpp(b), "scale_indexes_that_differ": differ,
           "mean_abs_scale_difference": float((si - sf).abs().mean()), "scale_range": [float(sf.min()), float(sf.max())],
           "mean_abs_mean_difference": None if mi is None else float((mi - mf).abs().mean()),
           "mean_range": None if mf is None else [float(mf.min()), float(mf.max())]}
    row["bpp_exact_over_float"] = row["bpp_exact"] / row["bpp_float"]
    print(f"(b) {name}: bpp exact {row['bpp_exact']:.4f} / float {row['bpp_float']:.4f} = {row['bpp_exact_over_float']:.4f}; "
          f"{100 * differ:.2f} % of the scale indexes differ; mean |d scale| {row['mean_abs_scale_difference']:.4f} (untrained weights)", flush=True)
    report["rate"].append(row)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("wrote", args.out)
