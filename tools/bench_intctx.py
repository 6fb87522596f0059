"""Measurements for the integer context model of mbt2018-checkerboard (csrc/int_rows.hip, clc_amd/intnet.py)
-> profiles/intctx_bench.json.

One process, every leg warmed up, the legs interleaved round by round, device time under events over `reps` calls per timing, median
[min .. max] over `rounds` timings.  NOTHING IS GATED: the numbers go into DESIGN 33.  N = 192, M = 192.

  (a) TIME PER PASS: the integer chain (the y_hat quantiser and ctx_int.chain: 3 launches for the anchors, 1 + 4 for the non-anchors)
      against the float chain (_ckbd_chain, plus context_prediction for the non-anchors), per pass kind.
  (b) TIME PER CALL: compress / decompress with exact=True against the default, on the one-stream format and at lanes=4 (device events
      around whole calls: they include the host coder and the host hops of the one-stream format).
  (c) RATE: eval-forward bpp with exact=True against the float eval forward on four seeded 256x256 images, the share of scale indexes
      that differ between the two coders' (scales | means) rows and the mean |d scale|.  The weights are the rescaled recipe's,
      UNTRAINED, and the conversion is post-training with two calibration images and no fine-tuning: the column shows what the
      approximation costs on this net, not what a trained and calibrated model would pay.

Fails without a GPU; there is no fallback.
usage: python tools/bench_intctx.py [--rounds 9] [--reps 10] [--call-reps 2] [--out profiles/intctx_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--call-reps", type=int, default=2)
ap.add_argument("--call-rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intctx_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_intctx.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import intnet, models
from clc_amd.recipe import apply_weight_recipe, synthetic_image

N, M = 192, 192
SHAPES = ((1, 256, 256), (8, 256, 256), (1, 512, 768), (8, 512, 768))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us per call


def stats(v):
    v = sorted(v)
    return {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1], "timings": len(v)}


def race(legs, rounds, reps):
    for fn in legs.values():   # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    acc = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            acc[k].append(timed(fn, reps))
    return {k: stats(v) for k, v in acc.items()}


def show(tag, res):
    print(tag + ": " + " | ".join(f"{k} {v['median_us']:.1f} [{v['min_us']:.1f} .. {v['max_us']:.1f}] us" for k, v in res.items() if isinstance(v, dict)),
          flush=True)


base = models.JointCheckerboardHierarchicalPriors(N, M)
apply_weight_recipe(base, 3)
with torch.no_grad():   # as the tests: the bare recipe gives a flat latent and parameters near zero
    base.g_a[6].weight.mul_(20.0)
    base.h_s[4].weight.mul_(4.0)
    base.h_s[4].bias.add_(0.6)
    base.entropy_parameters[4].weight.mul_(8.0)
    base.entropy_parameters[4].bias[:M].add_(0.6)
m = models.JointCheckerboardHierarchicalPriors(N, M, integer_context=True)
m.load_state_dict(base.state_dict(), strict=False)
m = m.to(dev).eval()
m.update(force=True)
h = m.integerize(synthetic_image(2, 256, 256, 11, smooth=True).to(dev))
print(f"mbt2018-checkerboard N={N} M={M}: hash 0x{h:08x}, f0 = {int(m.h_s_int.fixed_point[0])}, (f_y, f_out) = {m.ctx_int.fixed_point.tolist()}", flush=True)

report = {"rounds": args.rounds, "reps": args.reps, "call_rounds": args.call_rounds, "call_reps": args.call_reps, "device": torch.cuda.get_device_name(0),
          "N": N, "M": M, "hash": h, "pass": [], "call": [], "rate": [],
          "weights": "rescaled recipe weights, untrained; post-training conversion, calibrated on two seeded 256x256 images, no fine-tuning"}

for B, hh, ww in SHAPES:
    x = synthetic_image(B, hh, ww, 31 + B, smooth=True).to(dev)
    with torch.no_grad():
        # ---- (a) per pass
        y, params, _, _ = m._code_inputs(x)
        _, psi, _, _ = m._exact_inputs(x)
        params = params.contiguous(memory_format=torch.channels_last)
        _, _, y_hat = m._ckbd_encode(y, params)
        _, _, H, W = y.shape
        fs, es = m._pass_schedule(B, H, W, dev), m._pass_schedule(B, H, W, dev, exact=True)
        na = len(fs.steps[0])
        pa, pn = fs.pix[:na], fs.pix[na:]
        filt, psi_n, net = m._ckbd_filters(), psi.permute(0, 2, 3, 1), m.ctx_int
        res = race({"anchor_integer": lambda: net.chain(pa, B, H, W, psi_n, None, es.ws),
                    "anchor_float": lambda: m._ckbd_chain(pa, B, H, W, params, fs.ctx0, fs.ws, filt),
                    "non_anchor_integer": lambda: net.chain(pn, B, H, W, psi_n, intnet.int_quantize(y_hat, net.f_y), es.ws),
                    "non_anchor_float": lambda: m._ckbd_chain(pn, B, H, W, params, m.context_prediction(y_hat), fs.ws, filt)}, args.rounds, args.reps)
        res["anchor_integer_over_float"] = res["anchor_integer"]["median_us"] / res["anchor_float"]["median_us"]
        res["non_anchor_integer_over_float"] = res["non_anchor_integer"]["median_us"] / res["non_anchor_float"]["median_us"]
        show(f"(a) {B}x{hh}x{ww} (rows per pass {B * na})", res)
        report["pass"].append({"image": [B, hh, ww], "latent": [H, W], "rows_per_pass": B * na, **res})
        # ---- (b) per call
        for lanes in (None, 4):
            kw = {} if lanes is None else {"lanes": lanes}
            ie, ifl = m.compress(x, exact=True, **kw), m.compress(x, **kw)
            res = race({"compress_exact": lambda: m.compress(x, exact=True, **kw), "compress_float": lambda: m.compress(x, **kw),
                        "decompress_exact": lambda: m.decompress(ie["strings"], ie["shape"], exact=ie["exact"], **kw),
                        "decompress_float": lambda: m.decompress(ifl["strings"], ifl["shape"], **kw)}, args.call_rounds, args.call_reps)
            res["compress_exact_over_float"] = res["compress_exact"]["median_us"] / res["compress_float"]["median_us"]
            res["decompress_exact_over_float"] = res["decompress_exact"]["median_us"] / res["decompress_float"]["median_us"]
            show(f"(b) {B}x{hh}x{ww} lanes={lanes}", res)
            report["call"].append({"image": [B, hh, ww], "lanes": lanes, "y_bytes_exact": sum(len(s) for s in ie["strings"][0]),
                                   "y_bytes_float": sum(len(s) for s in ifl["strings"][0]), **res})

# ---- (c)
x = synthetic_image(4, 256, 256, 77, smooth=True).to(dev)
with torch.no_grad():
    a, b = m(x, exact=True), m(x)
    rows = {}
    for name, inputs in (("exact", m._exact_inputs), ("float", m._code_inputs)):
        y, p, _, _ = inputs(x)
        B, _, H, W = y.shape
        gp_map = torch.empty((B, H, W, 2 * M), device=dev)

        def passes(params, y_hat):
            for cnt, px, gp in m._ckbd_passes(params, y_hat):
                gp_map[:, px[:, 0].long(), px[:, 1].long()] = gp[:B * cnt].view(B, cnt, 2 * M)
                yield cnt, px, gp

        _, idx, _ = m._encode_passes("bench", y, p, passes)
        rows[name] = (gp_map, idx)
px = x.shape[0] * x.shape[2] * x.shape[3]
bpp = lambda o: float(sum(-torch.log2(v).sum() for v in o["likelihoods"].values())) / px
se, sf = rows["exact"][0][..., :M], rows["float"][0][..., :M]
row = {"images": list(x.shape), "bpp_exact": bpp(a), "bpp_float_eval_forward": bpp(b),
       "scale_indexes_that_differ": float((rows["exact"][1] != rows["float"][1]).float().mean()),
       "mean_abs_scale_difference": float((se - sf).abs().mean()), "scale_range": [float(sf.min()), float(sf.max())],
       "mean_abs_mean_difference": float((rows["exact"][0][..., M:] - rows["float"][0][..., M:]).abs().mean())}
row["bpp_exact_over_float"] = row["bpp_exact"] / row["bpp_float_eval_forward"]
print(f"(c) bpp exact {row['bpp_exact']:.4f} / float eval forward {row['bpp_float_eval_forward']:.4f} = {row['bpp_exact_over_float']:.4f}; "
      f"{100 * row['scale_indexes_that_differ']:.2f} % of the scale indexes differ; mean |d scale| {row['mean_abs_scale_difference']:.4f} "
      "(untrained weights)", flush=True)
report["rate"].append(row)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("wrote", args.out)
