"""Measurements for variable-rate coding (the quantisation-step kernels of csrc/qstep.hip) -> profiles/vbr_bench.json.

One process, every leg warmed up, the legs of a comparison interleaved round by round, device time under events over `reps` calls per
timing, median [min .. max] over `rounds` timings.  NOTHING IS GATED: the numbers go into DESIGN 31.

  (a) clc_gauss_rate_sweep at K = 16 against 16 launches of clc_gauss_lik_fwd (eval mode: the launches a caller without the sweep
      would make; the per-image reductions it would still need are not even counted) and against the torch-op composition, on
      latents 8x16x16x192 and 1x32x48x192.
  (b) clc_gauss_lik_step_fwd / _bwd and clc_quantize_build_indexes_step against their unit-step siblings on the same tensors.
  (c) ScaleSpaceFlow(mid_planes=128, planes=192, rate_levels=5) with the rescaled recipe weights on an 8-frame 256x256 sequence: bpp
      and PSNR-YUV at each integer q.  The weights are untrained: the rate column shows that the knob moves the rate, the distortion
      column means nothing.

Fails without a GPU; there is no fallback.
usage: python tools/bench_vbr.py [--rounds 15] [--reps 20] [--out profiles/vbr_bench.json]"""
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
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbr_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_vbr.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import frames as fr
from clc_amd import lib, models, ops
from clc_amd.models.clc import get_scale_table
from clc_amd.recipe import apply_weight_recipe, synthetic_image

L = lib.load()
st = ops._stream


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


def show(what, res):
    print(what + ": " + " | ".join(f"{k} {v['median_us']:.1f} [{v['min_us']:.1f} .. {v['max_us']:.1f}] us" for k, v in res.items()), flush=True)


report = {"rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sweep": [], "siblings": []}
table = torch.tensor([float(s) for s in get_scale_table()], dtype=torch.float32, device=dev)

for B, H, W, C in ((8, 16, 16, 192), (1, 32, 48, 192)):
    g = torch.Generator().manual_seed(B)
    rows, n = B * H * W, H * W
    mu = torch.randn((rows, C), generator=g).to(dev)
    scale = (torch.rand((rows, C), generator=g) * 3 + 0.05).to(dev)
    y = (mu.cpu() + torch.randn((rows, C), generator=g) * 2).to(dev)
    noise = (torch.rand((rows, C), generator=g) - 0.5).to(dev)
    dlik = (torch.rand((rows, C), generator=g) - 0.7).to(dev)
    K = 16
    steps = torch.exp(torch.linspace(0.6931, -0.6931, K)).reshape(K, 1).repeat(1, C).contiguous().to(dev)
    one = torch.ones(C, device=dev)
    lik, yh, dy, dmu, dsc = (torch.empty((rows, C), device=dev) for _ in range(5))
    dstep = torch.empty(C, device=dev)
    sym, idx = (torch.empty((rows, C), device=dev, dtype=torch.int32) for _ in range(2))
    p = lambda t: t.data_ptr()

    # ---- (a)
    bits = torch.empty((B, K), device=dev)
    nbytes = L.clc_gauss_rate_sweep_workspace_bytes(B, n, C, K)
    ws = torch.empty(nbytes // 4, device=dev)
    nb = L.clc_gauss_lik_partials(n, C)
    part = torch.empty((B, K, nb), device=dev)

    def sweep():
        lib.check(L.clc_gauss_rate_sweep(p(y), C, p(mu), C, p(scale), C, p(steps), K, B, n, C, p(bits), p(ws), nbytes, st()), "clc_gauss_rate_sweep")

    def sixteen():   # per candidate one launch over the whole batch (its per-image sums would need B launches or a reshaped reduction)
        for k in range(K):
            lib.check(L.clc_gauss_lik_fwd(p(y), C, p(mu), C, p(scale), C, None, 0, p(lik), C, None, 0, rows, C, 1, None, 0, st()), "clc_gauss_lik_fwd")

    y3, mu3 = y.reshape(B, n, C), mu.reshape(B, n, C)
    sg3 = scale.reshape(B, n, C).clamp(min=0.11)

    def torch_ops():
        out = []
        for k in range(K):
            s = steps[k]
            v = (torch.round((y3 - mu3) / s) * s).abs()
            up = 0.5 * torch.erfc(-(2 ** -0.5) * ((0.5 * s - v) / sg3))
            lo = 0.5 * torch.erfc(-(2 ** -0.5) * ((-0.5 * s - v) / sg3))
            out.append(-torch.log2((up - lo).clamp(min=1e-9)).sum((1, 2)))
        return torch.stack(out, 1)

    sweep()
    want = torch_ops()
    assert float((bits - want).abs().max()) <= n * C * 2e-3
    res = race({"rate_sweep_K16": sweep, "16_x_gauss_lik_fwd": sixteen, "torch_ops": torch_ops})
    elems = rows * C
    med = res["rate_sweep_K16"]["median_us"] * 1e-6
    res["derived"] = {"elements": elems, "read_bytes": 12 * elems, "achieved_GBps_of_the_12_B_bound": 12 * elems / med / 1e9,
                      "erfc_per_second": 2 * K * elems / med, "candidate_elements_per_second": K * elems / med,
                      "sixteen_launches_over_sweep": res["16_x_gauss_lik_fwd"]["median_us"] / res["rate_sweep_K16"]["median_us"],
                      "torch_over_sweep": res["torch_ops"]["median_us"] / res["rate_sweep_K16"]["median_us"]}
    show(f"(a) {B}x{H}x{W}x{C}", {k: v for k, v in res.items() if k != "derived"})
    print("    ", res["derived"], flush=True)
    report["sweep"].append({"latent": [B, H, W, C], **res})

    # ---- (b)
    wsb = L.clc_gauss_lik_step_bwd_workspace_bytes(rows, C)
    wsg = torch.empty(wsb // 4, device=dev)
    legs = {}
    for mode, tag in ((1, "eval"), (0, "train")):
        npn, ldn = (p(noise), C) if mode == 0 else (None, 0)
        legs[f"fwd_{tag}_unit"] = (lambda mode, npn, ldn: lambda: L.clc_gauss_lik_fwd(p(y), C, p(mu), C, p(scale), C, npn, ldn, p(lik), C, p(yh), C, rows, C, mode,
                                                                                       None, 0, st()))(mode, npn, ldn)
        legs[f"fwd_{tag}_step"] = (lambda mode, npn, ldn: lambda: L.clc_gauss_lik_step_fwd(p(y), C, p(mu), C, p(scale), C, npn, ldn, p(one), p(lik), C, p(yh), C,
                                                                                            rows, C, mode, None, 0, st()))(mode, npn, ldn)
    npn, ldn = p(noise), C
    legs["bwd_train_unit"] = lambda: L.clc_gauss_lik_bwd(p(dlik), C, p(y), C, p(mu), C, p(scale), C, npn, ldn, p(dy), C, p(dmu), C, p(dsc), C, rows, C, 0,
                                                          None, 0, st())
    legs["bwd_train_step"] = lambda: L.clc_gauss_lik_step_bwd(p(dlik), C, p(y), C, p(mu), C, p(scale), C, npn, ldn, p(one), p(dy), C, p(dmu), C, p(dsc), C,
                                                               p(dstep), rows, C, 0, None, 0, p(wsg), wsb, st())
    legs["quantize_unit"] = lambda: L.clc_quantize_build_indexes(p(y), C, p(mu), C, p(scale), C, p(table), table.numel(), p(sym), p(idx), p(yh), C, rows, C, st())
    legs["quantize_step"] = lambda: L.clc_quantize_build_indexes_step(p(y), C, p(mu), C, p(scale), C, p(one), p(table), table.numel(), p(sym), p(idx), p(yh), C,
                                                                      rows, C, st())
    for k, fn in legs.items():
        assert fn() == 0, k
    res = race(legs)
    res["step_over_unit"] = {k[:-5]: res[k]["median_us"] / res[k[:-5] + "_unit"]["median_us"] for k in legs if k.endswith("_step")}
    show(f"(b) {B}x{H}x{W}x{C}", {k: v for k, v in res.items() if k != "step_over_unit"})
    print("    step / unit medians:", {k: round(v, 3) for k, v in res["step_over_unit"].items()}, flush=True)
    report["siblings"].append({"latent": [B, H, W, C], **res})

# ---- (c)
fixed = models.ScaleSpaceFlow(mid_planes=128, planes=192)   # (the weight recipe knows the fixed-rate model's parameters)
apply_weight_recipe(fixed, 0)
with torch.no_grad():   # as tools/bench_ssf_codec.py: the bare recipe gives all-zero latents
    for enc_net in (fixed.img_encoder, fixed.res_encoder, fixed.motion_encoder):
        enc_net[6].weight.mul_(20.0)
    for hp in (fixed.img_hyperprior, fixed.res_hyperprior, fixed.motion_hyperprior):
        hp.hyper_decoder_scale.deconv3.weight.mul_(4.0)
        hp.hyper_decoder_scale.deconv3.bias.add_(0.6)
    fixed.motion_decoder[6].weight.mul_(0.3)
net = models.ScaleSpaceFlow(mid_planes=128, planes=192, rate_levels=5)
net.load_state_dict(fixed.state_dict(), strict=False)   # the three step tables keep their default ladder
net = net.to(dev).eval()
net.update(force=True)
h = w = 256
base = synthetic_image(1, h + 32, w + 32, 77, smooth=True)
seq = [(base[:, :, 16 + 2 * t:16 + 2 * t + h, 16 - t:16 - t + w] * (1.0 - 0.01 * t)).contiguous().to(dev) for t in range(args.frames)]
planes = [fr.rgb_to_yuv420(x, (h, w), bit_depth=8) for x in seq]
rows_c = []
for q in (None, 0.0, 1.0, 2.0, 3.0, 4.0):
    blob = fr.encode_yuv420(net, planes, bit_depth=8, lanes=4, q=q)
    dec = fr.decode_yuv420(net, blob)
    m = fr.sequence_metrics(planes, dec, 8, blob=blob)
    rows_c.append({"q": q, "step": None if q is None else float(net.img_hyperprior.y_step(q).detach()[0]), "bytes": len(blob), "bpp": m["bpp"],
                   "psnr_yuv": m["mean"]["psnr_yuv"]})
    print(f"(c) q = {q}: {len(blob)} bytes, {m['bpp']:.4f} bpp, PSNR-YUV {m['mean']['psnr_yuv']:.2f} dB (untrained weights)", flush=True)
bpps = [r["bpp"] for r in rows_c[1:]]
report["rate_knob"] = {"model": "ScaleSpaceFlow(mid_planes=128, planes=192, rate_levels=5), rescaled recipe weights (untrained)", "frames": args.frames,
                       "image": [h, w], "lanes": 4, "rows": rows_c, "bpp_rises_with_q": all(a < b for a, b in zip(bpps, bpps[1:]))}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("wrote", args.out)
