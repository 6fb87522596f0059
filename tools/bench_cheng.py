"""Measurements for cheng2020 (csrc/gmm.hip, clc_amd/models/cheng.py) -> profiles/cheng_bench.json.

  BAR      the mixture likelihood at [8, 192, 32, 48], K = 3 (a 512x768 batch of 8), training mode: forward, and forward + backward, of
           ops.gmm_likelihood_packed against the same likelihood composed from torch ops on the GPU (softmax, erfc, the two LowerBounds
           with their gradient rule through autograd) — the only earlier route to it.  Device time by events, every leg warmed up, at
           least `window-ms` of work per timing, `rounds` alternating timings per leg in one process; median [min .. max], the bytes
           the kernels must move from the shapes, and the share of the 6.3 TB/s achievable HBM rate.  The new kernel's median must be
           below the composition's and the two ranges must not overlap, else exit status 1.
  no bar   Cheng2020Attention(192) at 256x256 and 512x768, batch 1 and 8, K = 3 and K = 1: wall-clock compress / decompress (median of
           3 around a device synchronise), the share of escaped symbols, and the coded bits of y against -sum log2(likelihood) of the
           eval forward.  For information only: the streams differ.  This shows what the half-width R of the per-symbol rows costs.

Fails without a GPU; there is no fallback.
usage: python tools/bench_cheng.py [--rounds 7] [--window-ms 100] [--out profiles/cheng_bench.json] [--no-codec]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from clc_amd import layers, ops

HBM_TBS = 6.3
CL = torch.channels_last
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cheng_bench.json"))
ap.add_argument("--no-codec", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_cheng.py measures on the GPU: none found")
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
        out[k] = {"us_median": v[len(v) // 2], "us_min": v[0], "us_max": v[-1], "calls_per_timing": reps[k]}
        out[k]["tb_per_s_of_the_kernel_bytes"] = nbytes / out[k]["us_median"] / 1e6
        out[k]["share_of_achievable_hbm"] = out[k]["tb_per_s_of_the_kernel_bytes"] / HBM_TBS
    return out


B, C, H, W, K = 8, 192, 32, 48, 3
y = (torch.randn(B, C, H, W, generator=g) * 3.0).to(dev).contiguous(memory_format=CL).requires_grad_()
gp = torch.cat((torch.randn(B, K * C, H, W, generator=g) + 0.5, torch.randn(B, K * C, H, W, generator=g) * 2.0,
                torch.randn(B, K * C, H, W, generator=g) * 1.5), 1).to(dev).contiguous(memory_format=CL).requires_grad_()
noise = (torch.rand(B, C, H, W, generator=g) - 0.5).to(dev).contiguous(memory_format=CL)
up = (torch.rand(B, C, H, W, generator=g) - 0.7).to(dev).contiguous(memory_format=CL)
lb_scale, lb_lik = layers.LowerBound(0.11).to(dev), layers.LowerBound(1e-9).to(dev)


def phi(x):
    return 0.5 * torch.erfc(-(2 ** -0.5) * x)


def lik_torch():
    sc, mu, wt = (t.reshape(B, K, C, H, W) for t in gp.chunk(3, 1))
    sc = lb_scale(sc)
    d = torch.abs((y + noise).unsqueeze(1) - mu)
    return lb_lik((torch.softmax(wt, 1) * (phi((0.5 - d) / sc) - phi((-0.5 - d) / sc))).sum(1))


def lik_hip():
    return ops.gmm_likelihood_packed(y, gp, noise, True, K)


def both(fn):
    def run():
        y.grad = gp.grad = None
        fn().backward(up)
    return run


with torch.no_grad():
    a, b = lik_hip(), lik_torch()
both(lik_hip)()
ga, gy = gp.grad.clone(), y.grad.clone()
both(lik_torch)()
elems = B * C * H * W
report = {"shape": [B, C, H, W], "K": K, "rounds": args.rounds, "window_ms": args.window_ms, "achievable_hbm_tb_per_s": HBM_TBS,
          "device": torch.cuda.get_device_name(0),
          "max_diff_of_largest_element": {"likelihood": ((a - b).abs().max() / b.abs().max()).item(),
                                          "d_params": ((ga - gp.grad).abs().max() / gp.grad.abs().max()).item(),
                                          "d_y": ((gy - y.grad).abs().max() / y.grad.abs().max()).item()}, "legs": {}}
nb_f = 4.0 * elems * (2 + 3 * K + 1)                # read y, noise, 3 K parameters; write the likelihood
nb_b = 4.0 * elems * (3 + 3 * K + 1 + 3 * K)        # read dlik, y, noise, 3 K parameters; write dy and 3 K gradients
all_ok = True
with torch.no_grad():
    fwd = measure({"gmm_hip": lik_hip, "torch_ops": lik_torch}, nb_f)
for name, res, nb in (("forward", fwd, nb_f), ("forward_backward", measure({"gmm_hip": both(lik_hip), "torch_ops": both(lik_torch)}, nb_f + nb_b), nb_f + nb_b)):
    ok = res["gmm_hip"]["us_median"] < res["torch_ops"]["us_median"] and res["gmm_hip"]["us_max"] < res["torch_ops"]["us_min"]
    all_ok &= ok
    res["kernel_mbytes"] = nb / 1e6
    res["ratio_torch_over_hip"] = res["torch_ops"]["us_median"] / res["gmm_hip"]["us_median"]
    res["hip_wins_with_disjoint_ranges"] = ok
    report["legs"][name] = res
    print(f"{name:17s} {nb / 1e6:7.1f} MB | " + " | ".join(
        f"{k} {res[k]['us_median']:8.1f} us [{res[k]['us_min']:.1f} .. {res[k]['us_max']:.1f}] {100 * res[k]['share_of_achievable_hbm']:5.1f} % of {HBM_TBS} TB/s"
        for k in ("gmm_hip", "torch_ops")) + f" | x{res['ratio_torch_over_hip']:.2f} | bar {ok}", flush=True)
report["hip_wins_everywhere"] = bool(all_ok)
del y, gp, noise, up, a, b, ga, gy

# ---- for information: the coders
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

    report["codec"] = []
    nets = {}
    for Kc in (3, 1):
        net = models.Cheng2020Attention(192, Kc)
        apply_weight_recipe(net, 0)
        with torch.no_grad():   # the scalings of the tests: latents of a few bins, scales off the 0.11 bound
            net.g_a[7].weight.mul_(20.0)
            net.h_s[8].weight.mul_(4.0)
            net.h_s[8].bias.add_(0.6)
            net.entropy_parameters[4].weight.mul_(8.0)
            net.entropy_parameters[4].bias[:Kc * 192].add_(0.6)
        net = net.to(dev).eval()
        net.update(force=True)
        nets[Kc] = net
    for h, ww in ((256, 256), (512, 768)):
        for Bc in (1, 8):
            img = synthetic_image(Bc, h, ww, 100, smooth=True).to(dev)
            case = {"image": [h, ww], "batch": Bc}
            for Kc, net in nets.items():
                item = net.compress(img)   # warm-up
                net.decompress(item["strings"], item["shape"])
                tc, td = [], []
                for _ in range(3):
                    ms, item = wall_ms(lambda: net.compress(img))
                    tc.append(ms)
                    ms, _ = wall_ms(lambda: net.decompress(item["strings"], item["shape"]))
                    td.append(ms)
                with torch.no_grad():
                    ideal = -torch.log2(net(img)["likelihoods"]["y"]).sum().item()
                    yy, pp, _, _ = net._code_inputs(img)
                    if Kc > 1:
                        esc = (net._gmm_encode(yy, pp)[0][..., 2] >= 0).float().mean().item()
                    else:
                        sym, idx, _ = net._ar_encode(yy, pp)
                        _, ln, off = net.gaussian_conditional.host_tables()
                        v = sym.cpu().numpy() - off[idx.cpu().numpy()]
                        esc = float(((v < 0) | (v >= ln[idx.cpu().numpy()] - 2)).mean())
                coded = 8.0 * sum(len(s) for s in item["strings"][0])
                Hl, Wl = h // 16, ww // 16
                case[f"K={Kc}"] = {"compress_wall": stats(tc), "decompress_wall": stats(td), "escaped_share": esc, "coded_bits_y": coded,
                                   "ideal_bits_y": ideal, "coded_over_ideal": coded / ideal,
                                   "decoder_host_hops": (Wl + 3 * (Hl - 1) if Kc > 1 else Hl * Wl) + 1}
            report["codec"].append(case)
            print(f"{h}x{ww} batch {Bc}: " + " | ".join(
                f"K={Kc} compress {c['compress_wall']['ms_median']:.1f} ms, decompress {c['decompress_wall']['ms_median']:.1f} ms, escaped "
                f"{100 * c['escaped_share']:.3f} %, coded/ideal {c['coded_over_ideal']:.4f}" for Kc, c in ((k, case[f'K={k}']) for k in nets)), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("the mixture kernels beat the torch composition with disjoint ranges on every leg:", all_ok)
sys.exit(0 if all_ok else 1)
