"""Measurements for the lanes stream of mbt2018 and mbt2018-checkerboard and its fused step kernel (clc_ar_lanes_decode,
clc_rans_lanes_encode_list, csrc/rans_lanes.hip) -> profiles/ar_lanes_bench.json.

JointAutoregressiveHierarchicalPriors(192, 192) and JointCheckerboardHierarchicalPriors(192, 192) with the recipe weights, at 256x256
and 512x768, batch 1 and 8.  `decompress`, wall clock around a device synchronise, in ms, for
  (a) the default one-stream format (mbt2018: a hop to the host per raster pixel; checkerboard: one per pass) — untouched code, the yardstick,
  (b) the lanes stream on the host coder (device_coder=False), W = 4: a hop per wavefront step / per pass,
  (c) the lanes stream on the device coder, W = 1, 4 and 16 (check=True: the one download of the final states is inside),
  (d) W = 4 with the same loop driven through coding.DeviceLanesSymbols — ar_finish_decode + rans_lanes_decode_step + ar_commit, three
      launches where (c) makes one — assembled here from existing pieces: (c) against (d) is the fused kernel's share.
`compress` for (a) and (c).  Every leg is warmed up; `rounds` alternating timings per leg in one process; median [min .. max].  Beside
them: the device -> host copies of one call (counted), the lanes y strings' bytes over the default's, and the device time of the y pass
alone (events) for (c) and (d).  Every decompress leg must return the same image, bit for bit.

GATE: for mbt2018, (c) at W = 4 must have a lower decompress median than (a) with disjoint ranges at both sizes and both batches, else
exit status 1.  The checkerboard legs, (c) against (d) and compress are recorded, not gated.

Fails without a GPU; there is no fallback.
usage: python tools/bench_ar_lanes.py [--rounds 7] [--out profiles/ar_lanes_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ar_lanes_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ar_lanes.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import models
from clc_amd.models import coding
from clc_amd.recipe import apply_weight_recipe, synthetic_image

W_HOST, W_DEVICE, W_GATE = 4, (1, 4, 16), 4


class count_d2h:
    """device -> host copies: Tensor.copy_ into a CPU tensor from a GPU tensor, Tensor.cpu() of a GPU tensor"""

    def __enter__(self):
        self.n = 0
        self.copy_, self.cpu = torch.Tensor.copy_, torch.Tensor.cpu
        me = self

        def copy_(t, src, *a, **k):
            if not t.is_cuda and isinstance(src, torch.Tensor) and src.is_cuda:
                me.n += 1
            return me.copy_(t, src, *a, **k)

        def cpu(t, *a, **k):
            if t.is_cuda:
                me.n += 1
            return me.cpu(t, *a, **k)

        torch.Tensor.copy_, torch.Tensor.cpu = copy_, cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.copy_, torch.Tensor.cpu = self.copy_, self.cpu
        return False


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    v = sorted(v)
    return {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "timings": len(v)}


def wins(c, a):
    return bool(c["ms_median"] < a["ms_median"] and c["ms_max"] < a["ms_min"])


def unfused_y_pass(net, subs, params):
    """the lanes decoder's loop with the step's symbols from coding.DeviceLanesSymbols: three launches behind the chain -> (y_hat, state)"""
    params, y_hat = coding.decoder_start(params, len(subs), net.M)
    B, M, H, Wl = y_hat.shape
    gc = net.gaussian_conditional
    src = coding.DeviceLanesSymbols(subs, (gc._quantized_cdf, gc._cdf_length, gc._offset), B * net._lanes_most(H, Wl) * M, y_hat.device)
    return net._decode_from(src, params, y_hat, net._lanes_passes), src.state


@torch.no_grad()
def unfused_decompress(net, strings, shape, W):
    """decompress(lanes=W, check=True) with unfused_y_pass in place of the fused loop"""
    subs = coding.lanes_parse(strings[0], W)
    z_hat = net.entropy_bottleneck.decompress(strings[1], shape)
    y_hat, state = unfused_y_pass(net, subs, net._hyper_synthesis(z_hat))
    x_hat = net._synthesis(y_hat).clamp_(0, 1)
    coding.lanes_check(state, subs)
    return {"x_hat": x_hat}


report = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "models": {}}
gates = []
for name, cls in (("mbt2018", models.JointAutoregressiveHierarchicalPriors), ("mbt2018-checkerboard", models.JointCheckerboardHierarchicalPriors)):
    net = cls(192, 192)
    apply_weight_recipe(net, 0)
    net = net.to(dev).eval()
    net.update(force=True)
    cases = []
    for h, w in ((256, 256), (512, 768)):
        for B in (1, 8):
            img = synthetic_image(B, h, w, 100, smooth=True).to(dev)
            plain = net.compress(img)
            lanes = {W: net.compress(img, lanes=W) for W in sorted(set(W_DEVICE) | {W_HOST})}
            enc = {"a_default": lambda: net.compress(img)}
            dec = {"a_default": lambda: net.decompress(plain["strings"], plain["shape"]),
                   f"b_lanes_host_W{W_HOST}": lambda: net.decompress(lanes[W_HOST]["strings"], lanes[W_HOST]["shape"], lanes=W_HOST, device_coder=False)}
            for W in W_DEVICE:
                enc[f"c_lanes_device_W{W}"] = (lambda W: lambda: net.compress(img, lanes=W))(W)
                dec[f"c_lanes_device_W{W}"] = (lambda W: lambda: net.decompress(lanes[W]["strings"], lanes[W]["shape"], lanes=W))(W)
            dec[f"d_lanes_unfused_W{W_GATE}"] = lambda: unfused_decompress(net, lanes[W_GATE]["strings"], lanes[W_GATE]["shape"], W_GATE)
            ref, copies_dec, copies_enc = None, {}, {}
            for k, fn in dec.items():   # warm-up; every leg returns the same image, bit for bit
                fn()
                with count_d2h() as c:
                    out = fn()["x_hat"]
                copies_dec[k] = c.n
                ref = out if ref is None else ref
                assert torch.equal(out, ref), (name, k)
            for k, fn in enc.items():   # ... and run to run the same strings
                fn()
                with count_d2h() as c:
                    item = fn()
                copies_enc[k] = c.n
                assert item["strings"] == (plain if k == "a_default" else lanes[item["lanes"]])["strings"], (name, k)
            td, te = {k: [] for k in dec}, {k: [] for k in enc}
            for _ in range(args.rounds):
                for k, fn in dec.items():
                    td[k].append(wall_ms(fn)[0])
                for k, fn in enc.items():
                    te[k].append(wall_ms(fn)[0])
            H, Wl = h // 16, w // 16
            segs = net._lanes_segments(H, Wl)
            case = {"image": [h, w], "batch": B, "latent": [H, Wl], "dependent_steps_default": H * Wl if name == "mbt2018" else 2,
                    "dependent_steps_lanes": sum(1 for n in segs if n), "symbols_per_image": H * Wl * net.M,
                    "decompress": {k: dict(stats(td[k]), device_to_host_copies=copies_dec[k]) for k in dec},
                    "compress": {k: dict(stats(te[k]), device_to_host_copies=copies_enc[k]) for k in enc}}
            nplain = sum(len(s) for s in plain["strings"][0])
            case["y_bytes"] = dict({"default": nplain}, **{f"W{W}": sum(len(s) for s in item["strings"][0]) for W, item in lanes.items()})
            case["y_bytes_over_default"] = {f"W{W}": sum(len(s) for s in item["strings"][0]) / nplain for W, item in lanes.items()}
            # the y pass alone, device time by events (neither loop synchronises inside)
            params = net._hyper_synthesis(net.entropy_bottleneck.decompress(plain["strings"][1], plain["shape"]))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            case["y_pass_event_ms"] = {}
            passes = {f"c_lanes_device_W{W}": (W, lambda subs: net._decode_lanes(subs, params)) for W in W_DEVICE}
            passes[f"d_lanes_unfused_W{W_GATE}"] = (W_GATE, lambda subs: unfused_y_pass(net, subs, params))
            for k, (W, run) in passes.items():
                subs = coding.lanes_parse(lanes[W]["strings"][0], W)
                ev = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    e0.record()
                    run(subs)
                    e1.record()
                    torch.cuda.synchronize()
                    ev.append(e0.elapsed_time(e1))
                case["y_pass_event_ms"][k] = stats(ev)
            kc, kd = f"c_lanes_device_W{W_GATE}", f"d_lanes_unfused_W{W_GATE}"
            won = wins(case["decompress"][kc], case["decompress"]["a_default"])
            case["device_W4_beats_default_with_disjoint_ranges"] = won
            case["decompress_ratio_default_over_device_W4"] = case["decompress"]["a_default"]["ms_median"] / case["decompress"][kc]["ms_median"]
            case["decompress_ratio_unfused_over_fused_W4"] = case["decompress"][kd]["ms_median"] / case["decompress"][kc]["ms_median"]
            case["compress_ratio_default_over_device_W4"] = case["compress"]["a_default"]["ms_median"] / case["compress"][kc]["ms_median"]
            if name == "mbt2018":
                gates.append(won)
            cases.append(case)
            line = lambda legs: " | ".join(f"{k} {v['ms_median']:.2f} [{v['ms_min']:.2f} .. {v['ms_max']:.2f}] ms, {v['device_to_host_copies']} d2h"
                                           for k, v in legs.items())
            print(f"{name} {h}x{w} batch {B} decompress: {line(case['decompress'])}", flush=True)
            print(f"{name} {h}x{w} batch {B} compress:   {line(case['compress'])}", flush=True)
            print(f"{name} {h}x{w} batch {B} y pass (events): " + ", ".join(f"{k} {v['ms_median']:.2f} ms" for k, v in case["y_pass_event_ms"].items())
                  + " | bytes x" + ", ".join(f"{k} {v:.4f}" for k, v in case["y_bytes_over_default"].items()), flush=True)
    report["models"][name] = {"model": f"{cls.__name__}(192, 192)", "cases": cases}

gate = bool(gates) and all(gates)
report["gate"] = {"what": "mbt2018: (c) at W = 4 has a lower decompress median than (a), with disjoint ranges, at both sizes and both batches",
                  "per_case": gates, "passed": gate}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("mbt2018: the device coder at W = 4 beats the default decoder at every size and batch, with disjoint ranges:", gate)
sys.exit(0 if gate else 1)
