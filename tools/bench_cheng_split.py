"""Measurements for the split stream of cheng2020 and its device decoder (clc_gmm_decode_step, csrc/gmm.hip)
-> profiles/cheng_split_bench.json.

Cheng2020Attention(192, K = 3) with the recipe weights and the tests' scalings, at 256x256 and 512x768, batch 1 and 8.  `decompress`,
wall clock around a device synchronise, in ms, for
  (a) the default one-stream format (a hop to the host per wavefront step) — the yardstick,
  (b) the split stream on the host decoder (device_decoder=False), S = 16,
  (c) the split stream on the device decoder, S = 4, 16 and 64 (check=True: the one download of the final states is inside).
Every leg is warmed up; `rounds` alternating timings per leg in one process; median [min .. max].  Beside them: the device -> host copies
of one call (counted), the split y strings' bytes over the default's, and the device time of the hop-free pass alone (events).

GATE: (c) at S = 16, 512x768, batch 1 must have a lower median than (a) with disjoint ranges, else exit status 1.

Fails without a GPU; there is no fallback.
usage: python tools/bench_cheng_split.py [--rounds 7] [--out profiles/cheng_split_bench.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cheng_split_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_cheng_split.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import ans, models
from clc_amd.models import coding
from clc_amd.recipe import apply_weight_recipe, synthetic_image

K, N = 3, 192
S_HOST, S_DEVICE, S_GATE = 16, (4, 16, 64), 16
net = models.Cheng2020Attention(N, K)
apply_weight_recipe(net, 0)
with torch.no_grad():   # the scalings of the tests: latents of a few bins, scales off the 0.11 bound
    net.g_a[7].weight.mul_(20.0)
    net.h_s[8].weight.mul_(4.0)
    net.h_s[8].bias.add_(0.6)
    net.entropy_parameters[4].weight.mul_(8.0)
    net.entropy_parameters[4].bias[:K * N].add_(0.6)
net = net.to(dev).eval()
net.update(force=True)


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


report = {"model": f"Cheng2020Attention({N}, K={K})", "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "cases": []}
gate = None
for h, w in ((256, 256), (512, 768)):
    for B in (1, 8):
        img = synthetic_image(B, h, w, 100, smooth=True).to(dev)
        plain = net.compress(img)
        split = {S: net.compress(img, substreams=S) for S in sorted(set(S_DEVICE) | {S_HOST})}
        legs = {"a_default": lambda: net.decompress(plain["strings"], plain["shape"]),
                f"b_split_host_S{S_HOST}": lambda: net.decompress(split[S_HOST]["strings"], split[S_HOST]["shape"], substreams=S_HOST,
                                                                  device_decoder=False)}
        for S in S_DEVICE:
            legs[f"c_split_device_S{S}"] = (lambda S: lambda: net.decompress(split[S]["strings"], split[S]["shape"], substreams=S))(S)
        ref, copies = None, {}
        for k, fn in legs.items():   # warm-up; every leg returns the same image, bit for bit
            fn()
            with count_d2h() as c:
                out = fn()["x_hat"]
            copies[k] = c.n
            ref = out if ref is None else ref
            assert torch.equal(out, ref), k
        t = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                t[k].append(wall_ms(fn)[0])
        case = {"image": [h, w], "batch": B, "latent": [h // 16, w // 16], "wavefront_steps": w // 16 + 3 * (h // 16 - 1), "legs": {}}
        nplain = sum(len(s) for s in plain["strings"][0])
        for k in legs:
            case["legs"][k] = dict(stats(t[k]), device_to_host_copies=copies[k])
        for S, item in split.items():
            n = sum(len(s) for s in item["strings"][0])
            case.setdefault("y_bytes", {"default": nplain})[f"S{S}"] = n
            case.setdefault("y_bytes_over_default", {})[f"S{S}"] = n / nplain
        # the hop-free pass alone, device time by events
        params = net._hyper_synthesis(net.entropy_bottleneck.decompress(plain["strings"][1], plain["shape"]))
        subs = coding.stream_parse(ans.SPLIT_STREAM, split[S_GATE]["strings"][0], S_GATE, "substreams")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev = []
        for _ in range(3):
            torch.cuda.synchronize()
            e0.record()
            net._gmm_decode_split(subs, params)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        case[f"device_pass_S{S_GATE}_event_ms"] = stats(ev)
        report["cases"].append(case)
        print(f"{h}x{w} batch {B}: " + " | ".join(
            f"{k} {v['ms_median']:.1f} [{v['ms_min']:.1f} .. {v['ms_max']:.1f}] ms, {v['device_to_host_copies']} d2h" for k, v in case["legs"].items())
            + f" | pass S{S_GATE} {case[f'device_pass_S{S_GATE}_event_ms']['ms_median']:.1f} ms | bytes x"
            + ", ".join(f"{k} {v:.4f}" for k, v in case["y_bytes_over_default"].items()), flush=True)
        if (h, w, B) == (512, 768, 1):
            a, c = case["legs"]["a_default"], case["legs"][f"c_split_device_S{S_GATE}"]
            gate = bool(c["ms_median"] < a["ms_median"] and c["ms_max"] < a["ms_min"])
            report["gate"] = {"case": "512x768 batch 1", "device_S16_wins_with_disjoint_ranges": gate,
                              "ratio_default_over_device": a["ms_median"] / c["ms_median"]}

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("the device decoder at S = 16 beats the default decoder at 512x768, batch 1, with disjoint ranges:", gate)
sys.exit(0 if gate else 1)
