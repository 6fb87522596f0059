"""Measurements for the lanes stream of elic2022 and its device coder (clc_rans_lanes_encode / clc_rans_lanes_decode_step,
csrc/rans_lanes.hip) -> profiles/scctx_lanes_bench.json.

Elic2022() at its default size with the recipe weights, at 256x256 and 512x768, batch 1 and 8.  `compress` and `decompress`, wall clock
around a device synchronise, in ms, for
  (a) the default one-stream format (a hop to the host per pass, one sequential host coder per image) — the yardstick,
  (b) the lanes stream on the host coder (device_coder=False), W = 4 (its compress is the device encoder's: there is no other),
  (c) the lanes stream on the device coder, W = 1, 4 and 16 (check=True: the one download of the final states is inside).
Every leg is warmed up; `rounds` alternating timings per leg in one process; median [min .. max].  Beside them: the device -> host copies
of one call (counted), the lanes y strings' bytes over the default's, and the device time of the y pass alone (events), default excluded
(it synchronises inside).  Every leg must return the same image, bit for bit.

GATE: (c) at W = 4, 512x768, batch 8 must have a lower median than (a) with disjoint ranges, for decompress AND for compress, else exit
status 1.

Fails without a GPU; there is no fallback.
usage: python tools/bench_scctx_lanes.py [--rounds 7] [--out profiles/scctx_lanes_bench.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scctx_lanes_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_scctx_lanes.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import models
from clc_amd.models import coding
from clc_amd.recipe import apply_weight_recipe, synthetic_image

W_HOST, W_DEVICE, W_GATE = 4, (1, 4, 16), 4
GATE_CASE = (512, 768, 8)
net = models.Elic2022()
apply_weight_recipe(net, 0)
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


def wins(c, a):
    return bool(c["ms_median"] < a["ms_median"] and c["ms_max"] < a["ms_min"])


report = {"model": "Elic2022()", "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "cases": []}
gate = None
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
        ref, copies_dec, copies_enc = None, {}, {}
        for k, fn in dec.items():   # warm-up; every leg returns the same image, bit for bit
            fn()
            with count_d2h() as c:
                out = fn()["x_hat"]
            copies_dec[k] = c.n
            ref = out if ref is None else ref
            assert torch.equal(out, ref), k
        for k, fn in enc.items():   # ... and run to run the same strings
            fn()
            with count_d2h() as c:
                item = fn()
            copies_enc[k] = c.n
            assert item["strings"] == (plain if k == "a_default" else lanes[item["lanes"]])["strings"], k
        td, te = {k: [] for k in dec}, {k: [] for k in enc}
        for _ in range(args.rounds):
            for k, fn in dec.items():
                td[k].append(wall_ms(fn)[0])
            for k, fn in enc.items():
                te[k].append(wall_ms(fn)[0])
        H, Wl = h // 16, w // 16
        case = {"image": [h, w], "batch": B, "latent": [H, Wl], "passes": 2 * len(net.groups), "symbols_per_image": H * Wl * net.M,
                "decompress": {k: dict(stats(td[k]), device_to_host_copies=copies_dec[k]) for k in dec},
                "compress": {k: dict(stats(te[k]), device_to_host_copies=copies_enc[k]) for k in enc}}
        nplain = sum(len(s) for s in plain["strings"][0])
        case["y_bytes"] = dict({"default": nplain}, **{f"W{W}": sum(len(s) for s in item["strings"][0]) for W, item in lanes.items()})
        case["y_bytes_over_default"] = {f"W{W}": sum(len(s) for s in item["strings"][0]) / nplain for W, item in lanes.items()}
        # the y pass alone, device time by events (the device coder never synchronises inside)
        params = net._hyper_synthesis(net.entropy_bottleneck.decompress(plain["strings"][1], plain["shape"]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        case["y_pass_event_ms"] = {}
        for W in W_DEVICE:
            subs = coding.lanes_parse(lanes[W]["strings"][0], W)
            ev = []
            for _ in range(3):
                torch.cuda.synchronize()
                e0.record()
                net._scctx_decode_lanes(subs, params)
                e1.record()
                torch.cuda.synchronize()
                ev.append(e0.elapsed_time(e1))
            case["y_pass_event_ms"][f"W{W}"] = stats(ev)
        report["cases"].append(case)
        line = lambda legs: " | ".join(f"{k} {v['ms_median']:.1f} [{v['ms_min']:.1f} .. {v['ms_max']:.1f}] ms, {v['device_to_host_copies']} d2h"
                                       for k, v in legs.items())
        print(f"{h}x{w} batch {B} decompress: {line(case['decompress'])}", flush=True)
        print(f"{h}x{w} batch {B} compress:   {line(case['compress'])}", flush=True)
        print(f"{h}x{w} batch {B} y pass (events): " + ", ".join(f"{k} {v['ms_median']:.1f} ms" for k, v in case["y_pass_event_ms"].items())
              + " | bytes x" + ", ".join(f"{k} {v:.4f}" for k, v in case["y_bytes_over_default"].items()), flush=True)
        if (h, w, B) == GATE_CASE:
            k = f"c_lanes_device_W{W_GATE}"
            g_dec, g_enc = wins(case["decompress"][k], case["decompress"]["a_default"]), wins(case["compress"][k], case["compress"]["a_default"])
            gate = g_dec and g_enc
            report["gate"] = {"case": "512x768 batch 8, W = 4", "decompress_wins_with_disjoint_ranges": g_dec, "compress_wins_with_disjoint_ranges": g_enc,
                              "decompress_ratio_default_over_device": case["decompress"]["a_default"]["ms_median"] / case["decompress"][k]["ms_median"],
                              "compress_ratio_default_over_device": case["compress"]["a_default"]["ms_median"] / case["compress"][k]["ms_median"]}

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("the device coder at W = 4 beats the default coder at 512x768, batch 8, with disjoint ranges, for decompress and compress:", gate)
sys.exit(0 if gate else 1)
