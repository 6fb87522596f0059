"""Measurements for clc_amd.codec.ContextCodecEngine — mbt2018 and mbt2018-checkerboard on the lanes stream, one captured graph per
call -> profiles/ctx_engine_bench.json.

JointAutoregressiveHierarchicalPriors(192, 192) and JointCheckerboardHierarchicalPriors(192, 192) with tools/bench_ar_lanes.py's
weights, at 256x256 and 512x768, batch 1 and 8, W = 4.  `decompress` and `compress`, wall clock around a device synchronise, in ms, for
  (a) model.decompress(..., lanes=4) / model.compress(x, lanes=4): the model's own calls, eager launches — untouched, the yardstick,
  (b) the engine with use_graph=True: one replay per call,
  (c) the engine with use_graph=False: the same plan functions run eagerly.
Every leg is warmed up (the engines' plans are built there: `capture_ms` is what that cost); `rounds` alternating timings per leg in one
process; median [min .. max].  Beside them: the device -> host copies of one call (counted) and capture_ms.  Every decompress leg must
return the same image, bit for bit, and every compress leg the model's strings.

GATE: for mbt2018, decompress at batch 1, (b) must have a lower median than (a) with disjoint ranges at both sizes, else exit status 1.
The checkerboard model, batch 8 and compress are recorded, not gated.

Fails without a GPU; there is no fallback.
usage: python tools/bench_ctx_engine.py [--rounds 7] [--out profiles/ctx_engine_bench.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctx_engine_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ctx_engine.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import models
from clc_amd.codec import ContextCodecEngine
from clc_amd.recipe import apply_weight_recipe, synthetic_image

W = 4


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


def wins(b, a):
    return bool(b["ms_median"] < a["ms_median"] and b["ms_max"] < a["ms_min"])


report = {"rounds": args.rounds, "lanes": W, "device": torch.cuda.get_device_name(0), "models": {}}
gates = []
for name, cls in (("mbt2018", models.JointAutoregressiveHierarchicalPriors), ("mbt2018-checkerboard", models.JointCheckerboardHierarchicalPriors)):
    net = cls(192, 192)
    apply_weight_recipe(net, 0)
    net = net.to(dev).eval()
    net.update(force=True)
    cases = []
    with ContextCodecEngine(net, lanes=W, use_graph=True) as graphed, ContextCodecEngine(net, lanes=W, use_graph=False) as eager:
        for h, w in ((256, 256), (512, 768)):
            for B in (1, 8):
                img = synthetic_image(B, h, w, 100, smooth=True).to(dev)
                want = net.compress(img, lanes=W)
                items = [{"strings": [[y], [z]], "shape": want["shape"], "kernel_config": want["kernel_config"], "lanes": W}
                         for y, z in zip(*want["strings"])]
                dec = {"a_model": lambda: net.decompress(want["strings"], want["shape"], lanes=W)["x_hat"],
                       "b_engine_graph": lambda: graphed.decompress(items), "c_engine_eager": lambda: eager.decompress(items)}
                strings = lambda out: [[it["strings"][0][0] for it in out], [it["strings"][1][0] for it in out]]
                enc = {"a_model": lambda: net.compress(img, lanes=W)["strings"], "b_engine_graph": lambda: strings(graphed.compress(img)),
                       "c_engine_eager": lambda: strings(eager.compress(img))}
                engines = {"b_engine_graph": graphed, "c_engine_eager": eager}
                ref, copies, capture = None, {"decompress": {}, "compress": {}}, {"decompress": {}, "compress": {}}
                for op, legs in (("decompress", dec), ("compress", enc)):
                    for k, fn in legs.items():   # warm-up (the engines build their plan here), then one counted call
                        fn()
                        if k in engines:
                            capture[op][k] = engines[k].last["capture_ms"]
                        with count_d2h() as c:
                            out = fn()
                        copies[op][k] = c.n
                        if op == "decompress":   # every leg returns the same image, bit for bit
                            ref = out if ref is None else ref
                            assert torch.equal(out, ref), (name, k)
                        else:
                            assert out == want["strings"], (name, k)
                        if k in engines:
                            assert engines[k].last["capture_ms"] == 0.0 and engines[k].last["graphs"] == (1 if k == "b_engine_graph" else 0)
                td, te = {k: [] for k in dec}, {k: [] for k in enc}
                for _ in range(args.rounds):
                    for k, fn in dec.items():
                        td[k].append(wall_ms(fn)[0])
                    for k, fn in enc.items():
                        te[k].append(wall_ms(fn)[0])
                H, Wl = h // 16, w // 16
                case = {"image": [h, w], "batch": B, "latent": [H, Wl], "dependent_steps": sum(1 for n in net._lanes_segments(H, Wl) if n),
                        "decompress": {k: dict(stats(td[k]), device_to_host_copies=copies["decompress"][k]) for k in dec},
                        "compress": {k: dict(stats(te[k]), device_to_host_copies=copies["compress"][k]) for k in enc},
                        "capture_ms": capture}
                for op in ("decompress", "compress"):
                    case[f"{op}_ratio_model_over_graph"] = case[op]["a_model"]["ms_median"] / case[op]["b_engine_graph"]["ms_median"]
                    case[f"{op}_ratio_eager_over_graph"] = case[op]["c_engine_eager"]["ms_median"] / case[op]["b_engine_graph"]["ms_median"]
                won = wins(case["decompress"]["b_engine_graph"], case["decompress"]["a_model"])
                case["graph_beats_model_decompress_with_disjoint_ranges"] = won
                if name == "mbt2018" and B == 1:
                    gates.append(won)
                cases.append(case)
                line = lambda legs: " | ".join(f"{k} {v['ms_median']:.2f} [{v['ms_min']:.2f} .. {v['ms_max']:.2f}] ms, {v['device_to_host_copies']} d2h"
                                               for k, v in legs.items())
                print(f"{name} {h}x{w} batch {B} decompress: {line(case['decompress'])}", flush=True)
                print(f"{name} {h}x{w} batch {B} compress:   {line(case['compress'])}", flush=True)
                print(f"{name} {h}x{w} batch {B} capture_ms: " + ", ".join(f"{op} {k} {v:.0f}" for op, d in capture.items() for k, v in d.items()), flush=True)
    report["models"][name] = {"model": f"{cls.__name__}(192, 192)", "cases": cases}

gate = bool(gates) and all(gates)
report["gate"] = {"what": "mbt2018, decompress at batch 1: (b) the engine's graph has a lower median than (a) the model's call, with disjoint ranges, "
                          "at both sizes", "per_case": gates, "passed": gate}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("mbt2018: one replay beats the model's eager decompress at batch 1 at both sizes, with disjoint ranges:", gate)
sys.exit(0 if gate else 1)
