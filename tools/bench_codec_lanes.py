"""Measurements for the lanes stream of CLC / TCM and its device coder inside the CodecEngine (clc_rans_lanes_decode_gauss,
clc_rans_lanes_pack, csrc/rans_lanes.hip) -> profiles/codec_lanes_bench.json.

CLC() with one reference and the recipe weights, at 256x256 and 512x768, batch 1 and 8.  `compress` and `decompress`, wall clock around a
device synchronise, in ms, for
  (a) the default engine (the one-stream format: a hop to the host per slice, one sequential host coder per image) — the yardstick,
  (b) the lanes format on the host coder (model._decompress_eager(device_coder=False)), W = 4: launch by launch, a hop per slice,
  (c) the lanes format on the engine's device path, W = 1, 4 and 16 (check=True: the one download of the end states is inside).
Every leg is warmed up; `rounds` alternating timings per leg in one process; median [min .. max].  Beside them: the device -> host
copies of one call (counted), the lanes y strings' bytes over the default's, and — device time under events — the slice coder alone
over the five slices of the case: clc_rans_lanes_decode_gauss against the composition it replaces (quantize_build_indexes on a zero
tensor, clc_rans_lanes_decode_step, the int -> float conversion and the add).  Every leg must return the same image, bit for bit.

GATE: (c) at W = 4, 256x256, batch 8 must have a lower `decompress` median than (a) with disjoint ranges, else exit status 1.
Everything else is reported.

Fails without a GPU; there is no fallback.
usage: python tools/bench_codec_lanes.py [--rounds 7] [--out profiles/codec_lanes_bench.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_lanes_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_codec_lanes.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import ans, codec, models, ops
from clc_amd.models import coding
from clc_amd.recipe import apply_weight_recipe, synthetic_image

W_HOST, W_DEVICE, W_GATE = 4, (1, 4, 16), 4
GATE_CASE = (256, 256, 8)
net = models.CLC(num_ref_frames=1)
apply_weight_recipe(net, 0)
net = net.to(dev).eval()
net.update(force=True)
eng = codec.CodecEngine(net, threads=8)


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


def slice_coder_events(items, W, B, h, w):
    """the five slice steps' coder alone on the case's own streams, scales of the symbols' rows and zero means: fused against unfused"""
    gc = net.gaussian_conditional
    tables = (gc._quantized_cdf, gc._cdf_length, gc._offset)
    table = gc.scale_table
    S, Cs = net.num_slices, net.M // net.num_slices
    cdf, ln, off = gc.host_tables()
    subs = coding.lanes_parse([it["strings"][0][0] for it in items], W)
    n = h * w * Cs
    # the mean and scale maps of every slice, kept from one eager decode of the same strings
    maps = []
    slice_params = net._slice_params
    net._slice_params = lambda *a, **k: (lambda r: maps.append((r[1], r[2])) or r)(slice_params(*a, **k))
    try:
        strings = [[it["strings"][0][0] for it in items], [it["strings"][1][0] for it in items]]
        net._decompress_eager(strings, items[0]["shape"], refs_of[B], lanes=W, check=False)
    finally:
        del net._slice_params
    state0, spans, words = coding.upload_streams(subs, 2 * ans.LANES, dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def fused(state):
        return [ops.rans_lanes_decode_gauss(sc, mu, table, tables, words, spans, state) for mu, sc in maps]

    def unfused(state):
        out = []
        for mu, sc in maps:
            idx = gc.build_indexes(sc)                                                    # quantize_build_indexes on a zero tensor
            ib = idx.permute(0, 2, 3, 1).reshape(B, n)                                    # (a view: the NHWC buffer itself)
            sb = torch.empty((B, n), device=dev, dtype=torch.int32)
            ops.rans_lanes_decode_step(ib, n, tables, words, spans, state, sb)
            out.append(sb.view(B, h, w, Cs).permute(0, 3, 1, 2).float() + mu)             # the conversion and the add
        return out

    res = {}
    ref = None
    for name, fn in (("fused", fused), ("unfused", unfused)):
        ev = []
        for _ in range(5):
            state = state0.clone()
            torch.cuda.synchronize()
            e0.record()
            out = fn(state)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        ref = out if ref is None else ref
        assert all(torch.equal(a, b) for a, b in zip(out, ref)), name
        res[name] = stats(ev[1:])
    return res


report = {"model": "CLC(num_ref_frames=1)", "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "cases": []}
gate = None
refs_of = {}
for h, w in ((256, 256), (512, 768)):
    for B in (1, 8):
        img = synthetic_image(B, h, w, 100, smooth=True).to(dev)
        refs = [synthetic_image(B, h, w, 200, smooth=True).to(dev)]
        refs_of[B] = refs
        plain = eng.compress(img, refs)
        lanes = {W: eng.compress(img, refs, lanes=W) for W in sorted(set(W_DEVICE) | {W_HOST})}
        shape = plain[0]["shape"]
        host_strings = [[it["strings"][0][0] for it in lanes[W_HOST]], [it["strings"][1][0] for it in lanes[W_HOST]]]
        enc = {"a_default": lambda: eng.compress(img, refs)}
        dec = {"a_default": lambda: eng.decompress(plain, refs),
               f"b_lanes_host_W{W_HOST}": lambda: net._decompress_eager(host_strings, shape, refs, lanes=W_HOST, device_coder=False)["x_hat"]}
        for W in W_DEVICE:
            enc[f"c_lanes_device_W{W}"] = (lambda W: lambda: eng.compress(img, refs, lanes=W))(W)
            dec[f"c_lanes_device_W{W}"] = (lambda W: lambda: eng.decompress(lanes[W], refs, lanes=W))(W)
        ref, copies_dec, copies_enc = None, {}, {}
        for k, fn in dec.items():   # warm-up; every leg returns the same image, bit for bit
            fn()
            with count_d2h() as c:
                out = fn()
            copies_dec[k] = c.n
            ref = out if ref is None else ref
            assert torch.equal(out, ref), k
        for k, fn in enc.items():   # ... and run to run the same strings
            fn()
            with count_d2h() as c:
                items = fn()
            copies_enc[k] = c.n
            want = plain if k == "a_default" else lanes[items[0]["lanes"]]
            assert [it["strings"] for it in items] == [it["strings"] for it in want], k
        td, te = {k: [] for k in dec}, {k: [] for k in enc}
        for _ in range(args.rounds):
            for k, fn in dec.items():
                td[k].append(wall_ms(fn)[0])
            for k, fn in enc.items():
                te[k].append(wall_ms(fn)[0])
        H, Wl = h // 16, w // 16
        case = {"image": [h, w], "batch": B, "latent": [H, Wl], "slices": net.num_slices, "symbols_per_image": H * Wl * net.M,
                "decompress": {k: dict(stats(td[k]), device_to_host_copies=copies_dec[k]) for k in dec},
                "compress": {k: dict(stats(te[k]), device_to_host_copies=copies_enc[k]) for k in enc}}
        nplain = sum(len(it["strings"][0][0]) for it in plain)
        ybytes = {f"W{W}": sum(len(it["strings"][0][0]) for it in items) for W, items in lanes.items()}
        case["y_bytes"] = dict({"default": nplain}, **ybytes)
        case["y_bytes_over_default"] = {k: v / nplain for k, v in ybytes.items()}
        case["slice_coder_event_ms"] = {f"W{W}": slice_coder_events(lanes[W], W, B, H, Wl) for W in W_DEVICE}
        report["cases"].append(case)
        line = lambda legs: " | ".join(f"{k} {v['ms_median']:.2f} [{v['ms_min']:.2f} .. {v['ms_max']:.2f}] ms, {v['device_to_host_copies']} d2h"
                                       for k, v in legs.items())
        print(f"{h}x{w} batch {B} decompress: {line(case['decompress'])}", flush=True)
        print(f"{h}x{w} batch {B} compress:   {line(case['compress'])}", flush=True)
        print(f"{h}x{w} batch {B} slice coder x{net.num_slices} (events): "
              + ", ".join(f"{k} fused {v['fused']['ms_median']:.3f} / unfused {v['unfused']['ms_median']:.3f} ms" for k, v in case["slice_coder_event_ms"].items())
              + " | bytes x" + ", ".join(f"{k} {v:.4f}" for k, v in case["y_bytes_over_default"].items()), flush=True)
        if (h, w, B) == GATE_CASE:
            k = f"c_lanes_device_W{W_GATE}"
            gate = wins(case["decompress"][k], case["decompress"]["a_default"])
            report["gate"] = {"case": "256x256 batch 8, W = 4, decompress", "wins_with_disjoint_ranges": gate,
                              "ratio_default_over_device": case["decompress"]["a_default"]["ms_median"] / case["decompress"][k]["ms_median"]}

eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("the engine's lanes decompress at W = 4 beats the default engine at 256x256, batch 8, with disjoint ranges:", gate)
sys.exit(0 if gate else 1)
