"""Per-image codec time with references from a clc_amd.refbank.ReferenceBank against reference tensors, on one GPU.

usage: python tools/bench_refbank.py [--reps N] [--batch B]

Settings (CLC N=128, recipe weights): 256x256 and 512x768 images, R = 1 and R = 3.  Modes per setting:
  tensors  CodecEngine.compress(x, refs) / decompress(items, refs) with the prepared reference tensors (the existing path)
  cold     the bank path with an emptied cache before every call (every call encodes its references)
  warm     the bank path with the references resident (the gather only)
All settings and modes are interleaved in one process (round-robin per repetition); the table shows the median ms per image of
compress and decompress (host rANS included, as a caller sees it), and whether the bank path's streams and images equal the tensor path's.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from clc_amd import codec, models, refbank  # noqa: E402
from clc_amd.recipe import apply_weight_recipe, synthetic_image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch
    settings = []
    for R in (1, 3):
        m = models.CLC(N=128, num_ref_frames=R)
        apply_weight_recipe(m, 0)
        m = m.to(dev).eval()
        m.update(force=True)
        eng = codec.CodecEngine(m, threads=8)
        for hw in ((256, 256), (512, 768)):
            refs = {f"k{i}": synthetic_image(1, hw[0] + 37 * (i % 3), hw[1] - 29 * (i % 2), 700 + i, smooth=True)[0].to(dev) for i in range(2 * R * B)}
            bank = refbank.ReferenceBank(m, refs, capacity_bytes=1 << 30)
            keys = list(refs)
            rows = [keys[b * R:(b + 1) * R] for b in range(B)]
            x = torch.cat([synthetic_image(1, hw[0], hw[1], 800 + b, smooth=True) for b in range(B)]).to(dev)
            prep = [bank.prepare(r, hw) for r in rows]
            tens = [torch.cat([p[j:j + 1] for p in prep]) for j in range(R)]
            settings.append({"name": f"{hw[0]}x{hw[1]} R={R}", "eng": eng, "bank": bank, "rows": rows, "x": x, "refs": tens, "hw": hw,
                             "t": {k: ([], []) for k in ("tensors", "cold", "warm")}})

    def run(s, mode):
        eng, bank = s["eng"], s["bank"]
        if mode == "cold":
            bank.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "tensors":
            outs = eng.compress(s["x"], s["refs"])
        else:
            outs = eng.compress(s["x"], ref_keys=s["rows"], bank=bank)
        t1 = time.perf_counter()
        if mode == "cold":
            bank.clear()
        t2 = time.perf_counter()
        xh = eng.decompress(outs, s["refs"]) if mode == "tensors" else eng.decompress(outs, bank=bank)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return outs, xh, (t1 - t0) * 1e3 / B, (t3 - t2) * 1e3 / B

    # warm-up: every plan captured, and the bank path checked against the tensor path
    for s in settings:
        ref = run(s, "tensors")
        for mode in ("cold", "warm"):
            o, xh, _, _ = run(s, mode)
            s.setdefault("same", True)
            s["same"] &= [q["strings"] for q in o] == [q["strings"] for q in ref[0]] and torch.equal(xh, ref[1])
    for _ in range(a.reps):
        for s in settings:
            for mode in ("tensors", "cold", "warm"):
                _, _, c, d = run(s, mode)
                s["t"][mode][0].append(c)
                s["t"][mode][1].append(d)
    print(f"{torch.cuda.get_device_name(0)}; CLC N=128, batch {B}, median of {a.reps} interleaved repetitions, ms per image")
    print(f"{'setting':16s} {'tensors c/d':>16s} {'cold bank c/d':>16s} {'warm bank c/d':>16s}  same bits")
    for s in settings:
        med = {k: (statistics.median(v[0]), statistics.median(v[1])) for k, v in s["t"].items()}
        print(f"{s['name']:16s} " + " ".join(f"{med[k][0]:7.2f} /{med[k][1]:7.2f}" for k in ("tensors", "cold", "warm")) + f"  {s['same']}")


if __name__ == "__main__":
    main()
