"""Micro-benchmark of the on-device k-means (clc_amd/kmeans.py) -> profiles/kmeans_bench.json.

1. Assignment pass, device time by events, at least `reps` calls per timing (more where that is under `window-ms` of work): the fused kernel (clc_kmeans_assign: running arg-min in the GEMM epilogue,
   [N, K] never written) against the way the same labels were obtained before it existed: ReferenceIndex._scores(x, centres, |c|^2) on the
   1x1-convolution MFMA kernel, which materialises [N, K], followed by argmax(1).  The two alternate in one process, `rounds` timings
   each; median and range (min .. max) are reported.  TF = 2 N K D / t, share of the 157.3 TF f32-MFMA peak.  The labels of both are
   compared (they may differ on near-ties only: two summation orders).
2. Update and representatives launches on the labels of (1), same timing.
3. Context, not a ranking (the algorithms differ): wall time of a full DeviceKMeans.fit and of sklearn's
   MiniBatchKMeans(batch_size=1000, random_state=42) on the same features, and both inertias evaluated in float64.
usage: python tools/bench_kmeans.py [--reps 5] [--rounds 7] [--window-ms 100] [--out profiles/kmeans_bench.json] [--no-context]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from clc_amd import kmeans as km
from clc_amd.retrieval import ReferenceIndex

PEAK_TF = 157.3
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--window-ms", type=float, default=100.0, help="least timed window of the assignment pass; raises the calls per timing above --reps")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kmeans_bench.json"))
ap.add_argument("--no-context", action="store_true")
ap.add_argument("--shapes", default="100000x3000x2048,100000x1000x256", help="N x K x D, comma separated")
ap.add_argument("--context-shape", default="100000x1000x256")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_kmeans.py measures on the GPU: none found")
dev = torch.device("cuda:0")


def time_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def stats(v):
    v = sorted(v)
    return {"us_median": v[len(v) // 2], "us_min": v[0], "us_max": v[-1]}


def make(N, K, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, D, generator=g).to(dev)
    c = x[torch.randperm(N, generator=g)[:K].to(dev)].contiguous()
    return x, c


rows = []
for shape in args.shapes.split(","):
    N, K, D = (int(v) for v in shape.split("x"))
    x, c = make(N, K, D, 0)
    csq = (c.double() ** 2).sum(1).float()
    out = {}

    def fused():
        out["fused"] = km.kmeans_assign(x, c)[0]

    def baseline():
        out["baseline"] = ReferenceIndex._scores(None, x, c, csq).argmax(1)

    for fn in (fused, baseline):   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    differ = int((out["fused"].long() != out["baseline"]).sum())
    # a timed window of at least --window-ms for the faster of the two (a few milliseconds would measure the clock ramp and the scheduler)
    reps = max(args.reps, int(np.ceil(args.window_ms * 1e3 / min(time_us(fused, 2), time_us(baseline, 2)))))
    t = {"fused": [], "baseline": []}
    for _ in range(args.rounds):   # alternate, so a clock or thermal drift hits both alike
        t["fused"].append(time_us(fused, reps))
        t["baseline"].append(time_us(baseline, reps))
    labels = out["fused"]
    t_upd = [time_us(lambda: km.kmeans_update(x, labels, K, c), args.reps) for _ in range(args.rounds)]
    t_rep = [time_us(lambda: km.kmeans_representatives(x, labels, c), args.reps) for _ in range(args.rounds)]
    flop = 2.0 * N * K * D
    row = {"N": N, "K": K, "D": D, "gflop": flop / 1e9, "calls_per_timing": reps, "labels_differing_from_baseline": differ}
    for k in t:
        row[k] = stats(t[k])
        row[k]["tflops"] = flop / row[k]["us_median"] / 1e6
        row[k]["share_of_f32_mfma_peak"] = row[k]["tflops"] / PEAK_TF
    row["update_incl_argsort"], row["representatives_incl_argsort"] = stats(t_upd), stats(t_rep)
    row["fused_not_slower"] = row["fused"]["us_median"] <= row["baseline"]["us_median"]
    rows.append(row)
    print(f"({N}, {K}, {D}) {flop / 1e9:7.1f} GF | " + " | ".join(
        f"{k} {row[k]['us_median']:9.1f} us [{row[k]['us_min']:.1f} .. {row[k]['us_max']:.1f}] {row[k]['tflops']:5.1f} TF {100 * row[k]['share_of_f32_mfma_peak']:4.1f}%"
        for k in t) + f" | update {row['update_incl_argsort']['us_median']:.1f} us | representatives {row['representatives_incl_argsort']['us_median']:.1f} us"
        f" | labels differing {differ}", flush=True)
    del x, c, out, labels
    torch.cuda.empty_cache()


def inertia64(x, centres):
    """sum_i min_k |x_i - c_k|^2 in float64, row blocks of 4096"""
    c = torch.as_tensor(np.asarray(centres), device=dev).double()
    cs, tot = (c ** 2).sum(1), 0.0
    for i in range(0, x.shape[0], 4096):
        xb = x[i:i + 4096].double()
        tot += float(((xb ** 2).sum(1) + (cs[None] - 2.0 * xb @ c.T).min(1).values).sum())
    return tot


context = None
if not args.no_context:
    from sklearn.cluster import MiniBatchKMeans

    N, K, D = (int(v) for v in args.context_shape.split("x"))
    x, _ = make(N, K, D, 1)
    km.DeviceKMeans(K, max_iter=1).fit(x)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est = km.DeviceKMeans(K).fit(x)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    xh = x.cpu().numpy()
    t0 = time.perf_counter()
    sk = MiniBatchKMeans(n_clusters=K, random_state=42, batch_size=1000).fit(xh)
    t_sk = time.perf_counter() - t0
    context = {"N": N, "K": K, "D": D, "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
               "device_fit": {"wall_s": t_dev, "n_iter": est.n_iter_, "inertia_float64": inertia64(x, est.cluster_centers_.cpu().numpy())},
               "sklearn_minibatch": {"wall_s": t_sk, "n_iter": int(sk.n_iter_), "inertia_float64": inertia64(x, sk.cluster_centers_)}}
    print(f"context ({N}, {K}, {D}): DeviceKMeans.fit {t_dev:.2f} s, {est.n_iter_} iterations, inertia {context['device_fit']['inertia_float64']:.6g} | "
          f"sklearn MiniBatchKMeans {t_sk:.2f} s, inertia {context['sklearn_minibatch']['inertia_float64']:.6g}", flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"reps": args.reps, "rounds": args.rounds, "window_ms": args.window_ms, "peak_tf": PEAK_TF, "device": torch.cuda.get_device_name(0), "assign": rows, "context": context}, f, indent=1)
sys.exit(0 if all(r["fused_not_slower"] for r in rows) else 1)
