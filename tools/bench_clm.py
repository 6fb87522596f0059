"""Micro-benchmark of the CLM similarity op through the C ABI: the inference forward (clc_clm_sim_colsum), the recorded forward
(clc_clm_sim_colsum_train) and the backward (clc_clm_sim_colsum_bwd).  Graph replay, device time only; the two forwards alternate in
one process, `rounds` timed replays each, median and spread (min .. max) printed.
Algorithmic FLOP = 2 B HW^2 C per product: 1 for a forward, 5 for the backward (3 recomputations of s: D, dyt sweep, dyr sweep; 2 output
products).  Share of peak: 157.3 TF (f32 MFMA).
usage: python tools/bench_clm.py [reps] [rounds] [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from clc_amd import lib, ops

CL = torch.channels_last
PEAK_TF = 157.3
dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else None
SHAPES = [(8, 256, 320), (8, 1024, 320), (4, 1536, 320), (2, 4096, 320)]   # B, HW, C
L = lib.load()
tau = 0.5


def graph_of(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


rows = []
gen = torch.Generator().manual_seed(0)
for B, HW, C in SHAPES:
    a = (3.0 * tau / C ** 0.5) ** 0.5
    yt = (torch.randn(B, HW, C, generator=gen) * a).to(dev)
    yr = (torch.randn(B, HW, C, generator=gen) * a).to(dev)
    g = torch.randn(B, HW, generator=gen).to(dev)
    w_old, w_new, m, l = (torch.empty(B, HW, device=dev) for _ in range(4))
    dyt, dyr = torch.empty_like(yt), torch.empty_like(yr)
    nb_old = L.clc_clm_sim_colsum_workspace_bytes(B, HW)
    ws_old = torch.empty((nb_old + 3) // 4, device=dev)
    nb_bwd = L.clc_clm_sim_colsum_bwd_workspace_bytes(B, HW)
    ws_bwd = torch.empty((nb_bwd + 3) // 4, device=dev)

    def old():
        lib.check(L.clc_clm_sim_colsum(yt.data_ptr(), C, yr.data_ptr(), C, B, HW, C, tau, w_old.data_ptr(), ws_old.data_ptr(), nb_old, ops._stream()))

    def new():
        lib.check(L.clc_clm_sim_colsum_train(yt.data_ptr(), C, yr.data_ptr(), C, B, HW, C, tau, w_new.data_ptr(), m.data_ptr(), l.data_ptr(), ops._stream()))

    def bwd():
        lib.check(L.clc_clm_sim_colsum_bwd(yt.data_ptr(), C, yr.data_ptr(), C, m.data_ptr(), l.data_ptr(), g.data_ptr(), B, HW, C, tau, dyt.data_ptr(), C,
                                           dyr.data_ptr(), C, ws_bwd.data_ptr(), nb_bwd, ops._stream()))

    graphs = {"old_fwd": graph_of(old), "recorded_fwd": graph_of(new), "bwd": graph_of(bwd)}
    t = {k: [] for k in graphs}
    for _ in range(rounds):   # alternate, so a clock or thermal drift hits all three alike
        for k, gr in graphs.items():
            t[k].append(time_us(gr))
    prod = 2.0 * B * HW * HW * C
    row = {"B": B, "HW": HW, "C": C, "gflop_per_product": prod / 1e9}
    for k, nprod in (("old_fwd", 1), ("recorded_fwd", 1), ("bwd", 5)):
        v = sorted(t[k])
        med = v[len(v) // 2]
        tf = nprod * prod / med / 1e6
        row[k] = {"us_median": med, "us_min": v[0], "us_max": v[-1], "tflops": tf, "share_of_peak": tf / PEAK_TF}
    row["bwd_over_recorded_fwd"] = row["bwd"]["us_median"] / row["recorded_fwd"]["us_median"]
    row["recorded_not_slower"] = row["recorded_fwd"]["us_median"] <= row["old_fwd"]["us_median"]
    rows.append(row)
    print(f"({B}, {HW}, {C}) {prod / 1e9:6.2f} GF/product | " + " | ".join(
        f"{k} {row[k]['us_median']:8.1f} us [{row[k]['us_min']:.1f} .. {row[k]['us_max']:.1f}] {row[k]['tflops']:5.1f} TF {100 * row[k]['share_of_peak']:4.1f}%"
        for k in graphs) + f" | bwd / fwd {row['bwd_over_recorded_fwd']:.2f}", flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump({"reps": reps, "rounds": rounds, "peak_tf": PEAK_TF, "shapes": rows}, f, indent=1)
sys.exit(0 if all(r["recorded_not_slower"] for r in rows) else 1)
