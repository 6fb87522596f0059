#!/usr/bin/env python3
"""Headline benchmark of the CLC hot path on MI355X (BASELINE.json: images/sec fwd+bwd @256x256 bs8).

One "step" = one full training step of the reference loop (/root/reference/train_CLC.py:137-183) on one
synthetic batch already resident in HBM: forward (CLC N=64, lambda=0.0067, n_refs=1) + RD loss + backward +
clip_grad_norm_(1.0) + nan_to_num_ + AdamW + aux-loss step, fp32, through the HIP kernels of libclc_hip.so.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
K timed steps after W warm-up steps; `ms_per_step` is the wall time of the K timed steps / K.  --dump-outputs writes what the last
timed step returned, and the parameters it left, as DIR/<name>.npy (dump_outputs(); inputs and weights are seeded, so two builds
run with the same arguments can be compared file for file).
For N > 1 the driver launches it under torch.distributed.run (one rank per GPU, RCCL): every rank draws its
own synthetic shard (weak scaling), gradients are averaged with all-reduce over the flat gradient arena.
Rank 0 prints ONE JSON line.  A plain run does only what the headline needs: set-up, warm-up, the timed steps, --dump-outputs, the line.
--full also runs every other leg after the timed steps (each can still be dropped with its --no-* option) and adds their objects:
  "roofline"      dominant kernel's algorithmic FLOP / measured duration (HIP events on the launch stream) vs the
                  f32-MFMA peak of gfx950 (157.3 TFLOP/s, /opt/skills/guides/MI355X_MICROARCH.md)
  "cpu_baseline"  the CPU oracle (plain PyTorch restatement of the reference graph) timed on the host cores on
                  a bounded sample of the same workload.
  "parity", "codec", "reduced_precision", "reference_loop"   (one GPU): the HIP forward against the oracle on seeded images and the
                  codec's timings; the opt-in bf16-MFMA mode's step rate and gradient error; the reference's literal (eager) loop body
  "config.exposed_comm_ms"   (N > 1 or a forced one-rank group): the exposed gradient-exchange time of 5 extra steps
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32, MI355X_MICROARCH.md "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2516.6  # dense bf16 MFMA, same table (the headline 5 PF figure is 2:1 sparsity)
HBM_PEAK_GBS = 8000.0


def csrc_digest() -> str:
    """sha256[:16] over the kernel sources (clc_amd/csrc/*.{hip,h,cpp}, sorted): tools/pmc_traffic.py stamps the PMC traffic file with it, and
    `roofline.traffic` quotes a committed file only while the kernels it was measured on are the kernels being run."""
    import glob
    import hashlib

    h = hashlib.sha256()
    d = os.path.join(ROOT, "clc_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h")) + glob.glob(os.path.join(d, "*.cpp"))):
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def synthetic_batch(batch, size, seed, device):
    """uint8 noise / 255 (mirrors normalize_to_tensor, /root/reference/dataloader_ref_cluster.py:182-194)."""
    import torch

    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (batch, 3, size, size), generator=g, dtype=torch.uint8).float() / 255.0
    return x.to(device)


DUMP_BUDGET_BYTES = 64 << 20
DUMP_PARAM_SAMPLE = 8 << 20    # parameter elements kept when all of them do not fit the budget (32 MiB of float32)


def dump_outputs(out_dir, out, model):
    """--dump-outputs DIR: what the timed path handed its caller in its LAST timed step, so two builds can be compared output for output.
      <key>.npy     the step's returned device scalars (loss, bpp_loss, mse_loss / ms_ssim_loss, aux_loss), float64, shape ()
      params.npy    the model's parameters after that step's optimizer updates, named_parameters() order, flattened, float32: all of
                    them when they fit the budget, else the elements at a fixed seeded sample of positions (one per equal slice, ascending; seed 0)
    Returns {name: what} for the JSON line."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    files = {}
    for k, v in out.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), np.asarray(float(v.item()), dtype=np.float64))
        files[k] = "float64 scalar returned by the step"
    flat = torch.cat([p.detach().reshape(-1) for _, p in model.named_parameters()]).float()
    n = flat.numel()
    if n * 4 + 4096 <= DUMP_BUDGET_BYTES:
        sample, what = flat, f"all {n} parameter elements after the step, float32"
    else:
        # stratified: one seeded position inside each of k equal slices of the flattened parameters (no repeats, the whole model covered)
        k = DUMP_PARAM_SAMPLE
        lo = torch.arange(k + 1, dtype=torch.int64) * n // k
        u = torch.rand(k, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
        idx = lo[:-1] + (u * (lo[1:] - lo[:-1]).double()).long()
        sample, what = flat[idx.to(flat.device)], f"{DUMP_PARAM_SAMPLE} seeded sample positions of the {n} parameter elements after the step, float32"
    np.save(os.path.join(out_dir, "params.npy"), sample.cpu().numpy().astype(np.float32))
    files["params"] = what
    return files


def _host_threads():
    """threads this process may actually use: the affinity mask (os.cpu_count() over-reports inside a cpuset) capped at the
    16-CPU share a one-GPU box grants — an intra-op pool sized to the reported 128 cores oversubscribes the share and is slower"""
    usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(usable, int(os.environ.get("CLC_CPU_THREADS", "16"))))


def cpu_baseline(n_refs: int, sample_batch: int, size: int, timed_steps: int = 3, N: int = 64, lmbda: float = 0.0067, loss: str = "mse"):
    """the oracle (plain-PyTorch CPU restatement of the reference graph; the reference itself cannot be imported
    where this runs) — forward + RD loss + backward at the GPU run's batch, 1 warm-up + `timed_steps` timed iterations, median.
    The checker is used here as the reported baseline, never as the product."""
    import statistics

    import torch

    from clc_amd.recipe import apply_weight_recipe
    from oracle import graph as og
    from oracle.loss import RateDistortionLoss

    cores = _host_threads()
    torch.set_num_threads(cores)
    m = og.CLC(N=N, num_ref_frames=n_refs).train()
    apply_weight_recipe(m, 0)
    crit = RateDistortionLoss(lmbda, type=loss)
    x = synthetic_batch(sample_batch, size, 100, "cpu")
    refs = [synthetic_batch(sample_batch, size, 101 + i, "cpu") for i in range(n_refs)]

    def one():
        for p in m.parameters():
            p.grad = None
        t0 = time.perf_counter()
        out = crit(m(x, refs), x)
        out["loss"].backward()
        return time.perf_counter() - t0

    one()  # warm-up (first iteration pays allocator / thread-pool start-up)
    ts = [one() for _ in range(timed_steps)]
    dt = statistics.median(ts)
    cpu_model = ""
    try:
        with open("/proc/cpuinfo") as fh:
            cpu_model = next((l.split(":", 1)[1].strip() for l in fh if l.startswith("model name")), "")
    except OSError:
        pass
    return {"value": sample_batch / dt, "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": f"oracle (plain PyTorch CPU restatement of the reference graph) fwd+RD-loss({loss})+bwd at batch {sample_batch} (N={N}, {size}x{size}, "
                      f"n_refs={n_refs}), 1 warm-up + {timed_steps} timed steps, median {dt:.2f} s/step (all: {', '.join(f'{t:.2f}' for t in ts)}); "
                      f"{cores} torch threads of {os.cpu_count()} reported cores, torch {torch.__version__}, fp32; CPU: {cpu_model}"}


def parity_and_codec(dev):
    """BASELINE.md §3 parity columns + codec timing on one seeded 256x256 image (eval mode):
    |d bpp|, |d PSNR| of the HIP forward vs the oracle; y/z streams of the HIP compress() identical across the product's C++ coder,
    the plain-C oracle coder and the pure-Python oracle coder (on the product's symbols); decoder == encoder-side reconstruction;
    compress / decompress wall time per image on the GPU path and on the CPU oracle (CPU transforms + pure-Python rANS)."""
    import math

    import torch

    from clc_amd import models as pm
    from clc_amd.recipe import apply_weight_recipe, synthetic_image
    from oracle import graph as og
    from oracle import rans_c, rans_py
    from oracle.loss import compute_bpp

    torch.set_num_threads(_host_threads())
    o = og.CLC(N=64, num_ref_frames=1).eval()
    apply_weight_recipe(o, 0)
    p = pm.CLC(N=64, num_ref_frames=1)
    p.load_state_dict(o.state_dict())
    p = p.to(dev).eval()
    o.update(force=True)
    p.update(force=True)
    x, r = synthetic_image(1, 256, 256, 100, smooth=True), [synthetic_image(1, 256, 256, 101, smooth=True)]
    xd, rd = x.to(dev), [r[0].to(dev)]
    import clc_amd

    with torch.no_grad():
        a = o(x, r)
        b = p(xd, rd)
        clc_amd.set_precision("bf16")   # the opt-in reduced-precision mode, for the `reduced_precision` object
        try:
            b16 = p(xd, rd)
        finally:
            clc_amd.set_precision("f32")
    to_cpu = lambda d: {"x_hat": d["x_hat"].cpu(), "likelihoods": {k: v.cpu() for k, v in d["likelihoods"].items()}}
    bpp_o = compute_bpp(a)
    bpp_p = compute_bpp(to_cpu(b))
    psnr_of = lambda t, ref: -10 * math.log10(torch.mean((t.double().cpu() - ref.double()) ** 2).item())
    psnr = lambda t: psnr_of(t, x)
    # The parity bars are stated on a SAMPLE of images, not on one: a single latent within float error of a rounding boundary flips
    # on any change of summation order (on either side: the reference has the same property between two devices) and moves that one
    # image's bpp by up to ~1e-3.  Four seeded images; the mean is the number held against the bar, the max is reported beside it.
    per_seed = [{"seed": 100, "dbpp": abs(bpp_o - bpp_p), "dpsnr_db": abs(psnr(a["x_hat"]) - psnr(b["x_hat"]))}]
    with torch.no_grad():
        for sd in (110, 120, 130):
            xs, rs = synthetic_image(1, 256, 256, sd, smooth=True), [synthetic_image(1, 256, 256, sd + 1, smooth=True)]
            ao, bo = o(xs, rs), p(xs.to(dev), [rs[0].to(dev)])
            per_seed.append({"seed": sd, "dbpp": abs(compute_bpp(ao) - compute_bpp(to_cpu(bo))),
                             "dpsnr_db": abs(psnr_of(ao["x_hat"], xs) - psnr_of(bo["x_hat"], xs))})
    # codec: GPU path, reference surface (model.compress / decompress of ONE image: captured segments since round 5) ...
    for _ in range(2):
        enc = p.compress(xd, rd)
        dec = p.decompress(enc["strings"], enc["shape"], rd)
    torch.cuda.synchronize()
    n = 5
    t0 = time.perf_counter()
    for _ in range(n):
        enc = p.compress(xd, rd)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(n):
        dec = p.decompress(enc["strings"], enc["shape"], rd)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    # ... and the same calls launch by launch (what that surface cost before)
    for _ in range(2):
        enc_e = p._compress_eager(xd, rd)
    torch.cuda.synchronize()
    g0 = time.perf_counter()
    for _ in range(3):
        enc_e = p._compress_eager(xd, rd)
    torch.cuda.synchronize()
    g1 = time.perf_counter()
    for _ in range(3):
        dec_e = p._decompress_eager(enc_e["strings"], enc_e["shape"], rd)
    torch.cuda.synchronize()
    g2 = time.perf_counter()
    surface_same = bool(enc_e["strings"] == enc["strings"] and torch.equal(dec_e["x_hat"], dec["x_hat"]))
    # the batched, graph-captured codec service (clc_amd.codec): 8 images per call
    from clc_amd.codec import CodecEngine

    eng = CodecEngine(p, threads=8)
    xb = torch.cat([synthetic_image(1, 256, 256, 300 + i, smooth=True) for i in range(8)]).to(dev)
    rb = [torch.cat([synthetic_image(1, 256, 256, 400 + i, smooth=True) for i in range(8)]).to(dev)]
    for _ in range(2):
        outs = eng.compress(xb, rb)
        eng.decompress(outs, rb)
    torch.cuda.synchronize()
    e0 = time.perf_counter()
    for _ in range(3):
        outs = eng.compress(xb, rb)
    torch.cuda.synchronize()
    e1 = time.perf_counter()
    for _ in range(3):
        eng.decompress(outs, rb)
    torch.cuda.synchronize()
    e2 = time.perf_counter()
    gc = p.gaussian_conditional
    cdf, ln, off = gc.host_tables()
    sc, mu, y = b["para"]["scales"], b["para"]["means"], b["para"]["y"]
    idx = torch.cat([gc.build_indexes(s).contiguous().reshape(-1) for s in sc.chunk(5, 1)]).cpu().numpy()
    sym = torch.cat([torch.round(u - m).int().contiguous().reshape(-1) for u, m in zip(y.chunk(5, 1), mu.chunk(5, 1))]).cpu().numpy()
    ys = enc["strings"][0][0]
    identical = (rans_c.encode(sym, idx, cdf, ln, off) == ys
                 and rans_py.RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), ln.tolist(), off.tolist()) == ys
                 and bool(torch.equal(dec["x_hat"], b["x_hat"].clamp(0, 1))))
    # codec: CPU oracle (one image, one pass each)
    with torch.no_grad():
        c0 = time.perf_counter()
        enc_o = o.compress(x, r)
        c1 = time.perf_counter()
        o.decompress(enc_o["strings"], enc_o["shape"], r)
        c2 = time.perf_counter()
    nsd = len(per_seed)
    parity = {"dbpp": sum(q["dbpp"] for q in per_seed) / nsd, "dpsnr_db": sum(q["dpsnr_db"] for q in per_seed) / nsd,
              "dbpp_max": max(q["dbpp"] for q in per_seed), "dpsnr_db_max": max(q["dpsnr_db"] for q in per_seed), "per_seed": per_seed,
              "bitstream_identical": bool(identical),
              "within_bars": bool(sum(q["dbpp"] for q in per_seed) / nsd <= 1e-4 and max(q["dbpp"] for q in per_seed) <= 1e-3
                                  and sum(q["dpsnr_db"] for q in per_seed) / nsd <= 0.01 and max(q["dpsnr_db"] for q in per_seed) <= 0.02),
              "bpp_oracle": bpp_o, "bpp_hip": bpp_p, "bars": "mean dbpp <= 1e-4 and mean dpsnr <= 0.01 dB over the seeded images, AND no single image over 1e-3 bpp / 0.02 dB (the footprint of one "
              "hyper-latent rounding flip; tests/test_model_gpu.py::test_forward_parity_over_a_sample_of_images asserts both); y/z streams byte-identical across the "
              "C++ / C / Python coders and decoder output == encoder-side reconstruction",
              "sample": f"CLC N=64 n_refs=1, {nsd} seeded smooth 256x256 images (+1 reference each), eval mode, recipe weights; bpp_oracle / bpp_hip: seed 100"}
    codec = {"gpu_compress_ms_per_image": (t1 - t0) / n * 1e3, "gpu_decompress_ms_per_image": (t2 - t1) / n * 1e3,
             "gpu_eager_compress_ms_per_image": (g1 - g0) / 3 * 1e3, "gpu_eager_decompress_ms_per_image": (g2 - g1) / 3 * 1e3,
             "reference_surface_identical_to_eager": surface_same,
             "gpu_engine_compress_ms_per_image": (e1 - e0) / 24 * 1e3, "gpu_engine_decompress_ms_per_image": (e2 - e1) / 24 * 1e3,
             "cpu_compress_ms_per_image": (c1 - c0) * 1e3, "cpu_decompress_ms_per_image": (c2 - c1) * 1e3,
             "y_bytes": len(ys), "z_bytes": len(enc["strings"][1][0]),
             "note": "gpu_*: model.compress()/decompress() (the reference surface, batch 1, 256x256: hipGraph-captured segments of a lazily built "
                     "CodecEngine); gpu_eager_*: the same methods launch by launch (round 4's reference-surface numbers); gpu_engine_*: "
                     "clc_amd.codec.CodecEngine at batch 8, per-image streams coded on 8 host threads, wall time / 8; CPU: oracle transforms + "
                     "pure-Python rANS (the stand-in for CompressAI's coder), one pass; eval_shape: one 512x768 (Kodak, eval_CLC.py:146-160 pads to x128) "
                     "image through both surfaces with the device | rANS split and the forward-only roofline fraction"}
    codec["batch1_256x256"] = codec_shape_leg(p, dev, 256, 256)
    codec["eval_shape"] = codec_shape_leg(p, dev, 512, 768)
    bpp_16 = compute_bpp({"x_hat": b16["x_hat"].cpu(), "likelihoods": {k: v.cpu() for k, v in b16["likelihoods"].items()}})
    reduced = {"dbpp": abs(bpp_o - bpp_16), "dpsnr_db": abs(psnr(a["x_hat"]) - psnr(b16["x_hat"]))}
    return parity, codec, reduced


def codec_shape_leg(p, dev, H, W, R=1, n=5):
    """One image of H x W (already a multiple of 128, as eval_CLC.py:146-160 pads it) through BOTH codec surfaces at batch 1 — the way the
    reference evaluates (eval_CLC.py:314-338): model.compress() / decompress() (which ride on the captured segments of a CodecEngine) and the
    eager launch-by-launch methods; wall ms per image, the split device segments (+ their D2H / H2D hops) | host rANS, and the forward-only
    roofline fraction of the device part: algorithmic FLOPs of the launches of one pass (recorded through the C ABI) / graph-replay time."""
    import torch

    from clc_amd import ops
    from clc_amd.recipe import synthetic_image

    x = synthetic_image(1, H, W, 700, smooth=True).to(dev)
    refs = [synthetic_image(1, H, W, 701 + j, smooth=True).to(dev) for j in range(R)]
    out = {"shape": f"{H}x{W}", "batch": 1, "n_refs": R}

    def wall(fn, reps):
        fn()
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, r

    out["compress_ms"], enc = wall(lambda: p.compress(x, refs), n)
    eng = p.__dict__.get("_codec_eng")
    out["compress_split"] = {k: round(v, 3) for k, v in eng.last.items() if k != "op"} if eng is not None else None
    out["decompress_ms"], dec = wall(lambda: p.decompress(enc["strings"], enc["shape"], refs), n)
    out["decompress_split"] = {k: round(v, 3) for k, v in eng.last.items() if k != "op"} if eng is not None else None
    out["eager_compress_ms"], enc_e = wall(lambda: p._compress_eager(x, refs), 3)
    out["eager_decompress_ms"], dec_e = wall(lambda: p._decompress_eager(enc["strings"], enc["shape"], refs), 3)
    out["streams_identical_to_eager"] = bool(enc["strings"] == enc_e["strings"] and torch.equal(dec["x_hat"], dec_e["x_hat"]))
    out["y_bytes"], out["z_bytes"] = len(enc["strings"][0][0]), len(enc["strings"][1][0])
    out["bpp"] = 8.0 * (out["y_bytes"] + out["z_bytes"]) / (H * W)
    if eng is not None:
        # device part alone: the encoder graph / the six decoder graphs replayed back to back (no host hop in between), HIP events
        pe = list(eng._enc.values())[-1]      # (the plans of THIS shape: the newest of the engine's signatures)
        pd = list(eng._dec.values())[-1]

        def flops_of(fns):
            ops.PROFILE = []
            try:
                for f in fns:
                    f()
                torch.cuda.synchronize()
                return sum(r.flops for r in ops.PROFILE), len(ops.PROFILE)
            finally:
                ops.PROFILE = None

        def replay_ms(graphs, reps=10):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for g in graphs:
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            return sorted(ts)[len(ts) // 2]

        for name, fns, graphs in (("encoder", [pe.run], [pe.graph]), ("decoder", [f for _, f, _ in pd.segs], [g for g, _, _ in pd.segs])):
            if any(g is None for g in graphs):
                continue
            fl, nl = flops_of(fns)
            ms = replay_ms(graphs)
            out[name + "_device"] = {"gflop": round(fl / 1e9, 2), "graph_ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 2),
                                     "frac_of_f32_mfma_peak": round(fl / ms / 1e9 / F32_MFMA_PEAK_TFLOPS, 4), "c_abi_launches": nl}
    return out


def _kernel_name(L, r):
    """the name rocprofv3 --kernel-trace reports for a recorded conv / filter-gradient launch (template arguments from the C ABI's
    variant id); launches recorded through the proxy keep the name of their C entry point"""
    fam, variant, shape = r.fam, r.variant, str(r.label)
    splitk_pf = L.clc_set_tuning(6, 1)
    L.clc_set_tuning(6, splitk_pf)
    wgrad_dma = L.clc_set_tuning(9, 1)
    L.clc_set_tuning(9, wgrad_dma)
    if fam == "conv_wgrad_group":   # one kernel family of a grouped stream-K filter-gradient call (+ its fix-up launch)
        dma = "true" if shape.endswith("dma=1") and wgrad_dma else "false"   # <..., true>: LDS-DMA-staged instantiation
        if variant == 1:
            return "wgrad_small_kernel"
        # last argument (LDS-DMA-staged problems only): 0 = v_mfma_f32_32x32x2_f32, 1 = the reduced-precision mode's bf16 MFMA (tuning key 14), 2 = f32 products
        # from three-way bf16 splits on the bf16 matrix cores (tuning key 24: bit 0 the all-taps kernels, bit 1 the tiled ones)
        taps = variant in (64908, 64916, 64932)
        bf = 0
        if dma == "true":
            bf = 1 if L.clc_get_tuning(14) and "dma=1" in shape else (2 if (L.clc_get_tuning(24) & (1 if taps else 2)) and (taps or variant != 64064) else 0)   # (64 x 64 tiles keep the f32 MFMAs)
        if taps:
            return f"conv_wgrad_taps_sk_kernel<{variant - 64900}, {dma}, {bf}>"
        return f"conv_wgrad_sk_kernel<{variant // 1000}, {variant % 1000}, 2, 2, {dma}, {bf}>"
    if fam != "conv_igemm" or variant < (1 << 20):
        return fam   # conv_direct_small / single (non-deferred) wgrad calls / proxied entry points
    tr = "true" if shape.startswith("dgrad") else "false"
    f, bm, bn = (variant >> 20) & 15, (variant >> 3) & 0x1FF, (variant & 7) << 5
    if f == 3:   # <BN, TR, KW, PF>: 4-wave tiles keep one K-tile in flight, 8-wave ones CLC_TUNE_SPLITK_PF (key 6)
        kw = (variant >> 16) & 15
        ops_arith = "true" if ("+actbwd" in shape or "+sq" in shape) else "false"   # (<..., OPS>: operand arithmetic — a fused activation derivative or GDN's squared input: launch_splitk_o's rule)
        return f"conv_igemm_splitk_kernel<{bn}, {tr}, {kw}, {1 if kw == 4 or splitk_pf == 1 else 3}, {ops_arith}>"
    if f in (4, 5):   # family 5 = the 1x1 instantiation (its own symbol)
        return (f"conv_igemm_dma2_kernel<{bm}, {bn}, {(variant >> 16) & 15}, {(variant >> 12) & 15}, {tr}, {1 if f == 5 else 3}, "
                f"{(variant >> 24) & 3}, {'true' if (variant >> 26) & 1 else 'false'}>")   # (..., OP: 1 = squared operand (GDN's norm convolution), BF: bf16 MFMA)
    if f == 13:       # Winograd F(2x2, 3x3) kernel (csrc/conv_wino.hip): <SHUF>
        return f"conv_wino{'64' if (variant >> 12) & 1 else ''}_kernel<{'true' if variant & 1 else 'false'}>"   # (bit 12: the 64-wide instantiation)
    if f == 12:       # halo-resident 3x3 kernel (csrc/conv_halo.hip): <CI, TR, SHUF>
        return f"conv_halo3x3_kernel<{64 * ((variant >> 4) & 15)}, {'true' if (variant >> 1) & 1 else 'false'}, {'true' if variant & 1 else 'false'}>"
    if f == 11:       # the wave-private persistent kernel of the 128 -> 128 / 64 -> 64 1x1 layers on large maps (csrc/fused_mlp.hip)
        return f"lin_kernel<{(variant >> 16) & 15}, {(variant >> 8) & 15}, {variant & 15}>"
    if f == 10:       # 16-column MFMAs for the <= 16-channel tail of the synthesis transform
        return "conv_igemm_n16_kernel<3>"
    if f == 8:        # the persistent pipelined kernel of the large-map 1x1 layers
        return f"conv_igemm_p1x1_kernel<{(variant >> 24) & 3}>"
    return f"conv_igemm{ {1: '', 2: '_dma'}[f]}_kernel<{bm}, {bn}, {(variant >> 16) & 15}, {(variant >> 12) & 15}, {tr}>"


def _replay_ms(fn, reps=20, warm=2):
    """median wall time (ms, HIP events) of `fn` captured ONCE into a hipGraph and replayed `reps` times — how the timed region runs"""
    import statistics

    import torch

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    from clc_amd import ops as _ops

    with _ops.capture_guard(), torch.cuda.graph(g, capture_error_mode=_ops.graph_capture_mode()):
        fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), g


def transforms_leg(model, x, refs, engine=None):
    """The number north_star's target is stated on: the analysis / synthesis transforms (and the reference encoder) on their own —
    forward + data gradients + filter gradients of g_a, g_s, ref_encoder(+adapter) at the bench batch, EVERY kernel they launch
    (convolutions, GDN, LayerNorm, window attention, elementwise, grouped stream-K filter gradients and their fix-ups), each captured
    into a hipGraph and replayed 20x (median).  FLOPs = the algorithmic 2*MAC of the convolutions / linears / attention products
    launched in that pass (forward + data gradient + filter gradient), counted by clc_amd.ops' launch records."""
    import torch

    from clc_amd import ops

    CL = torch.channels_last
    with torch.no_grad():
        y = model.g_a(model._prep(x))
    g = torch.Generator(device=x.device).manual_seed(5)
    y_hat = torch.randn(y.shape, generator=g, device=x.device).contiguous(memory_format=CL).requires_grad_(True)
    xin = model._prep(x)
    cases = {"g_a": (lambda: model.g_a(xin)), "g_s": (lambda: model.g_s(y_hat)),
             "ref_encoder+adapter": (lambda: model._ref(refs))}
    if refs is None:
        cases.pop("ref_encoder+adapter")
    out = {}
    tot_f = tot_t = 0.0
    # In the training step the transposed filter images and the re-parametrised GDN tensors of ALL layers come from two batched launches at
    # the top of the step (0.14 ms, outside the sub-networks); the legs use those images too instead of one small launch per layer.
    cached = engine is not None and getattr(engine, "transposer", None) is not None
    if cached:
        engine.transposer.refresh()
        if getattr(engine, "halo_packer", None) is not None:
            engine.halo_packer.refresh()
        if getattr(engine, "wino_packer", None) is not None:
            engine.wino_packer.refresh()
        engine.gdn_cache.refresh()
    for name, fwd in cases.items():
        with torch.no_grad():
            shape = fwd().shape
        gout = torch.randn(shape, generator=g, device=x.device).contiguous(memory_format=CL)

        def step():
            y_hat.grad = None
            ops.WT_CACHE_VALID = cached    # (the engine's per-step images of the filters / GDN parameters, refreshed above: as in the step)
            try:
                o = fwd()
                torch.autograd.backward([o], [gout])
            finally:
                ops.WT_CACHE_VALID = False
            ops.join_side_streams()

        ops.PROFILE = []
        try:
            step()
            torch.cuda.synchronize()
            flops = sum(r.flops for r in ops.PROFILE)
            launches = len(ops.PROFILE)
        finally:
            ops.PROFILE = None
        ms, graph = _replay_ms(step)
        del graph
        out[name] = {"gflop": round(flops / 1e9, 1), "ms": round(ms, 3), "tflops": round(flops / ms / 1e9, 2), "c_abi_launches": launches}
        tot_f += flops
        tot_t += ms
    out["total"] = {"gflop": round(tot_f / 1e9, 1), "ms": round(tot_t, 3), "tflops": round(tot_f / tot_t / 1e9, 2),
                    "frac_of_f32_mfma_peak": round(tot_f / tot_t / 1e9 / F32_MFMA_PEAK_TFLOPS, 4), "target_frac": 0.5}
    out["method"] = ("each sub-network alone: forward + backward (data and filter gradients, all kernels incl. attention / LayerNorm / GDN / "
                     "elementwise / stream-K fix-ups) captured into one hipGraph, median of 20 replays; FLOPs = algorithmic 2*MAC x (fwd + dgrad + wgrad); "
                     "the transposed filter images / re-parametrised GDN tensors are the engine's per-step batched ones, as in the step")
    return out


def _tuning(key):
    from clc_amd import lib as _clib
    return int(_clib.load().clc_get_tuning(key))


def roofline_leg(engine, x, refs):
    """One eager (non-graph) step with every launch through the C ABI bracketed by HIP events on its launch stream (per-kernel table,
    dominant kernel, in-step attribution to the sub-networks); then the dominant kernel's launches re-issued inside a hipGraph and
    replayed — the way the timed region runs them — for `roofline.achieved`."""
    import torch

    from clc_amd import lib as _clib
    from clc_amd import ops

    torch.cuda.synchronize()
    # what an EMPTY event bracket reads on this stream (two back-to-back records): subtracted from every launch below, so the
    # ~5-15 us kernels of the slice loop are not charged the timestamp packets' own latency
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(200)]
    for a, b in pairs:
        a.record(); b.record()
    torch.cuda.synchronize()
    empty = sorted(a.elapsed_time(b) for a, b in pairs)[len(pairs) // 2] * 1e-3
    ops.PROFILE = []
    try:
        # The launches are ENQUEUED behind a ~0.15 s spin kernel, so the host (50-100 us of Python per launch) is out of the picture
        # by the time they run: the GPU executes them back to back, like the hipGraph replay of the timed region, instead of
        # idling (and down-clocking) between host-paced launches.
        torch.cuda._sleep(int(0.15 * 2.4e9))
        engine._eager_step(x, refs)
        torch.cuda.synchronize()
        rec = ops.PROFILE
    finally:
        ops.PROFILE = None
    _L = _clib.load()
    agg, by_owner = {}, {}
    for r in rec:
        key = _kernel_name(_L, r)
        t = max(r.ms() * 1e-3 - empty, 1e-7)
        a = agg.setdefault(key, [0.0, 0.0, 0, 0.0, []])
        a[0] += r.flops
        a[1] += t
        a[2] += 1
        a[3] += r.nbytes or 0.0
        a[4].append(r)
        # in-step attribution: a grouped filter-gradient launch is split over the owners of its problems by FLOP share
        shares = r.owner_flops if r.owner_flops else {r.owner: max(r.flops, 1.0)}
        tot = sum(shares.values())
        for ow, fl in shares.items():
            o = by_owner.setdefault(ow, [0.0, 0.0, 0])
            o[0] += (fl if r.owner_flops or r.flops else 0.0)
            o[1] += t * fl / tot
            o[2] += 1
    mfma = {k: v for k, v in agg.items() if v[0] > 0}
    total_t = sum(a[1] for a in mfma.values())
    total_f = sum(a[0] for a in mfma.values())
    # the dominant KERNEL by summed time; a stream-K filter-gradient family competes with its algorithmic FLOPs over the time of its
    # main kernel + fix-up launch (the bracket cannot separate them; the fix-up is ~1-3 % of it)
    single = {k: v for k, v in agg.items() if "_kernel<" in k}
    dom = max((single or agg).items(), key=lambda kv: kv[1][1])
    name, (f, t_eager, n, nb, recs) = dom
    # ... timed the way the timed region runs it: its launches of this step re-issued in order inside ONE hipGraph, replayed 20x
    relaunch = [r.relaunch for r in recs if r.relaunch is not None]
    t_replay = None
    if len(relaunch) == n:
        def again():
            for fn in relaunch:
                fn()
        ms, graph = _replay_ms(again)
        del graph
        t_replay = ms * 1e-3
    t = t_replay if t_replay is not None else t_eager
    # the 1x1 / linear instantiation (..., 1>) moves ~50 FLOP per byte on 128-channel layers — under the f32 ridge once the residual and
    # saved-activation streams are counted — so its roofline is HBM; everything else is MFMA
    hbm_bound = ((name.startswith("conv_igemm_dma2_kernel") and (", 1, 0, " in name or ", 1, 1, " in name)) or name.startswith("conv_igemm_p1x1_kernel")) and nb > 0
    achieved = (nb / t / 1e9) if hbm_bound else (f / t / 1e12)
    peak = HBM_PEAK_GBS if hbm_bound else F32_MFMA_PEAK_TFLOPS
    # HBM-side bytes per launch of that kernel from the committed PMC passes (separate `rocprofv3 --pmc FETCH_SIZE` /
    # `--pmc WRITE_SIZE` runs of this same command, gfx950 FETCH_SIZE correction applied: tools/pmc_traffic.py); null when the
    # file does not list the kernel
    traffic, traffic_source = None, None
    import glob

    digest = csrc_digest()
    for cand in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):
        try:
            with open(cand) as fh:
                doc = json.load(fh)
            if doc.get("csrc_sha16") != digest:
                traffic_source = (f"null: the newest PMC traffic file ({os.path.basename(cand)}) was measured on other kernel sources "
                                  f"(csrc_sha16 {doc.get('csrc_sha16')} != {digest}); re-run tools/gpu_profiles.sh")
                break
            k = doc["kernels"].get(name)
            if k and k["launches_per_step"]:
                traffic = round((k["fetch_bytes_per_step"] + k["write_bytes_per_step"]) / k["launches_per_step"])
                traffic_source = (f"profiles/{os.path.basename(cand)} (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command on these "
                                  f"kernel sources, csrc_sha16 {digest}; a --pmc pass cannot run inside this process)")
            else:
                traffic_source = f"null: profiles/{os.path.basename(cand)} does not list {name}"
            break
        except (OSError, KeyError, ValueError):
            continue
    table = {k: {"launches": v[2], "gflop": round(v[0] / 1e9, 2), "ms": round(v[1] * 1e3, 3),
                 **({"tflops": round(v[0] / v[1] / 1e12, 2)} if v[0] else {}),
                 **({"algorithmic_gb_per_s": round(v[3] / v[1] / 1e9, 1)} if v[3] else {})} for k, v in agg.items()}
    owners = {ow: {"launches": v[2], "gflop": round(v[0] / 1e9, 1), "ms": round(v[1] * 1e3, 3), "tflops": round(v[0] / v[1] / 1e12, 2)}
              for ow, v in by_owner.items()}
    tr = [v for ow, v in by_owner.items() if ow in ("g_a", "g_s", "ref_encoder")]
    if tr:
        ff, tt = sum(v[0] for v in tr), sum(v[1] for v in tr)
        owners["transforms"] = {"gflop": round(ff / 1e9, 1), "ms": round(tt * 1e3, 3), "tflops": round(ff / tt / 1e12, 2),
                                "frac_of_f32_mfma_peak": round(ff / tt / 1e12 / F32_MFMA_PEAK_TFLOPS, 4)}
    path = {}
    if not hbm_bound and name.startswith("conv_wgrad") and name.rstrip(">").endswith(", 2"):
        # f32 products from three-way bf16 splits: six v_mfma_f32_32x32x16_bf16 per algorithmic f32 multiply-add block (csrc/conv_wgrad.hip split3).  `peak`
        # stays the dense MFMA peak of the arithmetic type (f32), as the contract says; this is the ceiling of the instructions actually issued.
        path = {"instruction_path": "6 x v_mfma_f32_32x32x16_bf16 per 16 k (f32 operands split into three bf16 pieces in registers, f32 accumulate; error "
                                    "against fp64 equal to the f32-MFMA kernel's: tools/check_split_wgrad.py, tests/test_kernels_gpu.py::test_split_wgrad_*)",
                "instruction_path_peak": round(BF16_MFMA_PEAK_TFLOPS / 6, 1), "instruction_path_frac": round(achieved / (BF16_MFMA_PEAK_TFLOPS / 6), 4)}
    if not hbm_bound and name.startswith("conv_wino"):
        # Winograd F(2x2, 3x3): `achieved` counts the direct convolution's FLOPs (the algorithmic figure the contract asks for), of which the kernel issues 16 / 36
        path = {"instruction_path": "Winograd F(2x2, 3x3) on v_mfma_f32_32x32x2_f32: 16 of the direct convolution's 36 multiplications per 2x2 output tile "
                                    "(csrc/conv_wino.hip); achieved x 16 / 36 is the rate of the MFMAs actually issued",
                "instruction_path_peak": F32_MFMA_PEAK_TFLOPS, "instruction_path_frac": round(achieved * 16 / 36 / F32_MFMA_PEAK_TFLOPS, 4)}
    return {"bound": "hbm" if hbm_bound else "mfma", "kernel": name, "achieved": round(achieved, 2), "peak": peak, "unit": "GB/s" if hbm_bound else "TFLOP/s",
            "frac": round(achieved / peak, 4), **path, "traffic": traffic, "traffic_source": traffic_source,
            "launches_per_step": n, "avg_launch_ms": round(t / n * 1e3, 4),
            "avg_launch_ms_eager_bracketed": round(t_eager / n * 1e3, 4), "event_bracket_overhead_ms": round(empty * 1e3, 5),
            "timing_note": ("achieved / avg_launch_ms: this kernel's launches of one step (stream-K family: main grid + fix-up) re-issued in order inside "
                            "one hipGraph, median of 20 replays — comparable with rocprofv3's graph-replay averages in profiles/.  per_kernel / "
                            "in_step_by_owner: one eager step with every C-ABI launch bracketed by HIP events (they cannot be recorded inside a "
                            "hipGraph on ROCm 7.2), enqueued behind a spin kernel; brackets read 5-15 % long on a loaded box"),
            "all_mfma_kernels": {"tflops": round(total_f / total_t / 1e12, 2), "ms_per_step": round(total_t * 1e3, 2), "gflop_per_step": round(total_f / 1e9, 1)},
            "in_step_by_owner": owners,
            "per_kernel": table}


def reduced_precision_leg(args, dev, x, refs):
    """the opt-in bf16-in / f32-accumulate MFMA mode (clc_amd.set_precision("bf16"): the 3x3 convolutions, data and
    filter gradients of the analysis / synthesis transforms and the reference encoder; everything on the 16x16 latents, the
    likelihoods, the codec and the optimizer stay f32).  NEVER the headline `value` (narrower arithmetic than the reference's fp32):
    the same training step timed in that mode, and its gradient error against the f32 mode on one batch."""
    import torch

    import clc_amd
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe
    from clc_amd.train import TrainEngine

    model = models.CLC(N=args.N, num_ref_frames=args.n_refs)
    apply_weight_recipe(model, 0)
    model = model.to(dev).train()
    eng = TrainEngine(model, lmbda=args.lmbda, loss_type=args.loss, lr=1e-4, aux_lr=1e-3, clip_max_norm=1.0, use_graph=not args.no_graph, precision="bf16")
    for _ in range(max(1, args.warmup)):
        out = eng.step(x, refs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = eng.step(x, refs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"value": args.batch * args.steps / dt, "unit": "images/sec", "ms_per_step": dt / args.steps * 1e3, "dtype": "bf16 operands, f32 accumulate (MFMA "
           "v_mfma_f32_32x32x16_bf16) in the large-map 3x3 conv / dgrad / wgrad kernels; f32 everywhere else", "final_loss": float(out["loss"].item())}
    del eng, model
    # gradient error of the mode: one eval-mode (deterministic rounding) step at batch 2, bf16 vs f32, same weights and inputs
    xb, rb = x[:2], ([r[:2] for r in refs] if refs is not None else None)
    grads = {}
    for mode in ("f32", "bf16"):
        m = models.CLC(N=args.N, num_ref_frames=args.n_refs)
        apply_weight_recipe(m, 0)
        m = m.to(dev)
        e = TrainEngine(m, lmbda=args.lmbda, loss_type=args.loss, use_graph=False, train_mode=False)
        clc_amd.set_precision(mode)
        try:
            e._discover(xb, rb)
            e._fwd_bwd(xb, rb)
        finally:
            clc_amd.set_precision("f32")
        torch.cuda.synchronize()
        grads[mode] = {n: q.grad.clone() for n, q in m.named_parameters() if q.grad is not None}
        del e, m
    errs = sorted(((grads["bf16"][n] - g).abs().max().item() / g.abs().max().item()) for n, g in grads["f32"].items() if g.abs().max().item() > 1e-12)
    res["grad_rel_err"] = {"max": errs[-1], "median": errs[len(errs) // 2], "p99": errs[int(len(errs) * 0.99)],
                           "definition": "per parameter tensor: max |g_bf16 - g_f32| / max |g_f32|, one eval-mode step at batch 2"}
    return res


def reference_loop_leg(args, dev, x, refs, steps: int = 5, warm: int = 2):
    """The LITERAL loop body of /root/reference/train_CLC.py:137-183 on clc_amd.models.CLC, eager (no TrainEngine, no hipGraph, no fused
    optimizer, no arenas): optimizer.zero_grad / aux_optimizer.zero_grad, model(sample, ref_samples), criterion, loss.backward(),
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0), the per-parameter `p.grad.nan_to_num_()` loop, optimizer.step(),
    model.aux_loss().backward(), aux_optimizer.step() — with the reference's own optimizer pair (configure_optimizers, train_CLC.py:81-117:
    two torch.optim.AdamW).  What `train_CLC.py` gets when it runs unmodified over this package.  Reported beside `value`, never as it.
    The split comes from a second pass with a device synchronisation after each phase (so its parts sum to more than the free-running step)."""
    import types

    import torch

    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe
    from clc_amd.train import RateDistortionLoss, configure_optimizers

    torch.manual_seed(0)
    model = models.CLC(N=args.N, num_ref_frames=args.n_refs)
    apply_weight_recipe(model, 0)
    model = model.to(dev).train()
    criterion = RateDistortionLoss(lmbda=args.lmbda, type=args.loss)
    optimizer, aux_optimizer = configure_optimizers(model, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3))
    clip_max_norm = 1.0
    marks = []

    def body(sync_phases=False):
        def mark(name):
            if sync_phases:
                torch.cuda.synchronize()
                marks.append((name, time.perf_counter()))
        mark("start")
        optimizer.zero_grad()
        aux_optimizer.zero_grad()
        out_net = model(x, refs)
        out_criterion = criterion(out_net, x)
        mark("forward + criterion")
        out_criterion["loss"].backward()
        mark("backward")
        if clip_max_norm > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip_max_norm)
        for p in model.parameters():
            if p.grad is not None:
                p.grad.nan_to_num_()
        mark("clip_grad_norm_ + nan_to_num_ loop")
        optimizer.step()
        mark("optimizer.step (torch.optim.AdamW)")
        aux_loss = model.aux_loss()
        aux_loss.backward()
        aux_optimizer.step()
        mark("aux loss + aux optimizer")
        return out_criterion

    for _ in range(warm):
        out = body()
    torch.cuda.synchronize()
    # host-bound timing on a shared box jitters by tens of per cent: three blocks of `steps` free-running steps, the MEDIAN block is the number
    blocks = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            out = body()
        hi = (time.perf_counter() - t0) / steps     # the host has returned from the last launch; the GPU may still be busy
        torch.cuda.synchronize()
        blocks.append(((time.perf_counter() - t0) / steps, hi))
    dt, host_issue = sorted(blocks)[1]
    split = {}
    for _ in range(2):
        marks.clear()
        body(sync_phases=True)
    for (_, ta), (name, tb) in zip(marks[:-1], marks[1:]):
        split[name] = round((tb - ta) * 1e3, 2)
    n_params = sum(1 for p in model.parameters() if p.grad is not None)
    res = {"value": args.batch / dt, "unit": "images/sec", "ms_per_step": round(dt * 1e3, 2), "host_issue_ms_per_step": round(host_issue * 1e3, 2),
           "steps": steps, "warmup": warm, "blocks_ms": [round(b[0] * 1e3, 2) for b in blocks], "final_loss": float(out["loss"].item()), "parameters_with_grad": n_params,
           "phase_ms_with_a_sync_after_each": split,
           "what": ("literal body of train_CLC.py:137-183 on clc_amd.models.CLC, eager: two torch.optim.AdamW from configure_optimizers "
                    "(train_CLC.py:81-117), clip_grad_norm_, per-parameter nan_to_num_ loop, aux_loss.backward(); no TrainEngine / hipGraph / arenas")}
    del optimizer, aux_optimizer, model
    torch.cuda.empty_cache()
    return res


def launcher_command(n_gpus: int, port, argv):
    """The command line of /root/reference/run_ddp.sh:7 (`python -m torch.distributed.run --nproc_per_node=8 train_CLC.py ...`) for this
    script: one rank per GPU on one node, rendezvous on the loopback address (the container hostname may not resolve).
    port = None: the c10d rendezvous binds port 0 itself (no window between probing a free port and using it)."""
    rdzv = (["--rdzv-backend=c10d", "--rdzv-endpoint=127.0.0.1:0", "--local-addr", "127.0.0.1"] if port is None
            else ["--master-addr", "127.0.0.1", "--master-port", str(port)])
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", *rdzv, os.path.abspath(__file__), *argv]


def self_launch(n_gpus: int, argv) -> int:
    """`python bench.py --gpus N` (N > 1) outside torchrun: start the N ranks as a FRESH child process tree and hand its exit code back.
    This process has not touched the GPU and never will (no exec of a GPU-initialised process, no retry); the ranks inherit stdout /
    stderr, so rank 0's JSON line is this command's JSON line."""
    import subprocess

    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    port = int(os.environ["CLC_BENCH_MASTER_PORT"]) if os.environ.get("CLC_BENCH_MASTER_PORT") else None
    cmd = launcher_command(n_gpus, port, argv)
    print(f"[bench.py] --gpus {n_gpus} without WORLD_SIZE: launching the ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--n-refs", type=int, default=1)
    ap.add_argument("--lmbda", type=float, default=0.0067)
    ap.add_argument("--loss", choices=("mse", "ms_ssim"), default="mse", help="distortion term (train_CLC.py:52-57); configs[4] uses ms_ssim")
    ap.add_argument("--N", type=int, default=64, help="transform width: 64 (eval_CLC.py:264, the headline) or 128 (train_CLC.py:356 default)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run every other leg: roofline (+ transforms), parity + codec, "
                    "reduced precision, reference loop, CPU baseline and (multi-rank) exposed communication; the --no-* options drop single legs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-sample-batch", type=int, default=0, help="CPU-baseline batch (default: the GPU batch, BASELINE.md §3)")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-reduced", action="store_true", help="skip the reduced-precision (bf16 MFMA) leg")
    ap.add_argument("--no-reference-loop", action="store_true", help="skip the leg that times the reference's literal (eager) training loop body")
    ap.add_argument("--launch-selftest", action="store_true", help="ranks only rendezvous (gloo, CPU), all-reduce a counter and exit: checks the "
                    "self-launcher / torchrun wiring of --gpus N on a box without N GPUs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step returned and the "
                    "parameters it left (a seeded sample when large) as DIR/<name>.npy, at most 64 MB in all")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (the number of timed steps)")

    # Launched bare with --gpus N > 1 (no torchrun environment): become the launcher, BEFORE anything imports torch or touches the GPU.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))

    import torch
    import torch.distributed as dist

    if os.environ.get("CLC_BENCH_WATCHDOG"):   # debugging aid: dump every thread's Python stack after N seconds (a hung collective / capture)
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["CLC_BENCH_WATCHDOG"]), repeat=True, file=sys.stderr)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.launch_selftest:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world > 1:
            dist.init_process_group("gloo")
        t = torch.ones(1)
        if world > 1:
            dist.all_reduce(t)
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"launch_selftest": True, "n_gpus": args.gpus, "ranks_seen": int(t.item())}), flush=True)
        return
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch as `python bench.py --gpus N` (self-launching) or as "
                         "`python -m torch.distributed.run --nnodes=1 --nproc-per-node N bench.py --gpus N`")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: there is no CPU fallback for the product path")
    # Rehearsal knobs (one-GPU box): CLC_SINGLE_DEVICE=1 puts every rank on cuda:0 and CLC_DIST_BACKEND=gloo exchanges the gradients
    # through gloo — RCCL refuses two ranks on one device — so the multi-rank step structure (graphs A1 | exchange | A2 | exchange | B)
    # can be exercised with real kernels.  The driver's runs use neither: one rank per GPU over RCCL.
    if os.environ.get("CLC_SINGLE_DEVICE", "0") == "1":
        local_rank = 0
    backend = os.environ.get("CLC_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # CLC_FORCE_COLLECTIVES=1 at N = 1: a ONE-rank process group, every all-reduce of the multi-GPU step really issued — the way to make
    # RCCL execute this code (communicator, bucket views of the arena, stream order around the three graph replays) on a one-GPU box
    force_coll = os.environ.get("CLC_FORCE_COLLECTIVES", "0") == "1"
    use_dist = world > 1 or force_coll
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            import socket
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(s.getsockname()[1]))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from clc_amd import models
    from clc_amd.train import TrainEngine, broadcast_parameters
    from clc_amd.recipe import apply_weight_recipe  # by-name seeded weights: the cpu_baseline leg gives the oracle the same ones

    torch.manual_seed(0)
    model = models.CLC(N=args.N, num_ref_frames=args.n_refs)
    apply_weight_recipe(model, 0)
    model = model.to(dev).train()
    broadcast_parameters(model)
    x = synthetic_batch(args.batch, args.size, 100 + rank, dev)
    refs = [synthetic_batch(args.batch, args.size, 1000 + 10 * rank + i, dev) for i in range(args.n_refs)]

    engine = TrainEngine(model, lmbda=args.lmbda, loss_type=args.loss, lr=1e-4, aux_lr=1e-3, clip_max_norm=1.0, use_graph=not args.no_graph,
                         train_mode=os.environ.get("CLC_BENCH_EVAL_ROUNDING", "0") != "1")
    trace = [] if os.environ.get("CLC_BENCH_LOSS_TRACE", "0") == "1" else None   # (tests: the loss of every step, read after the timed region)
    for _ in range(max(1, args.warmup)):
        out = engine.step(x, refs)
        if trace is not None:
            trace.append(out["loss"].clone())
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = engine.step(x, refs)
        if trace is not None:
            trace.append(out["loss"].clone())
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    loss = float(out["loss"].item())
    # (before anything below runs another step: the roofline leg's eager step and exposed_comm_ms() update the parameters again)
    dumped = dump_outputs(args.dump_outputs, out, model) if (args.dump_outputs and rank == 0) else None
    exposed_comm = engine.exposed_comm_ms(x, refs) if (args.full and use_dist and not args.no_graph) else None

    result = {
        "metric": "images/sec fwd+bwd @256x256 bs8; bpp+PSNR parity vs ref",
        "value": world * args.batch * args.steps / dt,
        "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"CLC N={args.N} lambda={args.lmbda} {'MSE' if args.loss == 'mse' else 'MS-SSIM'}, {args.size}x{args.size} bs{args.batch}/GPU, "
                               f"n_refs={args.n_refs}: fwd + RD loss + bwd + clip_grad_norm + AdamW + aux step" +
                               (" (configs[1])" if (args.N, args.loss, args.size, args.batch, args.n_refs) == (64, "mse", 256, 8, 1) else ""),
                   "global_batch": world * args.batch, "parallelism": f"dp{world}", "ranks_seen": (dist.get_world_size() if use_dist else 1),
                   "collective": ((("RCCL" if backend == "nccl" else backend) + " all-reduce of the flat fp32 gradient arena (64 MiB buckets) in two phases: everything "
                                   "downstream of the encoders goes on the wire while the analysis-transform / reference-encoder backward runs")
                                  if use_dist else "none"), "hip_graph": not args.no_graph, "final_loss": loss,
                   # what the f32 arithmetic of the TRAINING launches runs on (inference, parity and codec launches: direct f32-MFMA kernels only)
                   "training_kernels": {"winograd_f2x2_3x3 (tuning key 23)": _tuning(23), "wgrad_f32_products_from_bf16_splits (tuning key 24)": _tuning(24),
                                        "note": "f32 operands and f32 accumulation throughout; key 23: 16/36 of the multiplications in the 3x3 / stride-1 layers of the "
                                                "transforms; key 24: filter-gradient products formed from three bf16 pieces per operand on the bf16 matrix cores "
                                                "(six MFMAs per 16 k), error against fp64 equal to the f32-MFMA kernels'"}},
    }
    if use_dist:
        # exposed_comm_ms: HIP events around the wait for the exchange (after graph A2), mean of 5 extra steps behind the timed region
        result["config"].update({"exposed_comm_ms": exposed_comm, "collectives_issued": engine.sync.launched + engine.aux_sync.launched,
                                 "buckets_per_step": len(engine.sync.buckets) + len(engine.aux_sync.buckets), "dist_backend": engine.sync.backend,
                                 "graphs_per_step": (len(engine.graph) if isinstance(engine.graph, tuple) else 1),
                                 "forced_one_rank_group": bool(force_coll and world == 1)})
    if dumped is not None:
        result["dump_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "files": dumped}
    if trace is not None:
        result["config"]["loss_trace"] = [float(t.item()) for t in trace]
    # everything below the headline is --full only: a plain run prints its line now
    if args.full and not args.no_roofline:  # every rank runs it (the eager step contains the gradient all-reduce); rank 0 reports
        result["roofline"] = roofline_leg(engine, x, refs)
        if rank == 0 and world == 1:
            result["roofline"]["transforms"] = transforms_leg(model, x, refs, engine)
            # (flat copy: a consumer that keeps only the top level of `roofline` still sees the number north_star's target is stated on)
            result["roofline"]["transforms_frac"] = result["roofline"]["transforms"]["total"]["frac_of_f32_mfma_peak"]
            result["roofline"]["transforms_ms"] = result["roofline"]["transforms"]["total"]["ms"]
        if rank == 0:
            # flat copies (a consumer that keeps only the top level of `roofline` sees them): the whole step's algorithmic FLOPs over the
            # TIMED region's ms_per_step, and the transforms' share of one step by owner-tagged launches
            rl = result["roofline"]
            rl["whole_step_frac"] = round(rl["all_mfma_kernels"]["gflop_per_step"] / result["ms_per_step"] / F32_MFMA_PEAK_TFLOPS, 4)
            rl["in_step_transforms_frac"] = rl["in_step_by_owner"].get("transforms", {}).get("frac_of_f32_mfma_peak")
    if rank == 0:
        reduced_parity = None
        if args.full and world == 1 and not args.no_parity:
            result["parity"], result["codec"], reduced_parity = parity_and_codec(dev)
        if args.full and world == 1 and not args.no_reduced:
            result["reduced_precision"] = reduced_precision_leg(args, dev, x, refs)
            if reduced_parity:
                result["reduced_precision"].update(reduced_parity)
            result["reduced_precision"]["vs_f32_value"] = result["reduced_precision"]["value"] / result["value"]
        if args.full and world == 1 and not use_dist and not args.no_reference_loop:
            result["reference_loop"] = reference_loop_leg(args, dev, x, refs)
            result["reference_loop"]["vs_engine_value"] = round(result["reference_loop"]["value"] / result["value"], 4)
        if args.full and world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(args.n_refs, args.cpu_sample_batch or args.batch, args.size, N=args.N, lmbda=args.lmbda, loss=args.loss)
        print(json.dumps(result), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
