"""Measurements for the video path of ssf2020 -> profiles/ssf_codec_bench.json.

CODEC.  ScaleSpaceFlow(mid_planes=128, planes=192) with the recipe weights (the last encoder layers and the scale decoders rescaled as
in tests/test_ssf_model_gpu.py, so the latents are not all zero), one keyframe and seven P-frames, at 256x256 and 512x768
with batch 1 and 256x256 with batch 4.  `decompress` and `compress`, each on the lanes stream at W = 4 and W = 16 against the
untouched default format (the baseline: one hop to the host per latent, 2 F - 1 per sequence).  One process, the legs interleaved,
every leg warmed up; per leg `rounds` timings of the whole call, by wall clock around a device synchronise AND by device events
around the call; median [min .. max] of each.  Beside them the device -> host copies of one call (counted) and the y bytes of the
lanes strings over the default's.  Every decompress leg must return the same frames, bit for bit.

GATE: the lanes decompress at W = 4 must not have a higher wall-clock median than the default at any shape.  The result is recorded
either way; a failed gate is exit status 1.

FRAME KERNELS.  yuv420_to_rgb (both modes) and rgb_to_yuv420 at 8 and 10 bits, 1920x1080 -> 1152x1920 padded and 256x256, against the
same composition in torch ops on the GPU (what tests/frames_ref.py runs, in float32).  Device events around `--reps` back-to-back
calls, `rounds` timings; achieved GB/s against the bytes the definition must move: the sample planes once and the f32 frame once.

Fails without a GPU; there is no fallback.
usage: python tools/bench_ssf_codec.py [--rounds 7] [--reps 20] [--out profiles/ssf_codec_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssf_codec_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ssf_codec.py measures on the GPU: none found")
dev = torch.device("cuda:0")

from clc_amd import frames, models
from clc_amd.recipe import apply_weight_recipe, synthetic_image

LANES = (4, 16)
KR, KG, KB = 0.2126, 0.7152, 0.0722


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


def timed(fn, reps=1):
    """-> (wall ms, event ms) of `reps` back-to-back calls, per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, e0.elapsed_time(e1) / reps


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "timings": len(v)}


def sequence(B, h, w, n):
    """a smooth image and shifted, dimmed copies of it: frames a motion field can partly explain"""
    base = synthetic_image(B, h + 32, w + 32, 77, smooth=True)
    return [(base[:, :, 16 + 2 * t:16 + 2 * t + h, 16 - t:16 - t + w] * (1.0 - 0.01 * t)).contiguous().to(dev) for t in range(n)]


def y_bytes(strings):
    return sum(len(s) for t, fs in enumerate(strings) for pair in ([fs] if t == 0 else [fs["motion"], fs["residual"]]) for s in pair[0])


report = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "frames": args.frames}

# ------------------------------------------------------------------------------------------------ the codec
net = models.ScaleSpaceFlow(mid_planes=128, planes=192)
apply_weight_recipe(net, 0)
with torch.no_grad():   # as tests/test_ssf_model_gpu.py: the bare recipe gives all-zero latents, streams of a coder's flush and nothing else
    for enc_net in (net.img_encoder, net.res_encoder, net.motion_encoder):
        enc_net[6].weight.mul_(20.0)                                  # latents with a few quantisation bins of spread
    for hp in (net.img_hyperprior, net.res_hyperprior, net.motion_hyperprior):
        hp.hyper_decoder_scale.deconv3.weight.mul_(4.0)               # predicted scales of order one
        hp.hyper_decoder_scale.deconv3.bias.add_(0.6)
    net.motion_decoder[6].weight.mul_(0.3)                            # flows of a few pixels
net = net.to(dev).eval()
net.update(force=True)
cases, gates = [], []
for (h, w), B in (((256, 256), 1), ((512, 768), 1), ((256, 256), 4)):
    seq = sequence(B, h, w, args.frames)
    coded = {None: net.compress(seq)}
    coded.update({W: net.compress(seq, lanes=W) for W in LANES})
    key = lambda W: "default" if W is None else f"lanes_W{W}"
    dec = {key(W): (lambda W: lambda: net.decompress(*coded[W], lanes=W))(W) for W in coded}
    enc = {key(W): (lambda W: lambda: net.compress(seq, lanes=W))(W) for W in coded}
    ref, copies_dec, copies_enc = None, {}, {}
    for k, fn in dec.items():   # warm-up; every leg returns the same frames, bit for bit
        fn()
        with count_d2h() as c:
            out = fn()
        copies_dec[k] = c.n
        ref = out if ref is None else ref
        assert all(torch.equal(a, b) for a, b in zip(out, ref)), k
    for (k, fn), W in zip(enc.items(), coded):   # ... and run to run the same strings
        fn()
        with count_d2h() as c:
            got = fn()
        copies_enc[k] = c.n
        assert got[0] == coded[W][0], k
    td, te = {k: ([], []) for k in dec}, {k: ([], []) for k in enc}
    for _ in range(args.rounds):
        for legs, acc in ((dec, td), (enc, te)):
            for k, fn in legs.items():
                wall, event = timed(fn)
                acc[k][0].append(wall)
                acc[k][1].append(event)
    leg = lambda acc, copies: {k: {"wall_ms": stats(v[0]), "event_ms": stats(v[1]), "device_to_host_copies": copies[k]} for k, v in acc.items()}
    case = {"image": [h, w], "batch": B, "frames": args.frames, "hops_default": 2 * args.frames - 1, "decompress": leg(td, copies_dec),
            "compress": leg(te, copies_enc), "y_bytes": {key(W): y_bytes(coded[W][0]) for W in coded}}
    case["y_bytes_over_default"] = {k: v / case["y_bytes"]["default"] for k, v in case["y_bytes"].items()}
    d = case["decompress"]
    case["lanes_W4_decompress_median_not_above_default"] = bool(d["lanes_W4"]["wall_ms"]["median"] <= d["default"]["wall_ms"]["median"])
    case["decompress_ratio_default_over_lanes_W4"] = d["default"]["wall_ms"]["median"] / d["lanes_W4"]["wall_ms"]["median"]
    case["compress_ratio_default_over_lanes_W4"] = case["compress"]["default"]["wall_ms"]["median"] / case["compress"]["lanes_W4"]["wall_ms"]["median"]
    gates.append(case["lanes_W4_decompress_median_not_above_default"])
    cases.append(case)
    line = lambda legs: " | ".join(f"{k} {v['wall_ms']['median']:.2f} [{v['wall_ms']['min']:.2f} .. {v['wall_ms']['max']:.2f}] ms wall, "
                                   f"{v['event_ms']['median']:.2f} ms events, {v['device_to_host_copies']} d2h" for k, v in legs.items())
    print(f"ssf2020 {h}x{w} batch {B} decompress: {line(case['decompress'])}", flush=True)
    print(f"ssf2020 {h}x{w} batch {B} compress:   {line(case['compress'])}", flush=True)
report["codec"] = {"model": "ScaleSpaceFlow(mid_planes=128, planes=192)", "cases": cases}
gate = bool(gates) and all(gates)
report["gate"] = {"what": "decompress: the wall-clock median of lanes = 4 does not exceed the default format's, at every shape", "per_case": gates,
                  "passed": gate}


# ------------------------------------------------------------------------------------------------ the frame kernels
def torch_to_rgb(Y, U, V, bits, mode, size):
    mx = float(2 ** bits - 1)
    c = F.interpolate(torch.stack((U, V), dim=1).float() / mx, scale_factor=2, mode=mode, align_corners=False)
    y, cb, cr = Y.float() / mx, c[:, 0], c[:, 1]
    r = y + (2 - 2 * KR) * (cr - 0.5)
    b = y + (2 - 2 * KB) * (cb - 0.5)
    rgb = torch.stack((r, (y - KR * r - KB * b) / KG, b), dim=1)
    rgb = F.pad(rgb, (0, size[1] - rgb.shape[3], 0, size[0] - rgb.shape[2]), mode="replicate")
    return rgb.contiguous(memory_format=torch.channels_last)


def torch_to_yuv(rgb, size, bits):
    mx = float(2 ** bits - 1)
    r, g, b = rgb[:, :, :size[0], :size[1]].clamp(0, 1).unbind(1)
    y = KR * r + KG * g + KB * b
    c = F.avg_pool2d(torch.stack((0.5 * (b - y) / (1 - KB) + 0.5, 0.5 * (r - y) / (1 - KR) + 0.5), dim=1), 2)
    q = lambda v: torch.round(v.clamp(0, 1) * mx).to(torch.uint8 if bits == 8 else torch.int16)
    return q(y), q(c[:, 0]), q(c[:, 1])


kernels = []
for (H, W), (Hp, Wp) in (((1080, 1920), (1152, 1920)), ((256, 256), (256, 256))):
    for bits in (8, 10):
        g = torch.Generator().manual_seed(1)
        dt, sz = (torch.uint8, 1) if bits == 8 else (torch.int16, 2)
        Y, U, V = (torch.randint(0, 2 ** bits, s, generator=g).to(dt).to(dev) for s in ((1, H, W), (1, H // 2, W // 2), (1, H // 2, W // 2)))
        rgb = frames.yuv420_to_rgb(Y, U, V, bit_depth=bits, size=(Hp, Wp))
        legs = {}
        for mode in ("bilinear", "bicubic"):
            legs[f"yuv420_to_rgb_{mode}"] = (lambda mode: lambda: frames.yuv420_to_rgb(Y, U, V, bit_depth=bits, mode=mode, size=(Hp, Wp)))(mode)
            legs[f"torch_to_rgb_{mode}"] = (lambda mode: lambda: torch_to_rgb(Y, U, V, bits, mode, (Hp, Wp)))(mode)
        legs["rgb_to_yuv420"] = lambda: frames.rgb_to_yuv420(rgb, (H, W), bit_depth=bits)
        legs["torch_to_yuv"] = lambda: torch_to_yuv(rgb, (H, W), bits)
        # the torch composition computes the same frame to f32 rounding, and the same samples but for rounding ties
        for mode in ("bilinear", "bicubic"):
            diff = (legs[f"yuv420_to_rgb_{mode}"]() - legs[f"torch_to_rgb_{mode}"]()).abs().max().item()
            assert diff < 1e-4, (mode, diff)
        off = max((a.int() - b.int()).abs().max().item() for a, b in zip(legs["rgb_to_yuv420"](), legs["torch_to_yuv"]()))
        assert off <= 1, off
        t = {k: [] for k in legs}
        for k, fn in legs.items():
            timed(fn, 3)
        for _ in range(args.rounds):
            for k, fn in legs.items():
                t[k].append(timed(fn, args.reps)[1])
        moved = {"to_rgb": 1.5 * H * W * sz + 12 * Hp * Wp, "to_yuv": 12 * H * W + 1.5 * H * W * sz}
        row = {"size": [H, W], "padded": [Hp, Wp], "bit_depth": bits, "bytes_the_definition_moves": moved, "event_ms": {}, "achieved_GB_per_s": {}}
        for k, v in t.items():
            row["event_ms"][k] = stats(v)
            row["achieved_GB_per_s"][k] = moved["to_rgb" if "to_rgb" in k else "to_yuv"] / (row["event_ms"][k]["median"] * 1e-3) / 1e9
        kernels.append(row)
        print(f"frames {H}x{W} -> {Hp}x{Wp}, {bits} bits: " + " | ".join(
            f"{k} {v['median'] * 1e3:.1f} us [{v['min'] * 1e3:.1f} .. {v['max'] * 1e3:.1f}], {row['achieved_GB_per_s'][k]:.0f} GB/s" for k, v in row["event_ms"].items()),
            flush=True)
report["frame_kernels"] = kernels

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
print("ssf2020: the lanes decompress at W = 4 is not slower than the default format at any shape:", gate)
sys.exit(0 if gate else 1)
