"""Seeds for the whole-module gradient test of clc_amd.clm.CLM (tests/test_clm_train_gpu.py::test_clm_module_gradients).

The bilinear slope and the validity mask of the deformable sampling jump where a sampling coordinate crosses a grid line, so a
gradient comparison between a float32 implementation and the float64 oracle is only meaningful on inputs whose coordinates all keep
a distance from the integers.  For each seed this runs the float64 oracle forward on the test's set-up (CLM(64, 0.5), weight recipe 11,
offset_conv.weight x6, offset_conv.bias x20, B = 1, two references, 16x16) and prints the smallest distance of any sampling coordinate
in (-0.5, H - 0.5) to an integer; the test needs >= 5e-4.
usage: python tools/scan_clm_seeds.py [first_seed] [count] [min_distance]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from oracle import clm as oc
from oracle.recipe import apply_weight_recipe


def min_distance(m, seed, B=1, n_refs=2, C=64, H=16, W=16):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, C, H, W, generator=g)
    refs = [torch.randn(B, C, H, W, generator=g) for _ in range(n_refs)]
    offsets = []
    hook = m.alignment.offset_conv.register_forward_hook(lambda _m, _i, out: offsets.append(out.detach()))
    with torch.no_grad():
        m(y.double(), [r.double() for r in refs])
    hook.remove()
    d = 1.0
    for off in offsets:
        o = off.reshape(B, 9, 2, H, W)
        for c, n in ((torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) + o[:, :, 0], H),
                     (torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) + o[:, :, 1], W)):
            c = c[(c > -0.5) & (c < n - 0.5)]
            d = min(d, (c - c.round()).abs().min().item())
    return d


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    need = float(sys.argv[3]) if len(sys.argv) > 3 else 5e-4
    m = oc.CLM(64, temperature=0.5).eval()
    apply_weight_recipe(m, 11)
    with torch.no_grad():
        m.alignment.offset_conv.weight.mul_(6.0)
        m.alignment.offset_conv.bias.mul_(20.0)
    m = m.double()
    for seed in range(first, first + count):
        d = min_distance(m, seed)
        if d >= need:
            print(f"seed {seed}: {d:.2e}", flush=True)


if __name__ == "__main__":
    main()
