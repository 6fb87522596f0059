"""The reference's literal training-loop body over clc_amd.models, eager vs clc_amd.graphed_training, in one process.

The loop body is bench.py's reference_loop_leg (train_CLC.py:137-183): zero_grad of the reference's optimizer pair (configure_optimizers,
two torch.optim.AdamW), forward, criterion, backward, clip_grad_norm_(1.0), the per-parameter nan_to_num_ loop, optimizer.step, aux loss
backward and aux step.  Per configuration the two modes run on two copies of the same seeded model, in interleaved blocks: three blocks
of --steps free-running steps per mode, each ending in a device synchronise; the median block is the number.  A last pass with a device
synchronise after each phase gives the split (its parts sum to more than the free-running step).  `loss_match_eval` runs four
eval-mode steps (deterministic rounding) of both modes from the same weights and reports the largest loss / bpp / aux difference.

    python tools/bench_reference_loop.py [--steps 10] [--warmup 3] [--configs 1,2,tcm] [--modes eager,graphed]

One JSON line per configuration: configs[1] = CLC N=64, 256x256, batch 8, 1 reference; configs[2] = the same with 3 references;
tcm = TCM N=64, 256x256, batch 8.
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {"1": ("clc", 1), "2": ("clc", 3), "tcm": ("tcm", 0)}


def make(kind, R, dev, graphed):
    import clc_amd
    from clc_amd import models
    from clc_amd.recipe import apply_weight_recipe

    m = models.CLC(N=64, num_ref_frames=R) if kind == "clc" else models.TCM(N=64)
    apply_weight_recipe(m, 0)
    m = m.to(dev).train()
    return clc_amd.graphed_training(m, graphed)


class Loop:
    def __init__(self, model, lmbda=0.0067):
        from clc_amd.train import RateDistortionLoss, configure_optimizers

        self.model = model
        self.criterion = RateDistortionLoss(lmbda=lmbda, type="mse")
        self.optimizer, self.aux_optimizer = configure_optimizers(model, types.SimpleNamespace(learning_rate=1e-4, aux_learning_rate=1e-3))
        self.marks = []

    def body(self, x, refs, sync_phases=False):
        import torch

        def mark(name):
            if sync_phases:
                torch.cuda.synchronize()
                self.marks.append((name, time.perf_counter()))
        model, optimizer, aux_optimizer, clip_max_norm = self.model, self.optimizer, self.aux_optimizer, 1.0
        mark("start")
        optimizer.zero_grad()
        aux_optimizer.zero_grad()
        out_net = model(x, refs)
        out_criterion = self.criterion(out_net, x)
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
        return out_criterion, aux_loss

    def block(self, x, refs, steps):
        import torch

        t0 = time.perf_counter()
        for _ in range(steps):
            self.body(x, refs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    def split(self, x, refs):
        self.marks.clear()
        self.body(x, refs, sync_phases=True)
        return {name: round((tb - ta) * 1e3, 2) for (_, ta), (name, tb) in zip(self.marks[:-1], self.marks[1:])}


def loss_match(kind, R, dev, x, refs, steps=4):
    seqs = []
    for graphed in (False, True):
        lp = Loop(make(kind, R, dev, graphed).eval())
        seq = []
        for _ in range(steps):
            out, aux = lp.body(x, refs)
            seq.append((out["loss"].item(), out["bpp_loss"].item(), aux.item()))
        seqs.append(seq)
        del lp
    diff = max(abs(a - b) for sa, sb in zip(*seqs) for a, b in zip(sa, sb))
    return {"max_abs_diff": diff, "bit_identical": seqs[0] == seqs[1], "eager": [s[0] for s in seqs[0]], "graphed": [s[0] for s in seqs[1]]}


def run(name, kind, R, args, dev):
    import torch

    from clc_amd.recipe import synthetic_image

    B = args.batch
    x = synthetic_image(B, 256, 256, 100, smooth=True).to(dev)
    refs = [synthetic_image(B, 256, 256, 101 + i, smooth=True).to(dev) for i in range(R)] if R else None
    loops = {k: Loop(make(kind, R, dev, k == "graphed")) for k in args.modes.split(",")}
    for lp in loops.values():
        for _ in range(args.warmup):
            lp.body(x, refs)
    torch.cuda.synchronize()
    blocks = {k: [] for k in loops}
    for _ in range(3):
        for k, lp in loops.items():
            blocks[k].append(lp.block(x, refs, args.steps))
    res = {"config": name, "model": kind, "N": 64, "size": 256, "batch": B, "n_refs": R, "steps": args.steps, "warmup": args.warmup}
    for k, lp in loops.items():
        dt = sorted(blocks[k])[1]
        res[k] = {"ms_per_step": round(dt * 1e3, 2), "img_per_s": round(B / dt, 1), "blocks_ms": [round(b * 1e3, 2) for b in blocks[k]],
                  "phase_ms_with_a_sync_after_each": lp.split(x, refs)}
    for k in loops:
        if "eager" in res:
            res[k]["vs_eager"] = round(res["eager"]["ms_per_step"] / res[k]["ms_per_step"], 3)
        if k == "graphed":
            g = loops[k].model.__dict__.get("_clc_graphed")
            res[k]["captured_plans"] = len(g.plans) if g is not None else 0
    del loops
    torch.cuda.empty_cache()
    if not args.no_loss_match:
        res["loss_match_eval"] = loss_match(kind, R, dev, x[:2], [r[:2] for r in refs] if refs else None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--configs", default="1,2,tcm")
    ap.add_argument("--modes", default="eager,graphed", help="which modes to time (a profiler run takes one)")
    ap.add_argument("--no-loss-match", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_reference_loop.py needs an MI355X")
    dev = torch.device("cuda:0")
    for c in args.configs.split(","):
        kind, R = CONFIGS[c]
        print(json.dumps(run(f"configs[{c}]" if c != "tcm" else "tcm", kind, R, args, dev)), flush=True)


if __name__ == "__main__":
    main()
