"""Graph-captured forward / backward of CLC / TCM for plain PyTorch training loops (``clc_amd.graphed_training``).

The reference's own loop (train_CLC.py:137-183) — or any loop with its own optimizer, scheduler, EMA or logging between backward()
and step() — drives the model through autograd.  Eagerly that is ~1 250 Python autograd Functions per step, and the step is bound by
their host cost, not by the GPU.  In this mode a training forward of the model instead replays a hipGraph captured from the eager
forward, and its outputs hang off ONE autograd node whose backward replays a second hipGraph captured from the eager backward and
hands the parameter gradients to autograd.  The kernels are the eager path's, in the eager order; only the per-use filter images
(transposed filters, halo / Winograd packs, GDN re-parametrisation) come from the batched refresh launches of clc_amd.train inside the
forward graph — bit-identical images, four launches instead of one per layer.

When the captured path is taken (anything else runs the eager forward, unchanged):
  * the mode is on for the model: graphed_training(model) or CLC_GRAPH_TRAIN=1 in the environment (default off);
  * grad mode is on, at least one parameter requires grad, the inputs do not, and they are CUDA tensors;
  * the model is not owned by a clc_amd.train.TrainEngine (claim()), is not a DataParallel replica, no process group is initialised
    (DDP steps aside to eager) and no other capture is in progress;
  * the call's signature (signature()) has a captured plan.  A plan is captured the first time a signature is met while the model has
    none, or when the same new signature comes on two consecutive calls: a one-off shape such as the short last batch of an epoch runs
    eagerly and the next full batch replays again.  At most CLC_GRAPH_TRAIN_PLANS (default 2) plans are captured per model, all in one
    private memory pool; once that many exist, further signatures run eagerly.  Plans are never evicted.

Parameters follow the graphs: the optimizer updates parameter storage in place and every derived image is rebuilt inside the forward
graph on each replay.  A parameter, buffer or sub-module that is REPLACED (load_state_dict resizing a buffer, .to(), update(), a new
Parameter object) changes the model's fingerprint — identities and data_ptr()s of every parameter and buffer, checked on each call —
and every plan is released before the next replay.  So are the plans of a model a TrainEngine takes over.

A model whose plans have been released is never captured again: it runs eagerly from then on (with one warning), and
graphed_training(model) refuses it.  Nothing is evicted either, and switching the mode off keeps the plans (unused): a release is
always final, so no capture ever follows one on the same model.  Build the model again (or enable the mode after replacing its
parameters) to train it graphed.  Captures differentiate with respect to stand-in leaves (_StandIns), never the parameters themselves.
"""
from __future__ import annotations

import itertools
import operator
import os
import weakref

import torch

from . import ops
from .train import StepImages

ENV = "CLC_GRAPH_TRAIN"
_TRUE, _FALSE = ("1", "true", "on", "yes"), ("", "0", "false", "off", "no")


def parse_env(value) -> bool:
    """CLC_GRAPH_TRAIN value -> on / off.  Unset or empty is off; anything unrecognised is an error rather than a guess."""
    v = ("" if value is None else str(value)).strip().lower()
    if v in _TRUE:
        return True
    if v in _FALSE:
        return False
    raise ValueError(f"{ENV}={value!r}: expected one of 1/true/on/yes or 0/false/off/no")


GRAPH_TRAIN = parse_env(os.environ.get(ENV))   # process default of the switch, read once at import
_DATA_PTR, _REQ_GRAD = torch.Tensor.data_ptr, operator.attrgetter("requires_grad")
MAX_PLANS = max(1, int(os.environ.get("CLC_GRAPH_TRAIN_PLANS", "2")))

# models driven by a TrainEngine (it captures the whole step itself, with its own filter images on the same Parameters): weak keys, so a
# released engine releases the claim
_OWNERS = weakref.WeakKeyDictionary()


def claim(model, engine) -> None:
    """Called by TrainEngine: from now on the model's forwards run eagerly (inside the engine's capture) and captured plans are dropped."""
    _OWNERS[model] = weakref.ref(engine)


def owner(model):
    r = _OWNERS.get(model)
    return r() if r is not None else None


def graphed_training(model, enabled: bool = True):
    """Turn the captured forward / backward on (or off) for `model`, whatever CLC_GRAPH_TRAIN says.  Returns the model.
    Switching off keeps the captured plans (unused) so that switching on again replays them."""
    if enabled and owner(model) is not None:
        raise RuntimeError("clc_amd.graphed_training: this model is driven by a clc_amd.train.TrainEngine, which captures the whole step "
                           "itself; use one or the other")
    if enabled and model.__dict__.get(_RELEASED):
        raise RuntimeError("clc_amd.graphed_training: this model's captured graphs were released (a parameter or buffer was replaced, or a "
                           "TrainEngine took it over) and a model is not captured a second time; build the model again, or switch the mode on "
                           "after replacing its parameters")
    model.__dict__["_clc_graph_train"] = bool(enabled)
    return model


def is_enabled(model) -> bool:
    flag = model.__dict__.get("_clc_graph_train")
    return GRAPH_TRAIN if flag is None else bool(flag)


_RELEASED = "_clc_graph_released"


def drop(model, why: str) -> None:
    """Release every captured plan of `model` (outstanding graphed outputs can no longer be back-propagated).  The model runs eagerly from
    then on: it is never captured again (module docstring)."""
    st = model.__dict__.pop("_clc_graphed", None)
    if st is not None:
        st.invalidate()
    if not model.__dict__.get(_RELEASED):
        model.__dict__[_RELEASED] = True
        import warnings

        warnings.warn(f"clc_amd.graphed_training: {why}; the model's captured graphs are released and it runs eagerly from now on "
                      "(build the model again, or switch the mode on after replacing its parameters, to train it graphed)",
                      RuntimeWarning, stacklevel=3)


# ------------------------------------------------------------------------------------------------ signature
_N_TUNING = []


def kernel_state():
    """Everything in the native library's state that selects kernels or summation orders: the kernel-configuration tag and hash
    (precision, order-affecting tuning keys) and the raw tuning table (kernel-selection keys such as the halo / Winograd switches)."""
    from . import lib

    L = lib.load()
    if not _N_TUNING:
        n = 0
        while n < 256 and L.clc_get_tuning(n) != -1:
            n += 1
        _N_TUNING.append(n)
    return (int(L.clc_kernel_config_tag()), int(L.clc_kernel_config_hash()), tuple(L.clc_get_tuning(k) for k in range(_N_TUNING[0])))


def _ops_state():
    """the Python-side switches of clc_amd.ops that change which launches a forward / backward issues"""
    return (ops.WGRAD_DEFER, ops.DEFER_REDUCTIONS, ops.PAIR_SLICES, ops.SUPPORT_BUFFER, ops.PROFILE is not None)


def signature(model, x, refs, kstate=None):
    """Key of a captured plan: input shapes / dtypes, the reference count, the train / eval state of the model and of its two entropy
    models (which decide whether the noise proxy is drawn), the output set (`_lean_outputs`), the structural switches of the model,
    and the kernel state (kernel_state(), ops switches)."""
    gc = getattr(model, "gaussian_conditional", None)
    eb = getattr(model, "entropy_bottleneck", None)
    return (tuple(x.shape), x.dtype,
            None if refs is None else tuple((tuple(r.shape), r.dtype) for r in refs),
            bool(model.training), bool(gc.training) if gc is not None else None, bool(eb.training) if eb is not None else None,
            bool(getattr(model, "_lean_outputs", False)), bool(getattr(model, "wire_clm", False)),
            getattr(model, "use_ref", None), getattr(model, "max_support_slices", None),
            kernel_state() if kstate is None else kstate, _ops_state())


# ------------------------------------------------------------------------------------------------ outputs
def _flatten(out):
    ts = [out["x_hat"], out["likelihoods"]["y"], out["likelihoods"]["z"]]
    if "para" in out:
        ts += [out["para"]["means"], out["para"]["scales"], out["para"]["y"]]
    return ts


def _unflatten(ts):
    out = {"x_hat": ts[0], "likelihoods": {"y": ts[1], "z": ts[2]}}
    if len(ts) > 3:
        out["para"] = {"means": ts[3], "scales": ts[4], "y": ts[5]}
    return out


# ------------------------------------------------------------------------------------------------ stand-in leaves
class _StandIns:
    """During warm-up and capture every parameter of the model is swapped for a fresh leaf on the SAME storage (same attributes), and the
    captured graphs differentiate with respect to those leaves.

    Why: a parameter's AccumulateGrad node is cached on the parameter for as long as any autograd graph that uses it is alive — e.g. the
    `out` of the previous step that a training loop still holds — and it keeps the stream it was created on.  autograd.grad inside a
    capture then synchronises the capturing stream with that outside stream (an event round trip and a record_stream on the gradients),
    and hipStreamEndCapture crashed on it: the second capture of a model whose earlier forward's graph was still referenced faulted in
    capture_end.  Fresh leaves have no outside history, so everything the engine does in the capture stays on the capturing stream.
    Sharing the storage is what makes the replays follow the optimizer's in-place updates; the real parameters receive their gradients
    from the graphed node's backward, as before."""

    def __init__(self, model):
        self.slots = [(m._parameters, n, p) for m in model.modules() for n, p in m._parameters.items() if p is not None]
        self.sub = {}
        for _, _, p in self.slots:
            if id(p) not in self.sub:
                leaf = p.detach().requires_grad_(p.requires_grad)
                leaf.__dict__.update(p.__dict__)   # (ops' markers such as `_clc_is_filter`)
                self.sub[id(p)] = leaf
        self.leaves = list(self.sub.values())

    def of(self, p):
        return self.sub[id(p)]

    def __enter__(self):
        for d, n, p in self.slots:
            d[n] = self.sub[id(p)]
        return self

    def __exit__(self, *exc):
        for d, n, p in self.slots:
            d[n] = p
        return False


# ------------------------------------------------------------------------------------------------ one captured signature
class _Plan:
    def __init__(self, state, sig):
        self.state, self.sig = state, sig
        self.dead = False
        self.fwd = self.bwd = None

    def capture(self, x, refs):
        st = self.state
        model = st.model
        cl = lambda t: t.detach().float().clone(memory_format=ops.CL) if t.dim() == 4 else t.detach().float().clone()
        self.sx = cl(x)
        self.srefs = [cl(r) for r in refs] if refs is not None else None
        inputs = [p for p in st.params if p.requires_grad]
        with _StandIns(model) as si:
            params = [si.of(p) for p in inputs]
            # warm-up on a side stream (allocator, lazy kernel attributes, which filters take the halo / Winograd kernels).  Gradients
            # come back from autograd.grad: the user's p.grad is never touched.
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with ops.collecting_uses() as uses:
                    outs = _flatten(model._forward_eager(self.sx, self.srefs))
                    diff = [o for o in outs if o.requires_grad]
                    grads = torch.autograd.grad(diff, params, grad_outputs=[torch.ones_like(o) for o in diff], allow_unused=True)
                    ops.join_side_streams()
                live_idx = [i for i, g in enumerate(grads) if g is not None]
                del outs, diff, grads
                self.live = [params[i] for i in live_idx]
                # (the plan's own images, of its stand-in leaves: the model's Parameters and any other owner's images are not involved)
                self.images = StepImages(model, self.live, uses)
                self.images.refresh()
                with self.images.valid():
                    outs = _flatten(model._forward_eager(self.sx, self.srefs))
                    diff = [o for o in outs if o.requires_grad]
                    torch.autograd.grad(diff, self.live, grad_outputs=[torch.ones_like(o) for o in diff], allow_unused=True)
                    ops.join_side_streams()
                del outs, diff
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            # index of each differentiated parameter in the node's inputs (all parameters that require grad, in named order)
            self.live_pos = live_idx
            self.n_inputs = len(inputs)
            self.inputs = inputs
            self.fwd, self.bwd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            # (the default CUDA generator is registered with the capture: each replay draws fresh noise for the training-mode proxy)
            with ops.capture_guard(), torch.cuda.graph(self.fwd, pool=st.pool, capture_error_mode=ops.graph_capture_mode()):
                self.images.refresh()
                with self.images.valid():
                    self.souts = _flatten(model._forward_eager(self.sx, self.srefs))
            self.diff_idx = [i for i, o in enumerate(self.souts) if o.requires_grad]
            self.sgos = [torch.zeros_like(self.souts[i]) for i in self.diff_idx]
            self.go_dirty = [False] * len(self.sgos)
            with ops.capture_guard(), torch.cuda.graph(self.bwd, pool=st.pool, capture_error_mode=ops.graph_capture_mode()):
                with self.images.valid():
                    g = torch.autograd.grad([self.souts[i] for i in self.diff_idx], self.live, grad_outputs=self.sgos, allow_unused=True)
                    ops.join_side_streams()
            self.souts = [o.detach() for o in self.souts]   # (the autograd graph of the capture is not needed past this point)
            self.grad_pos = [self.live_pos[j] for j, t in enumerate(g) if t is not None]
            self.sgrads = [t for t in g if t is not None]
        torch.cuda.synchronize()

    def close(self):
        self.dead = True
        self.fwd = self.bwd = None
        self.souts = self.sgos = self.sgrads = None
        self.images = None


class _GraphedForward(torch.autograd.Function):
    """forward: replay the captured forward, return copies of its outputs.  backward: the ONE node of the model's training forward."""

    @staticmethod
    def forward(ctx, plan, *params):
        ctx.set_materialize_grads(False)
        plan.fwd.replay()
        ctx.plan, ctx.gen, ctx.done = plan, plan.state.bump(), False
        # copies: the caller may keep the outputs (logging, a second criterion) past the next replay, which rewrites the static ones
        return tuple(o.clone() for o in plan.souts)

    @staticmethod
    def backward(ctx, *gos):
        plan = ctx.plan
        if ctx.done:
            raise RuntimeError("clc_amd.graphed_training: backward through the same graphed forward a second time (its captured "
                               "activations were consumed by the first backward; run the forward again)")
        if plan.dead or plan.state.gen != ctx.gen:
            raise RuntimeError("clc_amd.graphed_training: backward through a stale forward — a later graphed forward of this model (or "
                               "a re-capture) has overwritten its captured activations; call backward before the next forward")
        ctx.done = True
        for j, i in enumerate(plan.diff_idx):
            g = gos[i]
            if g is None:   # (the criterion did not use this output: a zero gradient, written only when the buffer holds another)
                if plan.go_dirty[j]:
                    plan.sgos[j].zero_()
                    plan.go_dirty[j] = False
            else:
                plan.sgos[j].copy_(g)
                plan.go_dirty[j] = True
        plan.bwd.replay()
        # Hand-off = COPY.  The captured gradients live in the graph's pool and the next replay rewrites them, so autograd must never
        # keep them: one multi-tensor pass (torch._foreach_mul by 1.0, exact) makes fresh tensors with the parameters' layouts, ~2 reads +
        # 1 write of the live gradient size (0.2 GB at N = 64) and a handful of launches.  Autograd's AccumulateGrad then STEALS a copy
        # where p.grad is None (zero_grad(set_to_none=True)) and ACCUMULATES it in place where p.grad exists (set_to_none=False), exactly
        # as for eager gradients; a copy never aliases p.grad, so `p.grad += g` cannot double it.
        copies = torch._foreach_mul(plan.sgrads, 1.0)
        res = [None] * plan.n_inputs
        for k, t in zip(plan.grad_pos, copies):
            res[k] = t
        return (None,) + tuple(res)


class _State:
    """Per-model captured plans (at most MAX_PLANS, one private pool) and the fingerprint they were captured under."""

    def __init__(self, model):
        self.model = model
        mods = list(model.modules())
        self.pdicts = [m._parameters for m in mods if m._parameters]
        self.bdicts = [m._buffers for m in mods if m._buffers]
        self.mdicts = [m._modules for m in mods if m._modules]
        self.params = list(model.parameters())
        self.fp = self.fingerprint()
        self.plans = {}
        self.pool = torch.cuda.graph_pool_handle()
        self.gen = 0
        self.last_sig = None

    def fingerprint(self):
        """identities and storage addresses of every parameter and buffer, identities of the sub-modules, and which parameters require
        grad (~0.6 ms at N = 64: 1 441 parameters, 60 buffers, 1 548 modules)"""
        ch = itertools.chain.from_iterable
        ps = list(ch([d.values() for d in self.pdicts]))
        bs = list(ch([d.values() for d in self.bdicts]))
        live_p = [v for v in ps if v is not None]
        live_b = [v for v in bs if v is not None]
        return (tuple(map(id, ps)), tuple(map(_DATA_PTR, live_p)), tuple(map(_REQ_GRAD, live_p)), tuple(map(id, bs)),
                tuple(map(_DATA_PTR, live_b)), tuple(map(id, ch([d.values() for d in self.mdicts]))))

    def bump(self):
        self.gen += 1
        return self.gen

    def invalidate(self):
        for p in self.plans.values():
            p.close()
        self.plans.clear()
        self.gen += 1

    def run(self, x, refs):
        sig = signature(self.model, x, refs)
        plan = self.plans.get(sig)
        if plan is None:
            if self.plans and sig != self.last_sig:
                self.last_sig = sig
                return None   # a one-off signature: eager for this call
            if len(self.plans) >= MAX_PLANS:
                self.last_sig = sig
                return None   # as many plans as allowed: no eviction (a release followed by a capture is never taken)
            self.gen += 1   # (a capture reuses the pool: no earlier graphed forward may be back-propagated after it)
            plan = _Plan(self, sig)
            try:
                plan.capture(x, refs)
            except BaseException:
                plan.close()
                raise
            self.plans[sig] = plan
        else:
            self.last_sig = sig
        plan.sx.copy_(x)
        if refs is not None:
            for d, r in zip(plan.srefs, refs):
                d.copy_(r)
        return _unflatten(list(_GraphedForward.apply(plan, *plan.inputs)))


def _steps_aside(model, x, refs) -> bool:
    if not torch.is_grad_enabled() or not isinstance(x, torch.Tensor) or not x.is_cuda or x.requires_grad:
        return True
    if refs is not None and not (isinstance(refs, (list, tuple)) and all(isinstance(r, torch.Tensor) and r.is_cuda and not r.requires_grad for r in refs)):
        return True
    if owner(model) is not None or getattr(model, "_is_replica", False) or getattr(model, "_keep_boundary", False):
        return True
    if torch.cuda.is_current_stream_capturing() or ops.PROFILE is not None:
        return True
    import torch.distributed as dist

    return dist.is_available() and dist.is_initialized()


def forward(model, x, refs):
    """The model's forward in graphed mode, or None: the caller runs its eager forward."""
    if not is_enabled(model) or _steps_aside(model, x, refs):
        if "_clc_graphed" in model.__dict__ and owner(model) is not None:
            drop(model, "a TrainEngine took the model over")
        return None
    if model.__dict__.get(_RELEASED):
        return None
    refs = list(refs) if refs is not None else None
    st = model.__dict__.get("_clc_graphed")
    if st is not None and st.fingerprint() != st.fp:
        drop(model, "a parameter, buffer or sub-module of the model was replaced after its capture")
        return None
    if st is None:
        st = _State(model)
        if not any(p.requires_grad for p in st.params):
            return None
        model.__dict__["_clc_graphed"] = st
    if not any(p.requires_grad for p in st.params):
        return None
    return st.run(x, refs)
