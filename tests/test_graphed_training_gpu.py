"""clc_amd.graphed_training: the captured forward / backward behind ONE autograd node, driven by plain PyTorch training loops.

The graphed path issues the eager path's kernels in the eager order (only the per-layer filter images come from the four batched
refresh launches, which compute the same images), so the graphed literal reference loop is held to BIT-IDENTITY with the eager loop:
losses, gradients and parameters.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LMBDA, LR, AUX_LR, CLIP = 0.0067, 1e-4, 1e-3, 1.0


def _model(dev, kind="clc", R=1, seed=0):
    from clc_amd import models as pm
    from clc_amd.recipe import apply_weight_recipe

    m = pm.CLC(N=64, num_ref_frames=R) if kind == "clc" else pm.TCM(N=64)
    apply_weight_recipe(m, seed)
    return m.to(dev)


def _inputs(dev, B, R, size=256, seed=100):
    from clc_amd.recipe import synthetic_image

    x = synthetic_image(B, size, size, seed, smooth=True).to(dev)
    return x, ([synthetic_image(B, size, size, seed + 1 + i, smooth=True).to(dev) for i in range(R)] if R else None)


def _reference_loop(model, x, refs, steps):
    """train_CLC.py:137-183 in behaviour: zero_grad, forward, loss.backward, clip_grad_norm_, nan_to_num_, AdamW pair, aux step."""
    from clc_amd.train import RateDistortionLoss

    params = [p for n, p in model.named_parameters() if not n.endswith(".quantiles")]
    aux = [p for n, p in model.named_parameters() if n.endswith(".quantiles")]
    opt, aux_opt = torch.optim.AdamW(params, lr=LR), torch.optim.AdamW(aux, lr=AUX_LR)
    crit = RateDistortionLoss(LMBDA, "mse")
    seq = []
    for _ in range(steps):
        opt.zero_grad()
        aux_opt.zero_grad()
        out = crit(model(x, refs), x)
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
        for p in model.parameters():
            if p.grad is not None:
                p.grad.nan_to_num_()
        opt.step()
        aux_loss = model.aux_loss()
        aux_loss.backward()
        aux_opt.step()
        seq.append((out["loss"].item(), out["bpp_loss"].item(), aux_loss.item()))
    return seq


def _is_graphed(t):
    from clc_amd.graphed import _GraphedForward

    return t.grad_fn is not None and getattr(t.grad_fn, "_forward_cls", None) is _GraphedForward


def _clc_nodes(root):
    """every autograd node reachable from `root` whose Function is defined in clc_amd"""
    seen, stack, found = set(), [root], []
    while stack:
        n = stack.pop()
        if n is None or id(n) in seen:
            continue
        seen.add(id(n))
        cls = getattr(n, "_forward_cls", None)
        if cls is not None and cls.__module__.startswith("clc_amd"):
            found.append(cls.__name__)
        stack.extend(f for f, _ in n.next_functions)
    return found


@pytest.mark.parametrize("kind,R", [("clc", 1), ("clc", 3), ("tcm", 0)])
def test_graphed_reference_loop_is_bit_identical(dev, kind, R):
    """4 steps of the literal reference loop (AdamW pair, clip 1.0, nan_to_num_, aux step), eval-mode rounding: graphed == eager, bit for bit
    (loss / bpp / aux sequences and every final parameter).  This is stricter than the bars of
    test_engine_equals_reference_training_loop[use_graph-f32_mfma]."""
    import clc_amd

    x, refs = _inputs(dev, 2, R)
    m_eager = _model(dev, kind, R).eval()
    seq_eager = _reference_loop(m_eager, x, refs, 4)
    m = clc_amd.graphed_training(_model(dev, kind, R).eval())
    seq = _reference_loop(m, x, refs, 4)
    assert len(m._clc_graphed.plans) == 1
    assert seq == seq_eager, (seq, seq_eager)
    assert seq_eager[3][0] < seq_eager[0][0]
    pe = dict(m_eager.named_parameters())
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), pe[n].detach()), n


def test_one_autograd_node_and_misuse_raises(dev):
    """Under the switch the training forward's outputs hang off ONE clc_amd node; a stale backward (forward A, forward B, A.backward())
    and a second backward of the same forward raise instead of returning wrong gradients."""
    import clc_amd
    from clc_amd.graphed import _GraphedForward
    from clc_amd.train import RateDistortionLoss

    x, refs = _inputs(dev, 2, 1)
    m = clc_amd.graphed_training(_model(dev).train())
    crit = RateDistortionLoss(LMBDA, "mse")
    out = m(x, refs)
    assert _is_graphed(out["x_hat"]) and _is_graphed(out["likelihoods"]["y"])
    for t in (out["x_hat"], out["likelihoods"]["y"], out["likelihoods"]["z"], out["para"]["means"]):
        assert _clc_nodes(t.grad_fn) == [_GraphedForward.__name__]
    loss = crit(out, x)["loss"]
    found = _clc_nodes(loss.grad_fn)
    assert found.count(_GraphedForward.__name__) == 1
    criterion_fns = {"_RDLossMseFn", "_SumLog2Fn", "_SqDiffSumFn"}   # (the criterion's own fused Functions, not the model's)
    assert set(found) - {_GraphedForward.__name__} <= criterion_fns, found
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    m.zero_grad()
    a = crit(m(x, refs), x)["loss"]
    b = crit(m(x, refs), x)["loss"]
    with pytest.raises(RuntimeError, match="stale"):
        a.backward()
    b.backward()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


@pytest.mark.parametrize("set_to_none", [True, False])
def test_zero_grad_modes_match_eager(dev, set_to_none):
    """Two steps of zero_grad / forward / backward / SGD: every gradient equals the eager one (none doubled, none missing), and a gradient
    handed out by step 1 is not rewritten by step 2's replay (it does not alias the graph's buffers)."""
    import clc_amd
    from clc_amd.train import RateDistortionLoss

    x, refs = _inputs(dev, 2, 1)
    crit = RateDistortionLoss(LMBDA, "mse")
    runs = {}
    for mode in ("eager", "graphed"):
        m = _model(dev).eval()
        if mode == "graphed":
            clc_amd.graphed_training(m)
        opt = torch.optim.SGD(m.parameters(), lr=1e-3)
        grads = []
        for step in range(2):
            opt.zero_grad(set_to_none=set_to_none)
            crit(m(x, refs), x)["loss"].backward()
            grads.append({n: (p.grad if set_to_none else p.grad.clone()) for n, p in m.named_parameters() if p.grad is not None})
            if step == 0:
                kept = {n: (g, g.clone()) for n, g in grads[0].items()}
            opt.step()
        if set_to_none:
            for n, (g, c) in kept.items():
                assert torch.equal(g, c), f"{mode}: step 1's gradient of {n} changed after step 2"
        runs[mode] = grads
        if mode == "graphed":
            assert _is_graphed(m(x, refs)["x_hat"])
    for step in range(2):
        e, g = runs["eager"][step], runs["graphed"][step]
        assert e.keys() == g.keys(), step
        for n in e:
            assert torch.equal(e[n], g[n]), (step, n)


def test_load_state_dict_and_shape_change(dev):
    """load_state_dict of another seed's weights after the capture: the next graphed step equals an eager step on those weights.  A
    Parameter replaced by a new object releases the captured plans (the model then runs eagerly for good).  A batch of another size runs eagerly (and equals eager); the next
    batch of the captured size replays again."""
    import clc_amd
    from clc_amd.train import RateDistortionLoss

    x, refs = _inputs(dev, 2, 1)
    crit = RateDistortionLoss(LMBDA, "mse")
    m = clc_amd.graphed_training(_model(dev).eval())
    crit(m(x, refs), x)["loss"].backward()
    m.zero_grad()
    other = _model(dev, seed=1).eval()
    m.load_state_dict(other.state_dict())
    out = m(x, refs)
    assert _is_graphed(out["x_hat"])
    lg = crit(out, x)["loss"]
    lg.backward()
    le = crit(other(x, refs), x)["loss"]
    le.backward()
    assert torch.equal(lg.detach(), le.detach())
    po = dict(other.named_parameters())
    for n, p in m.named_parameters():
        assert (p.grad is None) == (po[n].grad is None), n
        if p.grad is not None:
            assert torch.equal(p.grad, po[n].grad), n

    # shape change: eager for the odd batch, replay for the next full one
    x1, refs1 = x[:1].clone(), [refs[0][:1].clone()]
    o1 = m(x1, refs1)
    assert not _is_graphed(o1["x_hat"])
    e1 = other(x1, refs1)
    assert torch.equal(o1["x_hat"].detach(), e1["x_hat"].detach()) and torch.equal(o1["likelihoods"]["y"].detach(), e1["likelihoods"]["y"].detach())
    st = m._clc_graphed
    assert _is_graphed(m(x, refs)["x_hat"]) and m._clc_graphed is st

    # a Parameter replaced by another object: the plans are released before the next replay, the model runs eagerly for good (one
    # warning) and re-arming it is refused
    w = m.g_a[0].conv1.weight
    m.g_a[0].conv1.weight = torch.nn.Parameter(w.detach().clone())
    with pytest.warns(RuntimeWarning, match="runs eagerly"):
        assert not _is_graphed(m(x, refs)["x_hat"])
    assert "_clc_graphed" not in m.__dict__ and not st.plans
    with pytest.raises(RuntimeError, match="not captured a second time"):
        clc_amd.graphed_training(m)
    assert not _is_graphed(m(x, refs)["x_hat"])


def test_second_plan_and_plan_limit(dev):
    """Several signatures on one model: A is captured, B after it comes twice in a row (a second plan in the same pool, A still live),
    C twice in a row stays eager (the plan limit is reached; nothing is evicted), and A and B replay again.  Every call's loss and
    gradients equal an eager model's, bit for bit."""
    import clc_amd
    from clc_amd import graphed
    from clc_amd.train import RateDistortionLoss

    assert graphed.MAX_PLANS == 2
    crit = RateDistortionLoss(LMBDA, "mse")
    xs = {b: _inputs(dev, b, 1, seed=100 + b) for b in (1, 2, 4)}
    m = clc_amd.graphed_training(_model(dev).eval())
    e = _model(dev).eval()
    for b, want in ((2, True), (1, False), (1, True), (4, False), (4, False), (2, True), (1, True)):
        x, refs = xs[b]
        m.zero_grad()
        e.zero_grad()
        out = m(x, refs)
        assert _is_graphed(out["x_hat"]) == want, (b, want)
        lg = crit(out, x)["loss"]
        lg.backward()
        le = crit(e(x, refs), x)["loss"]
        le.backward()
        assert torch.equal(lg.detach(), le.detach()), b
        pe = dict(e.named_parameters())
        for n, p in m.named_parameters():
            assert (p.grad is None) == (pe[n].grad is None), (b, n)
            if p.grad is not None:
                assert torch.equal(p.grad, pe[n].grad), (b, n)
    assert len(m._clc_graphed.plans) == 2
    # each plan owns its image set: distinct sets, disjoint buffers, and nothing of either on the model's Parameters
    a, b = (pl.images for pl in m._clc_graphed.plans.values())
    assert a is not b and a.map is not b.map and a.count("wt") > 0 and b.count("wt") > 0
    spans = sorted((part.buf.data_ptr(), part.buf.data_ptr() + 4 * part.buf.numel()) for im in (a, b) for part in im.parts if part.n)
    assert len(spans) >= 4 and all(s0[1] <= s1[0] for s0, s1 in zip(spans, spans[1:])), spans
    for p in m.parameters():
        assert {k for k in p.__dict__ if k.startswith("_clc_")} <= {"_clc_is_filter", "_clc_direct"}


def test_noise_is_fresh_per_replay(dev):
    """Training mode (noise proxy), lr = 0: two consecutive graphed forwards of the same input draw different noise."""
    import clc_amd
    from clc_amd.train import RateDistortionLoss

    x, refs = _inputs(dev, 2, 1)
    m = clc_amd.graphed_training(_model(dev).train())
    opt = torch.optim.AdamW(m.parameters(), lr=0.0, weight_decay=0.0)
    liks = []
    for _ in range(3):
        opt.zero_grad()
        out = m(x, refs)
        assert _is_graphed(out["x_hat"])
        RateDistortionLoss(LMBDA, "mse")(out, x)["loss"].backward()
        opt.step()
        liks.append(out["likelihoods"]["y"].detach().clone())
    assert all(torch.isfinite(t).all() for t in liks)
    assert not torch.equal(liks[1], liks[2]) and not torch.equal(liks[0], liks[1])


def test_off_by_default_and_eval_untouched(dev):
    """Switch off (the default): the forward dispatches to the eager body (`_forward_eager`, the previous forward moved without edits) and
    builds no graphed node or capture state.  Switch on: an eval / no_grad forward is identical to the switch-off one and never captures."""
    import clc_amd
    from clc_amd import graphed

    assert graphed.GRAPH_TRAIN is False
    x, refs = _inputs(dev, 2, 1)
    m = _model(dev).eval()
    a = m(x, refs)
    b = m._forward_eager(x, refs)
    assert not _is_graphed(a["x_hat"]) and "_clc_graphed" not in m.__dict__
    for k in ("x_hat",):
        assert torch.equal(a[k].detach(), b[k].detach())
    assert torch.equal(a["likelihoods"]["y"].detach(), b["likelihoods"]["y"].detach())
    with torch.no_grad():
        off = m(x, refs)
        clc_amd.graphed_training(m)
        on = m(x, refs)
    assert "_clc_graphed" not in m.__dict__
    assert torch.equal(off["x_hat"], on["x_hat"]) and torch.equal(off["likelihoods"]["y"], on["likelihoods"]["y"])
    assert torch.equal(off["likelihoods"]["z"], on["likelihoods"]["z"])
