"""The quantisation step without a GPU: the specification (tests/qstep_ref.py) against the unit-step definitions it must
reduce to, StepTable, the integer path through the host rANS coder, the CLVQ wrapper and every new refusal — argument checks come
before the GPU check, as in tests/test_frames_cpu.py."""
import math
import struct

import numpy as np
import pytest
import torch

import qstep_ref as R


def _latent(rows=37, C=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn((rows, C), generator=g, dtype=torch.float64) * 4
    mu = torch.randn((rows, C), generator=g, dtype=torch.float64)
    scale = torch.rand((rows, C), generator=g, dtype=torch.float64) * 3 + 0.02   # some below the bound 0.11
    noise = torch.rand((rows, C), generator=g, dtype=torch.float64) - 0.5
    return y, mu, scale, noise


# ---- the specification at step == 1 ----

@pytest.mark.parametrize("training", [False, True])
def test_unit_step_equals_unit_restatement_and_oracle_leaf(training):
    from oracle import leaves

    y, mu, scale, noise = _latent()
    one = torch.ones(y.shape[1], dtype=torch.float64)
    ins = [t.clone().requires_grad_(True) for t in (y, mu, scale)]
    lik, yh = R.forward(*ins, one, noise if training else None)
    ins1 = [t.clone().requires_grad_(True) for t in (y, mu, scale)]
    lik1, yh1 = R.unit_forward(*ins1, noise if training else None)
    assert torch.equal(lik, lik1) and torch.equal(yh, yh1)
    w = torch.linspace(-1, 1, y.numel(), dtype=torch.float64).reshape(y.shape)
    ((lik * w).sum() + (yh * w.flip(0)).sum()).backward()
    ((lik1 * w).sum() + (yh1 * w.flip(0)).sum()).backward()
    for a, b in zip(ins, ins1):
        assert torch.equal(a.grad, b.grad)
    # the oracle's leaf: likelihood of quantize("noise" / "dequantize") under LowerBound(0.11) and LowerBound(1e-9)
    gc = leaves.GaussianConditional(None).double()
    if training:
        out = y + noise
        lik_o = gc.likelihood_lower_bound(gc._likelihood(out, scale, mu))
    else:
        out, lik_o = gc(y, scale, mu, training=False)
        assert torch.equal(out, yh.detach())
    assert torch.equal(lik_o, lik.detach())


def test_step_gradient_is_the_three_paths():
    """autograd through the restatement = the closed form clc_gauss_lik_step_bwd implements (the half width, y_in, y_hat)"""
    for training in (False, True):
        y, mu, scale, noise = _latent(seed=3)
        step = torch.tensor([0.25, 1.0, 3.7, 0.5, 2.0], dtype=torch.float64, requires_grad=True)
        lik, yh = R.forward(y, mu, scale, step, noise if training else None)
        g = torch.linspace(0.5, 2, y.numel(), dtype=torch.float64).reshape(y.shape)
        gh = torch.linspace(-1, 1, y.numel(), dtype=torch.float64).reshape(y.shape)
        ((lik * g).sum() + (yh * gh).sum()).backward()
        with torch.no_grad():
            s = step.detach()
            t = (y - mu) / s
            q = torch.round(t)
            w = noise if training else q
            d = (y + s * noise - mu) if training else s * q
            sg = scale.clamp(min=R.SCALE_BOUND)
            a, b = (s / 2 - d.abs()) / sg, (-s / 2 - d.abs()) / sg
            pdf = lambda x: torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
            gate = ((R.phi(a) - R.phi(b)) >= R.LIK_BOUND) | (g < 0)
            gg = g * gate
            want = (gg * (pdf(a) + pdf(b)) / (2 * sg) + gg * (pdf(b) - pdf(a)) / sg * torch.sign(d) * w + gh * (q - t)).sum(0)
        assert torch.allclose(step.grad, want, rtol=1e-12, atol=1e-12), (step.grad, want)


# ---- StepTable ----

def test_step_table_ladder_and_interpolation():
    from clc_amd.vbr import StepTable

    t = StepTable(6)
    assert list(t.state_dict()) == ["log_step"] and t.log_step.shape == (5, 6) and t.log_step.dtype == torch.float32
    want = torch.tensor(R.ladder(), dtype=torch.float64).float()
    assert torch.equal(t.log_step.detach(), want.reshape(5, 1).expand(5, 6))
    assert float(t.log_step.detach()[2, 0]) == 0.0
    one = t(2.0)
    assert one.dtype == torch.float32 and one.shape == (6,) and torch.equal(one, torch.ones(6))   # exactly 1.0 at the middle level
    assert torch.equal(t(2), one)
    for q, s in ((0.0, 2.0), (4.0, 0.5), (1.0, math.sqrt(2.0)), (3.0, math.sqrt(0.5))):
        assert torch.allclose(t(q).double(), torch.full((6,), s, dtype=torch.float64), rtol=2e-7)
    steps = [float(t(q).detach()[0]) for q in t.candidates(16)]
    assert len(steps) == 16 and all(a > b for a, b in zip(steps, steps[1:])) and steps[0] == 2.0 and steps[-1] == 0.5
    with torch.no_grad():
        t.log_step[1].copy_(torch.linspace(-0.3, 0.4, 6))
        t.log_step[2].copy_(torch.linspace(0.2, -0.5, 6))
    for q in (1.0, 1.25, 1.5, 2.0):
        assert torch.equal(t(q), R.step_of(t.log_step.detach(), q))
    f = 0.25
    want = torch.exp(0.75 * t.log_step[1].double() + f * t.log_step[2].double()).float()
    assert torch.equal(t(1.25).detach(), want.detach())
    # two tables from the same parameters give the same bits
    u = StepTable(6)
    u.load_state_dict(t.state_dict())
    assert torch.equal(u(1.7), t(1.7))


def test_step_table_clamp_and_refusals():
    from clc_amd.vbr import StepTable

    t = StepTable(3, levels=2, coarsest=16.0, finest=1.0 / 16)
    with torch.no_grad():
        t.log_step[0].fill_(5.0)
        t.log_step[1].fill_(-5.0)
    assert torch.equal(t(0.0), torch.full((3,), 16.0)) and torch.equal(t(1.0), torch.full((3,), 1.0 / 16))
    assert StepTable(3, levels=1)(0.0).shape == (3,)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"q must be in \[0, 1\]"):
            t(bad)
    for bad in ("1", None, True, torch.tensor(1.0)):
        with pytest.raises(TypeError, match="q must be a Python float"):
            t(bad)
    with pytest.raises(ValueError, match="channels and levels must be positive"):
        StepTable(0)
    with pytest.raises(ValueError, match="finest <= coarsest"):
        StepTable(3, coarsest=0.5, finest=2.0)
    with pytest.raises(ValueError, match="finest <= coarsest"):
        StepTable(3, coarsest=32.0)


def test_step_table_gradient_against_finite_differences():
    from clc_amd.vbr import StepTable

    t = StepTable(4, levels=3).double()
    with torch.no_grad():
        t.log_step.copy_(torch.randn(3, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 0.3)
    w = torch.tensor([1.0, -2.0, 0.5, 3.0], dtype=torch.float64)

    def value(ls, q):   # the float64 expression before its single rounding to f32
        i = int(math.floor(q))
        f = q - i
        return (torch.exp((1 - f) * ls[i] + f * ls[min(i + 1, 2)]) * w).sum()

    for q in (0.0, 0.3, 1.0, 1.75, 2.0):
        t.log_step.grad = None
        (t(q).double() * w).sum().backward()
        grad = t.log_step.grad.clone()
        fd = torch.zeros_like(grad)
        eps = 1e-6
        for i in range(3):
            for c in range(4):
                lo, hi = t.log_step.detach().clone(), t.log_step.detach().clone()
                lo[i, c] -= eps
                hi[i, c] += eps
                fd[i, c] = (value(hi, q) - value(lo, q)) / (2 * eps)
        # backward passes through the f32 rounding as the identity; forward's own value was rounded, the derivative is float64's
        assert torch.allclose(grad, fd, rtol=1e-6, atol=1e-8), (q, grad, fd)


# ---- the integer path through the host coder ----

@pytest.fixture(scope="module")
def tables():
    from clc_amd.entropy_models import GaussianConditional
    from clc_amd.models.clc import get_scale_table

    gc = GaussianConditional(None)
    gc.update_scale_table(get_scale_table())
    return gc.host_tables(), gc.scale_table.numpy().astype(np.float32)


@pytest.mark.parametrize("s", [0.5, 3.0])
def test_round_trip_through_the_host_coder(tables, s):
    from clc_amd import ans

    (cdf, ln, off), table = tables
    rng = np.random.default_rng(7)
    rows, C = 64, 6
    mu = rng.normal(size=(rows, C)).astype(np.float32)
    scale = (rng.random((rows, C)) * 4 + 0.02).astype(np.float32)
    y = (mu + rng.normal(size=(rows, C)) * scale * 1.5).astype(np.float32)
    y[::7, 0] += 400.0     # far outside the support of its row: the escape path
    y[3::11, 1] -= 900.0
    scale[::7, 0] = 0.05
    step = np.full(C, s, np.float32)
    step[1] = np.float32(s * 1.25)
    sym, idx, y_hat = R.integer_path(y, mu, scale, step, table)
    width = ln[idx] - 2    # symbols of the row: offset .. offset + width - 1 in the table, the rest escape
    assert ((sym < off[idx]) | (sym >= off[idx] + width)).sum() >= 10, "the case must leave the table's support"
    stream = ans.encode(sym.reshape(-1), idx.reshape(-1), cdf, ln, off)
    _, idx_dec, _ = R.integer_path(scale, np.zeros_like(scale), scale, step, table)   # the decoder knows the scales only
    assert np.array_equal(idx_dec, idx)
    back = ans.decode(stream, idx_dec.reshape(-1), cdf, ln, off).reshape(rows, C)
    assert np.array_equal(back, sym)
    assert np.array_equal(R.dequantise(back, mu, step).view(np.uint32), y_hat.view(np.uint32))
    assert np.all(np.abs(y_hat - y) <= 0.5 * step * (1 + 1e-6) + 1e-4)
    # a finer step codes more bytes
    coarse = R.integer_path(y, mu, scale, step * 4, table)
    assert len(ans.encode(coarse[0].reshape(-1), coarse[1].reshape(-1), cdf, ln, off)) < len(stream)


def test_integer_path_unit_step_is_the_unit_expression(tables):
    _, table = tables
    rng = np.random.default_rng(2)
    y, mu = rng.normal(size=(50, 3)).astype(np.float32) * 5, rng.normal(size=(50, 3)).astype(np.float32)
    scale = (rng.random((50, 3)) * 300).astype(np.float32)
    scale[0, 0], scale[1, 0] = 0.01, 1000.0
    sym, idx, y_hat = R.integer_path(y, mu, scale, np.ones(3, np.float32), table)
    q = np.rint(y - mu)
    assert np.array_equal(sym, q.astype(np.int32)) and np.array_equal(y_hat, (q + mu).astype(np.float32))
    assert np.array_equal(idx, R.scale_index(np.maximum(scale, np.float32(0.11)), table))
    assert idx.min() == 0 and idx.max() == len(table) - 1


# ---- the CLVQ wrapper ----

def _clv1(frames=3):
    from clc_amd import codec

    strings = [[[b"ky"], [b"kz"]]] + [{"motion": [[b"my%d" % t], [b"mz"]], "residual": [[b"ry"], [b"rz"]]} for t in range(1, frames)]
    shape = torch.Size([1, 1])
    infos = [shape] + [{"motion": shape, "residual": shape} for _ in range(1, frames)]
    return codec.pack_sequence(strings, infos, lanes=None, image_hw=(100, 120))


def test_clvq_round_trip_and_refusals():
    from clc_amd import codec

    inner = _clv1()
    qs = [3.0, 1.5, 0.25]
    blob = codec.pack_sequence_q(inner, qs)
    assert blob[:4] == b"CLVQ" and struct.unpack("<H", blob[4:6])[0] == 3 and blob[18:] == inner
    got, got_q = codec.unpack_sequence_q(blob)
    assert got == inner and got_q == qs
    assert codec.unpack_sequence(got)[2]["frames"] == 3
    with pytest.raises(ValueError, match="wrong magic"):   # a reader without qualities refuses the wrapper
        codec.unpack_sequence(blob)
    with pytest.raises(ValueError, match="unpack_sequence_q: wrong magic"):
        codec.unpack_sequence_q(inner)
    with pytest.raises(ValueError, match="unpack_sequence_q: wrong magic"):
        codec.unpack_sequence_q(b"CL")
    with pytest.raises(ValueError, match="cut short"):
        codec.unpack_sequence_q(blob[:5])
    with pytest.raises(ValueError, match="cut short"):
        codec.unpack_sequence_q(blob[:20])
    with pytest.raises(ValueError, match="wrong inner magic"):
        codec.unpack_sequence_q(blob[:18] + b"XXXX" + blob[22:])
    two = b"CLVQ" + struct.pack("<H2f", 2, 1.0, 2.0) + inner
    with pytest.raises(ValueError, match="frame count 2 disagrees with the inner header's 3"):
        codec.unpack_sequence_q(two)
    nan = b"CLVQ" + struct.pack("<H3f", 3, 1.0, float("nan"), 2.0) + inner
    with pytest.raises(ValueError, match="non-finite q"):
        codec.unpack_sequence_q(nan)
    with pytest.raises(ValueError, match="cut short"):   # the inner container's own check still runs
        codec.unpack_sequence(codec.unpack_sequence_q(blob[:-1])[0])
    with pytest.raises(ValueError, match="2 qualities for the 3 frames"):
        codec.pack_sequence_q(inner, [1.0, 2.0])
    with pytest.raises(ValueError, match="non-finite q"):
        codec.pack_sequence_q(inner, [1.0, float("inf"), 2.0])
    with pytest.raises(ValueError, match="not a whole"):
        codec.pack_sequence_q(b"nope", [1.0])


# ---- refusals: arguments first, the GPU check after them ----

def test_ops_refuse_bad_steps_before_the_gpu_check():
    from clc_amd import ops

    y = torch.zeros(1, 4, 2, 2)
    table = torch.tensor([0.11, 1.0, 2.0])
    calls = {
        "gaussian_likelihood_step": lambda s: ops.gaussian_likelihood_step(y, y, y, s, None, False),
        "quantize_build_indexes_step": lambda s: ops.quantize_build_indexes_step(y, y, y, table, s),
    }
    for who, call in calls.items():
        with pytest.raises(TypeError, match=f"{who}: step must be a tensor"):
            call(1.0)
        with pytest.raises(ValueError, match=rf"{who}: step must have shape \[4\]"):
            call(torch.ones(3))
        with pytest.raises(ValueError, match=rf"{who}: step must have shape \[4\]"):
            call(torch.ones(1, 4))
        with pytest.raises(ValueError, match=f"{who}: step must be float32"):
            call(torch.ones(4, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"gauss_rate_sweep: steps must be a \[K, C\] tensor"):
        ops.gauss_rate_sweep(y, y, y, torch.ones(4))
    with pytest.raises(ValueError, match="between 1 and 16 candidates"):
        ops.gauss_rate_sweep(y, y, y, torch.ones(17, 4))
    with pytest.raises(ValueError, match="between 1 and 16 candidates"):
        ops.gauss_rate_sweep(y, y, y, torch.ones(0, 4))
    with pytest.raises(ValueError, match=r"steps must have shape \[2, 4\]"):
        ops.gauss_rate_sweep(y, y, y, torch.ones(2, 5))
    if not torch.cuda.is_available():   # well-formed arguments reach the GPU check
        from clc_amd.lib import ClcError

        with pytest.raises(ClcError, match="GPU only"):
            ops.gauss_rate_sweep(y, y, y, torch.ones(2, 4))
        with pytest.raises(ClcError, match="GPU only"):
            ops.gaussian_likelihood_step(y, y, y, torch.ones(4), None, False)


def test_models_refuse_the_new_arguments_by_name():
    from clc_amd import codec, models

    x = torch.zeros(1, 3, 64, 64)
    fixed = models.ScaleHyperprior(12, 24)
    assert not any("step" in k for k in fixed.state_dict())
    assert sorted(fixed.state_dict()) == sorted(models.ScaleHyperprior(12, 24, rate_levels=0).state_dict())
    for call in (lambda: fixed(x, q=1.0), lambda: fixed.compress(x, q=1.0), lambda: fixed.decompress([[b""], [b""]], (1, 1), q=1.0)):
        with pytest.raises(ValueError, match="needs a step table .* rate_levels > 0"):
            call()
    vbr = models.MeanScaleHyperprior(12, 24, rate_levels=3)
    assert [k for k in vbr.state_dict() if "step" in k] == ["y_step.log_step"] and vbr.y_step.log_step.shape == (3, 24)
    assert set(vbr.state_dict()) - set(models.MeanScaleHyperprior(12, 24).state_dict()) == {"y_step.log_step"}
    for bad in (-1.0, 2.5, float("nan")):
        with pytest.raises(ValueError, match=r"MeanScaleHyperprior.forward: q must be in \[0, 2\]"):
            vbr(x, q=bad)
    with pytest.raises(TypeError, match="MeanScaleHyperprior.compress: q must be a Python float"):
        vbr.compress(x, q="2")
    with pytest.raises(ValueError, match="q and target_bytes exclude each other"):
        vbr.compress(x, q=1.0, target_bytes=100)
    with pytest.raises(ValueError, match="rate_levels must not be negative"):
        models.ScaleHyperprior(12, 24, rate_levels=-1)
    # the families outside the feature's scope.  Where a method simply has no such parameter the refusal is Python's own
    # unexpected-keyword TypeError, provoked on the unbound method: no project code runs, and what it pins is the signature — a
    # later **kwargs that swallowed q or target_bytes would be caught here.
    for cls in (models.JointAutoregressiveHierarchicalPriors, models.JointCheckerboardHierarchicalPriors):
        with pytest.raises(ValueError, match=f"{cls.__name__} has no quantisation-step table: rate_levels"):
            cls(N=12, M=24, rate_levels=3)
        with pytest.raises(TypeError, match="'q'"):
            cls.compress(None, x, q=1.0)
        with pytest.raises(TypeError, match="'q'"):
            cls.forward(None, x, q=1.0)
    with pytest.raises(ValueError, match="has no quantisation-step table: rate_levels"):
        models.Cheng2020Anchor(N=12, rate_levels=3)
    with pytest.raises(ValueError, match="Elic2022 has no quantisation-step table: rate_levels"):
        models.Elic2022(rate_levels=3)
    for cls in (models.CLC, models.TCM):
        with pytest.raises(ValueError, match=f"{cls.__name__} has no quantisation-step table: rate_levels"):
            cls(N=64, rate_levels=3)
    # the video model: q before anything else
    frames3 = [torch.zeros(1, 3, 128, 128)] * 3
    ssf = models.ScaleSpaceFlow(mid_planes=8, planes=8)
    assert not any("step" in k for k in ssf.state_dict())
    for call in (lambda: ssf(frames3, q=1.0), lambda: ssf.compress(frames3, q=[1.0, 1.0, 1.0]), lambda: ssf.decompress([None] * 3, [None] * 3, q=1.0)):
        with pytest.raises(ValueError, match=r"ScaleSpaceFlow\.\w+ \(frame 0\): q=1.0 needs a step table"):
            call()
    ssf = models.ScaleSpaceFlow(mid_planes=8, planes=8, rate_levels=4)
    assert sorted(k for k in ssf.state_dict() if "step" in k) == [f"{h}_hyperprior.y_step.log_step" for h in ("img", "motion", "res")]
    with pytest.raises(ValueError, match=r"ScaleSpaceFlow.compress: q lists 2 qualities for 3 frames"):
        ssf.compress(frames3, q=[1.0, 2.0])
    with pytest.raises(ValueError, match=r"ScaleSpaceFlow.forward \(frame 1\): q must be in \[0, 3\]"):
        ssf(frames3, q=[1.0, 3.5, 2.0])
    with pytest.raises(TypeError, match=r"ScaleSpaceFlow.decompress \(frame 2\): q must be a Python float"):
        ssf.decompress([None] * 3, [None] * 3, q=[1.0, 1.0, "x"])
    with pytest.raises(ValueError, match="Hyperprior.compress: q=0.5 needs a step table"):
        models.ScaleSpaceFlow(mid_planes=8, planes=8).img_hyperprior.compress(torch.zeros(1, 8, 8, 8), q=0.5)
    with pytest.raises(ValueError, match="rate_levels must not be negative"):
        models.ScaleSpaceFlow(mid_planes=8, planes=8, rate_levels=-2)
    for eng in (codec.CodecEngine, codec.ContextCodecEngine):
        with pytest.raises(TypeError, match="'q'"):
            eng.compress(None, x, q=1.0)
        with pytest.raises(TypeError, match="'target_bytes'"):
            eng.compress(None, x, target_bytes=100)


def test_target_bytes_is_checked_before_any_launch():
    from clc_amd import models

    m = models.ScaleHyperprior(12, 24, rate_levels=3)
    x = torch.zeros(1, 3, 64, 64)
    for bad in (0, -5, 10.5, True, "9"):
        with pytest.raises(ValueError, match="target_bytes must be a positive int"):
            m.compress(x, target_bytes=bad)
    with pytest.raises(ValueError, match="target_bytes=100 needs a step table"):
        models.ScaleHyperprior(12, 24).compress(x, target_bytes=100)
