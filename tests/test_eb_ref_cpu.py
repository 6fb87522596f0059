"""tests/eb_ref.py checked on the CPU: the float64 specification against a .double() copy of oracle.leaves.EntropyBottleneck, the float32
oracle through every comparison of tests/test_eb_kernels_gpu.py (its figures are the reference's own float32 error, quoted in that
module's docstring), and the comparisons' eyesight against fifteen planted errors."""
import functools

import pytest
import torch

import eb_ref as R

MODES = [False, True]
MODE_IDS = ["eval", "train"]
IDS = [R.case_id(c) for c in R.CASES]
AUX_CASES = [(ps, C) for ps in ("A", "B", "C") for C in R.AUX_CS]


@functools.lru_cache(maxsize=None)
def _ref(case, training):
    """computed once, shared, never modified"""
    ps, rows, C, _ = case
    return R.reference(R.params(ps, C), R.latents(ps, rows, C), training)


@functools.lru_cache(maxsize=None)
def _aux(ps, C):
    return R.aux(R.params(ps, C))


def _same(name, a, b):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-12 * scale, (name, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("training", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_specification_is_the_oracle_in_float64(case, training):
    ps, rows, C, _ = case
    ref = _ref(case, training)
    o = R.oracle_result(R.params(ps, C), R.latents(ps, rows, C), training, R.F64)
    for k in ("raw", "lik", "dz"):
        _same(k, ref[k], o[k])
    for name, a, b in zip(R.GRAD_NAMES, ref["grads"], o["grads"]):
        _same(name, a, b)
    assert torch.equal(ref["z_hat"].double(), o["z_hat"])
    if not training:
        assert float(ref["dz"].abs().max()) == 0.0


@pytest.mark.parametrize("ps,C", AUX_CASES, ids=[f"{p}-C{c}" for p, c in AUX_CASES])
def test_aux_specification_is_the_oracle_in_float64(ps, C):
    ref, o = _aux(ps, C), R.oracle_aux(R.params(ps, C), R.F64)
    _same("per-channel loss", ref["loss"], o["loss"])
    _same("loss()", ref["loss"].sum(), o["total"])
    _same("dquantiles", ref["dq"], o["dq"])
    assert all(float(g.abs().max()) == 0.0 for g in ref["dparams"]) and all(float(g.abs().max()) == 0.0 for g in o["dparams"])


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_inputs_meet_both_conditions_and_reach_what_they_are_for(case):
    ps, rows, C, _ = case
    P, d = R.params(ps, C), R.latents(ps, rows, C)
    R.check_conditions(P, d, ps)          # every element, nothing left out
    n_ramp, huge, ties = R.layout(ps, rows)
    train, ev = _ref(case, True), _ref(case, False)
    if ps == "A" and n_ramp:              # heavy tails: the ramp never reaches the bound, only the +-1e4 row does
        assert float(train["raw"][:n_ramp].min()) > 10 * R.BOUND
    if ps == "B":                         # both arms of the LowerBound rule decide, in both modes
        for r in (train, ev):
            below = r["raw"] < R.BOUND
            assert int((below & (d["w"] > 0)).sum()) >= 8 and int((below & (d["w"] < 0)).sum()) >= 8
            assert int(((r["raw"] > R.BOUND) & (r["raw"] < 1e-6)).sum()) >= 4, "nothing just above the bound"
    if ps == "C":
        assert float(P["m"][1].max()) == 21.0 and float(P["m"][1].min()) == -30.0 and all(float(f.abs().max()) == 0.0 for f in P["f"])
        t = d["z"][ties] - P["q"][:, 0, 1][None, :]
        assert len(ties) == 12 and bool(((t - torch.floor(t)) == 0.5).all())
        k = torch.floor(t[:, 0]).long()
        assert int((k % 2 == 0).sum()) >= 4 and int((k % 2 == 1).sum()) >= 4
    if huge is not None:
        assert float(train["raw"][huge].max()) < R.BOUND and bool((d["z"][huge].abs() > 9000).all())


def _print(tag, figures):
    for k, (v, bar) in figures.items():
        print(f"{tag:34s} {k:28s} {v:10.3e}   bar {bar:.0e}")


def _f32_figures(case, training):
    ps, rows, C, _ = case
    got = R.oracle_result(R.params(ps, C), R.latents(ps, rows, C), training, R.F32)
    ref = _ref(case, training)
    fig = R.compare_forward(got, ref)
    fig.update(R.compare_backward(got, ref, training))
    return fig


@pytest.mark.parametrize("training", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_float32_oracle_is_accepted(case, training):
    fig = _f32_figures(case, training)
    _print(R.case_id(case) + (" train" if training else " eval"), fig)
    assert not R.failures(fig), R.failures(fig)


@pytest.mark.parametrize("ps,C", AUX_CASES, ids=[f"{p}-C{c}" for p, c in AUX_CASES])
def test_float32_oracle_aux_is_accepted(ps, C):
    fig = R.compare_aux(R.oracle_aux(R.params(ps, C), R.F32), _aux(ps, C))
    _print(f"aux {ps} C={C}", fig)
    assert not R.failures(fig), R.failures(fig)


def test_float32_oracle_worst_figures():
    """the table quoted in tests/test_eb_kernels_gpu.py: the worst float32-oracle figure per quantity over every case and mode (the
    largest dz figure is the single element of the 1 x 1 map, which is its own maximum)"""
    worst = {}
    for case in R.CASES:
        for training in MODES:
            for k, (v, bar) in _f32_figures(case, training).items():
                k = "parameter gradients" if k in R.GRAD_NAMES else k
                worst[k] = (max(v, worst.get(k, (0.0, bar))[0]), bar)
    for ps, C in AUX_CASES:
        for k, (v, bar) in R.compare_aux(R.oracle_aux(R.params(ps, C), R.F32), _aux(ps, C)).items():
            worst[k] = (max(v, worst.get(k, (0.0, bar))[0]), bar)
    _print("float32 oracle, worst", worst)
    for k, (v, bar) in worst.items():
        assert v <= bar, (k, v, bar)


MUTANT_CASES = [c for c in R.CASES if c[1:3] != (128, 192)]


def _kills(mutant):
    """the first (case, mode, quantity) at which the mutant's float64 result is at least 10 x over a bar, with the ratio"""
    if mutant.startswith("aux_"):
        for ps, C in AUX_CASES:
            got = R.aux(R.params(ps, C), mutant)
            for k, (v, bar) in R.compare_aux(got, _aux(ps, C)).items():
                if R.ratio(v, bar) >= 10:
                    return f"{ps}-C{C}", k, R.ratio(v, bar)
        return None
    for case in MUTANT_CASES:
        ps, rows, C, _ = case
        for training in MODES:
            got = R.reference(R.params(ps, C), R.latents(ps, rows, C), training, mutant)
            ref = _ref(case, training)
            fig = R.compare_forward(got, ref)
            fig.update(R.compare_backward(got, ref, training))
            for k, (v, bar) in fig.items():
                if R.ratio(v, bar) >= 10:
                    return R.case_id(case), "train" if training else "eval", k, R.ratio(v, bar)
    return None


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_rejected_ten_times_over(mutant):
    hit = _kills(mutant)
    print(mutant, "->", hit)
    assert hit is not None, f"{mutant} stays within 10 x every bar on every case: the inputs or the measures are too weak"


def test_the_specification_passes_its_own_comparisons_exactly():
    """the measures are zero on the specification itself (a comparison that could not return zero would hide a mutant's margin)"""
    for case in MUTANT_CASES:
        for training in MODES:
            ref = _ref(case, training)
            fig = R.compare_forward(ref, ref)
            fig.update(R.compare_backward(ref, ref, training))
            assert all(v == 0.0 for v, _ in fig.values()), fig
