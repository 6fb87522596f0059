"""Host logic of clc_amd.graphed (no device): the CLC_GRAPH_TRAIN switch, the capture signature, and the TrainEngine claim."""
import pytest
import torch

from clc_amd import graphed


def test_env_parsing():
    for v in ("1", "true", "ON", " yes "):
        assert graphed.parse_env(v) is True
    for v in (None, "", "0", "false", "Off", "no"):
        assert graphed.parse_env(v) is False
    with pytest.raises(ValueError, match="CLC_GRAPH_TRAIN"):
        graphed.parse_env("2")


def test_switch_defaults_off(monkeypatch):
    monkeypatch.setattr(graphed, "GRAPH_TRAIN", False)
    m = torch.nn.Linear(2, 2)
    assert not graphed.is_enabled(m)
    assert graphed.graphed_training(m) is m and graphed.is_enabled(m)
    graphed.graphed_training(m, False)
    assert not graphed.is_enabled(m)
    monkeypatch.setattr(graphed, "GRAPH_TRAIN", True)   # the environment turns it on for models left at the default ...
    assert graphed.is_enabled(torch.nn.Linear(2, 2))
    assert not graphed.is_enabled(m)                    # ... not for one switched off explicitly


class _Model(torch.nn.Module):
    """the attributes signature() reads, on a stand-in"""

    def __init__(self):
        super().__init__()
        self.gaussian_conditional = torch.nn.Identity()
        self.entropy_bottleneck = torch.nn.Identity()
        self.max_support_slices, self.use_ref = 5, True


def test_signature():
    m = _Model()
    ks = (1, 2, (0,))
    x, r = torch.zeros(2, 3, 8, 8), [torch.zeros(2, 3, 8, 8)]
    base = graphed.signature(m, x, r, kstate=ks)
    assert graphed.signature(m, x.clone(), [r[0].clone()], kstate=ks) == base        # values do not matter, shapes do
    assert graphed.signature(m, x[:1], [r[0][:1]], kstate=ks) != base                # batch size
    assert graphed.signature(m, x, r + r, kstate=ks) != base                         # reference count
    assert graphed.signature(m, x, None, kstate=ks) != base
    assert graphed.signature(m, x, r, kstate=(1, 3, (0,))) != base                   # kernel configuration (precision, tuning)
    m.eval()
    assert graphed.signature(m, x, r, kstate=ks) != base                             # train / eval
    m.train()
    m.gaussian_conditional.eval()
    assert graphed.signature(m, x, r, kstate=ks) != base                             # the noise proxy of one entropy model
    m.gaussian_conditional.train()
    m._lean_outputs = True
    assert graphed.signature(m, x, r, kstate=ks) != base                             # output set
    m._lean_outputs = False
    assert graphed.signature(m, x, r, kstate=ks) == base


def test_train_engine_claims_the_model():
    """A model handed to a TrainEngine is refused by graphed_training, and its forwards step aside to eager."""
    from clc_amd.train import TrainEngine

    m = torch.nn.Linear(2, 2)
    eng = TrainEngine(m, lmbda=0.0067, criterion=lambda out, x: {"loss": out.sum()}, use_graph=False)
    assert graphed.owner(m) is eng
    with pytest.raises(RuntimeError, match="TrainEngine"):
        graphed.graphed_training(m)
    assert graphed.forward(m, torch.zeros(1, 2), None) is None
    del eng
    import gc

    gc.collect()
    assert graphed.owner(m) is None            # the claim goes with the engine
    graphed.graphed_training(m)


def test_steps_aside_without_grad_or_gpu():
    m = graphed.graphed_training(torch.nn.Linear(2, 2))
    assert graphed.forward(m, torch.zeros(1, 2), None) is None            # a CPU tensor: eager (which refuses it on its own terms)
    with torch.no_grad():
        assert graphed.forward(m, torch.zeros(1, 2), None) is None


def test_released_model_is_not_captured_again():
    """Once a model's plans were released (a replaced parameter, a TrainEngine taking over) it runs eagerly for good, with one warning,
    and graphed_training refuses to switch it on again."""
    m = graphed.graphed_training(torch.nn.Linear(2, 2))
    with pytest.warns(RuntimeWarning, match="runs eagerly"):
        graphed.drop(m, "a parameter was replaced")
    with pytest.raises(RuntimeError, match="not captured a second time"):
        graphed.graphed_training(m)
    graphed.graphed_training(m, False)          # switching off stays allowed
    assert graphed.forward(m, torch.zeros(1, 2), None) is None
