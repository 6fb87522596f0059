"""Trainable Conditional Latent Matching, the part that needs no GPU: the C ABI of the recorded forward / backward ops, the loud
failure of a recording call on CPU tensors, and the integer plan of the deform scatter's workspace."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["clc_clm_sim_colsum_train", "clc_clm_sim_colsum_bwd_workspace_bytes", "clc_clm_sim_colsum_bwd", "clc_clm_sigmoid",
               "clc_clm_scale_rows_bwd", "clc_clm_deform_bwd_workspace_bytes", "clc_clm_deform_bwd", "clc_clm_fuse_bwd"]


def test_new_clm_symbols_declared_exported_and_bound():
    from clc_amd import lib

    header = open(os.path.join(ROOT, "include", "clc_hip.h")).read()
    L = lib.load()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/clc_hip.h"
        assert hasattr(L, n), f"{n} is not exported by libclc_hip.so"
        assert n in lib.SIGNATURES, f"{n} has no ctypes signature"


def test_workspace_sizes():
    """similarity backward: D only, O(B*HW) — never the [HW x HW] matrix; deform scatter: two counter arrays, the bucket starts (padded to
    16 bytes) and two (id, coefficient) lists of at most 36 entries per pixel (9 taps x 4 corners)."""
    from clc_amd import lib

    L = lib.load()
    for B, HW in ((1, 1), (2, 256), (8, 4096), (3, 768)):
        assert L.clc_clm_sim_colsum_bwd_workspace_bytes(B, HW) == 4 * B * HW
    for B, H, W in ((1, 1, 1), (2, 16, 16), (1, 17, 19), (3, 32, 24), (8, 64, 64)):
        n = B * H * W
        ints = 2 * n + (n + 1 + 3) // 4 * 4 + 2 * 36 * n
        assert L.clc_clm_deform_bwd_workspace_bytes(B, H, W) == 4 * (ints + 2 * 36 * n)


@pytest.mark.parametrize("kind", ["CLM", "SimpleCLM"])
def test_recording_call_on_cpu_tensors_raises(kind):
    from clc_amd import clm, lib

    m = getattr(clm, kind)(8, 0.5)
    y = torch.randn(1, 8, 4, 4, requires_grad=True)
    with pytest.raises(lib.ClcError):
        m(y, [torch.randn(1, 8, 4, 4)])
    with pytest.raises(lib.ClcError):
        clm.sim_colsum(y, torch.randn(1, 8, 4, 4), 0.5)


def test_state_dict_keeps_reference_shapes():
    """the recorded path pads the 18 / 9 / 1-channel heads inside the call; the parameters keep the reference's names and shapes"""
    from clc_amd import clm
    from oracle import clm as oc

    for kind in ("CLM", "SimpleCLM"):
        a, b = getattr(clm, kind)(16, 0.5).state_dict(), getattr(oc, kind)(16, 0.5).state_dict()
        assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    w, bias = clm._pad_rows(clm.CLM(16).alignment.offset_conv, 20)
    assert tuple(w.shape) == (20, 32, 3, 3) and tuple(bias.shape) == (20,) and float(w.detach()[18:].abs().max()) == 0.0 and float(bias.detach()[18:].abs().max()) == 0.0
