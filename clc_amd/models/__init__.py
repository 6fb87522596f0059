"""Drop-in for the reference's ``models`` package (/root/reference/models/__init__.py:1-2), plus the hyperprior baselines."""
from .clc import CLC, TCM  # noqa: F401
from .hyperprior import (JointAutoregressiveHierarchicalPriors, JointCheckerboardHierarchicalPriors, MeanScaleHyperprior,  # noqa: F401
                         ScaleHyperprior, ar_lanes_order, ar_schedule, ckbd_pixels)
from .elic import Elic2022, scctx_order  # noqa: F401
from .cheng import Cheng2020Anchor, Cheng2020Attention, ar_wavefront_order  # noqa: F401
from .video import ScaleSpaceFlow  # noqa: F401

__all__ = ["TCM", "CLC", "ScaleSpaceFlow","ScaleHyperprior", "MeanScaleHyperprior", "JointAutoregressiveHierarchicalPriors", "JointCheckerboardHierarchicalPriors",
           "Elic2022", "Cheng2020Anchor", "Cheng2020Attention", "ar_lanes_order", "ar_schedule", "ar_wavefront_order", "ckbd_pixels", "scctx_order"]
