"""Drop-in for the reference's ``models`` package (/root/reference/models/__init__.py:1-2), plus the hyperprior baselines."""
from .clc import CLC, TCM  # noqa: F401
from .hyperprior import JointAutoregressiveHierarchicalPriors, MeanScaleHyperprior, ScaleHyperprior, ar_schedule  # noqa: F401

__all__ = ["TCM", "CLC", "ScaleHyperprior", "MeanScaleHyperprior", "JointAutoregressiveHierarchicalPriors", "ar_schedule"]
