"""Counterpart of FusionDynMM/src/models/context_modules.py."""
from ...nn.context import AdaptivePyramidPoolingModule, PyramidPoolingModule, get_context_module  # noqa: F401
