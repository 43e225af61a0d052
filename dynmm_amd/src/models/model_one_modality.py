"""Counterpart of FusionDynMM/src/models/model_one_modality.py: the RGB-only / depth-only ESANet."""
from ...nn.esanet import ESANetOneModality  # noqa: F401
