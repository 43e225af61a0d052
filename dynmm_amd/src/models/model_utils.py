"""Counterpart of FusionDynMM/src/models/model_utils.py."""
import torch.nn as nn

from ... import ops
from ...nn.blocks import ConvBNAct  # noqa: F401
from ...nn.fusion import SqueezeAndExcitation  # noqa: F401


def swish(x):
    """x * sigmoid(x) (model_utils.py:100-101), on the HIP pointwise kernels (ops.activation)."""
    return ops.activation(x, 'swish')


class Swish(nn.Module):
    """model_utils.py:104-106"""

    def forward(self, x):
        return ops.activation(x, 'swish')


class Hswish(nn.Module):
    """x * relu6(x + 3) / 6 (model_utils.py:109-115; the `inplace` flag only concerns the reference's relu6)."""

    def __init__(self, inplace=True):
        super().__init__()
        self.inplace = inplace

    def forward(self, x):
        return ops.activation(x, 'hswish')
