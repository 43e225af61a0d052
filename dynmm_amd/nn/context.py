"""Context modules (context_modules.py:16-131): pyramid pooling (PPM) and adaptive pyramid pooling (APPM), their branches
resized back to the input size with 'nearest' or 'bilinear' (align_corners=False) interpolation."""
import torch.nn as nn

from .. import ops
from .blocks import ConvBNAct

CONTEXT_UPSAMPLING = ('nearest', 'bilinear')


def _check_mode(mode):
    if mode not in CONTEXT_UPSAMPLING:
        raise NotImplementedError('For the PyramidPoolingModule only nearest and bilinear interpolation are supported. '
                                  f'Got: {mode}')


class PyramidPoolingModule(nn.Module):
    def __init__(self, in_dim, out_dim, bins=(1, 5), upsampling_mode='nearest', activation='relu'):
        super().__init__()
        _check_mode(upsampling_mode)
        self.bins = tuple(bins)
        self.upsampling_mode = upsampling_mode
        red = in_dim // len(bins)
        # index 0 of each branch is the parameter-free adaptive pool of the reference Sequential
        self.features = nn.ModuleList([nn.Sequential(nn.Identity(), ConvBNAct(in_dim, red, 1, activation)) for _ in bins])
        self.final_conv = ConvBNAct(in_dim + red * len(bins), out_dim, 1, activation)

    def forward(self, x):
        branches = [f[1](ops.adaptive_avg_pool(x, b)) for f, b in zip(self.features, self.bins)]
        return self.final_conv(ops.resize_concat(x, *branches, mode=self.upsampling_mode))


class AdaptivePyramidPoolingModule(nn.Module):
    """context_modules.py:90-131: the bins scale with the input — each branch pools to bin * int(h / h_inp + 0.5) (per
    axis), for input_size = (height // 32, width // 32).  state_dict: features.i.conv.* (PPM: features.i.1.conv.*)."""

    def __init__(self, in_dim, out_dim, input_size, bins=(1, 2, 3, 6), upsampling_mode='bilinear', activation='relu'):
        super().__init__()
        _check_mode(upsampling_mode)
        self.bins = tuple(bins)
        self.input_size = tuple(input_size)
        self.upsampling_mode = upsampling_mode
        red = in_dim // len(bins)
        self.features = nn.ModuleList([ConvBNAct(in_dim, red, 1, activation) for _ in bins])
        self.final_conv = ConvBNAct(in_dim + red * len(bins), out_dim, 1, activation)

    def forward(self, x):
        h, w = x.shape[2:]
        h_inp, w_inp = self.input_size
        mh, mw = int(h / h_inp + 0.5), int(w / w_inp + 0.5)
        branches = [f(ops.adaptive_avg_pool(x, (b * mh, b * mw))) for f, b in zip(self.features, self.bins)]
        return self.final_conv(ops.resize_concat(x, *branches, mode=self.upsampling_mode))


def get_context_module(name, channels_in, channels_out, input_size=None, activation='relu', upsampling_mode='nearest'):
    """context_modules.py:16-44.  (activation: 'relu' | 'swish' | 'hswish', of every ConvBNAct in the module.
    upsampling_mode defaults to 'nearest', which is what the networks pass for the learned decoder modes.)"""
    if 'appm' in name:
        bins = (1, 2, 4, 8) if name == 'appm-1-2-4-8' else (1, 5)
        if input_size is None:
            raise ValueError('the appm context modules need input_size = (height // 32, width // 32)')
        return AdaptivePyramidPoolingModule(channels_in, channels_out, input_size, bins, upsampling_mode, activation), channels_out
    if 'ppm' in name:
        bins = (1, 2, 4, 8) if name == 'ppm-1-2-4-8' else (1, 5)
        return PyramidPoolingModule(channels_in, channels_out, bins, upsampling_mode, activation), channels_out
    return nn.Identity(), channels_in
