"""CPU restatement of the ESANet family with an `activation` argument.  *** TEST INFRASTRUCTURE — NOT PRODUCT CODE. ***

Plain torch.nn.functional on the CPU, float32 or float64 (the dtype follows the tensors handed in), no project ops.

The reference builds ONE activation module per network and uses it at every site where oracle/dynmm_oracle.py writes `F.relu`
(FusionDynMM/src/models/model.py:46-56: stems, every residual block, ConvBNAct, the SE hidden layers and
SqueezeAndExcitationWeight); tanh (global gate) and the sigmoids are written as `torch.tanh` / `torch.sigmoid` there and stay.
So the oracle's functions are reused unedited: `oracle(activation)` executes that file into a PRIVATE module object whose name
`F` resolves to torch.nn.functional with `relu` replaced by the chosen activation.  oracle.dynmm_oracle itself (the module every
other test imports) is not touched.  Pinned against fixtures made by the reference itself: tests/test_activations.py.
"""
import importlib.util
import os
import types

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIVATIONS = ('relu', 'swish', 'hswish')


def swish(x, inplace=False):
    """model_utils.py:100-101"""
    return x * torch.sigmoid(x)


def hswish(x, inplace=False):
    """model_utils.py:109-115: x * relu6(x + 3) / 6, in that order"""
    return x * F.relu6(x + 3.) / 6.


def act_fn(activation):
    return {'relu': F.relu, 'swish': swish, 'hswish': hswish, None: lambda x: x, 'tanh': torch.tanh}[activation]


def act_grad(z, activation):
    """d act / dz, closed form.  Hswish: torch's convention — the hardtanh gradient mask of relu6 is strict (0 < z + 3 < 6), so
    the derivative is 1 at exactly z = 3 and 0 at exactly z = -3."""
    if activation == 'swish':
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if activation == 'hswish':
        mid = (2 * z + 3) / 6
        return torch.where(z <= -3, torch.zeros_like(z), torch.where(z < 3, mid, torch.ones_like(z)))
    if activation == 'relu':
        return (z > 0).to(z.dtype)
    raise KeyError(activation)


_CACHE = {}
PROBES = None          # a list while record_preacts() is active: the argument of every activation site, in call order


class record_preacts:
    """Collect the pre-activation of every activation site the restatement evaluates (the Hswish kink rule of the tests)."""

    def __enter__(self):
        global PROBES
        PROBES = []
        return PROBES

    def __exit__(self, *a):
        global PROBES
        PROBES = None


def _site(base):
    def site(z, inplace=False):
        if PROBES is not None:
            PROBES.append(z.detach())
        return base(z)
    return site


def oracle(activation):
    """oracle/dynmm_oracle.py with `activation` at every activation site (see the module docstring)."""
    if activation not in ACTIVATIONS:
        raise KeyError(activation)
    if activation not in _CACHE:
        spec = importlib.util.spec_from_file_location(f'_dynmm_oracle_{activation}', os.path.join(REPO, 'oracle', 'dynmm_oracle.py'))
        mod = importlib.util.module_from_spec(spec)
        import sys
        sys.modules[spec.name] = mod                 # (dataclasses looks its module up while the file executes)
        spec.loader.exec_module(mod)
        fn = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith('__')})
        fn.relu = _site(act_fn(activation))
        mod.F = fn
        _CACHE[activation] = mod
    return _CACHE[activation]


# ---- pieces the oracle file does not have ------------------------------------------------------------------------------------
def adaptive_pyramid_pooling(sd, p, x, training, activation, input_size, bins=(1, 5), mode='nearest'):
    """AdaptivePyramidPoolingModule.forward (context_modules.py:90-131): bins scale with the input."""
    O = oracle(activation)
    h, w = x.shape[2:]
    mh, mw = int(h / input_size[0] + 0.5), int(w / input_size[1] + 0.5)
    outs = [x]
    for i, b in enumerate(bins):
        y = O.conv_bn_act(sd, f'{p}.features.{i}', F.adaptive_avg_pool2d(x, (b * mh, b * mw)), training)
        outs.append(F.interpolate(y, (h, w), mode=mode, **({} if mode == 'nearest' else {'align_corners': False})))
    return O.conv_bn_act(sd, p + '.final_conv', torch.cat(outs, 1), training)


def se_fuse_blend(params8, rgb, depth, activation, wc=None):
    """wc * rgb + (1 - wc) * (SE_rgb(rgb) + SE_depth(depth)) from the eight excitation tensors (ops.se_fuse_blend's contract)."""
    act = _site(act_fn(activation))

    def se(x, w1, b1, w2, b2):
        s = F.adaptive_avg_pool2d(x, 1)
        s = torch.sigmoid(F.conv2d(act(F.conv2d(s, w1, b1)), w2, b2))
        return x * s
    fused = se(rgb, *params8[:4]) + se(depth, *params8[4:])
    if wc is None:
        return fused
    w = wc.view(-1, 1, 1, 1)
    return w * rgb + (1 - w) * fused
