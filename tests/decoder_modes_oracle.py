"""fp64 restatement of the decoder variants (FusionDynMM/src/models/model.py:311-410, context_modules.py:47-131) for the
module-level tests of tests/test_decoder_modes.py.  Built on oracle.dynmm_oracle's conv / BN / block functions (unchanged)."""
import torch
import torch.nn.functional as F

from oracle import dynmm_oracle as O


def upsample(sd, p, x, mode):
    """Upsample.forward (model.py:404-410)."""
    size = (x.shape[2] * 2, x.shape[3] * 2)
    if mode == 'bilinear':
        return F.interpolate(x, size, mode='bilinear', align_corners=False)
    x = F.interpolate(x, size, mode='nearest')
    if mode == 'nearest':
        return x
    if mode == 'learned-3x3':
        return O._conv(sd, p + '.conv', F.pad(x, (1, 1, 1, 1), mode='replicate'), 1, 0, groups=x.shape[1])
    return O._conv(sd, p + '.conv', x, 1, 1, groups=x.shape[1])


def decoder_module(sd, p, x, skip, training, n_blocks, mode, fusion):
    """DecoderModule.forward (model.py:343-357)."""
    y = O.conv_bn_act(sd, p + '.conv3x3', x, training, padding=1)
    for i in range(n_blocks):
        y = O.non_bottleneck_1d(sd, f'{p}.decoder_blocks.{i}', y, training)
    side = O._conv(sd, p + '.side_output', y) if training else None
    y = upsample(sd, p + '.upsample', y, mode)
    if fusion == 'add':
        y = y + skip
    return y, side


def decoder(sd, p, enc_outs, training, n_blocks, mode, fusion):
    """Decoder.forward (model.py:295-308)."""
    out, s16, s8, s4 = enc_outs
    out, o32 = decoder_module(sd, p + '.decoder_module_1', out, s16, training, n_blocks[0], mode, fusion)
    out, o16 = decoder_module(sd, p + '.decoder_module_2', out, s8, training, n_blocks[1], mode, fusion)
    out, o8 = decoder_module(sd, p + '.decoder_module_3', out, s4, training, n_blocks[2], mode, fusion)
    out = O._conv(sd, p + '.conv_out', out, 1, 1)
    out = upsample(sd, p + '.upsample2', upsample(sd, p + '.upsample1', out, mode), mode)
    return (out, o8, o16, o32) if training else out


def _resize(y, h, w, mode):
    if mode == 'nearest':
        return F.interpolate(y, (h, w), mode='nearest')
    return F.interpolate(y, (h, w), mode='bilinear', align_corners=False)


def pyramid_pooling(sd, p, x, training, bins, mode):
    """PyramidPoolingModule.forward (context_modules.py:70-87)."""
    h, w = x.shape[2:]
    outs = [x]
    for i, b in enumerate(bins):
        y = O.conv_bn_act(sd, f'{p}.features.{i}.1', F.adaptive_avg_pool2d(x, b), training)
        outs.append(_resize(y, h, w, mode))
    return O.conv_bn_act(sd, p + '.final_conv', torch.cat(outs, 1), training)


def adaptive_pyramid_pooling(sd, p, x, training, bins, input_size, mode):
    """AdaptivePyramidPoolingModule.forward (context_modules.py:111-131)."""
    h, w = x.shape[2:]
    mh, mw = int(h / input_size[0] + 0.5), int(w / input_size[1] + 0.5)
    outs = [x]
    for i, b in enumerate(bins):
        y = O.conv_bn_act(sd, f'{p}.features.{i}', F.adaptive_avg_pool2d(x, (b * mh, b * mw)), training)
        outs.append(_resize(y, h, w, mode))
    return O.conv_bn_act(sd, p + '.final_conv', torch.cat(outs, 1), training)
