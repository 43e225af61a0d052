"""Restatement of ESANetOneModality.forward (FusionDynMM/src/models/model_one_modality.py:165-193) on a state_dict, in whatever
precision the state_dict and the input carry (the tests run it in float64).  Built on oracle.dynmm_oracle's conv / BN / block
functions and tests/decoder_modes_oracle.py's decoder variants (both unchanged)."""
import torch
import torch.nn.functional as F

from oracle import dynmm_oracle as O
from tests import decoder_modes_oracle as DO


def squeeze_excite(params, x, act=F.relu):
    """SqueezeAndExcitation.forward (model_utils.py:47-51) from (W1, b1, W2, b2)"""
    w1, b1, w2, b2 = params
    s = F.adaptive_avg_pool2d(x, 1)
    s = act(F.conv2d(s, w1, b1))
    return x * torch.sigmoid(F.conv2d(s, w2, b2))


def forward(sd, image, cfg: O.Config, training=False, weighting='SE-add', upsampling='learned-3x3-zeropad',
            fusion='add', bins=(1, 5)):
    """`out` (the decoder's 4-tuple in training mode).  cfg: encoder, block and decoder shape (O.Config; `fuse` is unused)."""
    def se(j, x):
        return O.squeeze_excite(sd, f'se_layer{j}', x) if weighting == 'SE-add' else x

    out = O.encoder_stem(sd, 'encoder', image, training)
    out = F.max_pool2d(se(0, out), 3, 2, 1)
    skips = []
    for j in (1, 2, 3, 4):
        out = se(j, O.encoder_stage(sd, 'encoder', out, training, cfg, j))
        if j < 4:
            skips.append(O._skip(sd, f'skip_layer{j}', out, training) if fusion == 'add' else None)
    # the context module resizes with 'nearest' for the learned up-samplings (model_one_modality.py:138-145)
    ctx_mode = 'nearest' if 'learned-3x3' in upsampling else upsampling
    ctx = DO.pyramid_pooling(sd, 'context_module', out, training, bins, ctx_mode)
    return DO.decoder(sd, 'decoder', [ctx, skips[2], skips[1], skips[0]], training, cfg.nr_decoder_blocks, upsampling, fusion)
