"""ESANet decoder (model.py:244-410): 3 x [ConvBNAct 3x3, n x NonBottleneck1D, side output (train),
2x upsample (+ skip add with encoder_decoder_fusion='add')], 3x3 classifier, two 2x upsamples."""
import contextlib

import torch
import torch.nn as nn

from .. import ops
from .blocks import ConvBNAct, NonBottleneck1D, chain_ok


UPSAMPLING_MODES = ('nearest', 'bilinear', 'learned-3x3', 'learned-3x3-zeropad')


@contextlib.contextmanager
def emitting_labels(model):
    """The scope of one `segment` forward: eval mode required, no_grad, the decoder's `emit_labels` set and restored."""
    if model.training:
        raise RuntimeError(f'{type(model).__name__}.segment needs eval mode: label maps exist at inference only '
                           '(call model.eval() first)')
    dec = model.decoder
    prev, dec.emit_labels = dec.emit_labels, True
    try:
        with torch.no_grad():
            yield
    finally:
        dec.emit_labels = prev


class Upsample(nn.Module):
    """Upsample(mode, channels) (model.py:360-410): x2 'nearest' / 'bilinear' (align_corners=False, no parameters: the
    reference's pad and conv are nn.Identity), or the learned modes — nearest x2 + depthwise 3x3 initialised to mimic
    bilinear (model.py:385-395), with zero borders ('learned-3x3-zeropad', conv padding 1) or replicated ones
    ('learned-3x3': ReplicationPad2d(1) + conv padding 0).  forward(x, skip) also adds the decoder's skip connection."""

    def __init__(self, mode='learned-3x3-zeropad', channels=None):
        super().__init__()
        if mode not in UPSAMPLING_MODES:
            raise NotImplementedError(f'Upsampling mode must be one of {UPSAMPLING_MODES}. Got {mode}')
        self.mode = mode
        if 'learned-3x3' in mode:
            self.pad = nn.Identity()          # (ReplicationPad2d for 'learned-3x3' has no state; the kernel clamps)
            self.conv = nn.Conv2d(channels, channels, 3, padding=1 if mode == 'learned-3x3-zeropad' else 0,
                                  groups=channels)
            k = torch.tensor([1., 2., 1.]) / 4
            with torch.no_grad():
                self.conv.weight.copy_((k[:, None] * k[None, :]).expand(channels, 1, 3, 3))
                self.conv.bias.zero_()
        else:
            self.pad = nn.Identity()
            self.conv = nn.Identity()

    def forward(self, x, skip=None):
        if self.mode == 'learned-3x3-zeropad':
            return ops.upsample2x_dw3x3(x, self.conv.weight, self.conv.bias, skip)
        if self.mode == 'learned-3x3':
            return ops.upsample2x_dw3x3(x, self.conv.weight, self.conv.bias, skip, border='replicate')
        return ops.upsample2x(x, self.mode, skip)


class DecoderModule(nn.Module):
    def __init__(self, channels_in, channels_dec, nr_decoder_blocks, num_classes, upsampling_mode='learned-3x3-zeropad',
                 encoder_decoder_fusion='add', activation='relu'):
        super().__init__()
        self.upsampling_mode = upsampling_mode
        self.encoder_decoder_fusion = encoder_decoder_fusion
        self.conv3x3 = ConvBNAct(channels_in, channels_dec, 3, activation)
        self.decoder_blocks = nn.Sequential(*[NonBottleneck1D(channels_dec, channels_dec, activation=activation)
                                              for _ in range(nr_decoder_blocks)])
        self.upsample = Upsample(upsampling_mode, channels_dec)
        self.side_output = nn.Conv2d(channels_dec, num_classes, 1)

    def forward(self, x, skip):
        y = self.conv3x3(x)
        blocks = list(self.decoder_blocks)
        for i, blk in enumerate(blocks):
            # (the chain contract of nn/blocks.py ResNetEncoder._stage: block i is the ONLY consumer of block i - 1's output)
            y = blk(y, chain=i > 0 and chain_ok(blocks[i - 1], blk))
        side = None
        if self.training:
            s = self.side_output
            y, ys = ops.fan_out(y, 2)            # y feeds the side output AND the up-sampling
            side = ops.conv2d(ys, s.weight, s.bias, 1, 0)
        # model.py:354-355: the encoder features are added only with encoder_decoder_fusion == 'add'
        return self.upsample(y, skip if self.encoder_decoder_fusion == 'add' else None), side


class Decoder(nn.Module):
    def __init__(self, channels_in, channels_decoder, nr_decoder_blocks, num_classes,
                 upsampling_mode='learned-3x3-zeropad', encoder_decoder_fusion='add', activation='relu'):
        super().__init__()
        cd = channels_decoder
        kw = dict(upsampling_mode=upsampling_mode, encoder_decoder_fusion=encoder_decoder_fusion, activation=activation)
        self.decoder_module_1 = DecoderModule(channels_in, cd[0], nr_decoder_blocks[0], num_classes, **kw)
        self.decoder_module_2 = DecoderModule(cd[0], cd[1], nr_decoder_blocks[1], num_classes, **kw)
        self.decoder_module_3 = DecoderModule(cd[1], cd[2], nr_decoder_blocks[2], num_classes, **kw)
        self.conv_out = nn.Conv2d(cd[2], num_classes, 3, padding=1)
        self.upsample1 = Upsample(upsampling_mode, num_classes)
        self.upsample2 = Upsample(upsampling_mode, num_classes)
        self.upsampling_mode = upsampling_mode
        # engine.TrainStep sets this: in training the full-resolution logits feed the loss only, so the last
        # up-sampling is fused with the cross entropy (ops.DeferredLogits, csrc/tail.hip) and never materialised.
        # The fused tail restates 'learned-3x3-zeropad' only: with any other mode the logits are materialised and the
        # loss takes the plain cross-entropy kernels (what TrainStep(fuse_tail=False) runs).
        self.defer_tail = False
        # segment() of the networks sets this for one eval-mode forward: the decoder returns the uint8 [N,H,W] label map.
        # The learned modes run the two up-samplings and the arg-max as ONE kernel (ops.tail_argmax, csrc/segment.hip);
        # 'nearest' / 'bilinear' take the arg-max of exactly the logits the forward returns otherwise.
        self.emit_labels = False

    def forward(self, enc_outs, unpermute=None):
        """unpermute = (index, inverse): the batch arrives in a permuted (branch-sorted, K16) order; the natural
        order is restored on the 40-channel map in front of the two final up-samplings (3 MB/img instead of
        49 MB/img; everything after it is per-sample) and on the small side outputs."""
        out, s16, s8, s4 = enc_outs
        out, o32 = self.decoder_module_1(out, s16)
        out, o16 = self.decoder_module_2(out, s8)
        out, o8 = self.decoder_module_3(out, s4)
        c = self.conv_out
        out = ops.conv2d(out, c.weight, c.bias, 1, 1)
        if unpermute is not None:
            out = ops.batch_permute(out, *unpermute)
        if self.training and self.defer_tail and torch.is_grad_enabled() and self.upsampling_mode == 'learned-3x3-zeropad':
            out = ops.DeferredLogits(self.upsample1(out), self.upsample2.conv)
        elif self.emit_labels and not self.training:
            if 'learned-3x3' in self.upsampling_mode:
                border = 'zero' if self.upsampling_mode == 'learned-3x3-zeropad' else 'replicate'
                out = ops.tail_argmax(out, self.upsample1.conv, self.upsample2.conv, border)
            else:
                out = ops.argmax_resize(self.upsample2(self.upsample1(out)))
        else:
            out = self.upsample2(self.upsample1(out))
        if self.training:
            if unpermute is not None:
                o8, o16, o32 = (ops.batch_permute(o, *unpermute) for o in (o8, o16, o32))
            return out, o8, o16, o32
        return out
