"""ESANet — the STATIC RGB-D network (FusionDynMM/src/models/model.py:19-241): depth features are fused into the RGB
encoder at the stem and after every stage, no gate.  It is what `build_model` returns without `--dynamic`
(src/build_model.py:93-113) and what the README's baseline mIoU was produced with.

On the HIP path it is SkipGateESANet's forward with the gate pinned to "fuse everywhere" (the blend of
model_skip_mod_globalgate.py:282-310 with weight = e_4 is exactly model.py:196-238), minus the gate parameters: same
kernels, the reference's own state_dict (892 entries for ResNet-34 / NonBottleneck1D / SE-add, checked against the
reference in tests/test_esanet.py), the reference's forward contract `forward(rgb, depth) -> out` where `out` is the
decoder's 4-tuple in training mode (model.py:306-308).

ESANetOneModality — the RGB-only / depth-only networks (src/models/model_one_modality.py) — is below: one encoder, the
single-input squeeze-and-excitation of ops.se_scale at the fusion points, the same decoder side."""
import torch
import torch.nn as nn

from .. import ops
from .blocks import ResNetEncoder, normalize_activation
from .decoder import emitting_labels
from .fusion import SqueezeAndExcitation
from .net import SkipGateESANet, build_decoder_side, check_decoder_options, decoder_skip


class ESANet(SkipGateESANet):
    def __init__(self, height=480, width=640, num_classes=37, encoder_rgb='resnet18', encoder_depth='resnet18',
                 encoder_block='BasicBlock', channels_decoder=None, pretrained_on_imagenet=True,
                 pretrained_dir='./trained_models/imagenet', activation='relu', encoder_decoder_fusion='add',
                 context_module='ppm', nr_decoder_blocks=None, fuse_depth_in_rgb_encoder='SE-add',
                 upsampling='bilinear'):
        # the reference's defaults (model.py:20-35): bilinear up-sampling, PPM resized bilinearly, skip adds
        super().__init__(height=height, width=width, num_classes=num_classes, encoder_rgb=encoder_rgb,
                         encoder_depth=encoder_depth, encoder_block=encoder_block, channels_decoder=channels_decoder,
                         pretrained_on_imagenet=pretrained_on_imagenet, pretrained_dir=pretrained_dir,
                         activation=activation, encoder_decoder_fusion=encoder_decoder_fusion,
                         context_module=context_module,
                         nr_decoder_blocks=[1, 1, 1] if nr_decoder_blocks is None else nr_decoder_blocks,
                         fuse_depth_in_rgb_encoder=fuse_depth_in_rgb_encoder, upsampling=upsampling)
        del self.gate_layer                      # no gate parameters: the reference ESANet has none
        self.baseline = True

    def forward(self, rgb, depth, test=True, return_weight=False):
        # model.py:189-241: every stage fuses; SkipGateESANet with baseline = True computes the same blend with w = e_4.
        # The reference's ESANet.forward takes (rgb, depth) only; the two extra arguments are what train.py's `validate`
        # / eval.py pass to the dynamic models (train.py:438, eval.py:106) and are accepted so that engine.evaluate and
        # those callers work on either model: there is no gate, hence no FLOP loss to return and `weight` is e_4.
        self.baseline = True
        if return_weight:
            return super().forward(rgb, depth, test=True, return_weight=True)
        return super().forward(rgb, depth, test=True)

    def forward_front(self, rgb, depth):
        self.baseline = True                 # (engine.InferStep enters here, not through forward)
        return super().forward_front(rgb, depth)

    def freeze(self):
        raise NotImplementedError('ESANet has no gate to keep trainable (model.freeze() belongs to the --dynamic models)')


class ESANetOneModality(nn.Module):
    """The uni-modal baselines (FusionDynMM/src/models/model_one_modality.py:19-193; src/build_model.py:119-141 for
    `--modality rgb | depth`): ONE encoder, a stand-alone SqueezeAndExcitation after the stem and after every stage
    (weighting_in_encoder 'SE-add'; anything else: identity), then the skip layers, context module and decoder of the RGB-D
    networks.  Same constructor arguments and defaults as the reference, its state_dict (encoder.*, se_layer0..4.*,
    skip_layer1..3.*, context_module.*, decoder.*: 560 entries for ResNet-34 / NonBottleneck1D / SE-add / [3,3,3], 530 without
    SE — tests/test_one_modality.py), and its forward contract `forward(image) -> out`, the decoder's 4-tuple in training mode.

    There is no second tensor to blend, so the fusion points run on the single-input kernels of csrc/se_scale.hip
    (ops.se_scale; the stem's fused with the max-pool that follows, ops.se_scale_pool).

    The callers' two-input protocol `model(rgb, depth, test=True, return_weight=False)` is accepted as well (ESANet.forward
    set the precedent): the network takes the tensor of its own modality — the one with `input_channels` channels — and launches
    nothing on the other, so engine.TrainStep / evaluate / validate / InferStep, train.run and eval.run work on it unchanged."""
    # engine.InferStep: nothing in this forward is decided on the host, whatever gate attributes (hard_gate, baseline, ...) the
    # drivers have set on the instance — one captured graph
    gate_free = True

    def __init__(self, height=480, width=640, num_classes=37, encoder='resnet18', encoder_block='BasicBlock',
                 channels_decoder=None, pretrained_on_imagenet=True, pretrained_dir='./trained_models/imagenet',
                 activation='relu', input_channels=3, encoder_decoder_fusion='add', context_module='ppm',
                 nr_decoder_blocks=None, weighting_in_encoder='None', upsampling='bilinear'):
        super().__init__()
        channels_decoder = [128, 128, 128] if channels_decoder is None else list(channels_decoder)
        nr_decoder_blocks = [1, 1, 1] if nr_decoder_blocks is None else list(nr_decoder_blocks)
        self.activation = activation = normalize_activation(activation)
        check_decoder_options(upsampling, encoder_decoder_fusion)
        if input_channels not in (1, 3):
            raise NotImplementedError(f'input_channels must be 3 (rgb) or 1 (depth). Got {input_channels}')
        self.weighting_in_encoder = weighting_in_encoder
        self.input_channels = input_channels
        self.modality = 'rgb' if input_channels == 3 else 'depth'
        self.height, self.width = height, width

        self.encoder = ResNetEncoder(encoder, encoder_block, input_channels=input_channels, activation=activation)
        if pretrained_on_imagenet:
            # resnet.py:395-509, from local files (FileNotFoundError when they are absent: never a silent random initialisation)
            from ..src.pretrained import load_imagenet_encoder
            load_imagenet_encoder(self.encoder, encoder, encoder_block, input_channels, pretrained_dir)
        enc = self.encoder
        self.channels_decoder_in = enc.down_32_channels_out
        for j, ch in enumerate((64, enc.down_4_channels_out, enc.down_8_channels_out, enc.down_16_channels_out,
                                enc.down_32_channels_out)):
            setattr(self, f'se_layer{j}', SqueezeAndExcitation(ch, activation=activation)
                    if weighting_in_encoder == 'SE-add' else nn.Identity())
        # (the context module resizes with 'nearest' for the learned up-samplings, model_one_modality.py:138-145)
        build_decoder_side(self, channels_decoder, nr_decoder_blocks, num_classes, context_module, upsampling,
                           encoder_decoder_fusion, activation, encoder=enc)

    def _own(self, image, other):
        """the input of this network's modality out of what the caller passed"""
        for t in (image, other):
            if t is not None and t.dim() == 4 and t.shape[1] == self.input_channels:
                return t
        shapes = [tuple(t.shape) for t in (image, other) if t is not None]
        raise ValueError(f'ESANetOneModality ({self.modality}): no input with {self.input_channels} channels among {shapes}')

    def _se(self, j):
        return getattr(self, f'se_layer{j}').mlp_params() if self.weighting_in_encoder == 'SE-add' else None

    def forward(self, image, depth=None, test=True, return_weight=False):
        # model_one_modality.py:165-193.  `test` changes nothing (no gate, hence no FLOP loss to return beside the outputs);
        # `return_weight` returns (out, None): there are no gate weights.
        enc, act = self.encoder, self.activation
        infer = not torch.is_grad_enabled()
        if self.training:
            ops.begin_step()
        out = enc.forward_first_conv(self._own(image, depth))
        se = self._se(0)
        # stem: scale + 3x3/s2 max-pool in one pass where the kernels serve the shape (ops.se_scale_pool composes otherwise)
        out = ops.se_scale_pool(out, se, act) if se else ops.max_pool_3x3_s2(out)
        skips = []
        for j in (1, 2, 3, 4):
            # The stage's last block hands its output to the squeeze and the scale (or, without SE, to the next STAGE), never to
            # a block called with chain=True: nothing picks up its `_bn_out_link`, so its bn2 backward does its own reductions
            # (ops._BatchNormAct.backward: bwd_link.sums stays None) — no BatchNorm backward waits for a launch that never comes.
            out = getattr(enc, f'forward_layer{j}')(out)
            se = self._se(j)
            if se:
                out = ops.se_scale(out, se, act, inplace=infer)       # (inference: the stage output has no other reader)
            if j < 4 and self.encoder_decoder_fusion == 'add':
                out, f_skip = ops.fan_out(out, 2)                     # next stage + decoder skip connection
                skips.append(decoder_skip(self, j, f_skip))
            elif j < 4:
                skips.append(None)
        out = self.context_module(out)
        out = self.decoder([out, skips[2], skips[1], skips[0]])
        return (out, None) if return_weight else out

    def segment(self, image, depth=None, return_weight=False):
        """The uint8 [N,H,W] label map of the eval-mode forward (nn/net.py SkipGateESANet.segment); no gate, so
        `return_weight` gives (labels, None).  Raises in training mode."""
        with emitting_labels(self):
            return self.forward(image, depth, True, return_weight)
