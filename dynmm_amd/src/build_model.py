"""build_model(args, n_classes) -> (model, device): the factory train.py / eval.py call
(FusionDynMM/src/build_model.py:18-218): `--dynamic --global-gate` (SkipGateESANet), `--dynamic` (SkipESANet, per-stage
Gumbel gates) and the static RGB-D ESANet (no --dynamic, --modality rgbd).  ImageNet / SceneNet weights are read from local
files (src/pretrained.py; a missing file is an error, never a silent random init).  The single-modality networks
(`--modality rgb|depth`, build_model.py:119-141) come from `build_one_modality(args, n_classes)`, to which the drivers dispatch;
`build_model` itself keeps refusing them."""
import warnings

import torch
from torch import nn

from ..nn.esanet import ESANet, ESANetOneModality
from ..nn.net import SkipGateESANet
from ..nn.net_skip import SkipESANet
from .pretrained import load_scenenet


def _decoder_shape(args):
    if 'decreasing' in args.decoder_channels_mode:
        warnings.warn('Argument --channels_decoder is ignored when --decoder_chanels_mode decreasing is set.')
        channels = [512, 256, 128]
    else:
        channels = [args.channels_decoder] * 3
    nb = args.nr_decoder_blocks
    if isinstance(nb, int):
        nb = [nb] * 3
    elif len(nb) == 1:
        nb = list(nb) * 3
    assert len(nb) == 3
    return channels, list(nb)


def build_model(args, n_classes):
    pretrained = bool(args.pretrained_on_imagenet) and not args.last_ckpt and args.pretrained_scenenet == ''
    channels_decoder, nr_decoder_blocks = _decoder_shape(args)
    if args.encoder_depth in (None, 'None'):
        args.encoder_depth = args.encoder
    common = dict(height=args.height, width=args.width, num_classes=n_classes,
                  pretrained_on_imagenet=pretrained, pretrained_dir=args.pretrained_dir,
                  encoder_rgb=args.encoder, encoder_depth=args.encoder_depth, encoder_block=args.encoder_block,
                  activation=args.activation, encoder_decoder_fusion=args.encoder_decoder_fusion,
                  context_module=args.context_module, nr_decoder_blocks=nr_decoder_blocks,
                  channels_decoder=channels_decoder, fuse_depth_in_rgb_encoder=args.fuse_depth_in_rgb_encoder,
                  upsampling=args.upsampling)
    if args.dynamic:
        block_rule = [int(ch) for ch in args.block_rule]
        assert len(block_rule) == 4
        model = (SkipGateESANet if args.global_gate else SkipESANet)(temp=args.temp, block_rule=block_rule, **common)
    elif getattr(args, 'modality', 'rgbd') == 'rgbd':
        model = ESANet(**common)                                          # build_model.py:93-113
    else:
        raise NotImplementedError(f'--modality {args.modality}: build_model returns the RGB-D networks; the single-modality '
                                  'ESANetOneModality (src/build_model.py:119-141) is built by build_one_modality(args, n_classes)')
    return _place_and_initialise(model, args, n_classes, pretrained)


def build_one_modality(args, n_classes):
    """(model, device) for `--modality rgb | depth` (build_model.py:119-141): ESANetOneModality on 3 or 1 input channels, with
    `--fuse_depth_in_rgb_encoder` as its `weighting_in_encoder`; the same tail as build_model."""
    if getattr(args, 'modality', 'rgbd') not in ('rgb', 'depth'):
        raise ValueError(f'build_one_modality: --modality must be rgb or depth, got {getattr(args, "modality", "rgbd")}')
    if args.dynamic:
        raise NotImplementedError('--dynamic selects the RGB-D DynMM networks (build_model); it has no single-modality form')
    pretrained = bool(args.pretrained_on_imagenet) and not args.last_ckpt and args.pretrained_scenenet == ''
    channels_decoder, nr_decoder_blocks = _decoder_shape(args)
    model = ESANetOneModality(height=args.height, width=args.width, pretrained_on_imagenet=pretrained, encoder=args.encoder,
                              encoder_block=args.encoder_block, activation=args.activation,
                              input_channels=3 if args.modality == 'rgb' else 1,
                              encoder_decoder_fusion=args.encoder_decoder_fusion, context_module=args.context_module,
                              num_classes=n_classes, pretrained_dir=args.pretrained_dir, nr_decoder_blocks=nr_decoder_blocks,
                              channels_decoder=channels_decoder, weighting_in_encoder=args.fuse_depth_in_rgb_encoder,
                              upsampling=args.upsampling)
    return _place_and_initialise(model, args, n_classes, pretrained)


def build_for_args(args, n_classes):
    """What the drivers call: build_one_modality for `--modality rgb | depth` without --dynamic (the reference's dispatch,
    build_model.py:18-141), build_model otherwise."""
    if not args.dynamic and getattr(args, 'modality', 'rgbd') != 'rgbd':
        return build_one_modality(args, n_classes)
    return build_model(args, n_classes)


def _place_and_initialise(model, args, n_classes, pretrained):
    """build_model.py:143-218: device, He init, SceneNet weights, --finetune"""
    device = torch.device('cuda:0') if torch.cuda.is_available() else torch.device('cpu')
    print('Device:', device)
    model.to(device)

    if getattr(args, 'he_init', False):
        from ..nn.blocks import ResNetEncoder
        # (already initialised: the ImageNet-pre-trained encoders, build_model.py:152-156)
        mods = [m for child in model.children() if not (pretrained and isinstance(child, ResNetEncoder))
                for m in child.modules()]
        for i, m in enumerate(mods):
            if isinstance(m, nn.Conv2d):
                followed_by_sigmoid = isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and \
                    i + 1 < len(mods) and isinstance(mods[i + 1], nn.Identity) and m.bias is not None \
                    and m.out_channels > m.in_channels
                if m.out_channels == n_classes or followed_by_sigmoid or m.groups == m.in_channels:
                    continue
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        print('Applied He init.')

    if getattr(args, 'pretrained_scenenet', '') != '':                   # build_model.py:181-205
        load_scenenet(model, args.pretrained_scenenet, args.context_module)

    if getattr(args, 'finetune', None) is not None:
        ckpt = torch.load(args.finetune, map_location=device)
        model.load_state_dict(ckpt['state_dict'], strict=False)
        print(f'Loaded weights for finetuning: {args.finetune}')
    return model, device
