"""Generate tests/golden/decoder_modes_96x128.npz from the REFERENCE ITSELF: the decoder variants of ESANet's flags
(--upsampling, --context_module, --encoder_decoder_fusion) on the three network classes.

Runs only where the reference is readable (like make_goldens.py, whose `.cuda()` shim, model builders and seeding it
imports unchanged); never on the GPU box.

    python tests/golden/make_decoder_modes_goldens.py

What is stored (arrays and key lists only; inputs are regenerated from dynmm_amd.synth on both sides):
  <cls>/full/keys, shapes            the whole state_dict for the default flags (the encoders, fusions and gates do not
                                     depend on the three flags);
  <cls>/<combo>/keys, shapes         the entries under decoder., context_module. and skip_layer for each value of each
                                     flag (the other two at their defaults) and for one all-non-default combination;
  out/<combo>/eval_*, train_*        SkipGateESANet config P / SE-add, batch 2: eval logits (gate pinned to fuse
                                     everywhere), train-mode logits, side outputs and the train_loss probe;
  step/*                             one SGD-Nesterov step as train.py runs it (train_steps_fixture's recipe) in the
                                     all-non-default combination: the 4-scale losses, the flop loss, the total, and the
                                     parameter norms after the update.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402  (reference on sys.path, .cuda() no-op, seeding)

from dynmm_amd import synth  # noqa: E402

DEFAULTS = dict(upsampling='learned-3x3-zeropad', context_module='ppm', encoder_decoder_fusion='add')
FLAG_VALUES = {
    'upsampling': ['nearest', 'bilinear', 'learned-3x3', 'learned-3x3-zeropad'],
    'context_module': ['ppm', 'ppm-1-2-4-8', 'appm', 'appm-1-2-4-8', 'None'],
    'encoder_decoder_fusion': ['add', 'None'],
}
ALL_NON_DEFAULT = dict(upsampling='bilinear', context_module='appm', encoder_decoder_fusion='None')
# combinations with stored outputs: every up-sampling mode, both appm variants, PPM resized bilinearly, fusion 'None'
OUT_COMBOS = [
    dict(upsampling='nearest', context_module='ppm', encoder_decoder_fusion='add'),
    dict(upsampling='bilinear', context_module='appm', encoder_decoder_fusion='None'),
    dict(upsampling='learned-3x3', context_module='appm-1-2-4-8', encoder_decoder_fusion='add'),
    dict(upsampling='bilinear', context_module='ppm', encoder_decoder_fusion='add'),
    dict(upsampling='learned-3x3-zeropad', context_module='appm', encoder_decoder_fusion='None'),
]
PREFIXES = ('decoder.', 'context_module.', 'skip_layer')
H, W, N = 96, 128, 2
OUT_STRIDE = 16


def combo_name(c):
    return '{}|{}|{}'.format(c['upsampling'], c['context_module'], c['encoder_decoder_fusion'])


def combos():
    out = [dict(DEFAULTS)]
    for flag, values in FLAG_VALUES.items():
        for v in values:
            c = dict(DEFAULTS, **{flag: v})
            if c not in out:
                out.append(c)
    out.append(dict(ALL_NON_DEFAULT))
    return out


P = dict(encoder_rgb='resnet34', encoder_depth='resnet34', encoder_block='NonBottleneck1D',
         channels_decoder=[128, 128, 128], nr_decoder_blocks=[3, 3, 3], pretrained_on_imagenet=False,
         fuse_depth_in_rgb_encoder='SE-add')


def make(cls, combo):
    """The configurations of make_goldens.py: build() for SkipGateESANet ('P_se'), skip_fixture and esanet_fixture."""
    kw = dict(P, **combo)
    if cls == 'gate':
        return MG.SkipGateESANet(height=H, width=W, num_classes=40, **kw)
    if cls == 'skip':
        return MG.SkipESANet(height=H, width=W, num_classes=40, temp=1, block_rule=None, **kw)
    return MG.ESANet(height=H, width=W, num_classes=40, **kw)


def sides(outs):
    return [o.detach()[:, :, ::2, ::2].contiguous().numpy() for o in outs[1:]]


def main():
    torch.manual_seed(0)
    blob = {'meta': np.array([H, W, N, OUT_STRIDE])}
    names = []
    for cls in ('gate', 'skip', 'esanet'):
        for i, c in enumerate(combos()):
            sd = make(cls, c).state_dict()
            if i == 0:
                blob[f'{cls}/full/keys'] = np.array(list(sd.keys()))
                blob[f'{cls}/full/shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
            sub = [k for k in sd if k.startswith(PREFIXES)]
            blob[f'{cls}/{combo_name(c)}/keys'] = np.array(sub, dtype=str) if sub else np.zeros(0, dtype='<U1')
            blob[f'{cls}/{combo_name(c)}/shapes'] = np.array([','.join(map(str, sd[k].shape)) for k in sub], dtype=str) \
                if sub else np.zeros(0, dtype='<U1')
            if cls == 'gate':
                names.append(combo_name(c))
    blob['combos'] = np.array(names)

    rgb, depth = synth.synth_inputs(N, H, W, seed=1234)
    blob['out_combos'] = np.array([combo_name(c) for c in OUT_COMBOS])
    for c in OUT_COMBOS:
        tag = f'out/{combo_name(c)}'
        print(' ', tag, flush=True)
        m = make('gate', c)
        synth.fill_state_dict(m.state_dict(), seed=0)
        m.eval()
        m.baseline = True
        with torch.no_grad():
            out = m(rgb, depth, test=True)
        blob[f'{tag}/eval_strided'] = out[:, :, ::OUT_STRIDE, ::OUT_STRIDE].contiguous().numpy()
        blob[f'{tag}/eval_csum'] = out.sum(dim=(2, 3)).numpy()
        m = make('gate', c)
        synth.fill_state_dict(m.state_dict(), seed=0)
        m.train()
        m.temp, m.hard_gate = 0.8, False
        outs, lf = m(rgb, depth)
        loss = MG.train_loss(outs, lf)
        blob[f'{tag}/train_strided'] = outs[0].detach()[:, :, ::OUT_STRIDE, ::OUT_STRIDE].contiguous().numpy()
        blob[f'{tag}/train_csum'] = outs[0].detach().sum(dim=(2, 3)).numpy()
        for i, s in enumerate(sides(outs)):
            blob[f'{tag}/train_side{i}'] = s
        blob[f'{tag}/train_loss'] = np.float64(loss.item())

    # one optimisation step (train_steps_fixture's recipe: reference CE, SGD-Nesterov, total-loss rule)
    c = ALL_NON_DEFAULT
    m = make('gate', c)
    synth.fill_state_dict(m.state_dict(), seed=0)
    m.train()
    m.temp, m.hard_gate = 0.8, False
    labels = [synth.synth_labels(N, H // s, W // s, seed=300 + s).float() for s in (1, 8, 16, 32)]
    cw = np.linspace(0.5, 2.0, 40).astype(np.float32)
    ce = MG.ref_utils.CrossEntropyLoss2d(torch.device('cpu'), cw)
    opt = torch.optim.SGD(m.parameters(), lr=0.002, weight_decay=1e-4, momentum=0.9, nesterov=True)
    ratio, budget = 0.5, 1.0
    blob['step/combo'] = np.array(combo_name(c))
    blob['step/cw'] = cw
    blob['step/hyper'] = np.array([0.002, 1e-4, 0.9, ratio, budget, 0.8])
    opt.zero_grad()
    outs, lf = m(rgb, depth)
    losses = ce(outs, labels)
    total = sum(losses) + ratio * max(torch.zeros_like(lf), lf - budget)
    total.backward()
    opt.step()
    blob['step/losses'] = np.array([v.item() for v in losses], np.float64)
    blob['step/loss_flop'] = np.float64(lf.item())
    blob['step/total'] = np.float64(total.item())
    sd = m.state_dict()
    blob['step/param_names'] = np.array([k for k in sd if sd[k].dtype.is_floating_point and 'running_' not in k])
    blob['step/param_norms'] = np.array([sd[k].double().norm().item() for k in blob['step/param_names']])
    path = os.path.join(HERE, 'decoder_modes_96x128.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
