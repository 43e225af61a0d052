"""Generate tests/golden/one_modality_96x128.npz from the REFERENCE ITSELF: ESANetOneModality
(src/models/model_one_modality.py — what src/build_model.py:119-141 returns for --modality rgb | depth).

Runs only where the reference is readable (like make_goldens.py, whose `.cuda()` shim, seeding and train_loss probe it
imports unchanged); never on the GPU box.

    python tests/golden/make_one_modality_goldens.py

Three configurations (arrays and key lists only; inputs are regenerated from dynmm_amd.synth on both sides):
  rgb     config P (ResNet-34 / NonBottleneck1D / [128,128,128] / [3,3,3] / learned-3x3-zeropad / SE-add), input_channels 3
  depth   the same with input_channels 1 (the input is the second tensor of synth.synth_inputs)
  plain   weighting_in_encoder 'None' (se_layer0..4 = nn.Identity), upsampling 'bilinear', input_channels 3
For each, as esanet_fixture does: keys / shapes / dtypes, strided eval logits and channel sums, train-mode strided logits,
the three side outputs, the train_loss probe, all parameter-gradient names and norms, three full gradients (the SE ones only
where the configuration has them), and one SGD-Nesterov step by train_steps_fixture's recipe: the four losses, the total,
the parameter norms after the update.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as MG  # noqa: E402  (reference on sys.path, .cuda() no-op, seeding)

from src.models.model_one_modality import ESANetOneModality  # noqa: E402

from dynmm_amd import synth  # noqa: E402

H, W, N = 96, 128, 2
P = dict(encoder='resnet34', encoder_block='NonBottleneck1D', channels_decoder=[128, 128, 128],
         nr_decoder_blocks=[3, 3, 3], pretrained_on_imagenet=False)
CONFIGS = {
    'rgb': dict(P, input_channels=3, weighting_in_encoder='SE-add', upsampling='learned-3x3-zeropad'),
    'depth': dict(P, input_channels=1, weighting_in_encoder='SE-add', upsampling='learned-3x3-zeropad'),
    'plain': dict(P, input_channels=3, weighting_in_encoder='None', upsampling='bilinear'),
}
FULL_GRADS = ('encoder.conv1.weight', 'se_layer0.fc.0.weight', 'se_layer3.fc.2.bias')


def make(cfg):
    m = ESANetOneModality(height=H, width=W, num_classes=40, **CONFIGS[cfg])
    synth.fill_state_dict(m.state_dict(), seed=0)
    return m


def main():
    blob = {'meta': np.array([H, W, N, MG.STRIDE]), 'configs': np.array(list(CONFIGS))}
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234)
    labels = [synth.synth_labels(N, H // s, W // s, seed=300 + s).float() for s in (1, 8, 16, 32)]
    cw = np.linspace(0.5, 2.0, 40).astype(np.float32)
    blob['step/cw'] = cw
    blob['step/hyper'] = np.array([0.002, 1e-4, 0.9])
    for cfg, kw in CONFIGS.items():
        print(' ', cfg, flush=True)
        image = rgb if kw['input_channels'] == 3 else depth
        m = make(cfg)
        sd = m.state_dict()
        blob[f'{cfg}/keys'] = np.array(list(sd.keys()))
        blob[f'{cfg}/shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
        blob[f'{cfg}/dtypes'] = np.array([str(v.dtype) for v in sd.values()])
        m.eval()
        with torch.no_grad():
            out = m(image)
        for k, v in MG.summarize_logits(out).items():
            blob[f'{cfg}/eval/{k}'] = v
        m = make(cfg)
        m.train()
        outs = m(image)
        loss = MG.train_loss(outs, torch.zeros(()))
        loss.backward()
        for k, v in MG.summarize_logits(outs[0]).items():
            blob[f'{cfg}/train/{k}'] = v
        for i, o in enumerate(outs[1:]):
            blob[f'{cfg}/train/side{i}'] = o.detach().numpy()
        blob[f'{cfg}/train/loss'] = np.float32(loss.item())
        params = dict(m.named_parameters())
        blob[f'{cfg}/train/grad_names'] = np.array(list(params))
        blob[f'{cfg}/train/grad_norms'] = np.array([p.grad.norm().item() for p in params.values()], np.float64)
        for name in FULL_GRADS:
            if name in params:
                blob[f'{cfg}/train/grad:{name}'] = params[name].grad.numpy()

        # one optimisation step (train_steps_fixture's recipe: reference CE, SGD-Nesterov; no gate, hence no flop loss)
        m = make(cfg)
        m.train()
        ce = MG.ref_utils.CrossEntropyLoss2d(torch.device('cpu'), cw)
        opt = torch.optim.SGD(m.parameters(), lr=0.002, weight_decay=1e-4, momentum=0.9, nesterov=True)
        opt.zero_grad()
        losses = ce(m(image), labels)
        total = sum(losses)
        total.backward()
        opt.step()
        blob[f'{cfg}/step/losses'] = np.array([v.item() for v in losses], np.float64)
        blob[f'{cfg}/step/total'] = np.float64(total.item())
        sd = m.state_dict()
        names = [k for k in sd if sd[k].dtype.is_floating_point and 'running_' not in k]
        blob[f'{cfg}/step/param_names'] = np.array(names)
        blob[f'{cfg}/step/param_norms'] = np.array([sd[k].double().norm().item() for k in names])
    path = os.path.join(HERE, 'one_modality_96x128.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
