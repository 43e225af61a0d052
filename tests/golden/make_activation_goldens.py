"""Generate tests/golden/activations_{swish,hswish}_96x128.npz from the REFERENCE ITSELF with `activation=swish|hswish`.

Runs only where the reference is mounted (see make_goldens.py, whose process-local `.cuda()` no-op, loss, sampling and noise
helpers are imported from there unchanged); never on the GPU box.  The reference files are untouched.

    python tests/golden/make_activation_goldens.py

Per activation, config P_se (ResNet-34 / NonBottleneck1D / SE-add / 3 decoder blocks), 96x128, N = 2, weights from
synth.fill_state_dict and inputs from synth.synth_inputs on both sides (never the reference's own initialisation):
  gate/...   SkipGateESANet: eval_baseline, eval_soft, eval_hard, train_soft     (make_goldens.run_mode's entries)
  skip/...   SkipESANet with injected Exp(1) noise: eval_test, train_soft        (make_goldens.skip_fixture's entries)
  esanet/... ESANet: eval, train                                                  (make_goldens.esanet_fixture's entries)
  <net>/keys, <net>/shapes: the state_dict contract (identical for every activation).
One file per activation: together they would pass the size limit of a committed file.  Arrays and name strings only.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_goldens', os.path.join(HERE, 'make_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                     # imports the reference, installs the .cuda() no-op

from dynmm_amd import synth                     # noqa: E402

H, W, N = 96, 128, 2
COMMON = dict(height=H, width=W, num_classes=40, encoder_rgb='resnet34', encoder_depth='resnet34',
              encoder_block='NonBottleneck1D', channels_decoder=[128, 128, 128], nr_decoder_blocks=[3, 3, 3],
              pretrained_on_imagenet=False, fuse_depth_in_rgb_encoder='SE-add', upsampling='learned-3x3-zeropad')
GATE_MODES = ['eval_baseline', 'eval_soft', 'eval_hard', 'train_soft']
SKIP_MODES = ['eval_test', 'train_soft']


def contract(blob, tag, m):
    sd = m.state_dict()
    blob[f'{tag}/keys'] = np.array(list(sd.keys()))
    blob[f'{tag}/shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])


def grads(blob, tag, m):
    names = [k for k, _ in m.named_parameters()]
    blob[f'{tag}/grad_names'] = np.array(names)
    blob[f'{tag}/grad_norms'] = np.array([0.0 if p.grad is None else p.grad.norm().item() for _, p in m.named_parameters()],
                                         np.float64)


def gate_fixture(blob, act):
    def build():
        m = G.SkipGateESANet(activation=act, **COMMON)
        synth.fill_state_dict(m.state_dict(), seed=0)
        return m
    contract(blob, 'gate', build())
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234)
    for mode in GATE_MODES:
        print(f'  {act} gate {mode}', flush=True)
        m = build()
        training = mode.startswith('train')
        m.train() if training else m.eval()
        m.baseline = mode == 'eval_baseline'
        m.hard_gate = mode == 'eval_hard'
        m.temp = 1.0
        t = f'gate/{mode}'
        if training:
            outs, lf = m(rgb, depth)
            loss = G.train_loss(outs, lf)
            loss.backward()
            for k, v in G.summarize_logits(outs[0]).items():
                blob[f'{t}/{k}'] = v
            for i, o in enumerate(outs[1:]):
                blob[f'{t}/side{i}'] = o.detach().numpy()
            blob[f'{t}/loss_flop'] = np.float32(lf.item())
            blob[f'{t}/loss'] = np.float32(loss.item())
            grads(blob, t, m)
        else:
            with torch.no_grad():
                out, weight = m(rgb, depth, test=True, return_weight=True)
                _, lf = m(rgb, depth)
            for k, v in G.summarize_logits(out).items():
                blob[f'{t}/{k}'] = v
            blob[f'{t}/weight'] = weight.numpy()
            blob[f'{t}/loss_flop'] = np.float32(lf.item())


def skip_fixture(blob, act):
    real_exp = torch.Tensor.exponential_
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234)
    for mode in SKIP_MODES:
        print(f'  {act} skip {mode}', flush=True)
        training, test, hard, temp, rule = G.SKIP_MODES[mode]
        m = G.SkipESANet(activation=act, temp=temp, block_rule=rule, **COMMON)
        synth.fill_state_dict(m.state_dict(), seed=0)
        m.train() if training else m.eval()
        m.hard_gate = hard
        noise = G.skip_noise(N, mode)
        calls = [0]

        def fake_exponential(self, *a, **k):
            self.copy_(noise[calls[0]])
            calls[0] += 1
            return self
        torch.Tensor.exponential_ = fake_exponential
        try:
            m.start_weight()
            if training:
                outs = m(rgb, depth, test=test)
                loss = G.train_loss(outs, torch.zeros(()))
                loss.backward()
            else:
                with torch.no_grad():
                    outs = m(rgb, depth, test=test)
        finally:
            torch.Tensor.exponential_ = real_exp
        assert calls[0] == 4
        t = f'skip/{mode}'
        for k, v in G.summarize_logits(outs[0] if training else outs).items():
            blob[f'{t}/{k}'] = v
        for j in range(4):
            blob[f'{t}/noise{j}'] = noise[j].numpy()
            blob[f'{t}/weight{j}'] = m.weight_list[j].detach().numpy().copy()
        blob[f'{t}/cfg'] = np.array([int(training), int(test), int(hard)] + list(rule), np.int64)
        blob[f'{t}/temp'] = np.float32(temp)
        if training:
            blob[f'{t}/loss'] = np.float32(loss.item())
            for i, o in enumerate(outs[1:]):
                blob[f'{t}/side{i}'] = o.detach().numpy()
            grads(blob, t, m)
    contract(blob, 'skip', m)


def esanet_fixture(blob, act):
    def build():
        m = G.ESANet(activation=act, **COMMON)
        synth.fill_state_dict(m.state_dict(), seed=0)
        return m
    print(f'  {act} esanet', flush=True)
    m = build()
    contract(blob, 'esanet', m)
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234)
    m.eval()
    with torch.no_grad():
        out = m(rgb, depth)
    for k, v in G.summarize_logits(out).items():
        blob[f'esanet/eval/{k}'] = v
    m = build()
    m.train()
    outs = m(rgb, depth)
    loss = G.train_loss(outs, torch.zeros(()))
    loss.backward()
    for k, v in G.summarize_logits(outs[0]).items():
        blob[f'esanet/train/{k}'] = v
    for i, o in enumerate(outs[1:]):
        blob[f'esanet/train/side{i}'] = o.detach().numpy()
    blob['esanet/train/loss'] = np.float32(loss.item())
    grads(blob, 'esanet/train', m)


if __name__ == '__main__':
    for act in ('swish', 'hswish'):
        blob = {'meta': np.array([H, W, N, G.STRIDE])}
        gate_fixture(blob, act)
        skip_fixture(blob, act)
        esanet_fixture(blob, act)
        path = os.path.join(HERE, f'activations_{act}_96x128.npz')
        np.savez_compressed(path, **blob)
        print(path, os.path.getsize(path), 'bytes')
    print('done')
