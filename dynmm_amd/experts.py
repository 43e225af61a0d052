"""Step I of the modality-level DynMM: train the expert networks that Step II (dynmm_amd.imdb / dynmm_amd.affect) gates.

The reference trains them with four scripts (ModalityDynMM/multimedia/imdb_uni.py, imdb_mm.py, affect/affect_uni.py,
affect_mm.py); dynmm_amd.imdb_uni, .imdb_mm, .affect_uni and .affect_mm mirror their flags.  This module holds what the four
share: the expert builders, the single-model train step, the training and test protocols and the file contract.

Protocols.
  Late-fusion experts (imdb_mm, affect_mm) follow the vendored training_structures/Supervised_Learning.py `train` /
  `single_test` without moe_model: objective per batch, clip_grad_norm_(8), AdamW; validation with the same objective after
  every epoch; the best model by validation F1-macro (multilabel, strictly greater than the best so far, which starts at 0)
  or validation loss (regression, strictly less, starting at 10000); patience reset on a new best and incremented otherwise,
  stop when patience > 7; test with single_test (multilabel F1, or posneg-classification for MOSEI).
  Uni-modal experts (imdb_uni, affect_uni) use MultiBench's training_structures/unimodal.py, which the reference does not
  vendor: nn.Sequential(encoder, head) runs through the same loop.  The points that rest on an assumption are listed in
  DESIGN.md ("Step I: training the experts").

File contract (state_dicts, read with strict=True by imdb.load_pretrained and affect.load_pretrained / expert_files):
  imdb_uni --mod 0 / 1     encoder_{text,image}.pt, head_{text,image}.pt
  imdb_mm --fuse 1 / 0     best_lf.pt / best_ef.pt
  affect_uni --mod 0/1/2   reg_transformer_{encoder,head}_{visual,audio,text}.pt; text also b1_reg_transformer_{encoder,head}_text.pt
  affect_mm --fusion 3     lf_tran.pt and b2_lf_tran.pt
  affect_uni_gru(mod)      reg_gru_{encoder,head}_{visual,audio,text}.pt      (builders: the command-line switches --enc gru /
  affect_mm_gru(1 / 0)     lf_gru.pt / ef_gru.pt                               --fusion 0 | 1 are not wired yet)
  imdb_mm_lrtf()           best_lrtf.pt                                       (builders: --fuse 2 / --fusion 5 are not wired
  affect_mm_lrtf()         lrtf.pt                                             yet)
  imdb_mm_mim()            best_mim.pt                                        (builder: --fuse 3 is not wired yet)
  affect_mm_ef_tran()      ef_tran.pt                                         (builder: --fusion 2 is not wired yet)
  affect_mm_mult()         mult.pt                                            (builder: --fusion 4 is not wired yet)
The b1_ / b2_ copies are the names affect_dyn.py:211 (`--model v2`) reads, which a reference user makes by renaming.
"""
import copy
import os
import time

import numpy as np
import torch
import torch.nn as nn

from . import engine
from . import ops
from . import ops_mlp as M
from . import ops_seq as S
from .nn import affect as A
from .nn import imdb as I
from .nn import mult as MU

PATIENCE = 7                 # Supervised_Learning.train: `if early_stop and patience > 7: break`


# ---------------------------------------------------------------------------------------------------------------------
# experts
# ---------------------------------------------------------------------------------------------------------------------
Identity = A.Identity        # MultiBench unimodals.common_models.Identity

IMDB_MODS = ('text', 'image')
A_MODS = ('visual', 'audio', 'text')
IMDB_FUSE = {0: 'ef', 1: 'lf', 2: 'lrtf', 3: 'mim'}
AFFECT_FUSION = {0: 'ef_gru', 1: 'lf_gru', 2: 'ef_tran', 3: 'lf_tran', 4: 'mult', 5: 'lrtf'}


def _not_wired(switch, model, where):
    """The refusal of a command-line switch whose model is built by a function of its own."""
    return NotImplementedError(f'{switch}: the driver switch is not wired yet; the {model} itself runs on the HIP path: {where}')


_FUSION_5 = ('affect_mm --fusion 5 (lrtf)', 'LowRankTensorFusion model over GRUWithLinear encoders',
             'dynmm_amd.nn.affect.low_rank_fusion_gru, experts.affect_mm_lrtf')


def imdb_uni(mod):
    """imdb_uni.py: (encoder, head) of modality `mod` (0 text, 1 image)."""
    if mod not in (0, 1):
        raise ValueError(f'--mod {mod}: 0 (text) or 1 (image)')
    enc = I.MLP(300, 512, 512) if mod == 0 else I.MLP(4096, 1024, 512)
    return enc, I.MLP(512, 512, I.NUM_CLASSES)


def _tag_maxout(model):
    for name, m in model.named_modules():
        if isinstance(m, I.MaxOut_MLP):
            m.tag = name                         # dropout sites named after the module path (tests inject masks by name)
    return model


def imdb_mm(fuse):
    """imdb_mm.py: the MMDL of `--fuse` (1: late fusion, DynMMNet's branch3; 0: early fusion) and its learning rate."""
    if fuse in (0, 1):
        if fuse == 1:
            model, lr = I.late_fusion_maxout(), 8e-3
        else:
            model, lr = I.MMDL([Identity(), Identity()], I.Concat(), I.MaxOut_MLP(I.NUM_CLASSES, 512, 4396)), 4e-2
        return _tag_maxout(model), lr
    if fuse in (2, 3):
        fusion = 'LowRankTensorFusion' if fuse == 2 else 'MultiplicativeInteractions2Modal'
        raise _not_wired(f'imdb_mm --fuse {fuse} ({IMDB_FUSE[fuse]})', f'{fusion} model',
                         f'dynmm_amd.nn.imdb.{fusion}, experts.imdb_mm_{IMDB_FUSE[fuse]}')
    raise ValueError(f'--fuse {fuse}: one of 0-3')


def imdb_mm_lrtf(rank=128):
    """imdb_mm.py `--fuse 2` (lrtf: two MaxOut_MLPs, LowRankTensorFusion([512, 512], 512, 128), Linear(512, 23); best_lrtf.pt
    through imdb_mm.file_name(dir, 2)) and its learning rate."""
    return _tag_maxout(I.low_rank_fusion_maxout(rank)), 8e-3


def imdb_mm_mim(output_dim=1024):
    """imdb_mm.py `--fuse 3` (mim: two MaxOut_MLPs, MultiplicativeInteractions2Modal([512, 512], 1024, 'matrix'),
    Linear(1024, 23); best_mim.pt through imdb_mm.file_name(dir, 3)) and its learning rate."""
    return _tag_maxout(I.multiplicative_fusion_maxout(output_dim)), 8e-3


def affect_uni(mod, enc='transformer', hidden_dim1=0, hidden_dim2=0, clf=False):
    """affect_uni.py: (encoder, head, modality name) of modality `mod` (0 visual, 1 audio, 2 text)."""
    if enc != 'transformer':
        raise _not_wired(f'--enc {enc}', 'GRU expert', 'dynmm_amd.nn.affect.GRU, experts.affect_uni_gru')
    if clf:
        raise NotImplementedError('--clf: the 2-output posneg-clf head trains with CrossEntropyLoss, which has no HIP '
                                  'objective kernel (only the regression head with L1Loss runs)')
    if mod not in (0, 1, 2):
        raise ValueError(f'--mod {mod}: 0 (visual), 1 (audio) or 2 (text)')
    name = A_MODS[mod]
    h1 = hidden_dim1 if hidden_dim1 > 0 else 120
    h2 = hidden_dim2 if hidden_dim2 > 0 else 64
    return A.Transformer(A.FEATURES[name], h1), A.MLP(h1, h2, 1), name


def affect_mm(fusion):
    """affect_mm.py: the MMDL of `--fusion` (3: late-fusion transformers, DynMMNetV2's branch2).  The other switches are refused;
    the models of 0 / 1 (affect_mm_gru), 2 (affect_mm_ef_tran), 4 (affect_mm_mult) and 5 (affect_mm_lrtf) are built by their own
    functions."""
    if fusion == 3:
        return A.late_fusion_transformer()
    if fusion in (0, 1):
        raise _not_wired(f'affect_mm --fusion {fusion} ({AFFECT_FUSION[fusion]})', 'GRU model',
                         'dynmm_amd.nn.affect.GRU, experts.affect_mm_gru')
    if fusion == 5:
        raise _not_wired(*_FUSION_5)
    if fusion == 4:
        raise _not_wired('affect_mm --fusion 4 (mult)', 'MULT model (MULTModel(3, [35, 74, 300]))',
                         'dynmm_amd.nn.mult.MULTModel, experts.affect_mm_mult')
    if fusion == 2:
        raise _not_wired('affect_mm --fusion 2 (ef_tran)', 'early-fusion Transformer(409, 300) model',
                         'dynmm_amd.nn.affect.early_fusion_transformer, experts.affect_mm_ef_tran')
    raise ValueError(f'--fusion {fusion}: one of 0-5')


GRU_DIMS = {0: (64, 32), 1: (128, 64), 2: (512, 256)}        # affect_uni.py:38-60 (`--enc gru`): (hidden_dim1, hidden_dim2)


def affect_uni_gru(mod, hidden_dim1=0, hidden_dim2=0):
    """affect_uni.py `--enc gru`: (GRU encoder, MLP head, modality name) of modality `mod` (0 visual, 1 audio, 2 text); saved
    as reg_gru_{encoder,head}_{name}.pt (affect_uni.file_names)."""
    if mod not in (0, 1, 2):
        raise ValueError(f'--mod {mod}: 0 (visual), 1 (audio) or 2 (text)')
    name = A_MODS[mod]
    h1 = hidden_dim1 if hidden_dim1 > 0 else GRU_DIMS[mod][0]
    h2 = hidden_dim2 if hidden_dim2 > 0 else GRU_DIMS[mod][1]
    return A.GRU(A.FEATURES[name], h1, dropout=True, has_padding=True), A.MLP(h1, h2, 1), name


def affect_mm_gru(fusion):
    """affect_mm.py `--fusion 1` (lf_gru: three GRUs, Concat, MLP(704, 512, 1); lf_gru.pt) and `--fusion 0` (ef_gru: Identity
    encoders, ConcatEarly, Sequential(GRU(409, 512), MLP(512, 256, 1)); ef_gru.pt)."""
    if fusion == 1:
        return A.late_fusion_gru()
    if fusion == 0:
        return A.early_fusion_gru()
    if fusion == 5:
        raise _not_wired(*_FUSION_5)
    raise ValueError(f'affect_mm_gru({fusion}): 0 (ef_gru) or 1 (lf_gru)')


def affect_mm_lrtf(rank=32):
    """affect_mm.py `--fusion 5` (lrtf: three GRUWithLinear encoders, LowRankTensorFusion([32, 32, 128], 128, 32),
    MLP(128, 512, 1); lrtf.pt through affect_mm.file_names(dir, 5))."""
    return A.low_rank_fusion_gru(rank)


def affect_mm_ef_tran():
    """affect_mm.py `--fusion 2` (ef_tran: Identity encoders, ConcatEarly, Sequential(Transformer(409, 300), MLP(300, 128, 1));
    ef_tran.pt through affect_mm.file_names(dir, 2)).  nhead = 5 at d_model = 300 is head dimension 60: ops_seq.mha_wide."""
    return A.early_fusion_transformer()


def affect_mm_mult():
    """affect_mm.py `--fusion 4` (mult: Identity encoders, MULTModel(3, [35, 74, 300], HParams) as the fusion, Identity head;
    mult.pt through affect_mm.file_names(dir, 4)).  Nine cross-modal transformers (embed_dim 40, 10 heads: head dimension 4) and
    three memory transformers (120 channels: head dimension 12), all pre-norm with the future mask: ops_seq.cross_attention."""
    return MU.mult_model()


# ---------------------------------------------------------------------------------------------------------------------
# train step
# ---------------------------------------------------------------------------------------------------------------------
def _map(x, fn):
    """x with fn applied to every device tensor of its nested lists (host tensors and other leaves as they are)."""
    if isinstance(x, (list, tuple)):
        return [_map(v, fn) for v in x]
    return fn(x) if torch.is_tensor(x) and x.is_cuda else x


def _leaves(x):
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _leaves(v)]
    return [x] if torch.is_tensor(x) and x.is_cuda else []


def _host_leaves(x):
    """is any leaf of the nested lists x not a device tensor?"""
    if isinstance(x, (list, tuple)):
        return any(_host_leaves(v) for v in x)
    return not (torch.is_tensor(x) and x.is_cuda)


class ExpertTrainStep(engine.FlatAdamWStep):
    """engine.FlatAdamWStep for ONE model (no moe_model, no additional loss): the objective ('bce': BCEWithLogitsLoss, 'l1':
    L1Loss) and its backward seed come out of one kernel (ops_mlp.head_loss).  `loss_acc` (fp64 device [1]) collects loss * B
    of every step, so an epoch's training loss costs one host read.  use_graph: only for models without BatchNorm (a capture's
    warm-up step would update running statistics)."""

    def __init__(self, model, objective, lr, weight_decay, clip_val=8.0, use_graph=False):
        if objective not in M.HEAD_LOSSES:
            raise ValueError(f'objective must be one of {sorted(M.HEAD_LOSSES)}, got {objective!r}')
        depth = [len(m.layers) for m in model.modules() if isinstance(m, (nn.TransformerEncoder, MU.TransformerEncoder))]
        self.has_bn = any(isinstance(m, nn.BatchNorm1d) for m in model.modules())
        if use_graph and self.has_bn:
            raise ValueError('ExpertTrainStep(use_graph=True): only for models without BatchNorm (the transformer experts)')
        # the transformer experts take AffectTrainStep's launch savings: one weight re-layout launch per step and grouped
        # weight-gradient launches per same-shape layer stack
        super().__init__(model, lr, weight_decay, clip_val, use_graph, prepack=ops.PackedWeights() if depth else None,
                         wgrad_group=min(8, max(depth)) if depth else None)
        self.objective = objective
        self.loss_acc = torch.zeros(1, device=self.flat_g.device, dtype=torch.float64)

    def _backward(self, inputs, target):
        out = self.model(inputs)
        loss, seed = M.head_loss(out, target, self.objective, seed=True, loss_acc=self.loss_acc)
        torch.autograd.backward([out], [seed])
        A.join_branches()
        return loss, {'out': out.detach(), 'loss': loss}

    def _extra_state(self):
        return [self.loss_acc]

    def _graph_key(self, inputs, target):
        return (tuple(tuple(t.shape) for t in _leaves(inputs)), tuple(target.shape), bool(self.model.training))

    def _clone_inputs(self, inputs):
        # (called once per capture) a GRU reads its padding lengths on the device: host lengths would be uploaded inside the
        # capture and frozen into it
        grus = (A.GRU, A.GRUWithLinear)
        if any(isinstance(m, grus) and m.has_padding for m in self.model.modules()) and _host_leaves(inputs[1]):
            raise ValueError('ExpertTrainStep(use_graph=True) on a GRU expert: pass the padding lengths as device tensors (host '
                             'lengths would be frozen into the capture)')
        return _map(inputs, lambda t: t.clone())

    _input_tensors = staticmethod(_leaves)


# ---------------------------------------------------------------------------------------------------------------------
# protocols
# ---------------------------------------------------------------------------------------------------------------------
class EarlyStop:
    """Supervised_Learning.train's best-model and patience bookkeeping.  mode 'max': multilabel, validation F1-macro, best
    starts at 0 (bestf1); 'min': regression, validation loss, best starts at 10000 (bestvalloss).  Only a strict improvement
    counts; patience is reset on a new best and incremented otherwise; the run stops once patience > 7."""

    def __init__(self, mode):
        if mode not in ('max', 'min'):
            raise ValueError(f"mode must be 'max' or 'min', got {mode!r}")
        self.mode = mode
        self.best = 0.0 if mode == 'max' else 10000.0
        self.patience = 0
        self.best_epoch = None

    def update(self, epoch, metric):
        """True when `metric` is a new best (the caller saves the model)."""
        better = metric > self.best if self.mode == 'max' else metric < self.best
        if better:
            self.best, self.patience, self.best_epoch = metric, 0, epoch
        else:
            self.patience += 1
        return better

    @property
    def stop(self):
        return self.patience > PATIENCE


def evaluate_multilabel(model, loader, adapt):
    """(f1_micro, f1_macro, mean BCE) of one pass, counts on the device, one host read."""
    counts = None
    model.eval()
    with torch.no_grad():
        for inputs, y in loader:
            out = model(adapt(inputs))
            if counts is None:
                counts = M.MultilabelCounts(y.shape[1], y.device)
            counts.add(out, y)
    r = counts.read()
    micro, macro = M.f1_from_counts(r['tp'], r['fp'], r['fn'])
    return micro, macro, r['loss']


def evaluate_posneg(model, loader, adapt):
    """single_test's posneg-classification with criterion L1Loss() (the mean per batch, times len(batch)): {'Accuracy',
    'Loss' (the mean absolute error), 'Corr'} — PosnegCounts' 'valid' form with no regulariser."""
    counts = None
    model.eval()
    with torch.no_grad():
        for inputs, y in loader:
            out = model(adapt(inputs))
            if counts is None:
                counts = S.PosnegCounts(y.device, 'valid', 0.0)
            counts.add(out, y)
    return counts.metrics()


def train(model, loaders, adapt, objective, lr, weight_decay, n_epochs, save, protocol='mm', clip_val=8.0,
          use_graph=False, step=None):
    """Supervised_Learning.train for one model (objective 'bce' -> task multilabel, 'l1' -> task regression).  save(): write
    the model's files (called on every new best, as the reference torch.save()s).  protocol 'mm' prints the reference's
    per-epoch lines, 'uni' MultiBench unimodal.train's.  Returns (per-epoch training loss, EarlyStop, best state_dict)."""
    train_loader, valid_loader = loaders[0], loaders[1]
    if step is None:
        step = ExpertTrainStep(model, objective, lr, weight_decay, clip_val=clip_val, use_graph=use_graph)
    stopper = EarlyStop('max' if objective == 'bce' else 'min')
    history, best_sd = [], None
    for epoch in range(n_epochs):
        model.train()
        step.loss_acc.zero_()
        nb = 0
        for inputs, y in train_loader:
            if step.has_bn and y.shape[0] < 2:
                continue                                # BatchNorm1d in training mode needs 2 samples
            step(adapt(inputs), y)
            nb += y.shape[0]
        loss = float(step.loss_acc.item()) / max(nb, 1)   # the epoch's one host read of the training loss
        step.opt.check_finite()
        history.append(loss)
        if objective == 'bce':
            micro, macro, vloss = evaluate_multilabel(model, valid_loader, adapt)
            metric = macro
            if protocol == 'uni':
                print(f'Epoch {epoch} train loss: {loss:.4f}')
                print(f'Epoch {epoch} valid loss: {vloss:.4f} f1_micro: {micro:.4f} f1_macro: {macro:.4f}')
            else:
                print('-' * 50)
                print(f'Epoch {epoch} | Train loss {loss:.4f} | Train CE loss {loss:.4f} | Val loss {vloss:.4f} | '
                      f'patience {stopper.patience}\nf1 micro: {micro:.3f} | f1 macro: {macro:.3f} ')
        else:
            metric = evaluate_posneg(model, valid_loader, adapt)['Loss']
            print(f'Epoch {epoch} | train loss {loss:.3f} | valid loss {metric:.3f}')
        if stopper.update(epoch, metric):
            best_sd = copy.deepcopy(model.state_dict())
            print('Saving Best')
            save()
        if stopper.stop:
            break
    return history, stopper, best_sd


def load_state(module, path, device):
    module.load_state_dict(torch.load(path, map_location=device, weights_only=True))


def save_state(module, *paths):
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    for p in paths:
        torch.save(sd, p)


class Timer:
    """--measure: wall time of a test pass (device work included)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            torch.cuda.synchronize()
            self.t0 = time.time()
        return self

    def __exit__(self, *exc):
        if self.on:
            torch.cuda.synchronize()
            print(f'Inference Time: {time.time() - self.t0:.4f} s')


def f1_summary(log1, log2):
    print(log1, log2)
    print(f'Finish {len(log1)} runs')
    print(f'f1 micro {np.mean(log1) * 100:.2f} ± {np.std(log1) * 100:.2f}')
    print(f'f1 macro {np.mean(log2) * 100:.2f} ± {np.std(log2) * 100:.2f}')


def posneg_summary(log, loss_std_digits):
    print(log)
    print(f'Finish {log.shape[0]} runs')
    print(f'Test Accuracy {np.mean(log[:, 0]) * 100:.2f} ± {np.std(log[:, 0]) * 100:.2f}')
    print(f'Loss {np.mean(log[:, 1]):.4f} ± {np.std(log[:, 1]):.{loss_std_digits}f}')
    print(f'Corr {np.mean(log[:, 2]):.4f} ± {np.std(log[:, 2]):.{loss_std_digits}f}')


def posneg_line(r):
    print(f"Loss: {r['Loss']:.4f} | Accuracy {r['Accuracy'] * 100:.2f} | Corr {r['Corr']:.3f}")


def ensure_dir(path):
    os.makedirs(path, exist_ok=True)
    return path
