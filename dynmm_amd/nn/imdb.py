"""Modality-level DynMM on MM-IMDB features (ModalityDynMM/multimedia/imdb_dyn.py) on the HIP path.

PARITY UNPINNED.  The reference builds its experts from MultiBench (`unimodals.common_models.MLP / Linear / MaxOut_MLP`,
`fusions.common_fusions.Concat`, `training_structures.Supervised_Learning.MMDL`), which is neither vendored by the reference
nor pinned to a commit (imdb_dyn.py:10-13).  The modules below restate MultiBench's published definitions:

  MLP(i, h, o)                    fc -> ReLU -> fc2 (dropout=False, the default)
  Linear(i, o)                    fc
  Maxout(d, m, k=2)               lin = Linear(d, m*k); lin(x).view(B, m, k).max(-1): output j = max of columns 2j, 2j + 1
  MaxOut_MLP(num_outputs, first_hidden, number_input_feats, second_hidden=None, linear_layer=True)
                                  op0 = BatchNorm1d(in, eps=1e-4), op1 = Maxout(in, first_hidden, 2),
                                  op2 = Sequential(BatchNorm1d(first_hidden), Dropout(0.3)),
                                  op3 = Maxout(first_hidden, second_hidden, 2),
                                  op4 = Sequential(BatchNorm1d(second_hidden), Dropout(0.3)),
                                  hid2val = Linear(second_hidden, num_outputs) or None (linear_layer=False)
  Concat                          cat([m.flatten(1)], 1)
  LowRankTensorFusion             nn.affect.LowRankTensorFusion (one class for both data sets)
  MultiplicativeInteractions2Modal(input_dims=[n, m], output_dim=D, output='matrix', flatten=False, clip=None,
                                   grad_clip=None, flip=False)
                                  parameters (state_dict keys, in this order) W [n, m, D], U [n, D], V [m, D]: xavier_normal_;
                                  b [D]: normal_.  forward(modalities): m1, m2 = modalities (swapped under flip, each
                                  flattened to [B, -1] under flatten);
                                    Wprime = einsum('bn,nmd->bmd', m1, W) + V        # [B, m, D]
                                    bprime = m1 @ U + b
                                    out    = einsum('bm,bmd->bd', m2, Wprime) + bprime
                                  that is out[b,d] = sum_{n,m} m1[b,n] m2[b,m] W[n,m,d] + (m2 V)[b,d] + (m1 U)[b,d] + b[d]; one
                                  operator here (ops_mlp.mim, csrc/mim.hip), which never writes Wprime.  The other outputs
                                  ('vector', 'scalar'), clip and grad_clip are not built by the reference and are refused.
  MMDL(encoders, fusion, head)    head(fusion([enc_i(x_i)]))   (has_padding=False)

and, from the reference's own file, DynMMNet (imdb_dyn.py:29-114): expert 1 = text MLP encoder + MLP head, expert 2 =
`branch3`, the late-fusion MMDL of two MaxOut_MLPs and a Linear; gate = MLP(4396, 128, 2) on [text | image]; DiffSoftmax,
convex blend of the two experts' 23 logits, regulariser mean(w[:, 1]).

Modules are parameter containers with torch's own state_dict keys, so the state_dict of trained MultiBench modules loads
with load_state_dict (the reference torch.load()s pickled modules, which cannot be unpickled without MultiBench).  Every
Linear is the 1x1 MFMA GEMM of ops_seq.linear_bdt; each Maxout -> BatchNorm1d -> Dropout and the input BatchNorm1d are one
kernel of csrc/mlp.hip.  Dropout (p = 0.3) acts in training mode with a Philox site of its own (ops.manual_seed; torch's
generator cannot be reproduced bit for bit, the tests inject the keep flags on both sides).

Hard-gate inference runs each expert only on the samples routed to it (DynMMNet.compact): the gate's decisions become
stable index lists on the device, one host read of the two counts sizes the experts' batches, and the rows are scattered
back.  Under the hard gate the blend weights are exactly 1 and 0 and eval-mode BatchNorm acts per sample, so this equals
the dense blend up to the GEMMs' fp32 rounding at a different row count.
"""
import torch
import torch.nn as nn

from .. import engine, ops
from .. import ops_mlp as M
from .. import ops_seq as S
from .affect import LowRankTensorFusion, join_branches, run_branches     # noqa: F401 (LowRankTensorFusion: one class)

NUM_CLASSES = 23
FEATURES = {'text': 300, 'image': 4096}


class MLP(nn.Module):
    def __init__(self, indim, hiddim, outdim):
        super().__init__()
        self.fc = nn.Linear(indim, hiddim)
        self.fc2 = nn.Linear(hiddim, outdim)

    def forward(self, x):
        return S.linear_bdt(S.linear_bdt(x, self.fc.weight, self.fc.bias, act='relu'), self.fc2.weight, self.fc2.bias)


class Linear(nn.Module):
    def __init__(self, indim, outdim):
        super().__init__()
        self.fc = nn.Linear(indim, outdim)

    def forward(self, x):
        return S.linear_bdt(x, self.fc.weight, self.fc.bias)


class Maxout(nn.Module):
    """Parameter container of MultiBench's Maxout; the max over each pair runs fused with the BatchNorm that follows it in
    MaxOut_MLP (its only user here), so gemm() is all this module computes on its own."""

    def __init__(self, d, m, k=2):
        super().__init__()
        if k != 2:
            raise ValueError('Maxout: only pool_size 2 (MaxOut_MLP) is implemented')
        self.d_in, self.d_out, self.pool_size = d, m, k
        self.lin = nn.Linear(d, m * k)

    def gemm(self, x):
        return S.linear_bdt(x, self.lin.weight, self.lin.bias)

    def forward(self, x):
        raise NotImplementedError('Maxout runs fused with the BatchNorm1d of MaxOut_MLP (ops_mlp.maxout_bn)')


class MaxOut_MLP(nn.Module):  # noqa: N801 (MultiBench's name)
    def __init__(self, num_outputs, first_hidden=64, number_input_feats=300, second_hidden=None, linear_layer=True):
        super().__init__()
        if second_hidden is None:
            second_hidden = first_hidden
        self.op0 = nn.BatchNorm1d(number_input_feats, 1e-4)
        self.op1 = Maxout(number_input_feats, first_hidden, 2)
        self.op2 = nn.Sequential(nn.BatchNorm1d(first_hidden), nn.Dropout(0.3))
        self.op3 = Maxout(first_hidden, second_hidden, 2)
        self.op4 = nn.Sequential(nn.BatchNorm1d(second_hidden), nn.Dropout(0.3))
        self.hid2val = nn.Linear(second_hidden, num_outputs) if linear_layer else None
        self.tag = 'maxout_mlp'                  # prefix of the dropout sites' names (tests inject masks by name)
        self._sites = None

    def forward(self, x):
        if self._sites is None:
            self._sites = S.new_sites(2)
        h = M.maxout_bn(x, self.op0, maxout=False)
        h = M.maxout_bn(self.op1.gemm(h), self.op2[0], (float(self.op2[1].p), self._sites, self.tag + '.op2'))
        h = M.maxout_bn(self.op3.gemm(h), self.op4[0], (float(self.op4[1].p), self._sites + 1, self.tag + '.op4'))
        if self.hid2val is None:
            return h
        return S.linear_bdt(h, self.hid2val.weight, self.hid2val.bias)


class Concat(nn.Module):
    def forward(self, modalities):
        return torch.cat([m.flatten(1) for m in modalities], dim=1)


class MultiplicativeInteractions2Modal(nn.Module):
    """fusions.common_fusions.MultiplicativeInteractions2Modal with output='matrix' (the module docstring holds the
    definition) on ops_mlp.mim."""

    def __init__(self, input_dims, output_dim, output, flatten=False, clip=None, grad_clip=None, flip=False):
        super().__init__()
        if len(input_dims) != 2:
            raise NotImplementedError(f'MultiplicativeInteractions2Modal takes two modalities, got input_dims {input_dims}')
        if output != 'matrix':
            raise NotImplementedError(f"MultiplicativeInteractions2Modal(output={output!r}): only 'matrix' has HIP kernels")
        if clip is not None or grad_clip is not None:
            raise NotImplementedError('MultiplicativeInteractions2Modal: clip / grad_clip are not built on the HIP path')
        self.input_dims, self.output_dim, self.output = list(input_dims), output_dim, output
        self.flatten, self.clip, self.grad_clip, self.flip = flatten, clip, grad_clip, flip
        n, m = self.input_dims
        self.W = nn.Parameter(torch.empty(n, m, output_dim))
        nn.init.xavier_normal_(self.W)
        self.U = nn.Parameter(torch.empty(n, output_dim))
        nn.init.xavier_normal_(self.U)
        self.V = nn.Parameter(torch.empty(m, output_dim))
        nn.init.xavier_normal_(self.V)
        self.b = nn.Parameter(torch.empty(output_dim))
        nn.init.normal_(self.b)

    def forward(self, modalities):
        if len(modalities) != 2:
            raise ValueError(f'MultiplicativeInteractions2Modal takes two modalities, got {len(modalities)}')
        m1, m2 = (modalities[1], modalities[0]) if self.flip else (modalities[0], modalities[1])
        if self.flatten:
            m1, m2 = torch.flatten(m1, start_dim=1), torch.flatten(m2, start_dim=1)
        return M.mim(m1, m2, self.W, self.U, self.V, self.b)


class MMDL(nn.Module):
    """Supervised_Learning.MMDL with has_padding=False and tensor-valued encoders; the encoders run side by side."""

    def __init__(self, encoders, fusion, head, has_padding=False):
        super().__init__()
        if has_padding:
            raise ValueError('MMDL(has_padding=True) is not used on MM-IMDB features')
        self.encoders = nn.ModuleList(encoders)
        self.fuse, self.head, self.has_padding = fusion, head, has_padding

    def branch_fns(self, inputs):
        return [lambda i=i, enc=enc: enc(inputs[i]) for i, enc in enumerate(self.encoders)]

    def forward(self, inputs):
        return self.head(self.fuse(run_branches(self.branch_fns(inputs))))


def late_fusion_maxout():
    """imdb_mm.py --fuse 1 (saved as best_lf.pt): the third expert of DynMMNet."""
    return MMDL([MaxOut_MLP(512, 512, 300, linear_layer=False), MaxOut_MLP(512, 1024, 4096, 512, False)], Concat(),
                Linear(1024, NUM_CLASSES))


def low_rank_fusion_maxout(rank=128):
    """imdb_mm.py:43-47 (`--fuse 2`, saved as best_lrtf.pt)."""
    return MMDL([MaxOut_MLP(512, 512, 300, linear_layer=False), MaxOut_MLP(512, 1024, 4096, 512, False)],
                LowRankTensorFusion([512, 512], 512, rank), Linear(512, NUM_CLASSES))


def multiplicative_fusion_maxout(output_dim=1024):
    """imdb_mm.py:49-53 (`--fuse 3`, saved as best_mim.pt)."""
    return MMDL([MaxOut_MLP(512, 512, 300, linear_layer=False), MaxOut_MLP(512, 1024, 4096, 512, False)],
                MultiplicativeInteractions2Modal([512, 512], output_dim, 'matrix'), Linear(output_dim, NUM_CLASSES))


class DynMMNet(nn.Module):
    """imdb_dyn.py:29-114.  The reference loads pickled experts (`pretrain=True`: torch.load of ./log/imdb/*.pt); here they
    are constructed (random init) and filled with load_state_dict."""

    compact = True          # hard-gate eval runs each expert on its own samples only (False: the dense blend, for A/B runs)

    def __init__(self, branch_num=2, pretrain=False, freeze=True, temp=1.0, hard_gate=True):
        super().__init__()
        if pretrain:
            raise NotImplementedError('pickled MultiBench modules cannot be loaded without MultiBench; export their '
                                      'state_dict (torch.save(torch.load(path).state_dict(), out)) and use load_state_dict')
        self.branch_num = branch_num
        self.text_encoder = MLP(300, 512, 512)
        self.text_head = MLP(512, 512, NUM_CLASSES)
        self.image_encoder = MLP(4096, 1024, 512)         # used by forward_separate_branch(path=2) only
        self.image_head = MLP(512, 512, NUM_CLASSES)
        self.branch3 = late_fusion_maxout()
        for i, enc in enumerate(self.branch3.encoders):
            enc.tag = f'branch3.encoders.{i}'
        if freeze:
            for m in (self.text_encoder, self.text_head, self.image_encoder, self.image_head, self.branch3):
                self.freeze_branch(m)
        self.gate = MLP(4396, 128, branch_num)
        self.temp = temp
        self.hard_gate = hard_gate
        self.weight_list = torch.Tensor()
        self.store_weight = False
        self.infer_mode = 0
        self.flop = torch.Tensor([1.25261, 10.86908])
        self.last_counts = None            # (text, branch3) sample counts of the last compacted forward

    @staticmethod
    def freeze_branch(m):
        for p in m.parameters():
            p.requires_grad = False

    def reset_weight(self):
        self.weight_list = torch.Tensor()
        self.store_weight = True

    def weight_stat(self):
        tmp = torch.mean(self.weight_list, dim=0)
        print(f'mean branch weight {tmp[0].item():.4f}, {tmp[1].item():.4f}')
        self.store_weight = False
        return tmp[1].item()

    def cal_flop(self):
        tmp = torch.mean(self.weight_list, dim=0)
        total = (self.flop * tmp).sum()
        print(f'Total Flops {total.item():.2f}M')
        return total.item()

    def _record(self, weight):
        if self.store_weight:
            self.weight_list = torch.cat((self.weight_list, weight.detach().cpu()))

    def text_expert(self, x):
        return self.text_head(self.text_encoder(x))

    def gate_and_experts(self, inputs):
        """(gate logits, [text expert, branch3]) with the gate, the text expert and branch3's two encoders side by side."""
        x = torch.cat([inputs[0], inputs[1]], dim=1)
        b3 = self.branch3
        outs = run_branches([lambda: self.gate(x), lambda: self.text_expert(inputs[0])] + b3.branch_fns(inputs))
        return outs[0], [outs[1], b3.head(b3.fuse(outs[2:]))]

    def _compacting(self):
        return (self.compact and not self.training and self.hard_gate and self.infer_mode == 0 and
                not torch.is_grad_enabled())

    def forward(self, inputs):
        if self._compacting():
            return self._forward_compact(inputs)
        logits, preds = self.gate_and_experts(inputs)
        # the gate's DiffSoftmax weight is computed and RECORDED first, whatever infer_mode then does (imdb_dyn.py:95-101)
        out, aux, weight = M.ml_blend(logits, preds, self.temp, self.hard_gate)
        self._record(weight)
        if self.infer_mode > 0:
            return preds[self.infer_mode - 1], 0
        return out, aux

    def _forward_compact(self, inputs):
        text, image = inputs[0], inputs[1]
        logits = self.gate(torch.cat([text, image], dim=1))
        weight, aux = M.gate_weight(logits, self.temp, True)
        self._record(weight)
        order, inv, counts = M.partition(weight)
        n0, n1 = (int(v) for v in counts.cpu())           # the one host read of a compacted forward
        self.last_counts = (n0, n1)
        b3 = self.branch3
        fns = []
        if n0:
            rows0 = order[:n0]
            fns.append(lambda: self.text_expert(ops.batch_gather(text, rows0)))
        if n1:
            rows1 = order[n0:]
            sub = [ops.batch_gather(text, rows1), ops.batch_gather(image, rows1)]
            fns += b3.branch_fns(sub)
        outs = run_branches(fns)
        parts = []
        if n0:
            parts.append(outs[0])
        if n1:
            parts.append(b3.head(b3.fuse(outs[1 if n0 else 0:])))
        sorted_out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        return ops.batch_gather(sorted_out, inv), aux[0]

    def forward_separate_branch(self, inputs, path, weight_enable=False):
        if weight_enable:
            M.gate_weight(self.gate(torch.cat([inputs[0], inputs[1]], dim=1)), self.temp, self.hard_gate)
        if path == 1:
            return self.text_expert(inputs[0])
        if path == 2:
            return self.image_head(self.image_encoder(inputs[1]))
        return self.branch3(inputs)


class ImdbTrainStep(engine.FlatAdamWStep):
    """engine.FlatAdamWStep for the MM-IMDB DynMM (`moe_model`, additional_loss=True, task "multilabel"): BCEWithLogitsLoss +
    lossw * gate regulariser, with the loss and the backward seeds computed on the device.  Never captured, no prepack.
    Frozen experts (no trainable parameter) run forward only: their BatchNorms still use batch statistics and update their
    running statistics, and their dropouts still drop, as under the reference's model.train()."""

    def __init__(self, model, lr=1e-4, weight_decay=1e-2, lossw=0.1, clip_val=8.0):
        super().__init__(model, lr, weight_decay, clip_val)
        self.lossw = float(lossw)

    def _backward(self, inputs, target):
        m = self.model
        logits, preds = m.gate_and_experts(inputs)
        last = M.ml_loss_backward(logits, preds, target, m.temp, m.hard_gate, self.lossw)
        join_branches()
        return last['total'], last
