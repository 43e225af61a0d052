"""fp64 CPU restatement of the MM-IMDB modality-level DynMM (ModalityDynMM/multimedia/imdb_dyn.py) from plain torch.nn layers
in MultiBench's structure (see dynmm_amd/nn/imdb.py for the definitions restated; parity is unpinned).  Dropout takes
injected keep flags: MASKS[name] is a uint8 [B, m] tensor for the site `name` ('branch3.encoders.<i>.op2' / '.op4')."""
import torch
import torch.nn as nn

MASKS = {}


class InjectedDropout(nn.Module):
    def __init__(self, p, name=''):
        super().__init__()
        self.p, self.name = p, name

    def forward(self, x):
        if not self.training or self.p == 0:
            return x
        m = MASKS[self.name].to(x.device, x.dtype)
        return x * m / (1 - self.p)


class MLP(nn.Module):
    def __init__(self, indim, hiddim, outdim):
        super().__init__()
        self.fc = nn.Linear(indim, hiddim)
        self.fc2 = nn.Linear(hiddim, outdim)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc(x)))


class Linear(nn.Module):
    def __init__(self, indim, outdim):
        super().__init__()
        self.fc = nn.Linear(indim, outdim)

    def forward(self, x):
        return self.fc(x)


class Maxout(nn.Module):
    def __init__(self, d, m, k):
        super().__init__()
        self.d_in, self.d_out, self.pool_size = d, m, k
        self.lin = nn.Linear(d, m * k)

    def forward(self, inputs):
        shape = list(inputs.size())
        shape[-1] = self.d_out
        shape.append(self.pool_size)
        out = self.lin(inputs)
        m, _ = out.view(*shape).max(dim=len(shape) - 1)
        return m


class MaxOut_MLP(nn.Module):  # noqa: N801
    def __init__(self, num_outputs, first_hidden=64, number_input_feats=300, second_hidden=None, linear_layer=True,
                 tag='maxout_mlp'):
        super().__init__()
        if second_hidden is None:
            second_hidden = first_hidden
        self.op0 = nn.BatchNorm1d(number_input_feats, 1e-4)
        self.op1 = Maxout(number_input_feats, first_hidden, 2)
        self.op2 = nn.Sequential(nn.BatchNorm1d(first_hidden), InjectedDropout(0.3, tag + '.op2'))
        self.op3 = Maxout(first_hidden, second_hidden, 2)
        self.op4 = nn.Sequential(nn.BatchNorm1d(second_hidden), InjectedDropout(0.3, tag + '.op4'))
        self.hid2val = nn.Linear(second_hidden, num_outputs) if linear_layer else None

    def forward(self, x):
        o = self.op4(self.op3(self.op2(self.op1(self.op0(x)))))
        return o if self.hid2val is None else self.hid2val(o)


class Concat(nn.Module):
    def forward(self, modalities):
        return torch.cat([m.flatten(1) for m in modalities], dim=1)


class MMDL(nn.Module):
    def __init__(self, encoders, fusion, head, has_padding=False):
        super().__init__()
        self.encoders = nn.ModuleList(encoders)
        self.fuse, self.head, self.has_padding = fusion, head, has_padding

    def forward(self, inputs):
        return self.head(self.fuse([enc(x) for enc, x in zip(self.encoders, inputs)]))


def diff_softmax(logits, tau=1.0, hard=False, dim=-1):
    y_soft = (logits / tau).softmax(dim)
    if not hard:
        return y_soft
    index = y_soft.max(dim, keepdim=True)[1]
    y_hard = torch.zeros_like(logits).scatter_(dim, index, 1.0)
    return y_hard - y_soft.detach() + y_soft


class DynMMNet(nn.Module):
    def __init__(self, branch_num=2, freeze=True):
        super().__init__()
        self.text_encoder = MLP(300, 512, 512)
        self.text_head = MLP(512, 512, 23)
        self.image_encoder = MLP(4096, 1024, 512)
        self.image_head = MLP(512, 512, 23)
        self.branch3 = MMDL([MaxOut_MLP(512, 512, 300, linear_layer=False, tag='branch3.encoders.0'),
                             MaxOut_MLP(512, 1024, 4096, 512, False, tag='branch3.encoders.1')], Concat(), Linear(1024, 23))
        if freeze:
            for m in (self.text_encoder, self.text_head, self.image_encoder, self.image_head, self.branch3):
                for p in m.parameters():
                    p.requires_grad = False
        self.gate = MLP(4396, 128, branch_num)
        self.temp, self.hard_gate, self.infer_mode = 1.0, True, 0

    def forward(self, inputs):
        weight = diff_softmax(self.gate(torch.cat(inputs, dim=1)), tau=self.temp, hard=self.hard_gate)
        preds = [self.text_head(self.text_encoder(inputs[0])), self.branch3(inputs)]
        if self.infer_mode > 0:
            return preds[self.infer_mode - 1], 0, weight
        out = weight[:, 0:1] * preds[0] + weight[:, 1:2] * preds[1]
        return out, weight[:, 1].mean(), weight

    def forward_separate_branch(self, inputs, path):
        if path == 1:
            return self.text_head(self.text_encoder(inputs[0]))
        if path == 2:
            return self.image_head(self.image_encoder(inputs[1]))
        return self.branch3(inputs)


def objective(out, aux, y, reg):
    """Supervised_Learning.train with additional_loss: BCEWithLogitsLoss(out, y) + reg * aux."""
    return nn.functional.binary_cross_entropy_with_logits(out, y) + reg * aux
