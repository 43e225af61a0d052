"""Modality-level DynMM on CMU-MOSEI features (ModalityDynMM/affect/affect_dyn.py) on the HIP path.

PARITY UNPINNED.  The reference builds its experts from MultiBench (`unimodals.common_models.Transformer / MLP`,
`fusions.common_fusions.Concat`, `training_structures.Supervised_Learning.MMDL`), which is neither vendored in
/root/reference nor pinned to a commit (ModalityDynMM README; affect_dyn.py:12-15).  The modules below restate
MultiBench's published definitions:

  Transformer(n_features, dim)   Conv1d(n_features, dim, 1, bias=False) over the feature axis, then
                                 nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=dim, nhead=5), num_layers=5)
                                 (post-norm, ReLU, dim_feedforward 2048), output = the LAST time step.  The padding
                                 lengths that accompany the input are ignored (`x = x[0]`).
  GRU(indim, hiddim, ...)        nn.GRU(indim, hiddim, batch_first=True); has_padding: h_n of the packed [x, lengths];
                                 last_only: the last step; else the sequence; then Dropout(dropoutp) and flatten.  Unlike the
                                 transformer a GRU has an exact yardstick: torch.nn.GRU in float64 (tests/test_gru.py).
  GRUWithLinear(indim, hiddim, outdim, ...)
                                 nn.GRU(indim, hiddim) then nn.Linear(hiddim, outdim); has_padding: h_n of the packed [x, lengths]
                                 (batch-first), Dropout, linear; else the linear layer on the whole state sequence
  MLP(indim, hiddim, outdim)     fc -> ReLU -> fc2
  Concat                         torch.cat(..., dim=1)
  LowRankTensorFusion(input_dims, output_dim, rank)
                                 factors[m] [rank, d_m + 1, out], fusion_weights [1, rank], fusion_bias [1, out]:
                                 sum_r w[r] prod_m ([1 | z_m] factors[m][r]) + bias      
  ConcatEarly                    torch.cat(..., dim=2)
  MMDL(encoders, fusion, head)   head(fusion([enc_i([x_i, len_i])]))          (Supervised_Learning.py:16-51 — vendored)

and, from the reference's own file, DynMMNetV2 (affect_dyn.py:107-175: expert 1 = text Transformer + MLP head,
expert 2 = 3-modality late-fusion MMDL, gate = Transformer(409, 10) + Linear(10, 2), DiffSoftmax, convex blend,
regulariser mean(w[:, 1])) and DynMMNet (affect_dyn.py:31-104: three uni-modal experts, 3-way gate).

Modules are parameter containers with torch's own state_dict keys (`conv.weight`, `transformer.layers.N.self_attn.
in_proj_weight`, ...), so `expert.state_dict()` of a trained MultiBench module loads with load_state_dict.  Dropout
(p = 0.1 inside nn.TransformerEncoderLayer) is applied in training mode at torch's four sites per layer, with a Philox
stream of its own (ops.manual_seed; torch's generator cannot be reproduced bit for bit, the tests inject the keep flags
on both sides); `.eval()` switches it off as in torch.

Hard-gate inference runs each expert only on the samples routed to it (`compact`, on by default): the gate transformer runs on
the whole batch, its one-hot decisions are recorded as the dense path records them, the samples are grouped by expert on the
device (ops_mlp.partition), one host read fetches the group sizes, and each expert runs on its rows alone (an expert with no
row launches nothing).  Training, the soft gate, infer_mode != 0 and anything under autograd keep the dense path.
"""

import torch
import torch.nn as nn

from .. import engine, ops
from .. import ops_mlp as M
from .. import ops_seq as S

FEATURES = {'visual': 35, 'audio': 74, 'text': 300}      # CMU-MOSEI (affect/count_flop.py:52)

# The gate transformer and the experts' encoders are independent until the mixture: each runs on a HIP stream of its own
# (five 5-layer transformers on 50-token sequences are chains of ~10-100 us kernels that do not fill 256 CUs one at a time).
# Autograd replays a node on its forward stream, so the backward is concurrent too; a captured step keeps the branches as
# parallel paths of the hipGraph.
BRANCH_STREAMS = True     # (module attribute; False: one stream)
LINK_RESIDUAL = True      # (module attribute; False: autograd sums the two gradients of a layer's input)
_POOL, _ALL = [], []


def run_branches(fns):
    """[f() for f in fns], fns[1:] each on a side stream forked from / joined to the current one."""
    if not (BRANCH_STREAMS and len(fns) > 1 and torch.cuda.is_available()):
        return [f() for f in fns]
    main = torch.cuda.current_stream()
    taken = []
    for _ in fns[1:]:
        if not _POOL:
            _POOL.append(torch.cuda.Stream())
            _ALL.append(_POOL[-1])
        taken.append(_POOL.pop())
    # fork BEFORE branch 0 is enqueued on `main`: a side stream that waited for `main` afterwards would wait for the whole of
    # branch 0 (in DynMMNetV2: the gate transformer), i.e. one branch followed by four instead of five in parallel — also in
    # the captured hipGraph.  The event marks the inputs' readiness only.
    fork = torch.cuda.Event()
    fork.record(main)
    if torch.cuda.is_current_stream_capturing():
        ops._CAPTURE_EVENTS.append(fork)           # an event recorded into a capture must outlive it (ops._queue_wgrad)
    first = fns[0]()                               # host order = list order (the injected-mask tests count calls)
    outs = []
    for st, f in zip(taken, fns[1:]):
        st.wait_event(fork)
        with torch.cuda.stream(st):
            outs.append(f())
    capturing = torch.cuda.is_current_stream_capturing()
    for st, o in zip(taken, outs):
        main.wait_stream(st)
        if not capturing:
            for t in (o if isinstance(o, (list, tuple)) else [o]):
                if torch.is_tensor(t):
                    t.record_stream(main)          # allocated on the side stream, consumed on `main`
    _POOL.extend(taken)
    return [first] + outs


def join_branches():
    """After a backward pass: the calling stream waits for every branch stream (their nodes ran there)."""
    ops.flush_wgrad_groups()                       # queued weight-gradient groups go out on their branch's stream
    if _ALL:
        main = torch.cuda.current_stream()
        for st in _ALL:
            main.wait_stream(st)


def encoder_layer(h, layer, heads):
    """nn.TransformerEncoderLayer.forward (post-norm): h [B, D, T].  In training mode the layer's four dropouts act where
    torch applies them: on the attention probabilities (MultiheadAttention.dropout), on the attention block's output
    (dropout1, fused into norm1's kernel), on the feed-forward hidden layer (dropout) and on the feed-forward output
    (dropout2, fused into norm2's kernel)."""
    sa = layer.self_attn
    train = layer.training
    site = getattr(layer, '_dynmm_sites', None)
    if site is None:
        site = layer._dynmm_sites = S.new_sites(4)
    p_att = float(sa.dropout) if train else 0.0
    p1, pf, p2 = ((float(m.p) if train else 0.0) for m in (layer.dropout1, layer.dropout, layer.dropout2))
    # h feeds in_proj and norm1's residual input: norm1's backward (which runs first) leaves the residual branch's gradient with
    # the link and in_proj's input-gradient epilogue adds it (no accumulation pass by autograd)
    link = ops.GradLink() if LINK_RESIDUAL else None
    qkv = S.linear_bdt(h, sa.in_proj_weight, sa.in_proj_bias, link=link)
    a = S.attention(qkv, heads, drop=(p_att, site, 'attn'))      # dh <= 32: mha_core, above: mha_wide
    o = S.linear_bdt(a, sa.out_proj.weight, sa.out_proj.bias)
    h1 = S.layernorm_bdt(o, layer.norm1.weight, layer.norm1.bias, layer.norm1.eps, residual=h, drop=(p1, site + 1, 'dropout1'),
                         res_link=link)
    if S.ffn_fused_ok(h1, layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias):
        # linear1 -> ReLU -> dropout -> linear2 -> dropout2 -> + h1 -> norm2: two launches (csrc/seq_ffn.hip)
        return S.ffn_block(h1, layer, (pf, site + 2, 'dropout'), (p2, site + 3, 'dropout2'))
    if pf > 0:
        f = S.linear_bdt(h1, layer.linear1.weight, layer.linear1.bias, act='relu')
        f = S.dropout_bdt(f, pf, site + 2, 'dropout')
        f = S.linear_bdt(f, layer.linear2.weight, layer.linear2.bias)
    else:
        # the ReLU backward of linear1 is applied in the input-gradient epilogue of linear2 (its only consumer)
        f = S.linear_bdt(h1, layer.linear1.weight, layer.linear1.bias, act='relu', defer_mask=True)
        f = S.linear_bdt(f, layer.linear2.weight, layer.linear2.bias, mask_input=True)
    return S.layernorm_bdt(f, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps, residual=h1, drop=(p2, site + 3, 'dropout2'))


class Transformer(nn.Module):
    def __init__(self, n_features, dim, nhead=5, num_layers=5, dim_feedforward=2048):
        super().__init__()
        self.embed_dim, self.nhead = dim, nhead
        self.conv = nn.Conv1d(n_features, dim, kernel_size=1, padding=0, bias=False)
        layer = nn.TransformerEncoderLayer(d_model=dim, nhead=nhead, dim_feedforward=dim_feedforward)
        self.transformer = nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False)

    def forward(self, x):
        if isinstance(x, (list, tuple)):
            x = x[0]                                            # [x, lengths]: the lengths are ignored
        h = S.linear_bdt(x.permute(0, 2, 1).contiguous(), self.conv.weight)      # [B, dim, T]
        for layer in self.transformer.layers:
            h = encoder_layer(h, layer, self.nhead)
        return h[:, :, -1].contiguous()                         # `self.transformer(x)[-1]`: the last time step


class MLP(nn.Module):
    def __init__(self, indim, hiddim, outdim):
        super().__init__()
        self.fc = nn.Linear(indim, hiddim)
        self.fc2 = nn.Linear(hiddim, outdim)

    def forward(self, x):
        return S.linear_bdt(S.linear_bdt(x, self.fc.weight, self.fc.bias, act='relu'), self.fc2.weight, self.fc2.bias)


class GRU(nn.Module):
    """MultiBench unimodals.common_models.GRU.  `self.gru` is torch's nn.GRU as a PARAMETER CONTAINER (state_dict keys
    gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0); its forward is never called: the input projection is
    the 1x1-convolution GEMM, the recurrence csrc/gru.hip (ops_seq.gru_seq).  The dropout site is named 'gru_dropout'."""

    def __init__(self, indim, hiddim, dropout=False, dropoutp=0.1, flatten=False, has_padding=False, last_only=False,
                 batch_first=True):
        super().__init__()
        if not batch_first:
            raise NotImplementedError('GRU(batch_first=False): the reference only builds batch-first GRUs')
        self.gru = nn.GRU(indim, hiddim, batch_first=True)
        self.dropout = dropout
        self.dropout_layer = nn.Dropout(dropoutp)
        self.flatten, self.has_padding, self.last_only, self.batch_first = flatten, has_padding, last_only, batch_first
        self.arm = None               # (tests: 'resident' | 'stepped' forces a dispatch arm)
        self._site = S.new_sites(1)

    def forward(self, x):
        g = self.gru
        w = (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
        if self.has_padding:
            out, _ = S.gru_seq(x[0], *w, lengths=x[1], arm=self.arm)
        else:
            hn, seq = S.gru_seq(x, *w, arm=self.arm)
            out = hn if self.last_only else seq
        if self.dropout and self.training:
            out = S.dropout_bdt(out, self.dropout_layer.p, self._site, 'gru_dropout')
        if self.flatten:
            out = torch.flatten(out, 1)
        return out


class GRUWithLinear(nn.Module):
    """MultiBench unimodals.common_models.GRUWithLinear: nn.GRU(indim, hiddim) (a parameter container, as in GRU above) followed by
    nn.Linear(hiddim, outdim); state_dict keys gru.*, linear.weight, linear.bias.  has_padding: h_n of the packed [x, lengths]
    (batch-first) -> Dropout -> linear, [B, outdim]; else the linear layer on the whole state sequence of x [B, T, F],
    [B, T, outdim].  The dropout site is named 'gru_dropout'."""

    def __init__(self, indim, hiddim, outdim, dropout=False, dropoutp=0.1, flatten=False, has_padding=False):
        super().__init__()
        self.gru = nn.GRU(indim, hiddim)
        self.linear = nn.Linear(hiddim, outdim)
        self.dropout = dropout
        self.dropout_layer = nn.Dropout(dropoutp)
        self.flatten, self.has_padding = flatten, has_padding
        self.arm = None               # (tests: 'resident' | 'stepped' forces a dispatch arm)
        self._site = S.new_sites(1)

    def forward(self, x):
        g = self.gru
        w = (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
        if self.has_padding:
            hidden, _ = S.gru_seq(x[0], *w, lengths=x[1], arm=self.arm)          # [B, H]
        else:
            hidden = S.gru_seq(x, *w, arm=self.arm)[1]                           # [B, T, H]
        if self.dropout and self.training:
            hidden = S.dropout_bdt(hidden, self.dropout_layer.p, self._site, 'gru_dropout')
        if hidden.dim() == 3:
            out = S.linear_bdt(hidden.permute(0, 2, 1).contiguous(), self.linear.weight, self.linear.bias)
            out = out.permute(0, 2, 1).contiguous()
        else:
            out = S.linear_bdt(hidden, self.linear.weight, self.linear.bias)
        if self.flatten:
            out = torch.flatten(out, 1)
        return out


class LowRankTensorFusion(nn.Module):
    """MultiBench fusions.common_fusions.LowRankTensorFusion(input_dims, output_dim, rank, flatten=True) on ops_seq.lrtf.  The
    factors, fusion_weights and fusion_bias are REGISTERED parameters (keys factors.0, factors.1, ..., fusion_weights,
    fusion_bias): MultiBench's `nn.Parameter(...).to(device)` leaves them out of parameters() and state_dict() on a GPU."""

    def __init__(self, input_dims, output_dim, rank, flatten=True):
        super().__init__()
        if not flatten:
            raise NotImplementedError('LowRankTensorFusion(flatten=False): the reference only builds flatten=True')
        if len(input_dims) not in (2, 3):
            raise NotImplementedError(f'LowRankTensorFusion over {len(input_dims)} modalities: the HIP kernels serve 2 or 3')
        self.input_dims, self.output_dim, self.rank, self.flatten = list(input_dims), output_dim, rank, flatten
        self.factors = nn.ParameterList(
            [nn.Parameter(nn.init.xavier_normal_(torch.empty(rank, d + 1, output_dim))) for d in input_dims])
        self.fusion_weights = nn.Parameter(nn.init.xavier_normal_(torch.empty(1, rank)))
        self.fusion_bias = nn.Parameter(torch.zeros(1, output_dim))
        self._register_state_dict_hook(self._factors_first)

    @staticmethod
    def _factors_first(module, state_dict, prefix, local_metadata):
        # the keys in the order the module creates its tensors (a ParameterList is a child module: torch lists it last)
        for k in ('fusion_weights', 'fusion_bias'):
            state_dict.move_to_end(prefix + k)

    def forward(self, modalities):
        return S.lrtf([m.flatten(1) for m in modalities], list(self.factors), self.fusion_weights, self.fusion_bias)


class Identity(nn.Module):
    """MultiBench unimodals.common_models.Identity."""

    def forward(self, x):
        return x


class Sequential(nn.Sequential):
    """MultiBench unimodals.common_models.Sequential: nn.Sequential whose first layer may take [x, lengths]."""


class ConcatEarly(nn.Module):
    """MultiBench fusions.common_fusions.ConcatEarly: the modalities side by side along the feature axis of [B, T, F]."""

    def forward(self, modalities):
        return torch.cat(modalities, dim=2)


class Concat(nn.Module):
    def forward(self, modalities):
        return torch.cat([m.flatten(1) for m in modalities], dim=1)


class MMDL(nn.Module):
    """Supervised_Learning.py:16-51.  With has_padding, encoders that return [x, lengths] (Identity under ConcatEarly) have
    their tensors fused and the head receives [fused, lengths of modality 0]."""

    def __init__(self, encoders, fusion, head, has_padding=True):
        super().__init__()
        self.encoders = nn.ModuleList(encoders)
        self.fuse, self.head, self.has_padding = fusion, head, has_padding

    def forward(self, inputs):
        fns = self.branch_fns(inputs)
        # (Identity encoders launch nothing: no side streams for them)
        outs = [f() for f in fns] if all(isinstance(e, Identity) for e in self.encoders) else run_branches(fns)
        if self.has_padding and not torch.is_tensor(outs[0]):
            out = self.head([self.fuse([o[0] for o in outs]), inputs[1][0]])
        else:
            out = self.head(self.fuse(outs))
        return out[0] if type(out) is list else out

    def branch_fns(self, inputs):
        if self.has_padding:
            return [lambda i=i, enc=enc: enc([inputs[0][i], inputs[1][i]]) for i, enc in enumerate(self.encoders)]
        return [lambda i=i, enc=enc: enc(inputs[i]) for i, enc in enumerate(self.encoders)]


def late_fusion_gru():
    """affect_mm.py:45-55 (`--fusion 1`, saved as lf_gru.pt)."""
    return MMDL([GRU(35, 64, dropout=True, has_padding=True), GRU(74, 128, dropout=True, has_padding=True),
                 GRU(300, 512, dropout=True, has_padding=True)], Concat(), MLP(704, 512, 1))


def low_rank_fusion_gru(rank=32):
    """affect_mm.py:88-93 (`--fusion 5`, saved as lrtf.pt)."""
    kw = dict(dropout=True, has_padding=True)
    return MMDL([GRUWithLinear(35, 64, 32, **kw), GRUWithLinear(74, 128, 32, **kw), GRUWithLinear(300, 512, 128, **kw)],
                LowRankTensorFusion([32, 32, 128], 128, rank), MLP(128, 512, 1))


def early_fusion_gru():
    """affect_mm.py:40-44 (`--fusion 0`, saved as ef_gru.pt)."""
    return MMDL([Identity(), Identity(), Identity()], ConcatEarly(),
                Sequential(GRU(409, 512, dropout=True, has_padding=True), MLP(512, 256, 1)))


def early_fusion_transformer():
    """affect_mm.py:56-59 (`--fusion 2`, saved as ef_tran.pt): one transformer over the three modalities side by side.
    d_model = 300 at nhead = 5 is head dimension 60: the attention core is ops_seq.mha_wide (csrc/attn.hip), the feed-forward
    block runs layer by layer (the fused block serves D <= 128)."""
    return MMDL([Identity(), Identity(), Identity()], ConcatEarly(), Sequential(Transformer(409, 300), MLP(300, 128, 1)))


def late_fusion_transformer():
    """affect_mm.py:61-66 (`--fusion 3`, saved as lf_tran.pt): the second expert of DynMMNetV2."""
    return MMDL([Transformer(35, 60), Transformer(74, 120), Transformer(300, 120)], Concat(), MLP(300, 128, 1))


class _GatedMixture(nn.Module):
    compact = True          # hard-gate eval runs each expert on its own samples only (False: the dense blend, for A/B runs)

    def _init_gate(self, branch_num, temp, hard_gate):
        self.branch_num = branch_num
        self.gate = nn.Sequential(Transformer(409, 10), nn.Linear(10, branch_num))       # affect_dyn.py:41,120
        self.temp, self.hard_gate = temp, hard_gate
        self.weight_list = torch.Tensor()
        self.store_weight = False
        self.infer_mode = 0
        self.last_counts = None            # per-expert sample counts of the last compacted forward

    @staticmethod
    def freeze_branch(m):
        for p in m.parameters():
            p.requires_grad = False

    def reset_weight(self):
        self.weight_list = torch.Tensor()
        self.store_weight = True

    def cal_flop(self):
        tmp = torch.mean(self.weight_list, dim=0)
        total = (self.flop * tmp).sum()
        print(f'Total Flops {total.item():.2f}M')
        return total.item()

    def gate_logits(self, inputs):
        x = torch.cat(inputs[0], dim=2)                                                   # [B, T, 409]
        return S.linear_bdt(self.gate[0]([x, inputs[1][0]]), self.gate[1].weight, self.gate[1].bias)

    def _mix(self, logits, preds):
        # affect_dyn.py:152-165: the gate's own DiffSoftmax weight is computed and RECORDED first, whatever infer_mode then
        # does with the prediction (cal_flop / weight_stat read weight_list after every evaluation mode)
        out, aux, weight = S.moe_blend(logits, preds, self.temp, self.hard_gate)
        if self.store_weight:
            self.weight_list = torch.cat((self.weight_list, weight.detach().cpu()))
        if self.infer_mode > 0:
            return preds[self.infer_mode - 1], 0
        if self.infer_mode == -1:                       # uniform weights (affect_dyn.py:161-162)
            out, aux, _ = S.moe_blend(torch.zeros_like(logits), preds, self.temp, False)
        return out, aux

    # ---- hard-gate compaction ----------------------------------------------------------------------------------------
    def _compacting(self):
        return (self.compact and not self.training and self.hard_gate and self.infer_mode == 0 and
                not torch.is_grad_enabled())

    def _route(self, inputs):
        """The gate on every sample, its weight recorded as _mix records it, the samples grouped by expert.  Returns
        (aux [1], inv [B], counts [K], device rows [K], host rows [K]) after ONE device -> host read (counts and order)."""
        weight, aux = M.gate_weight(self.gate_logits(inputs), self.temp, True)
        order, inv, counts = M.partition(weight)            # (enqueued before the recording below waits for the device)
        if self.store_weight:
            self.weight_list = torch.cat((self.weight_list, weight.detach().cpu()))
        K = weight.shape[1]
        host = torch.cat([counts, order]).cpu()
        n = [int(v) for v in host[:K]]
        self.last_counts = tuple(n)
        rows_d, rows_h, off = [], [], 0
        for k in range(K):
            rows_d.append(order[off:off + n[k]])
            rows_h.append(host[K + off:K + off + n[k]].long())
            off += n[k]
        return aux, inv, n, rows_d, rows_h

    @staticmethod
    def _rows(inputs, modalities, rows_d, rows_h):
        """[[x_i[rows]], [lengths_i[rows]]] for the listed modalities i (x_i [B, T, F] on the device; the lengths follow the
        same rows wherever they live)."""
        xs = [ops.batch_gather(inputs[0][i], rows_d) for i in modalities]
        lens = []
        for i in modalities:
            ln = inputs[1][i]
            if torch.is_tensor(ln):
                lens.append(ln[rows_d.long()] if ln.is_cuda else ln[rows_h])
            else:
                lens.append([ln[j] for j in rows_h.tolist()])
        return [xs, lens]

    @staticmethod
    def _merge(parts, inv):
        """The experts' [n_k, 1] outputs (in expert order) back in the batch's order."""
        if len(parts) == 1:
            return parts[0]                         # every sample took one expert: order and inv are the identity
        return ops.batch_gather(torch.cat(parts, dim=0), inv)


class DynMMNetV2(_GatedMixture):
    """affect_dyn.py:107-175.  The reference loads pickled experts (`torch.load(model_name_list[i])`); here they are
    constructed (random init) and filled with load_state_dict."""

    def __init__(self, temp=1.0, hard_gate=False, freeze=False, model_name_list=None):
        super().__init__()
        self.text_encoder = Transformer(300, 120)            # affect_uni.py:68-73 (`--enc transformer`, text)
        self.text_head = MLP(120, 64, 1)
        self.branch2 = late_fusion_transformer()
        if model_name_list:
            raise NotImplementedError('pickled MultiBench modules cannot be loaded without MultiBench; export their '
                                      'state_dict and use load_state_dict')
        if freeze:
            for m in (self.text_encoder, self.text_head, self.branch2):
                self.freeze_branch(m)
        self._init_gate(2, temp, hard_gate)
        self.flop = torch.Tensor([135.13226, 320.03205])     # affect_dyn.py:126

    def experts(self, inputs):
        return [self.text_head(self.text_encoder([inputs[0][2], inputs[1][2]])), self.branch2(inputs)]

    def gate_and_experts(self, inputs):
        """(gate logits, [expert predictions]) with the five transformers side by side."""
        b2 = self.branch2
        enc = run_branches([lambda: self.gate_logits(inputs), lambda: self.text_encoder([inputs[0][2], inputs[1][2]])]
                           + b2.branch_fns(inputs))
        return enc[0], [self.text_head(enc[1]), b2.head(b2.fuse(enc[2:]))]

    def forward(self, inputs):
        if self._compacting():
            return self._forward_compact(inputs)
        return self._mix(*self.gate_and_experts(inputs))

    def _forward_compact(self, inputs):
        """Expert 1 (text transformer + head) on its rows' text, expert 2 (the late-fusion model) on its rows' three modalities,
        the four transformers side by side."""
        aux, inv, n, rows_d, rows_h = self._route(inputs)
        b2 = self.branch2
        fns = []
        if n[0]:
            s1 = self._rows(inputs, (2,), rows_d[0], rows_h[0])
            fns.append(lambda: self.text_head(self.text_encoder([s1[0][0], s1[1][0]])))
        if n[1]:
            fns += b2.branch_fns(self._rows(inputs, (0, 1, 2), rows_d[1], rows_h[1]))
        outs = run_branches(fns)
        parts = [outs[0]] if n[0] else []
        if n[1]:
            parts.append(b2.head(b2.fuse(outs[1 if n[0] else 0:])))
        return self._merge(parts, inv), aux[0]

    def weight_stat(self):
        tmp = torch.mean(self.weight_list, dim=0)
        print(f'mean branch weight {tmp[0].item():.4f}, {tmp[1].item():.4f}')
        self.store_weight = False
        return tmp[1].item()


class DynMMNet(_GatedMixture):
    """affect_dyn.py:31-104 (`forward2`): three uni-modal experts (visual, audio, text), 3-way gate."""

    def __init__(self, temp=1.0, hard_gate=False, freeze=True):
        super().__init__()
        self.encoders = nn.ModuleList([Transformer(FEATURES[m], 120) for m in ('visual', 'audio', 'text')])
        self.heads = nn.ModuleList([MLP(120, 64, 1) for _ in range(3)])
        if freeze:
            self.freeze_branch(self.encoders)
            self.freeze_branch(self.heads)
        self._init_gate(3, temp, hard_gate)
        # MMAC per sample of each expert for cal_flop (the reference's DynMMNet defines none): the text expert is DynMMNetV2's
        # expert 1 (affect_dyn.py:126); the visual / audio experts differ from it only in the Conv1d (F -> 120 over 50 steps)
        self.flop = torch.Tensor([135.13226 - (300 - f) * 120 * 50 / 1e6 for f in (35, 74, 300)])

    def experts(self, inputs):
        return [self.heads[i](self.encoders[i]([inputs[0][i], inputs[1][i]])) for i in range(3)]

    def gate_and_experts(self, inputs):
        outs = run_branches([lambda: self.gate_logits(inputs)]
                            + [lambda i=i: self.heads[i](self.encoders[i]([inputs[0][i], inputs[1][i]])) for i in range(3)])
        return outs[0], outs[1:]

    def forward(self, inputs):
        if self._compacting():
            return self._forward_compact(inputs)
        return self._mix(*self.gate_and_experts(inputs))

    def _forward_compact(self, inputs):
        """Expert k (modality k's transformer + head) on its rows of modality k, side by side."""
        aux, inv, n, rows_d, rows_h = self._route(inputs)
        fns = [lambda k=k, s=self._rows(inputs, (k,), rows_d[k], rows_h[k]): self.heads[k](self.encoders[k]([s[0][0], s[1][0]]))
               for k in range(3) if n[k]]
        return self._merge(run_branches(fns), inv), aux[0]

    def weight_stat(self):
        """mean gate weight per expert; returns the text expert's (the one the regulariser penalises, affect_dyn.py:96)."""
        tmp = torch.mean(self.weight_list, dim=0)
        print(f'mean branch weight {tmp[0].item():.4f}, {tmp[1].item():.4f}, {tmp[2].item():.4f}')
        self.store_weight = False
        return tmp[2].item()


class AffectTrainStep(engine.FlatAdamWStep):
    """engine.FlatAdamWStep for a DynMM mixture (`moe_model`, additional_loss=True; Supervised_Learning.train :104-144): L1
    objective + lossw * gate regulariser, with the loss and the backward seeds computed on the device.  The step is ~700 small
    launches (5-layer transformers on 50-token sequences), launch-bound when issued eagerly: hence use_graph (temp, hard_gate
    and the batch shape are frozen into a capture)."""

    def __init__(self, model, lr=1e-6, weight_decay=1e-4, lossw=0.0, clip_val=8.0, use_graph=False):
        # a transformer is num_layers same-shape layers on one stream: its linear1 / linear2 / in_proj / out_proj weight gradients go
        # out as ONE grouped launch each (the library's default group of 4 left every fifth layer to a launch of its own, split
        # 16 ways over the pixel range to fill the chip)
        depth = max([len(m.layers) for m in model.modules() if isinstance(m, nn.TransformerEncoder)] or [1])
        super().__init__(model, lr, weight_decay, clip_val, use_graph, prepack=ops.PackedWeights(), wgrad_group=min(8, depth))
        self.lossw = float(lossw)

    def _backward(self, inputs, target):
        m = self.model
        logits, preds = m.gate_and_experts(inputs)
        last = S.moe_loss_backward(logits, preds, target, m.temp, m.hard_gate, self.lossw)
        join_branches()
        return last['total'], last

    def _graph_key(self, inputs, target):
        m = self.model
        return (tuple(tuple(x.shape) for x in inputs[0]), float(m.temp), bool(m.hard_gate), bool(m.training))

    def _clone_inputs(self, inputs):
        return [[x.clone() for x in inputs[0]], inputs[1]]       # (the padding lengths are ignored by the model: kept as they are)

    def _input_tensors(self, inputs):
        return inputs[0]
