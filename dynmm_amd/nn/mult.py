"""MULT, the multimodal transformer of `affect_mm.py --fusion 4` (ModalityDynMM/affect/affect_mm.py:68-86), on the HIP path.

PARITY UNPINNED, like the rest of the MultiBench modules (nn/affect.py): the reference builds
`MMDL([Identity()] * 3, MULTModel(3, [35, 74, 300], HParams), Identity())` from MultiBench's `fusions.mult`, which it neither
vendors nor pins.  The modules below restate the PUBLISHED definition of that file (MultiBench fusions/mult.py, itself the
multimodal transformer of Tsai et al. on fairseq's attention); nothing here rests on a file next to this project.

  MULTModel(M, n_features, hp), E = hp.embed_dim
      proj[i] = Conv1d(n_features[i], E, 1, bias=False)
      trans[i][j] (every i, j in 0..M-1, i == j included) = TransformerEncoder(E, heads, layers, attn_dropout =
                    hp.attn_dropout_modalities[j])
      trans_mems[i] = TransformerEncoder(M E, heads, max(layers, 3), attn_dropout = hp.attn_dropout)
      proj1, proj2 = Linear(M^2 E, M^2 E), out_layer = Linear(M^2 E, output_dim)
      forward: p_i = proj[i](x_i); for each target i: h_i = cat_j trans[i][j](p_i, p_j, p_j) along channels, then
      trans_mems[i](h_i), of which the LAST time step is kept ([B, M E]); z = cat_i of those; out =
      out_layer(proj2(dropout(relu(proj1(z)), out_dropout)) + z).
  TransformerEncoder(E, H, L, attn_dropout, relu_dropout, res_dropout, embed_dropout, attn_mask), called (x_q, x_k=None, x_v=None)
      every given input is embedded as dropout(sqrt(E) x + pos(x), embed_dropout), each with dropout decisions of its OWN (in
      training x_k and x_v differ although both come from p_j); pos(x)[b, :, t] is the sinusoid of position t + 1 (channels
      c < E/2: sin((t+1) w_c), c >= E/2: cos((t+1) w_{c-E/2}), w_c = exp(-c ln(10000) / (E/2 - 1))), zeros where x[b, 0, t] == 0.0
      exactly (a padded step: zero-padded MOSEI steps project to exactly 0 through the bias-free conv); pos carries no gradient.
      L pre-norm layers, then layer_norm = LayerNorm(E).  x_k and x_v stay the embedded inputs in every layer; only x evolves.
  TransformerEncoderLayer
      r = x; x = LN0(x) (cross-modal calls: also k = LN0(x_k), v = LN0(x_v), the same LN0);
      x = r + dropout(out_proj(attn(Wq x + bq, Wk k + bk, Wv v + bv)), res_dropout);
      r = x; x = r + dropout(fc2(dropout(relu(fc1(LN1(x))), relu_dropout)), res_dropout);   fc1 = Linear(E, 4E), fc2 = Linear(4E, E)
  MultiheadAttention
      dropout(softmax(q k^T / sqrt(dh) + mask), attn_dropout) v per head; the mask is -inf where key - query >= 1 + |Tk - Tq|
      (torch.triu(..., 1 + |Tk - Tq|)), applied whenever attn_mask — in self-attention calls too.

state_dict keys are the published module's: proj.{i}.weight; trans.{i}.{j}. and trans_mems.{i}. followed by
layers.{l}.self_attn.{in_proj_weight [3E, E], in_proj_bias, out_proj.weight, out_proj.bias}, layers.{l}.fc1.*, layers.{l}.fc2.*,
layers.{l}.layer_norms.{0,1}.*, layer_norm.*; proj1.*, proj2.*, out_layer.* (under MMDL: prefix `fuse.`).  The published encoder
also registers two non-parameter buffers, `version` ([2.]) and `embed_positions._float_tensor` (shape [1]): both are registered
here so that an exported MultiBench state_dict loads strictly; nothing reads their values.  3 080 321 parameters at the
reference's HParams.

The modules are parameter containers.  On the HIP path a layer is: the 1x1-convolution GEMMs (ops_seq.linear_bdt), masked
cross-modal attention (ops_seq.masked_attention / packed_masked_attention: csrc/xattn.hip up to 64 steps, the streaming kernels of
csrc/attn_long.hip beyond, so the modalities may differ in length), and ONE launch per residual connection that
returns both `r + dropout(x)` and the LayerNorm that follows it (ops_seq.prenorm_bdt) — the next layer's LN0 or the encoder's
final layer_norm.  Dropout sites come from ops_seq.new_sites and are named 'embed_q', 'embed_k', 'embed_v', 'attn', 'res1',
'relu', 'res2' (per encoder, in call order) and 'out' (the head); `.eval()` switches every site off, and then the key / value
embedding and its LN0 are computed once and shared.
"""
import math

import torch
import torch.nn as nn

from .. import ops
from .. import ops_seq as S


class HParams:
    """affect_mm.py:69-83."""
    num_heads = 10
    layers = 4
    attn_dropout = 0.1
    attn_dropout_modalities = [0, 0, 0.1]
    relu_dropout = 0.1
    res_dropout = 0.1
    out_dropout = 0.1
    embed_dropout = 0.2
    embed_dim = 40
    attn_mask = True
    output_dim = 1
    all_steps = False


def sinusoid_table(E, T):
    """[E, T] float64: column t = the embedding of position t + 1 (sin half | cos half; an odd E ends in a zero row)."""
    half = E // 2
    w = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000.0) / (half - 1)))
    ang = w[:, None] * torch.arange(1, T + 1, dtype=torch.float64)[None, :]
    tab = torch.cat([ang.sin(), ang.cos()], dim=0)
    if E % 2:
        tab = torch.cat([tab, torch.zeros(1, T, dtype=torch.float64)], dim=0)
    return tab


class SinusoidalPositionalEmbedding(nn.Module):
    """The published module's buffer `_float_tensor` (a device / dtype marker there) and the [E, T] table per length."""

    def __init__(self, embedding_dim):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.register_buffer('_float_tensor', torch.zeros(1))
        self.__dict__['_tables'] = {}

    def table(self, T, device):
        key = (T, str(device))
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = sinusoid_table(self.embedding_dim, T).float().to(device)
        return t


class MultiheadAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, attn_dropout=0.0):
        super().__init__()
        if embed_dim % num_heads:
            raise ValueError('embed_dim must be divisible by num_heads')
        self.embed_dim, self.num_heads, self.attn_dropout = embed_dim, num_heads, attn_dropout
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.xavier_uniform_(self.out_proj.weight)
        nn.init.constant_(self.out_proj.bias, 0.0)
        self.__dict__['_rows'] = {}

    def rows(self, name, lo, hi):
        """Rows lo..hi-1 of in_proj_weight / in_proj_bias as the operand of one projection.  Inside a training step the slice is a
        leaf of its own whose .grad is the matching slice of the parameter's gradient buffer, so that the GEMM's weight gradient
        is written in place (ops._grad_dst); under plain autograd it is an ordinary slice."""
        p = getattr(self, name)
        if not (torch.is_grad_enabled() and p.requires_grad):
            return p.detach()[lo:hi]
        if not (ops.in_step() and ops._direct_ok(p)):
            return p[lo:hi]
        a = self._rows.get((name, lo))
        g = p.grad[lo:hi]
        if a is None or a.data_ptr() != p[lo:hi].data_ptr() or a.grad is None or a.grad.data_ptr() != g.data_ptr():
            a = nn.Parameter(p.detach()[lo:hi])            # (a Parameter: the step's one-launch weight re-layout registers it)
            a.grad = g
            self._rows[(name, lo)] = a
        return a


class TransformerEncoderLayer(nn.Module):
    def __init__(self, embed_dim, num_heads=4, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, attn_mask=False):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.self_attn = MultiheadAttention(embed_dim, num_heads, attn_dropout)
        self.attn_mask, self.relu_dropout, self.res_dropout = attn_mask, relu_dropout, res_dropout
        self.normalize_before = True
        self.fc1 = nn.Linear(embed_dim, 4 * embed_dim)
        self.fc2 = nn.Linear(4 * embed_dim, embed_dim)
        self.layer_norms = nn.ModuleList([nn.LayerNorm(embed_dim) for _ in range(2)])

    def attention_block(self, y, xk, xv, site):
        """out_proj(attn(...)) of the normalised x `y`; xk / xv: the embedded key / value inputs (None: self-attention)."""
        sa, E, H = self.self_attn, self.embed_dim, self.num_heads
        p_att = float(sa.attn_dropout) if self.training else 0.0
        drop = (p_att, site, 'attn')
        if xk is None:
            qkv = S.linear_bdt(y, sa.in_proj_weight, sa.in_proj_bias)
            a = S.packed_masked_attention(qkv, H, self.attn_mask, drop)
        else:
            ln0 = self.layer_norms[0]
            kn = S.prenorm_bdt(xk, ln0.weight, ln0.bias, ln0.eps, shared=True)
            vn = kn if xv is xk else S.prenorm_bdt(xv, ln0.weight, ln0.bias, ln0.eps, shared=True)
            q = S.linear_bdt(y, sa.rows('in_proj_weight', 0, E), sa.rows('in_proj_bias', 0, E))
            k = S.linear_bdt(kn, sa.rows('in_proj_weight', E, 2 * E), sa.rows('in_proj_bias', E, 2 * E))
            v = S.linear_bdt(vn, sa.rows('in_proj_weight', 2 * E, 3 * E), sa.rows('in_proj_bias', 2 * E, 3 * E))
            a = S.masked_attention(q, k, v, H, self.attn_mask, drop)
        return S.linear_bdt(a, sa.out_proj.weight, sa.out_proj.bias)

    def feed_forward(self, y, site):
        pf = float(self.relu_dropout) if self.training else 0.0
        if pf > 0:
            f = S.linear_bdt(y, self.fc1.weight, self.fc1.bias, act='relu')
            f = S.dropout_bdt(f, pf, site, 'relu')
            return S.linear_bdt(f, self.fc2.weight, self.fc2.bias)
        # the ReLU backward of fc1 is applied in the input-gradient epilogue of fc2 (its only consumer)
        f = S.linear_bdt(y, self.fc1.weight, self.fc1.bias, act='relu', defer_mask=True)
        return S.linear_bdt(f, self.fc2.weight, self.fc2.bias, mask_input=True)


class TransformerEncoder(nn.Module):
    """(x_q [B, E, Tq], x_k = None, x_v = None [B, E, Tk]) -> [B, E, Tq] (activations are [B, D, T] as everywhere on this path)."""

    def __init__(self, embed_dim, num_heads, layers, attn_dropout=0.0, relu_dropout=0.0, res_dropout=0.0, embed_dropout=0.0,
                 attn_mask=False):
        super().__init__()
        self.dropout = embed_dropout
        self.attn_dropout = attn_dropout
        self.embed_dim = embed_dim
        self.embed_scale = math.sqrt(embed_dim)
        self.embed_positions = SinusoidalPositionalEmbedding(embed_dim)
        self.attn_mask = attn_mask
        self.layers = nn.ModuleList([TransformerEncoderLayer(embed_dim, num_heads, attn_dropout, relu_dropout, res_dropout,
                                                             attn_mask) for _ in range(layers)])
        self.register_buffer('version', torch.Tensor([2]))
        self.normalize = True
        self.layer_norm = nn.LayerNorm(embed_dim)
        self._site = S.new_sites(3 + 4 * layers)        # embed_q, embed_k, embed_v, then attn / res1 / relu / res2 per layer

    def embed(self, x_q, x_k, x_v):
        pe = float(self.dropout) if self.training else 0.0
        st, sc, pos = self._site, self.embed_scale, self.embed_positions
        x = S.pos_embed(x_q, pos.table(x_q.shape[2], x_q.device), sc, drop=(pe, st, 'embed_q'))
        if x_k is None:
            return x, None, None
        tk = pos.table(x_k.shape[2], x_k.device)
        if x_v is not x_k:
            return x, S.pos_embed(x_k, tk, sc, drop=(pe, st + 1, 'embed_k')), S.pos_embed(x_v, tk, sc, drop=(pe, st + 2, 'embed_v'))
        if pe > 0:
            # one source, two embeddings with decisions of their own: one launch, two sites
            xk, xv = S.pos_embed(x_k, tk, sc, drop=(pe, st + 1, 'embed_k'), drop2=(pe, st + 2, 'embed_v'))
            return x, xk, xv
        xk = S.pos_embed(x_k, tk, sc)
        return x, xk, xk

    def forward(self, x_q, x_k=None, x_v=None):
        if (x_k is None) != (x_v is None):
            raise ValueError('TransformerEncoder: give both x_k and x_v or neither')
        s, xk, xv = self.embed(x_q, x_k, x_v)
        cross = xk is not None
        pr = float(self.layers[0].res_dropout) if self.training else 0.0
        ln = self.layers[0].layer_norms[0]
        y = S.prenorm_bdt(s, ln.weight, ln.bias, ln.eps, shared=cross)
        n = len(self.layers)
        for idx, layer in enumerate(self.layers):
            site = self._site + 3 + 4 * idx
            a = layer.attention_block(y, xk, xv, site)
            ln = layer.layer_norms[1]
            s, y = S.prenorm_bdt(s, ln.weight, ln.bias, ln.eps, x=a, drop=(pr, site + 1, 'res1'))
            f = layer.feed_forward(y, site + 2)
            # the residual sum and the LayerNorm that reads it next: the next layer's LN0, or the encoder's final layer_norm
            last = idx + 1 == n
            ln = self.layer_norm if last else self.layers[idx + 1].layer_norms[0]
            s, y = S.prenorm_bdt(s, ln.weight, ln.bias, ln.eps, x=f, drop=(pr, site + 3, 'res2'), shared=cross and not last)
        return y


class MULTModel(nn.Module):
    """MultiBench fusions.mult.MULTModel(n_modalities, n_features, hyp_params): a fusion module, [x_i [B, T, F_i]] -> [B, output_dim]."""

    def __init__(self, n_modalities, n_features, hyp_params=HParams):
        super().__init__()
        hp = hyp_params
        if hp.all_steps:
            raise NotImplementedError('MULTModel(all_steps=True): the reference builds all_steps=False')
        self.n_modalities, self.embed_dim, self.num_heads, self.layers = n_modalities, hp.embed_dim, hp.num_heads, hp.layers
        self.attn_dropout, self.attn_dropout_modalities = hp.attn_dropout, list(hp.attn_dropout_modalities)
        self.relu_dropout, self.res_dropout, self.out_dropout = hp.relu_dropout, hp.res_dropout, hp.out_dropout
        self.embed_dropout, self.attn_mask, self.all_steps = hp.embed_dropout, hp.attn_mask, hp.all_steps
        M, E = n_modalities, hp.embed_dim
        combined = E * M * M
        self.proj = nn.ModuleList([nn.Conv1d(n_features[i], E, kernel_size=1, padding=0, bias=False) for i in range(M)])
        self.trans = nn.ModuleList([nn.ModuleList([self.get_network(j, mem=False) for j in range(M)]) for _ in range(M)])
        self.trans_mems = nn.ModuleList([self.get_network(i, mem=True, layers=3) for i in range(M)])
        self.proj1 = nn.Linear(combined, combined)
        self.proj2 = nn.Linear(combined, combined)
        self.out_layer = nn.Linear(combined, hp.output_dim)
        self._site = S.new_sites(1)

    def get_network(self, mod, mem, layers=-1):
        E = self.embed_dim * (self.n_modalities if mem else 1)
        return TransformerEncoder(E, self.num_heads, max(self.layers, layers),
                                  attn_dropout=self.attn_dropout if mem else self.attn_dropout_modalities[mod],
                                  relu_dropout=self.relu_dropout, res_dropout=self.res_dropout, embed_dropout=self.embed_dropout,
                                  attn_mask=self.attn_mask)

    def target(self, i, ps):
        """The last time step of trans_mems[i](cat_j trans[i][j](p_i, p_j, p_j)): [B, M E]."""
        h = torch.cat([self.trans[i][j](ps[i], ps[j], ps[j]) for j in range(self.n_modalities)], dim=1)
        return self.trans_mems[i](h)[:, :, -1].contiguous()

    def forward(self, x):
        from .affect import run_branches              # (nn.affect builds its MMDL around this module)
        ps = [S.linear_bdt(x[i].permute(0, 2, 1).contiguous(), self.proj[i].weight) for i in range(self.n_modalities)]
        # the targets are independent until the head: one branch each (three cross transformers + one memory transformer)
        z = torch.cat(run_branches([lambda i=i: self.target(i, ps) for i in range(self.n_modalities)]), dim=1)
        h = S.linear_bdt(z, self.proj1.weight, self.proj1.bias, act='relu')
        if self.training:
            h = S.dropout_bdt(h, float(self.out_dropout), self._site, 'out')
        h = S.linear_bdt(h, self.proj2.weight, self.proj2.bias)
        return S.linear_bdt(S.residual_add(z, h), self.out_layer.weight, self.out_layer.bias)


def mult_model():
    """affect_mm.py:68-86 (`--fusion 4`, saved as mult.pt)."""
    from .affect import MMDL, Identity
    return MMDL([Identity(), Identity(), Identity()], MULTModel(3, [35, 74, 300], HParams), Identity())
