"""Plain-torch restatement of MULT (MultiBench fusions.mult.MULTModel as `affect_mm.py --fusion 4` builds it) — a test helper,
not a test.  PARITY UNPINNED: the reference does not vendor MultiBench; this file restates the published module (the same
definition dynmm_amd/nn/mult.py's docstring spells out) with torch operations only, usable in any floating dtype (the tests run
it in float64 for the yardstick and in float32 as the twin a MultiBench user would run).  State-dict keys equal those of
dynmm_amd.nn.mult, so one deterministic fill drives both sides.

Dropout: in training mode the modules draw torch's own decisions, unless `MULTModel.dropout_masks` is set to a callable
next_mask(name, shape) -> keep flags (uint8) in the HIP path's layouts — 'embed_q' / 'embed_k' / 'embed_v' / 'res1' / 'res2'
[B, E, T], 'relu' [B, 4E, T], 'attn' [B*heads, Tq, Tk], 'out' [B, M^2 E] — which is then called once per ACTIVE site (p > 0), in
the order and with the names dynmm_amd.nn.mult uses.  Activations here are [B, T, E].
"""
import math
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def ref_xattn(q, k, v, heads, causal, keep=None):
    """q [B, D, Tq], k / v [B, D, Tk] -> (out [B, D, Tq], probs [B*heads, Tq, Tk] before dropout); causal: key j visible to query
    i iff j <= i + |Tk - Tq|; keep: multiplier of the probabilities [B*heads, Tq, Tk]."""
    B, D, Tq = q.shape
    Tk = k.shape[2]
    dh = D // heads
    qh, kh, vh = (t.reshape(B * heads, dh, t.shape[2]).transpose(1, 2) for t in (q, k, v))          # [B*H, T, dh]
    s = (qh * dh ** -0.5) @ kh.transpose(1, 2)
    if causal:
        s = s + torch.triu(torch.full((Tq, Tk), float('-inf'), dtype=s.dtype), 1 + abs(Tk - Tq))
    e = (s - s.max(dim=-1, keepdim=True).values.detach()).exp()
    p = e / e.sum(dim=-1, keepdim=True)
    pk = p if keep is None else p * keep
    return (pk @ vh).transpose(1, 2).reshape(B, D, Tq), p


def visible(Tq, Tk):
    """bool [Tq, Tk]: key <= query + |Tk - Tq|"""
    return torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + abs(Tk - Tq)


def position_table(E, T, dtype=torch.float64):
    """[T, E]: fairseq's SinusoidalPositionalEmbedding.get_embedding rows 1..T (padding_idx = 0, so the first real position is 1)."""
    half = E // 2
    step = math.log(10000) / (half - 1)
    freq = torch.exp(torch.arange(half, dtype=dtype) * -step)
    ang = torch.arange(1, T + 1, dtype=dtype).unsqueeze(1) * freq.unsqueeze(0)
    emb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    if E % 2 == 1:
        emb = torch.cat([emb, torch.zeros(T, 1, dtype=dtype)], dim=1)
    return emb


def embed_closed_form(x, scale):
    """scale x + pos for x [B, E, T] (the HIP layout): the positional term is dropped where x[b, 0, t] == 0 exactly."""
    B, E, T = x.shape
    pos = position_table(E, T, x.dtype).t()[None].expand(B, E, T)
    return scale * x + pos * (x[:, :1, :] != 0).to(x.dtype)


def _dropout(mod, x, p, name, hip_shape, to_mine):
    """dropout of x with probability p at the site `name`; to_mine: HIP-layout flags -> x's layout"""
    if not (mod.training and p > 0):
        return x
    hook = MULTModel.dropout_masks
    if hook is None:
        return F.dropout(x, p, True)
    return x * to_mine(hook(name, tuple(hip_shape)).to(x.dtype)) / (1.0 - p)


def _bet(x):
    """the [B, E, T] site of x [B, T, E]"""
    return (x.shape[0], x.shape[2], x.shape[1])


_T = lambda m: m.permute(0, 2, 1)       # noqa: E731


class SinusoidalPositionalEmbedding(nn.Module):
    def __init__(self, embedding_dim):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.register_buffer('_float_tensor', torch.zeros(1))
        self._tables = {}

    def forward(self, x):
        """x [B, T, E] (un-embedded) -> pos [B, T, E], zeros at the steps whose channel 0 is exactly 0"""
        key = (x.shape[1], x.dtype, str(x.device))
        if key not in self._tables:          # (the published module keeps its table too)
            self._tables[key] = position_table(self.embedding_dim, x.shape[1], x.dtype).to(x.device)
        tab = self._tables[key]
        return (tab[None] * (x[:, :, :1] != 0).to(x.dtype)).detach()


class MultiheadAttention(nn.Module):
    def __init__(self, embed_dim, num_heads, attn_dropout=0.0):
        super().__init__()
        self.embed_dim, self.num_heads, self.attn_dropout = embed_dim, num_heads, attn_dropout
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)

    def forward(self, q_in, k_in, v_in, attn_mask):
        E, H = self.embed_dim, self.num_heads
        B, Tq, _ = q_in.shape
        Tk = k_in.shape[1]
        dh = E // H
        w, b = self.in_proj_weight, self.in_proj_bias
        q = F.linear(q_in, w[:E], b[:E]) * dh ** -0.5
        k = F.linear(k_in, w[E:2 * E], b[E:2 * E])
        v = F.linear(v_in, w[2 * E:], b[2 * E:])
        q, k, v = (t.reshape(B, t.shape[1], H, dh).permute(0, 2, 1, 3) for t in (q, k, v))        # [B, H, T, dh]
        s = q @ k.transpose(2, 3)
        if attn_mask:
            s = s + torch.triu(torch.full((Tq, Tk), float('-inf'), dtype=s.dtype, device=s.device), 1 + abs(Tk - Tq))
        p = torch.softmax(s, dim=-1)
        p = _dropout(self, p, self.attn_dropout, 'attn', (B * H, Tq, Tk), lambda m: m.reshape(B, H, Tq, Tk))
        return self.out_proj((p @ v).permute(0, 2, 1, 3).reshape(B, Tq, E))


class TransformerEncoderLayer(nn.Module):
    def __init__(self, embed_dim, num_heads=4, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, attn_mask=False):
        super().__init__()
        self.self_attn = MultiheadAttention(embed_dim, num_heads, attn_dropout)
        self.attn_mask, self.relu_dropout, self.res_dropout = attn_mask, relu_dropout, res_dropout
        self.fc1 = nn.Linear(embed_dim, 4 * embed_dim)
        self.fc2 = nn.Linear(4 * embed_dim, embed_dim)
        self.layer_norms = nn.ModuleList([nn.LayerNorm(embed_dim) for _ in range(2)])

    def forward(self, x, x_k=None, x_v=None):
        r = x
        x = self.layer_norms[0](x)
        if x_k is None:
            a = self.self_attn(x, x, x, self.attn_mask)
        else:
            a = self.self_attn(x, self.layer_norms[0](x_k), self.layer_norms[0](x_v), self.attn_mask)
        x = r + _dropout(self, a, self.res_dropout, 'res1', _bet(a), _T)
        r = x
        f = F.relu(self.fc1(self.layer_norms[1](x)))
        f = _dropout(self, f, self.relu_dropout, 'relu', _bet(f), _T)
        f = self.fc2(f)
        return r + _dropout(self, f, self.res_dropout, 'res2', _bet(f), _T)


class TransformerEncoder(nn.Module):
    def __init__(self, embed_dim, num_heads, layers, attn_dropout=0.0, relu_dropout=0.0, res_dropout=0.0, embed_dropout=0.0,
                 attn_mask=False):
        super().__init__()
        self.dropout, self.embed_dim, self.embed_scale = embed_dropout, embed_dim, math.sqrt(embed_dim)
        self.embed_positions = SinusoidalPositionalEmbedding(embed_dim)
        self.layers = nn.ModuleList([TransformerEncoderLayer(embed_dim, num_heads, attn_dropout, relu_dropout, res_dropout,
                                                             attn_mask) for _ in range(layers)])
        self.register_buffer('version', torch.Tensor([2]))
        self.layer_norm = nn.LayerNorm(embed_dim)

    def _embed(self, x, name):
        e = self.embed_scale * x + self.embed_positions(x)
        return _dropout(self, e, self.dropout, name, _bet(e), _T)

    def forward(self, x_q, x_k=None, x_v=None):
        x = self._embed(x_q, 'embed_q')
        if x_k is not None:
            x_k, x_v = self._embed(x_k, 'embed_k'), self._embed(x_v, 'embed_v')
        for layer in self.layers:
            x = layer(x, x_k, x_v)
        return self.layer_norm(x)


class HParams:
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


class MULTModel(nn.Module):
    dropout_masks = None      # next_mask(name, shape): training-mode arithmetic with injected keep flags (module docstring)

    def __init__(self, n_modalities, n_features, hp=HParams):
        super().__init__()
        M, E = n_modalities, hp.embed_dim
        self.n_modalities, self.out_dropout = M, hp.out_dropout
        enc = lambda dim, att, layers: TransformerEncoder(dim, hp.num_heads, layers, att, hp.relu_dropout, hp.res_dropout,   # noqa: E731
                                                          hp.embed_dropout, hp.attn_mask)
        self.proj = nn.ModuleList([nn.Conv1d(n_features[i], E, kernel_size=1, padding=0, bias=False) for i in range(M)])
        self.trans = nn.ModuleList([nn.ModuleList([enc(E, hp.attn_dropout_modalities[j], hp.layers) for j in range(M)])
                                    for _ in range(M)])
        self.trans_mems = nn.ModuleList([enc(M * E, hp.attn_dropout, max(hp.layers, 3)) for _ in range(M)])
        self.proj1 = nn.Linear(M * M * E, M * M * E)
        self.proj2 = nn.Linear(M * M * E, M * M * E)
        self.out_layer = nn.Linear(M * M * E, hp.output_dim)

    def forward(self, x):
        M = self.n_modalities
        ps = [self.proj[i](x[i].transpose(1, 2)).transpose(1, 2) for i in range(M)]                   # [B, T, E]
        last = []
        for i in range(M):
            h = torch.cat([self.trans[i][j](ps[i], ps[j], ps[j]) for j in range(M)], dim=2)
            last.append(self.trans_mems[i](h)[:, -1])
        z = torch.cat(last, dim=1)
        h = F.relu(self.proj1(z))
        h = _dropout(self, h, self.out_dropout, 'out', h.shape, lambda m: m)
        return self.out_layer(self.proj2(h) + z)


class MMDL(nn.Module):
    """MMDL([Identity()] * 3, MULTModel(...), Identity()) of Supervised_Learning.py:16-51 with has_padding=True."""

    def __init__(self, fusion):
        super().__init__()
        self.encoders = nn.ModuleList([nn.Identity() for _ in range(3)])
        self.fuse = fusion
        self.head = nn.Identity()

    def forward(self, inputs):
        return self.fuse(list(inputs[0]))


def mult_twin():
    return MMDL(MULTModel(3, [35, 74, 300], HParams))


def fill_(module, seed=0):
    """Deterministic, well-conditioned weights keyed on the state_dict key; the two marker buffers keep their values."""
    with torch.no_grad():
        for k, t in module.state_dict().items():
            if k.endswith('version') or k.endswith('_float_tensor'):
                continue
            r = np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(k.encode())]))
            if 'layer_norm' in k and k.endswith('weight'):
                v = r.uniform(0.8, 1.2, size=tuple(t.shape))
            elif t.dim() >= 2:
                v = r.standard_normal(size=tuple(t.shape)) * np.sqrt(1.0 / int(np.prod(t.shape[1:])))
            else:
                v = 0.05 * r.standard_normal(size=tuple(t.shape))
            t.copy_(torch.from_numpy(v.astype(np.float32)))
    return module


def padded_batch(batch, seed, T=50):
    """oracle.affect_oracle.synth_batch with the first 7 steps of sample 0 and the first 19 of sample 1 zeroed in every modality"""
    from oracle import affect_oracle as O
    inputs, y = O.synth_batch(batch, T=T, seed=seed)
    for x in inputs[0]:
        x[0, :min(7, T - 1)] = 0
        if batch > 1:
            x[1, :min(19, T - 1)] = 0
    return inputs, y
