"""What the float64-restatement tests of the sequence and expert layer share (test_seq_kernels, test_affect, test_gru, test_lrtf,
test_mim, test_imdb, test_experts).  Imports torch alone: no oracle, no dynmm_amd."""
import torch
import torch.nn as nn


def rel(a, b):
    """max |a - b| / max |b| in float64, the denominator clamped at 1e-30 (a quantity that is identically zero compares as 0)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def compare_to_float64(tag, got, ref64, ref32, fwd_keys, fwd_bar, bwd_bar, absent=()):
    """Every quantity of ref64 against got.  The bar of a quantity is the project's (fwd_bar for the keys in fwd_keys, bwd_bar for
    the others), raised to 4 x the error the float32 restatement ref32 itself has against ref64 where that is larger; every value
    must be finite.  The keys in `absent` must be None in got.  Prints each figure, asserts once at the end."""
    bad = []
    for k in ref64:
        if k in absent:
            assert got[k] is None
            continue
        project = fwd_bar if k in fwd_keys else bwd_bar
        assert tuple(got[k].shape) == tuple(ref64[k].shape), (tag, k)
        err, yard = rel(got[k], ref64[k]), rel(ref32[k], ref64[k])
        bar = max(project, 4.0 * yard)
        finite = bool(torch.isfinite(got[k]).all())
        print(f'FIG {tag} {k} kernel={err:.3e} f32={yard:.3e} bar={bar:.3e}' + (' RAISED' if err >= project else ''))
        if not (finite and err < bar):
            bad.append((k, err, yard, bar, finite))
    assert not bad, (tag, bad)


def randomize_bn(model, seed=0):
    """affine parameters and running statistics of every BatchNorm1d away from their initial 1 / 0"""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm1d):
            n = m.num_features
            with torch.no_grad():
                m.weight.copy_(1 + 0.2 * torch.randn(n, generator=g))
                m.bias.copy_(0.2 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(n, generator=g))
                m.running_var.copy_(0.5 + torch.rand(n, generator=g))


class Masks:
    """The n-th dropout site of a forward pass keeps element e iff rand_n(e) >= p: one deterministic stream both sides
    walk in the same order (gate, experts; per layer: attn, dropout1, dropout, dropout2).  `names`: the sites served."""

    def __init__(self, p, seed, device='cpu'):
        self.p, self.seed, self.n, self.device = p, seed, 0, device
        self.names = []

    def __call__(self, name, shape):
        g = torch.Generator().manual_seed(self.seed * 100003 + self.n)
        self.n += 1
        self.names.append(name)
        return (torch.rand(shape, generator=g) >= self.p).to(torch.uint8).to(self.device)


def check_adam_params(mine, ref, lr, tag, names=None):
    """The parameters after one Adam step.  Adam's first update is lr * sign(g) whatever |g|, so an element whose gradient is
    rounding noise may move the other way (2 update sizes apart): almost every element agrees to a fraction of an update (at most
    max(1, 2e-3 n) further than 0.2 * 2 lr), none further than 2.2 * 2 lr.  names=None: every key of the two state_dicts."""
    sd, sd_r = mine.state_dict(), ref.state_dict()
    if names is None:
        assert sorted(sd) == sorted(sd_r)
        names = list(sd)
    for k in names:
        d = (sd[k].cpu().double() - sd_r[k].double()).abs()
        if k.endswith('in_proj_bias'):
            third = d.numel() // 3                 # the key bias has an analytically zero gradient: rounding noise both sides
            d = torch.cat([d[:third], d[2 * third:]])
        n_far = int((d > 0.2 * 2 * lr).sum().item())
        assert n_far <= max(1, int(2e-3 * d.numel())) and d.max().item() < 2.2 * 2 * lr, (tag, k, n_far, d.max().item())
