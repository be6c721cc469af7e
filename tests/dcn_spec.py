"""DCN's cross network and prediction head restated from their formulas, for the tests
(tests/test_dcn_cpu.py, tests/test_gpu_dcn.py). Reference
recbole/model/context_aware_recommender/dcn.py; line numbers below are that file's.

With x_0 [B, n] (the field rows viewed flat, :102-104), w_l and b_l [n] for l < L (:47-54):

    s_l[b]     = x_l[b] . w_l                                                  (:96)
    x_{l+1}[b] = x_0[b] s_l[b] + b_l + x_l[b]                                  (:97-98)
    y          = sigmoid(predict_layer(cat(x_L, mlp_layers(x_0))))             (:107-111)
               = sigmoid(x_L . wp + deep . wd + bias), wp = predict_layer.weight[0, :n]
    loss       = BCELoss(y, label) + reg_weight * sum_l ||w_l||_2              (:115-119)

The gradients, for an upstream g_L = gy wp + gL (either term may be absent), row by row with
l = L-1 .. 0:

    t      = g_{l+1} . x_0
    dW_l  += t x_l           dB_l += g_{l+1}          dx0 += s_l g_{l+1}
    g_l    = g_{l+1} + t w_l
    after the loop dx0 += g_0;  with a head  dwp += gy x_L

cross64 / cross_grads64 are these loops on float64 tensors, written out (no autograd).
DCNRef is a torch module with the reference's names and construction order (float32 as
built: the seeded-construction test compares it bit for bit; .double() carries a model's
weights).
"""
import torch
import torch.nn as nn

from tests.xdeepfm_spec import XDeepFMRef, _FMEmbedding, _FirstOrder


def cross64(x0, W, Bv):
    """(x_L [B, n], S [B, L], [x_0 .. x_L]) from float64 x0 [B, n], W [L, n], Bv [L, n]."""
    xs, S = [x0], []
    for l in range(W.shape[0]):
        s = (xs[-1] * W[l][None, :]).sum(dim=1)
        S.append(s)
        xs.append(x0 * s[:, None] + Bv[l][None, :] + xs[-1])
    return xs[-1], torch.stack(S, dim=1), xs


def cross_grads64(x0, W, Bv, wp=None, gy=None, gL=None):
    """dict(y, xL, S, dx0, dW, dB, dwp) for g_L = gy wp + gL; every operand float64. y and
    dwp are None without a head."""
    assert (wp is None) == (gy is None) and (gy is not None or gL is not None)
    L = W.shape[0]
    xL, S, xs = cross64(x0, W, Bv)
    g = torch.zeros_like(x0)
    if gy is not None:
        g = g + gy[:, None] * wp[None, :]
    if gL is not None:
        g = g + gL
    dx0 = torch.zeros_like(x0)
    dW, dB = torch.zeros_like(W), torch.zeros_like(Bv)
    for l in range(L - 1, -1, -1):
        t = (g * x0).sum(dim=1)
        dW[l] = (t[:, None] * xs[l]).sum(dim=0)
        dB[l] = g.sum(dim=0)
        dx0 = dx0 + S[:, l][:, None] * g
        g = g + t[:, None] * W[l][None, :]
    dx0 = dx0 + g
    out = {'y': None, 'xL': xL, 'S': S, 'dx0': dx0, 'dW': dW, 'dB': dB, 'dwp': None}
    if gy is not None:
        out['y'] = (xL * wp[None, :]).sum(dim=1)
        out['dwp'] = (gy[:, None] * xL).sum(dim=0)
    return out


def cross_inputs(B, n, L, seed=0):
    """The kernel tests' float64 inputs: x0, gy, gL uniform in [-1, 1], w and wp within
    +-1/sqrt(n), b within +-0.1 (so the c_l = 1 + sum_{k<l} s_k stay of order 1)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * n + L)

    def u(*shape, scale=1.0):
        return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale
    return {'x0': u(B, n), 'W': u(L, n, scale=n ** -0.5), 'Bv': u(L, n, scale=0.1),
            'wp': u(n, scale=n ** -0.5), 'gy': u(B), 'gL': u(B, n)}


class _MLPBN(nn.Module):
    """[Dropout, Linear, BatchNorm1d, ReLU] per layer, as MLPLayers(bn=True) builds them."""

    def __init__(self, sizes, p):
        super().__init__()
        mods = []
        for a, b in zip(sizes[:-1], sizes[1:]):
            mods += [nn.Dropout(p=p), nn.Linear(a, b), nn.BatchNorm1d(b), nn.ReLU()]
        self.mlp_layers = nn.Sequential(*mods)


class DCNRef(nn.Module):
    """Parameters created in the reference's order: the context base's tables (token, float,
    token_seq), first_order_linear, the L cross weights (torch.randn, :47-50), the L cross
    biases (zeros, :51-54), mlp_layers with BatchNorm (:61), predict_layer (:62); then
    xavier_normal_ on every Embedding and Linear and zero Linear biases in Module.apply's
    order (:68-76)."""

    fields = XDeepFMRef.fields

    def __init__(self, token_names, token_dims, seq_names, seq_dims, float_names, d, mlp_hidden,
                 cross_layer_num, reg_weight, dropout=0.0):
        super().__init__()
        import numpy as np
        self.token_names, self.seq_names = list(token_names), list(seq_names)
        self.float_names = list(float_names)
        self.offsets = np.array((0, *np.cumsum(token_dims)[:-1]), dtype=np.int64) \
            if token_dims else np.zeros(0, dtype=np.int64)
        self.reg_weight = reg_weight
        m = len(token_names) + len(seq_names) + len(float_names)
        n = m * d
        if token_dims:
            self.token_embedding_table = _FMEmbedding(token_dims, d)
        if float_names:
            self.float_embedding_table = nn.Embedding(len(float_names), d)
        if seq_dims:
            self.token_seq_embedding_table = nn.ModuleList(nn.Embedding(v, d) for v in seq_dims)
        self.first_order_linear = _FirstOrder(token_dims, seq_dims, len(float_names))
        self.cross_layer_w = nn.ParameterList(
            nn.Parameter(torch.randn(n)) for _ in range(cross_layer_num))
        self.cross_layer_b = nn.ParameterList(
            nn.Parameter(torch.zeros(n)) for _ in range(cross_layer_num))
        self.mlp_layers = _MLPBN([n] + list(mlp_hidden), dropout)
        self.predict_layer = nn.Linear(n + mlp_hidden[-1], 1)
        for mod in self.modules():
            if isinstance(mod, nn.Embedding):
                nn.init.xavier_normal_(mod.weight.data)
            elif isinstance(mod, nn.Linear):
                nn.init.xavier_normal_(mod.weight.data)
                if mod.bias is not None:
                    nn.init.constant_(mod.bias.data, 0)

    def logit(self, inter):
        X0, _ = self.fields(inter)
        x0 = X0.reshape(X0.shape[0], -1)
        n = x0.shape[1]
        W, Bv = torch.stack(list(self.cross_layer_w)), torch.stack(list(self.cross_layer_b))
        x = x0
        for l in range(W.shape[0]):            # autograd through the formula, float64
            x = x0 * (x * W[l]).sum(dim=1, keepdim=True) + Bv[l] + x
        deep = self.mlp_layers.mlp_layers(x0)
        pw = self.predict_layer.weight[0]
        return (x * pw[:n]).sum(dim=1) + (deep * pw[n:]).sum(dim=1) + self.predict_layer.bias

    def forward(self, inter):
        return torch.sigmoid(self.logit(inter))

    def calculate_loss(self, inter, label):
        y = self.forward(inter)
        t = label.to(y.dtype)
        bce = -(t * torch.log(y).clamp_min(-100) + (1 - t) * torch.log(1 - y).clamp_min(-100))
        reg = sum((w * w).sum().sqrt() for w in self.cross_layer_w)
        return bce.mean() + self.reg_weight * reg


def ref_of(model, dtype=torch.float64):
    """A DCNRef carrying `model`'s weights (and BatchNorm buffers) in `dtype` on the CPU."""
    ref = DCNRef(model.token_field_names, list(model.token_field_dims),
                 model.token_seq_field_names, list(model.token_seq_field_dims),
                 model.float_field_names, model.embedding_size, model.mlp_hidden_size,
                 model.cross_layer_num, model.reg_weight)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.to(dtype)
