"""AFM's pairwise-attention layer restated from its formulas, for the tests
(tests/test_afm_cpu.py, tests/test_gpu_afm.py). Reference
recbole/model/context_aware_recommender/afm.py and AttLayer (recbole/model/layers.py).

Per sample, with field rows e_0 .. e_{F-1} [d], the pairs p = (i, j), i < j (i ascending, then
j), W [A, d] (attlayer.w.weight, no bias), h [A] (attlayer.h) and pv [d] (the model's p):

    z_p = e_i * e_j              u_p = W z_p              a_p = max(u_p, 0)
    s_p = h . a_p                alpha = softmax_p(s)     v = sum_p alpha_p z_p
    y   = (k * v) . pv           k: keep flags / (1 - p_drop), or ones
    out = sigmoid(first_order + y)
    loss = BCE(out, label) + reg_weight * ||W||_2

and for an upstream gy [B]:

    dpv += gy (k * v)            gv = gy (k * pv)         c = gv . v
    t_p  = gv . z_p              ds_p = alpha_p (t_p - c)
    dh  += ds_p a_p              du_p = ds_p h * [u_p > 0]
    dW  += du_p z_p^T            dz_p = alpha_p gv + W^T du_p
    de_i += dz_p * e_j           de_j += dz_p * e_i

afm_grads64 is these loops on float64 tensors, written out (no autograd). AFMRef is a torch
module with the reference's names and construction order (float32 as built: the
seeded-construction test compares it bit for bit; .double() carries a model's weights).
"""
import torch
import torch.nn as nn

from tests.xdeepfm_spec import XDeepFMRef, _FMEmbedding, _FirstOrder

TAU_FACTOR = 16 * 2.0 ** -24


def pairs(F):
    return [(i, j) for i in range(F - 1) for j in range(i + 1, F)]


def afm_grads64(X, W, h, pv, gy, keep=None):
    """(y [B], v [B, d], dX, dW, dh, dpv) from float64 X [B, F, d], W [A, d], h [A], pv [d],
    gy [B]; keep [B, d]: the dropout factors (0 or 1 / (1 - p)), None for ones."""
    B, F, d = X.shape
    k = torch.ones(B, d, dtype=X.dtype) if keep is None else keep.to(X.dtype)
    pr = pairs(F)
    I, J = (torch.tensor(t) for t in zip(*pr))
    y, v = torch.zeros(B, dtype=X.dtype), torch.zeros(B, d, dtype=X.dtype)
    dX, dW = torch.zeros_like(X), torch.zeros_like(W)
    dh, dpv = torch.zeros_like(h), torch.zeros_like(pv)
    for b in range(B):
        z = torch.stack([X[b, i] * X[b, j] for i, j in pr])         # [P, d]
        u = z @ W.t()                                               # [P, A]
        a = u.clamp_min(0)
        s = a @ h
        e = torch.exp(s - s.max())
        alpha = e / e.sum()
        v[b] = (alpha[:, None] * z).sum(dim=0)
        y[b] = (k[b] * v[b] * pv).sum()
        dpv += gy[b] * k[b] * v[b]
        gv = gy[b] * k[b] * pv
        c = (gv * v[b]).sum()
        t = z @ gv
        ds = alpha * (t - c)
        dh += ds @ a
        du = ds[:, None] * h[None, :] * (u > 0).to(X.dtype)         # [P, A]
        dW += du.t() @ z
        dz = alpha[:, None] * gv[None, :] + du @ W                  # [P, d]
        dX[b].index_add_(0, I, dz * X[b, J])                        # de_i += dz_p * e_j
        dX[b].index_add_(0, J, dz * X[b, I])                        # de_j += dz_p * e_i
    return y, v, dX, dW, dh, dpv


def _margin_ok(X, W):
    """Every float64 |u_pa| at least tau_p = TAU_FACTOR * max over the units a of
    sum_k |W_ak z_pk| (the magnitude an fp32 sum of that pair's products works at)."""
    B, F, d = X.shape
    i, j = zip(*pairs(F))
    z = X[:, list(i)] * X[:, list(j)]                               # [B, P, d]
    u = z @ W.t()                                                   # [B, P, A]
    mag = (z.abs() @ W.abs().t()).max(dim=2, keepdim=True).values
    return bool((u.abs() >= TAU_FACTOR * mag).all())


def afm_inputs(B, F, d, A, seed=0):
    """The kernel tests' float64 inputs: X and gy uniform in [-1, 1], W within +-1/sqrt(d), h
    and pv within +-1. ReLU has a kink: a pre-activation within fp32 rounding of zero has an
    all-or-nothing gradient that depends on summation order, so the seed is advanced until
    every float64 |u| clears the margin above (about twice the expected fp32 error of a
    length-64 sum at the largest magnitude present). Returns the dict with the seed used."""
    for tried in range(64):
        g = torch.Generator().manual_seed(1000 * (seed + tried) + 7 * B + 5 * F + 3 * d + A)

        def u(*shape, scale=1.0):
            return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale
        inp = {'X': u(B, F, d), 'W': u(A, d, scale=d ** -0.5), 'h': u(A), 'pv': u(d), 'gy': u(B)}
        if _margin_ok(inp['X'], inp['W']):
            inp['seed'] = seed + tried
            return inp
    raise AssertionError(f'afm_inputs({B}, {F}, {d}, {A}): no seed of 64 clears the ReLU margin')


class _AttLayer(nn.Module):

    def __init__(self, in_dim, att_dim):
        super().__init__()
        self.w = nn.Linear(in_dim, att_dim, bias=False)
        self.h = nn.Parameter(torch.randn(att_dim), requires_grad=True)


class AFMRef(nn.Module):
    """Parameters created in the reference's order: the context base's tables (token, float,
    token_seq), first_order_linear, attlayer (w, then h = randn), p = randn; then
    xavier_normal_ on every Embedding and Linear in Module.apply's order."""

    fields = XDeepFMRef.fields

    def __init__(self, token_names, token_dims, seq_names, seq_dims, float_names, d,
                 attention_size, reg_weight):
        super().__init__()
        import numpy as np
        self.token_names, self.seq_names = list(token_names), list(seq_names)
        self.float_names = list(float_names)
        self.offsets = np.array((0, *np.cumsum(token_dims)[:-1]), dtype=np.int64) \
            if token_dims else np.zeros(0, dtype=np.int64)
        self.reg_weight = reg_weight
        if token_dims:
            self.token_embedding_table = _FMEmbedding(token_dims, d)
        if float_names:
            self.float_embedding_table = nn.Embedding(len(float_names), d)
        if seq_dims:
            self.token_seq_embedding_table = nn.ModuleList(nn.Embedding(v, d) for v in seq_dims)
        self.first_order_linear = _FirstOrder(token_dims, seq_dims, len(float_names))
        self.attlayer = _AttLayer(d, attention_size)
        self.p = nn.Parameter(torch.randn(d), requires_grad=True)
        for mod in self.modules():
            if isinstance(mod, nn.Embedding):
                nn.init.xavier_normal_(mod.weight.data)
            elif isinstance(mod, nn.Linear):
                nn.init.xavier_normal_(mod.weight.data)
                if mod.bias is not None:
                    nn.init.constant_(mod.bias.data, 0)

    def logit(self, inter):
        """Autograd through the formulas (dropout off)."""
        X, first = self.fields(inter)
        i, j = zip(*pairs(X.shape[1]))
        z = X[:, list(i)] * X[:, list(j)]
        s = torch.relu(z @ self.attlayer.w.weight.t()) @ self.attlayer.h
        alpha = torch.softmax(s, dim=1)
        v = (alpha[:, :, None] * z).sum(dim=1)
        return first + (v * self.p).sum(dim=1)

    def forward(self, inter):
        return torch.sigmoid(self.logit(inter))

    def calculate_loss(self, inter, label):
        y = self.forward(inter)
        t = label.to(y.dtype)
        bce = -(t * torch.log(y).clamp_min(-100) + (1 - t) * torch.log(1 - y).clamp_min(-100))
        W = self.attlayer.w.weight
        return bce.mean() + self.reg_weight * (W * W).sum().sqrt()


def ref_of(model, dtype=torch.float64):
    """An AFMRef carrying `model`'s weights in `dtype` on the CPU."""
    ref = AFMRef(model.token_field_names, list(model.token_field_dims),
                 model.token_seq_field_names, list(model.token_seq_field_dims),
                 model.float_field_names, model.embedding_size, model.attention_size,
                 model.reg_weight)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.to(dtype)
