"""xDeepFM's Compressed Interaction Network restated from its formulas, for the tests
(tests/test_xdeepfm_cpu.py, tests/test_gpu_xdeepfm.py). Reference
recbole/model/context_aware_recommender/xdeepfm.py; line numbers below are that file's.

Per layer k (the loop at :139-166, identity activation :145-146), with X0 [B, m, D],
Xk [B, H_k, D] (X_0 = X0, H_0 = m), W_k [N_k, H_k m] (the Conv1d weight, :60, without its
trailing 1) and b_k [N_k]:

    out_k[b, n, d] = b_k[n] + sum_{h < H_k} sum_{j < m} W_k[n, h m + j] Xk[b, h, d] X0[b, j, d]

(the einsum 'bmd,bhd->bhmd' of :140 viewed as [B, H_k m, D] at :141 is h-major, and the
1x1 convolution of :142 is a matrix product over that axis).

    direct: True   X_{k+1} = out_k, direct_k = out_k                          (:155-157)
    direct: False  X_{k+1} = out_k[:, :N_k/2], direct_k = out_k[:, N_k/2:]    (:159-160)
                   last layer: direct_k = out_k                                (:161-163)
                   every N_k rounded down to even first                         (:48-54)
    pooled[b, :]   = cat_k( sum_d direct_k[b, :, d] )                         (:167-168)
    y              = sigmoid(first_order + cin_linear(pooled) + mlp_layers(X0.view(B, -1)))
                                                                               (:171-185)
    loss           = BCELoss(y, label) + reg_weight * sum ||w||_2 over the *weight parameters
                     of mlp_layers, first_order_linear and the convolutions   (:90-114, :187-191)

cin64 / cin_grads64 work on float64 tensors (gradients by autograd in float64). XDeepFMRef is
a torch module with the reference's module names and construction order (float32 as built:
the seeded-construction test compares it bit for bit; .double() for the restatement that
carries a model's weights). Its convolutions may be left out of the module tree, as the
reference leaves them (:57-61): the values drawn are the same either way.
"""
import numpy as np
import torch
import torch.nn as nn


def even_sizes(sizes, direct):
    return list(sizes) if direct else [int(s) // 2 * 2 for s in sizes]


def field_nums(m, sizes, direct):
    """[m, H_1, ...] (:58-65) and final_len (:71-75) for sizes already made even."""
    nums = [m] + [s if direct else s // 2 for s in sizes]
    final_len = sum(sizes) if direct else sum(sizes[:-1]) // 2 + sizes[-1]
    return nums, final_len


def cin64(X0, Ws, bs, direct):
    """(pooled [B, final_len], [X_1, ..., X_{L-1}]) from float64 X0 [B, m, D], W_k [N_k, H_k m]
    and b_k [N_k]."""
    B, m, D = X0.shape
    Xk, hidden, parts = X0, [], []
    last = len(Ws) - 1
    for k, (W, b) in enumerate(zip(Ws, bs)):
        N, H = W.shape[0], Xk.shape[1]
        assert W.shape[1] == H * m
        out = torch.einsum('nhj,bhd,bjd->bnd', W.view(N, H, m), Xk, X0) + b.view(1, N, 1)
        if direct or k == last:
            nxt, dk = out, out
        else:
            nxt, dk = out[:, :N // 2], out[:, N // 2:]
        parts.append(dk.sum(dim=2))
        if k < last:
            hidden.append(nxt)
        Xk = nxt
    return torch.cat(parts, dim=1), hidden


def cin_grads64(X0, Ws, bs, direct, g_pooled):
    """pooled, the hidden X_k, dX0, [dW_k], [db_k] for the upstream gradient g_pooled; every
    operand a float64 tensor (copied; the arguments keep no graph)."""
    X0 = X0.detach().clone().requires_grad_(True)
    Ws = [w.detach().clone().requires_grad_(True) for w in Ws]
    bs = [b.detach().clone().requires_grad_(True) for b in bs]
    pooled, hidden = cin64(X0, Ws, bs, direct)
    pooled.backward(g_pooled)
    return (pooled.detach(), [h.detach() for h in hidden], X0.grad, [w.grad for w in Ws],
            [b.grad for b in bs])


class _FMEmbedding(nn.Module):

    def __init__(self, dims, d):
        super().__init__()
        self.embedding = nn.Embedding(int(sum(dims)), d)


class _FirstOrder(nn.Module):

    def __init__(self, token_dims, seq_dims, n_float):
        super().__init__()
        if token_dims:
            self.token_embedding_table = _FMEmbedding(token_dims, 1)
        if n_float:
            self.float_embedding_table = nn.Embedding(n_float, 1)
        if seq_dims:
            self.token_seq_embedding_table = nn.ModuleList(nn.Embedding(v, 1) for v in seq_dims)
        self.bias = nn.Parameter(torch.zeros((1,)), requires_grad=True)


class _MLP(nn.Module):
    """[Dropout, Linear, ReLU] per layer, as layers.py MLPLayers builds them."""

    def __init__(self, sizes, p):
        super().__init__()
        mods = []
        for a, b in zip(sizes[:-1], sizes[1:]):
            mods += [nn.Dropout(p=p), nn.Linear(a, b), nn.ReLU()]
        self.mlp_layers = nn.Sequential(*mods)


class XDeepFMRef(nn.Module):
    """Parameters created in the reference's order: the context base's tables (token, float,
    token_seq), first_order_linear, the convolutions (:57-65), mlp_layers (:68-69),
    cin_linear (:77); then xavier_normal_ on every Embedding and Linear and zero Linear biases
    in Module.apply's order (:80-88), which never touches a Conv1d."""

    def __init__(self, token_names, token_dims, seq_names, seq_dims, float_names, d, mlp_hidden,
                 cin_sizes, direct, reg_weight, register_convs=True, dropout=0.0):
        super().__init__()
        self.token_names, self.seq_names = list(token_names), list(seq_names)
        self.float_names = list(float_names)
        self.offsets = np.array((0, *np.cumsum(token_dims)[:-1]), dtype=np.int64) \
            if token_dims else np.zeros(0, dtype=np.int64)
        self.direct, self.reg_weight = direct, reg_weight
        m = len(token_names) + len(seq_names) + len(float_names)
        if token_dims:
            self.token_embedding_table = _FMEmbedding(token_dims, d)
        if float_names:
            self.float_embedding_table = nn.Embedding(len(float_names), d)
        if seq_dims:
            self.token_seq_embedding_table = nn.ModuleList(nn.Embedding(v, d) for v in seq_dims)
        self.first_order_linear = _FirstOrder(token_dims, seq_dims, len(float_names))
        self.cin_layer_size = even_sizes(cin_sizes, direct)
        self.field_nums, self.final_len = field_nums(m, self.cin_layer_size, direct)
        convs = [nn.Conv1d(h * m, n, 1) for h, n in zip(self.field_nums, self.cin_layer_size)]
        if register_convs:
            self.conv1d_list = nn.ModuleList(convs)
        else:
            self.__dict__['conv1d_list'] = convs
        self.mlp_layers = _MLP([d * m] + list(mlp_hidden) + [1], dropout)
        self.cin_linear = nn.Linear(self.final_len, 1, bias=False)
        for mod in self.modules():
            if isinstance(mod, nn.Embedding):
                nn.init.xavier_normal_(mod.weight.data)
            elif isinstance(mod, nn.Linear):
                nn.init.xavier_normal_(mod.weight.data)
                if mod.bias is not None:
                    nn.init.constant_(mod.bias.data, 0)

    def fields(self, inter):
        """(X0 [B, m, D], first-order term [B]) field by field: token rows through the shared
        table at the field's offset, token_seq fields as masked means sum(mask e) / (count +
        1e-8) with the masked sum of their first-order weights, float fields as E_f[j] x_j
        and w_j x_j; [token | token_seq | float]."""
        fo = self.first_order_linear
        rows, first = [], 0
        for f, name in enumerate(self.token_names):
            ids = inter[name].long() + int(self.offsets[f])
            rows.append(self.token_embedding_table.embedding.weight[ids])
            first = first + fo.token_embedding_table.embedding.weight[ids][:, 0]
        for f, name in enumerate(self.seq_names):
            ids = inter[name].long()
            E, E1 = self.token_seq_embedding_table[f].weight, fo.token_seq_embedding_table[f].weight
            mask = (ids != 0).to(E.dtype)
            rows.append((E[ids] * mask[:, :, None]).sum(1) / (mask.sum(1, keepdim=True) + 1e-8))
            first = first + (E1[ids][:, :, 0] * mask).sum(1)
        for j, name in enumerate(self.float_names):
            x = inter[name].to(self.float_embedding_table.weight.dtype)
            rows.append(self.float_embedding_table.weight[j][None, :] * x[:, None])
            first = first + fo.float_embedding_table.weight[j, 0] * x
        return torch.stack(rows, dim=1), first + fo.bias

    def logit(self, inter):
        X0, first = self.fields(inter)
        Ws = [c.weight[:, :, 0] for c in self.conv1d_list]
        pooled, _ = cin64(X0, Ws, [c.bias for c in self.conv1d_list], self.direct)
        dnn = self.mlp_layers.mlp_layers(X0.reshape(X0.shape[0], -1))
        return first + self.cin_linear(pooled)[:, 0] + dnn[:, 0]

    def forward(self, inter):
        return torch.sigmoid(self.logit(inter))

    def calculate_loss(self, inter, label):
        y = self.forward(inter)
        t = label.to(y.dtype)
        bce = -(t * torch.log(y).clamp_min(-100) + (1 - t) * torch.log(1 - y).clamp_min(-100))
        norms = [p.norm(2) for n, p in self.mlp_layers.named_parameters() if n.endswith('weight')]
        norms += [p.norm(2) for n, p in self.first_order_linear.named_parameters()
                  if n.endswith('weight')]
        norms += [c.weight.norm(2) for c in self.conv1d_list]
        return bce.mean() + self.reg_weight * sum(norms)


def ref_of(model, dtype=torch.float64):
    """An XDeepFMRef carrying `model`'s weights in `dtype` on the CPU."""
    ref = XDeepFMRef(model.token_field_names, list(model.token_field_dims),
                     model.token_seq_field_names, list(model.token_seq_field_dims),
                     model.float_field_names, model.embedding_size, model.mlp_hidden_size,
                     model.cin_layer_size, model.direct, model.reg_weight)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.to(dtype)
