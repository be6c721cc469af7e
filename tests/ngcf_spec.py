"""NGCF restated from its formulas, for the tests (tests/test_ngcf_cpu.py,
tests/test_gpu_ngcf.py). With A' the normalised adjacency (its values optionally replaced by
vals * mask / (1 - p_node)), for layer l mapping d_l -> d_{l+1}:

    x       = A' E_l
    z       = (E_l + x) W1^T + b1 + (x * E_l) W2^T + b2      (W1 = linear, W2 = interActTransform)
    h       = z > 0 ? z : 0.2 z
    m       = h * keep / (1 - p)                             (keep given; else m = h)
    E_{l+1} = m / max(||m||_2, 1e-12)                        per row
    all     = cat(E_0, ..., E_L, dim=1) -> user_all [U, D], item_all [I, D]
    loss    = mean -log(1e-10 + sigmoid(<u, pos> - <u, neg>))
              + reg_weight * (||u||_F + ||pos||_F + ||neg||_F) / B     on the rows of `all`

NGCFRef is a torch module with the reference's module names and construction order (float32
as built: the seeded-construction test compares it bit for bit; .double() for the float64
restatement that carries a model's weights, ref_of). layer64 is one layer as a function of
float64 tensors, for the kernel tests (gradients by autograd in float64).
"""
import numpy as np
import torch
import torch.nn as nn


class _BiLayer(nn.Module):

    def __init__(self, d_in, d_out):
        super().__init__()
        self.linear = nn.Linear(d_in, d_out)
        self.interActTransform = nn.Linear(d_in, d_out)


def sparse64(csr, vals=None):
    """The CSR (row_ptr, cols, vals) as a float64 torch sparse matrix; vals overrides."""
    row_ptr, cols, v = csr
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    v = torch.as_tensor(np.asarray(v if vals is None else vals, dtype=np.float64))
    idx = torch.as_tensor(np.stack([rows, np.asarray(cols, dtype=np.int64)]))
    return torch.sparse_coo_tensor(idx, v, (n, n)).coalesce()


def layer64(A, E, W1, b1, W2, b2, keep=None, p=0.0):
    """(E_next, ||m||, x) of one layer; every operand float64, keep a [N, d_out] bool array
    or None."""
    x = torch.sparse.mm(A, E)
    z = (E + x) @ W1.t() + b1 + (x * E) @ W2.t() + b2
    m = torch.where(z > 0, z, 0.2 * z)
    if keep is not None:
        m = m * torch.as_tensor(np.asarray(keep, dtype=np.float64)) / (1.0 - p)
    n = m.norm(dim=1)
    return m / n.clamp_min(1e-12)[:, None], n, x


class NGCFRef(nn.Module):

    def __init__(self, n_users, n_items, dims, reg_weight=1e-5):
        super().__init__()
        self.n_users, self.n_items, self.reg_weight = n_users, n_items, reg_weight
        self.sparse_dropout = nn.Identity()
        self.user_embedding = nn.Embedding(n_users, dims[0])
        self.item_embedding = nn.Embedding(n_items, dims[0])
        self.GNNlayers = nn.ModuleList(_BiLayer(a, b) for a, b in zip(dims[:-1], dims[1:]))
        # the Embeddings and Linears in registration order, the order Module.apply reaches them in
        for m in self.modules():
            if isinstance(m, nn.Embedding):
                nn.init.xavier_normal_(m.weight.data)
            elif isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight.data)
                nn.init.constant_(m.bias.data, 0)

    def forward(self, A, keeps=None, p=0.0):
        E = torch.cat([self.user_embedding.weight, self.item_embedding.weight], dim=0)
        out = [E]
        for l, g in enumerate(self.GNNlayers):
            E, _, _ = layer64(A, E, g.linear.weight, g.linear.bias, g.interActTransform.weight,
                              g.interActTransform.bias, None if keeps is None else keeps[l], p)
            out.append(E)
        return torch.split(torch.cat(out, dim=1), [self.n_users, self.n_items])

    def calculate_loss(self, A, user, pos, neg, keeps=None, p=0.0):
        ua, ia = self.forward(A, keeps, p)
        u, ps, ng = ua[user], ia[pos], ia[neg]
        mf = -torch.log(1e-10 + torch.sigmoid((u * ps).sum(1) - (u * ng).sum(1))).mean()
        reg = (u.norm() + ps.norm() + ng.norm()) / user.shape[0]
        return mf + self.reg_weight * reg

    def full_sort_predict(self, A, user):
        ua, ia = self.forward(A)
        return (ua[user] @ ia.t()).reshape(-1)


def ref_of(model):
    """The float64 restatement carrying an NGCF model's weights."""
    ref = NGCFRef(model.n_users, model.n_items, list(model.hidden_size_list),
                  model.reg_weight).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()})
    return ref
