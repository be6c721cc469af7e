"""NGCF (mirror of recbole/model/general_recommender/ngcf.py:35-193).

Same modules, names, construction order and init as the reference (sparse_dropout,
user_embedding, item_embedding, GNNlayers.{l}.linear / .interActTransform, mf_loss,
reg_loss; xavier_normal_initialization last), so state_dict keys and a seeded construction
match. The normalised adjacency is LightGCN's (the same matrix): norm_adj_csr + ops.SpmmPlan.

One layer, with x = A' E_l (A' = A_hat, or the node-dropped A_hat in training):

    z       = (E_l + x) W1^T + b1 + (x * E_l) W2^T + b2
    m       = dropout(leaky_relu_0.2(z))
    E_{l+1} = m / max(||m||, 1e-12)

and the model's output is cat(E_0, ..., E_L, dim=1) split into users and items. On the GPU
a layer is one K7 launch (x, the two tables read as split rows for l = 0) and one K16a
launch (csrc/ngcf.hip) that writes E_{l+1} straight into its column slice of the [N, D]
output; the backward is K16b + K16c + one K7 launch per layer (_NGCFPropagateFn). The loss
is BPR (K3) on the propagated rows + reg_weight * EmbLoss of the same propagated rows (the
reference's choice, ngcf.py:159-167) when D = sum of the widths is one of K3's. Layer widths
outside {64, 128}^2 take the torch op sequence for the whole propagation; so does a CPU
device.

Message dropout on the GPU is counter-based (K9d's rule, layer l's site word NGCF_SITE + l):
no CPU generator draw. Node dropout (default off) draws torch.rand(nnz) on the CPU
generator as the reference does, applied to the CSR values in this project's entry order
(not bit for bit the reference's COO order); the backward uses the transposed values
vals'[tperm].

The step runs eagerly (graph_step_safe = False). Like the reference, the tables cached for
full-sort evaluation are cleared only by calculate_loss.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from recbole_amd import ops
from recbole_amd.model.abstract_recommender import GeneralRecommender
from recbole_amd.model.general_recommender.bpr import _BPRLossFn
from recbole_amd.model.general_recommender.lightgcn import _EmbRegFn, norm_adj_csr
from recbole_amd.model.init import xavier_normal_initialization
from recbole_amd.model.layers import NGCF_SITE, BiGNNLayer, SparseDropout, site_seed
from recbole_amd.model.loss import BPRLoss, EmbLoss
from recbole_amd.utils import InputType

_K3_WIDTHS = (32, 64, 128, 256)


def transpose_perm(row_ptr, cols):
    """tperm[k] = the index of entry (c, r) for entry k = (r, c) of a CSR whose pattern is
    symmetric and whose entries are sorted by (row, column): values v of the pattern give
    the transposed matrix's values v[tperm]."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    key = rows * n + cols
    tperm = np.searchsorted(key, cols * n + rows)
    if not np.array_equal(key[np.minimum(tperm, len(key) - 1)], cols * n + rows):
        raise ValueError('transpose_perm: the pattern is not symmetric')
    return tperm.astype(np.int64)


class _NGCFPropagateFn(torch.autograd.Function):
    """All layers on the GPU. Inputs: the two tables, then (W1, b1, W2, b2) per layer, then
    the step's state st = dict(plan, vals, vals_t, dims, p, rngs). Saves x_l, ||m||_l, the
    [N, D] output and the drawn counter words."""

    @staticmethod
    def forward(ctx, EU, EI, st, *wb):
        plan, dims, p = st['plan'], st['dims'], st['p']
        L = len(dims) - 1
        U, N, dev = EU.shape[0], plan.n_rows, EU.device
        EU, EI = EU.detach(), EI.detach()
        wb = [t.detach() for t in wb]
        off = np.concatenate([[0], np.cumsum(dims)]).tolist()
        allb = torch.empty(N, off[-1], dtype=torch.float32, device=dev)
        allb[:U, :dims[0]].copy_(EU)
        allb[U:, :dims[0]].copy_(EI)
        xs, nrms, drawn = [], [], []
        E = (EU, EI)
        for l in range(L):
            W1, b1, W2, b2 = wb[4 * l:4 * l + 4]
            x = torch.empty(N, dims[l], dtype=torch.float32, device=dev)
            ops.spmm_csr(plan, E, y=x, vals=st['vals'])
            nxt = torch.empty(N, dims[l + 1], dtype=torch.float32, device=dev) \
                if l + 1 < L else None
            dw = torch.empty(1, dtype=torch.int64, device=dev) if p else None
            nrm = ops.ngcf_layer_fwd(E, x, W1, b1, W2, b2, allb[:, off[l + 1]:off[l + 2]],
                                     copy=nxt, p=p, rng=st['rngs'][l] if p else None, drawn=dw)
            xs.append(x)
            nrms.append(nrm)
            drawn.append(dw)
            E = nxt
        ctx.st, ctx.off, ctx.U = st, off, U
        ctx.save_for_backward(EU, EI, allb, *wb, *xs, *nrms, *drawn)
        return allb[:U], allb[U:]

    @staticmethod
    def backward(ctx, gU, gI):
        st, off, U = ctx.st, ctx.off, ctx.U
        plan, dims, p = st['plan'], st['dims'], st['p']
        L, N, D = len(dims) - 1, plan.n_rows, off[-1]
        EU, EI, allb, *rest = ctx.saved_tensors
        wb, xs, nrms, drawn = rest[:4 * L], rest[4 * L:5 * L], rest[5 * L:6 * L], rest[6 * L:]
        gU = torch.zeros(U, D, device=allb.device) if gU is None else gU.contiguous()
        gI = torch.zeros(N - U, D, device=allb.device) if gI is None else gI.contiguous()
        cut = lambda l: (gU[:, off[l]:off[l + 1]], gI[:, off[l]:off[l + 1]])
        G = cut(L)
        grads = [None] * (4 * L)
        dEU = dEI = None
        for l in range(L - 1, -1, -1):
            W1, _, W2, _ = wb[4 * l:4 * l + 4]
            E = (EU, EI) if l == 0 else allb[:, off[l]:off[l + 1]]
            gz, dE, gx = ops.ngcf_layer_bwd(G, allb[:, off[l + 1]:off[l + 2]], nrms[l], W1, W2, E,
                                            xs[l], add=cut(l), p=p,
                                            rng=st['rngs'][l] if p else None, drawn=drawn[l])
            dW1, dW2, db = ops.ngcf_wgrad(gz, E, xs[l], dims[l])
            grads[4 * l:4 * l + 4] = [dW1, db, dW2, db.clone()]
            if l > 0:                       # dE_l = A'^T gx + dE, in place of dE
                ops.spmm_csr(plan, gx, y=dE, add=dE, vals=st['vals_t'])
                G = dE
            else:
                dEU, dEI = torch.empty_like(EU), torch.empty_like(EI)
                ops.spmm_csr(plan, gx, y=(dEU, dEI), add=dE, vals=st['vals_t'])
        return (dEU, dEI, None, *grads)


class NGCF(GeneralRecommender):
    input_type = InputType.PAIRWISE
    graph_step_safe = False

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.interaction_matrix = dataset.inter_matrix(form='coo').astype(np.float32)
        self.embedding_size = config['embedding_size']
        self.hidden_size_list = [self.embedding_size] + list(config['hidden_size_list'])
        self.node_dropout = config['node_dropout']
        self.message_dropout = config['message_dropout']
        self.reg_weight = config['reg_weight']

        self.sparse_dropout = SparseDropout(self.node_dropout)
        self.user_embedding = nn.Embedding(self.n_users, self.embedding_size)
        self.item_embedding = nn.Embedding(self.n_items, self.embedding_size)
        self.GNNlayers = nn.ModuleList(
            BiGNNLayer(a, b) for a, b in zip(self.hidden_size_list[:-1], self.hidden_size_list[1:]))
        self.mf_loss = BPRLoss()
        self.reg_loss = EmbLoss()
        self.restore_user_e = None
        self.restore_item_e = None

        m = self.interaction_matrix
        self.norm_adj_csr = norm_adj_csr(m.row, m.col, self.n_users, self.n_items)
        self._plan = None
        self._tperm = None
        self._coo = None
        self._rngs = None
        self.apply(xavier_normal_initialization)

    # ------------------------------------------------------------------ the matrix
    @property
    def norm_adj_plan(self):
        """Device CSR + K7 plan, built on first use on the parameters' device."""
        dev = self.user_embedding.weight.device
        if self._plan is None or self._plan.row_ptr.device != dev:
            self._plan = ops.SpmmPlan(*self.norm_adj_csr, device=dev)
        return self._plan

    @property
    def tperm(self):
        if self._tperm is None:
            self._tperm = torch.as_tensor(transpose_perm(self.norm_adj_csr[0],
                                                         self.norm_adj_csr[1]))
        return self._tperm

    def _node_dropped_values(self):
        """None (A_hat itself), or the step's [nnz] float32 values of A' on the CPU: the
        keep draw of SparseDropout over the CSR entries, kept values / (1 - p)."""
        if not self.training or self.node_dropout == 0:
            return None
        vals = torch.as_tensor(self.norm_adj_csr[2])
        mask = self.sparse_dropout.keep_mask(vals.numel())
        return vals * mask / self.sparse_dropout.kprob

    def _torch_matrix(self, vals, dev):
        """A' as a torch sparse tensor on dev (the torch op sequence's operand)."""
        if self._coo is None or self._coo.device != dev:
            row_ptr, cols, _ = self.norm_adj_csr
            rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
            self._coo = torch.as_tensor(np.stack([rows, cols.astype(np.int64)])).to(dev)
        n = self.n_users + self.n_items
        v = torch.as_tensor(self.norm_adj_csr[2]) if vals is None else vals
        # entries are sorted by (row, column) and distinct: no coalesce per product
        return torch.sparse_coo_tensor(self._coo, v.to(dev), (n, n), is_coalesced=True)

    # ------------------------------------------------------------------ propagation
    def _kernel_path(self):
        w = self.user_embedding.weight
        dims = self.hidden_size_list
        return w.is_cuda and len(dims) > 1 and all(
            ops.ngcf_shape_ok(a, b) for a, b in zip(dims[:-1], dims[1:]))

    def _layer_rngs(self, dev):
        if self._rngs is None or self._rngs[0][1].device != dev:
            self._rngs = [(site_seed(dev, NGCF_SITE + l),
                           torch.zeros(1, dtype=torch.int64, device=dev))
                          for l in range(len(self.GNNlayers))]
        return self._rngs

    def _forward_torch(self, vals):
        dev = self.user_embedding.weight.device
        A = self._torch_matrix(vals, dev)
        E = torch.cat([self.user_embedding.weight, self.item_embedding.weight], dim=0)
        out = [E]
        for gnn in self.GNNlayers:
            E = gnn(A, None, E)
            E = F.leaky_relu(E, negative_slope=0.2)
            E = F.dropout(E, self.message_dropout, self.training)
            E = F.normalize(E, p=2, dim=1)
            out.append(E)
        return torch.split(torch.cat(out, dim=1), [self.n_users, self.n_items])

    def forward(self):
        vals = self._node_dropped_values()
        if not self._kernel_path():
            return self._forward_torch(vals)
        dev = self.user_embedding.weight.device
        p = float(self.message_dropout) if self.training else 0.0
        st = {'plan': self.norm_adj_plan, 'dims': self.hidden_size_list, 'p': p,
              'vals': None, 'vals_t': None, 'rngs': self._layer_rngs(dev) if p else None}
        if vals is not None:
            st['vals'] = vals.to(dev)
            st['vals_t'] = vals[self.tperm].to(dev)
        wb = []
        for g in self.GNNlayers:
            wb += [g.linear.weight, g.linear.bias, g.interActTransform.weight,
                   g.interActTransform.bias]
        return _NGCFPropagateFn.apply(self.user_embedding.weight, self.item_embedding.weight, st,
                                      *wb)

    # ------------------------------------------------------------------ plugin methods
    def calculate_loss(self, interaction):
        if self.restore_user_e is not None or self.restore_item_e is not None:
            self.restore_user_e, self.restore_item_e = None, None
        user = interaction[self.USER_ID].contiguous()
        pos_item = interaction[self.ITEM_ID].contiguous()
        neg_item = interaction[self.NEG_ITEM_ID].contiguous()
        user_all, item_all = self.forward()
        if self._kernel_width(user_all):
            user_all, item_all = user_all.contiguous(), item_all.contiguous()
            mf_loss = _BPRLossFn.apply(user_all, item_all, user, pos_item, neg_item)
            reg_loss = _EmbRegFn.apply(user_all, item_all, user, pos_item, neg_item)
            return mf_loss + self.reg_weight * reg_loss
        u, pos, neg = user_all[user], item_all[pos_item], item_all[neg_item]
        mf_loss = self.mf_loss((u * pos).sum(dim=1), (u * neg).sum(dim=1))
        return mf_loss + self.reg_weight * self.reg_loss(u, pos, neg)

    def _kernel_width(self, t):
        return t.is_cuda and t.shape[1] in _K3_WIDTHS

    def predict(self, interaction):
        with torch.no_grad():
            user_all, item_all = self.forward()
        user, item = interaction[self.USER_ID], interaction[self.ITEM_ID]
        if not self._kernel_width(user_all):
            return (user_all[user] * item_all[item]).sum(dim=1)
        return ops.dot_rows(user_all.contiguous(), item_all.contiguous(), user, item)

    def _restore(self):
        if self.restore_user_e is None or self.restore_item_e is None:
            with torch.no_grad():
                u, i = self.forward()
            self.restore_user_e, self.restore_item_e = u.contiguous(), i.contiguous()
        return self.restore_user_e, self.restore_item_e

    def full_sort_predict(self, interaction):
        user_e, item_e = self._restore()
        user = interaction[self.USER_ID]
        if not self._kernel_width(user_e):
            return torch.matmul(user_e[user], item_e.t()).view(-1)
        return ops.score_matrix(ops.gather_rows(user_e, user), item_e).view(-1)

    # ------------------------------------------------------------------ fused eval hooks
    # (K6 ranks widths 32 / 64 / 128 / 256: with another total width the hooks are absent and
    # the trainer evaluates through full_sort_predict)
    def _hook(self, fn):
        if sum(self.hidden_size_list) not in _K3_WIDTHS:
            raise AttributeError('NGCF: no fused full-sort hooks at this total width')
        return fn

    @property
    def fused_user_vectors(self):
        return self._hook(lambda user_ids: ops.gather_rows(self._restore()[0], user_ids))

    @property
    def fused_item_table(self):
        return self._hook(lambda: self._restore()[1])
