"""NeuMF (mirror of recbole/model/general_recommender/neumf.py:27-133).

Same modules, names, construction order and init as the reference (user / item MF and
MLP embeddings drawn normal(0, 0.01), mlp_layers and predict_layer with torch's default
Linear init), so state-dict keys and seeded initial weights match; input_type POINTWISE.

    logit(u, i) = w_mf . (U_mf[u] * I_mf[i]) + w_h . MLP([U_mlp[u] | I_mlp[i]]) + b

On the GPU (fp32):

* calculate_loss -> K14a (csrc/neumf.hip: the four gathers, the MLP input and the MF logit
  in one launch), K10 (model/mlp.py: mlp_layers + the head slice of predict_layer), the
  sigmoid + BCE launch (_SigmoidBCEFn); backward K14b (per-row gradients + dw_mf) and K2
  (one grouping per key set, fixed-order scatter). The four tables may run on the deferred
  Adam schedule (deferred_tables).
* predict -> the same kernels without a graph, sigmoid_prob.
* evaluation -> K14c, the fused pair-MLP full-sort scorer (fused_pair_scorer; the
  trainer's fused_pair_full_sort_eval), which ranks the LOGITS: the reference ranks the
  sigmoid outputs, which tie once fp32 saturates; logits order the same pairs and split
  those ties. full_sort_predict returns sigmoid(logits) from K14c's scores mode.
On a CPU device every step is the reference's torch op sequence.

use_pretrain is not supported.
"""
import torch
import torch.nn as nn
from torch.nn.init import normal_

from recbole_amd import ops
from recbole_amd.model.abstract_recommender import GeneralRecommender
from recbole_amd.model.context import _SigmoidBCEFn, sigmoid_prob
from recbole_amd.model.layers import MLPLayers
from recbole_amd.model.mlp import fused_deep_tensors, tensors_supported
from recbole_amd.utils import InputType

K6_WIDTHS = (32, 64, 128, 256)
DEFERRED_WIDTHS = (1, 4, 16, 32, 64, 128, 256)      # FusedAdam.enable_deferred's row widths


class _PairGatherFn(torch.autograd.Function):
    """K14a / K14b around the four embedding tables (a table pair may be None: that half
    of the model is off). Deferred tables (FusedAdam.enable_deferred) are caught up before
    the read and get their gradient rows stashed, as model/context.py's field Function;
    the user grouping serves both user tables, the item grouping both item tables."""

    @staticmethod
    def forward(ctx, user, item, U_mf, I_mf, U_mlp, I_mlp, w_mf):
        user, item = user.contiguous(), item.contiguous()
        segs = [None, None]
        for T, side, keys in ((U_mf, 0, user), (U_mlp, 0, user), (I_mf, 1, item),
                              (I_mlp, 1, item)):
            h = getattr(T, '_mirec_deferred', None) if T is not None else None
            if h is not None:
                segs[side] = h.catch_up(T, keys, segs=segs[side])
        det = lambda t: None if t is None else t.detach()
        x, z = ops.neumf_gather(user, item, det(U_mf), det(I_mf), det(w_mf), det(U_mlp),
                                det(I_mlp))
        ctx.tables = (U_mf, I_mf, U_mlp, I_mlp)
        ctx.segs = segs
        ctx.save_for_backward(user, item, w_mf)
        ctx.mark_non_differentiable(*([z] if U_mf is None else []))
        return x, z

    @staticmethod
    def backward(ctx, gx, gz):
        user, item, w_mf = ctx.saved_tensors
        U_mf, I_mf, U_mlp, I_mlp = ctx.tables
        mf, mlp = U_mf is not None, U_mlp is not None
        n_users = (U_mf if mf else U_mlp).shape[0]
        n_items = (I_mf if mf else I_mlp).shape[0]
        if mf and gz is None:
            gz = torch.zeros(user.numel(), dtype=torch.float32, device=user.device)
        if mlp and gx is None:
            gx = torch.zeros(user.numel(), 2 * U_mlp.shape[1], dtype=torch.float32,
                             device=user.device)
        rows = ops.neumf_gather_bwd(
            user, item, U_mf.detach() if mf else None, I_mf.detach() if mf else None,
            w_mf.detach() if mf else None, gz.contiguous() if mf else None,
            gx.contiguous() if mlp else None, n_users, n_items)
        gU_mf, gI_mf, gU_mlp, gI_mlp, dw = rows
        segs = list(ctx.segs)
        out = []
        for T, g, side, keys, n in ((U_mf, gU_mf, 0, user, n_users), (I_mf, gI_mf, 1, item, n_items),
                                    (U_mlp, gU_mlp, 0, user, n_users),
                                    (I_mlp, gI_mlp, 1, item, n_items)):
            if T is None:
                out.append(None)
                continue
            if segs[side] is None:                 # once per key set
                segs[side] = ops.segment_sort(keys, n)
            h = getattr(T, '_mirec_deferred', None)
            if h is not None:                      # compact rows to the deferred optimizer
                h.stash(T, g, keys, segs[side])
                out.append(None)
            else:
                out.append(ops.segment_scatter_add(g, segs[side], torch.zeros_like(T)))
        return (None, None, *out, dw)


class PairScorer(object):
    """One evaluation's K14c state: the item part Bm = I_mlp W1i^T (once), the layer
    descriptor, and per user batch A = U_mlp[u] W1u^T + b1 and Pq = U_mf[u] * w_mf.
    With the MLP off the model is a dot product: K6 ranks Pq against I_mf."""

    def __init__(self, model):
        self.mf, self.mlp = bool(model.mf_train), bool(model.mlp_train)
        w = model.predict_layer.weight.detach()
        self.bias = model.predict_layer.bias.detach()
        dmf = model.mf_embedding_size if self.mf else 0
        self.dmf = dmf
        if self.mf:
            self.U_mf = model.user_mf_embedding.weight.detach()
            self.I_mf = model.item_mf_embedding.weight.detach().contiguous()
            self.w_mf = w[0, :dmf].contiguous()
        else:
            self.U_mf = self.I_mf = self.w_mf = None
        self.device = self.bias.device
        if self.mlp:
            lins = [m for m in model.mlp_layers.mlp_layers if isinstance(m, nn.Linear)]
            Ws = [m.weight.detach().contiguous() for m in lins]
            bs = [m.bias.detach() if m.bias is not None else None for m in lins]
            self.U_mlp = model.user_mlp_embedding.weight.detach()
            self.dm = model.mlp_embedding_size
            self.W1, self.b1 = Ws[0], bs[0]
            self.Bm = ops.neumf_project(model.item_mlp_embedding.weight.detach().contiguous(),
                                        self.W1, self.dm)
            self.desc, self._keep = ops.pair_mlp_desc(Ws, bs, w[0, dmf:].contiguous(), self.bias,
                                                      dmf)

    def _user_side(self, uids):
        uids = uids.contiguous()
        Pq = A = None
        if self.mf:
            Pq = ops.gather_rows(self.U_mf, uids) * self.w_mf
        if self.mlp:
            A = ops.neumf_project(self.U_mlp, self.W1, 0, bias=self.b1, idx=uids)
        return A, Pq

    def topk(self, uids, K, hist_ptr=None, hist_cols=None, pos_ptr=None, pos_cols=None, out=None):
        A, Pq = self._user_side(uids)
        if not self.mlp:
            o = ops.fullsort_topk(Pq, self.I_mf, K, hist_ptr=hist_ptr, hist_cols=hist_cols,
                                  pos_ptr=pos_ptr, pos_cols=pos_cols, out=out)
            o['scores'] += self.bias
            return o
        return ops.pair_mlp_topk(self.desc, A, Pq, self.Bm, self.I_mf, K, hist_ptr=hist_ptr,
                                 hist_cols=hist_cols, pos_ptr=pos_ptr, pos_cols=pos_cols, out=out)

    def scores(self, uids):
        """The [len(uids), n_items] logits."""
        A, Pq = self._user_side(uids)
        if not self.mlp:
            return ops.score_matrix(Pq, self.I_mf) + self.bias
        return ops.pair_mlp_scores(self.desc, A, Pq, self.Bm, self.I_mf)


def pair_scorer_supported(model) -> bool:
    """The shapes PairScorer ranks: fp32 tables on the GPU; with the MLP on, K14c's — ReLU
    layers without BatchNorm, 2..4 hidden widths that are multiples of 16 in 16..256, dm a
    multiple of 4, dmf a multiple of 4 in 4..128 or MF off; with the MLP off, K6's widths."""
    w = model.predict_layer.weight
    if not (w.is_cuda and w.dtype == torch.float32):
        return False
    dmf = model.mf_embedding_size
    if not model.mlp_train:
        return dmf in K6_WIDTHS
    ml = model.mlp_layers
    act = getattr(ml, 'activation', 'relu')
    if ml.use_bn or not (isinstance(act, str) and act.lower() == 'relu'):
        return False
    if model.mlp_embedding_size % 4 or model.mlp_embedding_size > 512:
        return False
    if model.mf_train and (dmf % 4 or not 4 <= dmf <= 128):
        return False
    return ops.pair_mlp_supported(list(model.mlp_hidden_size), dmf if model.mf_train else 0)


class NeuMF(GeneralRecommender):
    input_type = InputType.POINTWISE

    # not offered to the trainer's HIP-graph capture (trainer/graph_step.py): the captured
    # step has not been checked against the eager one on a device
    graph_step_safe = False

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.LABEL = config['LABEL_FIELD']
        self.mf_embedding_size = config['mf_embedding_size']
        self.mlp_embedding_size = config['mlp_embedding_size']
        self.mlp_hidden_size = config['mlp_hidden_size']
        self.dropout_prob = config['dropout_prob']
        self.mf_train = config['mf_train']
        self.mlp_train = config['mlp_train']
        self.use_pretrain = config['use_pretrain']
        self.mf_pretrain_path = config['mf_pretrain_path']
        self.mlp_pretrain_path = config['mlp_pretrain_path']
        self._config = config                       # fused_eval is read when evaluating

        self.user_mf_embedding = nn.Embedding(self.n_users, self.mf_embedding_size)
        self.item_mf_embedding = nn.Embedding(self.n_items, self.mf_embedding_size)
        self.user_mlp_embedding = nn.Embedding(self.n_users, self.mlp_embedding_size)
        self.item_mlp_embedding = nn.Embedding(self.n_items, self.mlp_embedding_size)
        self.mlp_layers = MLPLayers([2 * self.mlp_embedding_size] + list(self.mlp_hidden_size),
                                    self.dropout_prob)
        self.mlp_layers.logger = None
        if self.mf_train and self.mlp_train:
            self.predict_layer = nn.Linear(self.mf_embedding_size + self.mlp_hidden_size[-1], 1)
        elif self.mf_train:
            self.predict_layer = nn.Linear(self.mf_embedding_size, 1)
        elif self.mlp_train:
            self.predict_layer = nn.Linear(self.mlp_hidden_size[-1], 1)
        self.sigmoid = nn.Sigmoid()
        self.loss = nn.BCELoss()

        if self.use_pretrain:
            raise NotImplementedError(
                'NeuMF: use_pretrain is not supported: the reference loads whole pickled models '
                '(mf_pretrain_path / mlp_pretrain_path) and overwrites the predict weight with '
                'the bias; train with use_pretrain: False')
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Embedding):
            normal_(module.weight.data, mean=0.0, std=0.01)

    # ------------------------------------------------------------------ the GPU path
    def _gpu_ok(self, user):
        if not (self.mf_train or self.mlp_train):
            raise RuntimeError('mf_train and mlp_train can not be False at the same time')
        W = self.predict_layer.weight
        if not (user.is_cuda and W.is_cuda and W.dtype == torch.float32):
            return False
        # the head slice of predict_layer.weight starts at column dmf: 16-byte aligned rows
        if self.mf_train and (self.mf_embedding_size % 4 or self.mf_embedding_size > 256):
            return False
        return not (self.mlp_train and self.mlp_embedding_size % 4)

    def _logits(self, user, item):
        """(z_mf [B], y_deep [B, 1] or [B]) whose sum is the logit, on the kernels."""
        mf, mlp = self.mf_train, self.mlp_train
        W, b = self.predict_layer.weight, self.predict_layer.bias
        dmf = self.mf_embedding_size if mf else 0
        x, z_mf = _PairGatherFn.apply(
            user, item, self.user_mf_embedding.weight if mf else None,
            self.item_mf_embedding.weight if mf else None,
            self.user_mlp_embedding.weight if mlp else None,
            self.item_mlp_embedding.weight if mlp else None, W[0, :dmf] if mf else None)
        if not mlp:
            return z_mf, b.expand(z_mf.shape[0])
        lins = [m for m in self.mlp_layers.mlp_layers if isinstance(m, nn.Linear)]
        Ws = [m.weight for m in lins] + [W[:, dmf:]]
        bs = [m.bias for m in lins] + [b]
        if tensors_supported(self.mlp_layers, Ws, x):
            return z_mf, fused_deep_tensors(self.mlp_layers, x, Ws, bs)
        return z_mf, nn.functional.linear(self.mlp_layers(x), Ws[-1], b)

    def forward(self, user, item):
        if self._gpu_ok(user):
            z_mf, y_deep = self._logits(user, item)
            return sigmoid_prob(z_mf, y_deep).squeeze()
        # the reference's op sequence
        parts = []
        if self.mf_train:
            parts.append(torch.mul(self.user_mf_embedding(user), self.item_mf_embedding(item)))
        if self.mlp_train:
            both = torch.cat((self.user_mlp_embedding(user), self.item_mlp_embedding(item)), -1)
            parts.append(self.mlp_layers(both))
        feat = parts[0] if len(parts) == 1 else torch.cat(parts, -1)
        return self.sigmoid(self.predict_layer(feat)).squeeze()

    def calculate_loss(self, interaction):
        user = interaction[self.USER_ID]
        item = interaction[self.ITEM_ID]
        label = interaction[self.LABEL]
        if self._gpu_ok(user):
            z_mf, y_deep = self._logits(user, item)
            return _SigmoidBCEFn.apply(z_mf, y_deep, label)
        return self.loss(self.forward(user, item), label)

    def predict(self, interaction):
        return self.forward(interaction[self.USER_ID], interaction[self.ITEM_ID])

    def full_sort_predict(self, interaction):
        """sigmoid of K14c's [users, items] logits, flattened — the values predict gives.
        Without the fused scorer (a CPU device, shapes K14c does not take, fused_eval:
        False) the trainer's generic path repeats the users over the catalogue instead."""
        if self._config['fused_eval'] is False or not self.pair_scorer_applies():
            raise NotImplementedError
        scorer = PairScorer(self)
        return torch.sigmoid(scorer.scores(interaction[self.USER_ID])).view(-1)

    # ------------------------------------------------------------------ trainer hooks
    def deferred_tables(self):
        """The embedding tables the trainer may run on the deferred K5 schedule (only the
        rows a batch reads are touched): those whose width FusedAdam.enable_deferred
        takes; the others get dense gradients."""
        tabs = []
        if self.mf_train:
            tabs += [self.user_mf_embedding.weight, self.item_mf_embedding.weight]
        if self.mlp_train:
            tabs += [self.user_mlp_embedding.weight, self.item_mlp_embedding.weight]
        return [t for t in tabs if t.is_cuda and t.dtype == torch.float32
                and t.shape[1] in DEFERRED_WIDTHS]

    def pair_scorer_applies(self):
        return bool(self.mf_train or self.mlp_train) and pair_scorer_supported(self)

    def fused_pair_scorer(self):
        """A PairScorer over the current weights, or None where its kernels do not apply."""
        return PairScorer(self) if self.pair_scorer_applies() else None
