"""AFM (mirror of recbole/model/context_aware_recommender/afm.py:23-115).

y = sigmoid(first_order_linear + afm_layer(field rows)) with, per sample, over the pairs
p = (i, j), i < j, of the F field rows:

    z_p = e_i * e_j,  alpha = softmax_p(h . relu(W z_p)),  y_afm = dropout(sum_p alpha_p z_p) . p

nn.BCELoss plus reg_weight * ||attlayer.w.weight||_2. Same class name, config keys
(attention_size, dropout_prob, reg_weight), parameter names (attlayer.w.weight, attlayer.h,
p), construction order and init as the reference, so seeded initial values are the
reference's and checkpoints are interchangeable.

Where things run on the GPU (fp32):
  field rows + first-order term   K8's first-order form (ContextRecommender.linear_fields)
  afm_layer                       K20 (csrc/afm.hip): one autograd Function (_AFMFn) from the
  (afm_kernel: 'fused')           rows, attlayer.w.weight, attlayer.h and p to y_afm [B]; one
                                  launch forward, one backward (+ the fixed-order finish). It
                                  saves the pooled vector [d], the softmax maximum and sum a
                                  sample; none of the reference's seven [B, P, .] tensors
                                  exists. Dropout is drawn in the kernel (drop.h, site AFM_SITE)
  sigmoid + BCE                   _SigmoidBCEFn (y_first | y_afm); forward / predict:
                                  sigmoid_prob
  regularisation                  one torch norm over attlayer.w.weight

afm_kernel: 'library', a CPU device, a dtype other than float32 and shapes K20 is not built
for (mirec_afm_shape_ok: F 2..64, embedding_size 2..64, attention_size 1..64) run
afm_library, the reference's op sequence, followed by the reference's sigmoid + BCELoss.

The [V, d] token table and the [V, 1] first-order table run on the deferred Adam schedule
at an embedding_size the deferred kernels take (4, 16, 32, ...; at the default 10 every table
takes the dense step: K8 catches the [V, 1] rows up beside the [V, d] ones, so the pair is
offered together or not at all). The step runs eagerly (graph_step_safe = False: no capture
around K20 was built) on one GPU.
"""
import torch
import torch.nn as nn

from recbole_amd import ops
from recbole_amd.model.abstract_recommender import ContextRecommender
from recbole_amd.model.context import _SigmoidBCEFn, sigmoid_prob
from recbole_amd.model.layers import AFM_SITE, AttLayer, site_seed


def afm_library(X, attlayer, pv, dropout):
    """The reference's op sequence (afm.py:55-99): gathers of the left and right rows of
    every pair, their product, the attention layer, the weighted product, the sum over the
    pairs, dropout, the product with p and its sum. [B, 1]."""
    F = X.shape[1]
    row, col = [], []
    for i in range(F - 1):
        for j in range(i + 1, F):
            row.append(i)
            col.append(j)
    pair_wise_inter = torch.mul(X[:, row], X[:, col])            # [B, P, d]
    att_signal = attlayer(pair_wise_inter).unsqueeze(dim=2)       # [B, P, 1]
    att_pooling = torch.sum(torch.mul(att_signal, pair_wise_inter), dim=1)
    att_pooling = dropout(att_pooling)
    return torch.sum(torch.mul(att_pooling, pv), dim=1, keepdim=True)


class _AFMFn(torch.autograd.Function):
    """y_afm [B] through K20. Saves X, the parameters, V [B, d], ML [B, 2] and, with dropout,
    the counter word drawn."""

    @staticmethod
    def forward(ctx, X, W, h, pv, p, rng):
        X, W = X.contiguous(), W.detach().contiguous()
        h, pv = h.detach().contiguous(), pv.detach().contiguous()
        drawn = torch.empty(1, dtype=torch.int64, device=X.device) if p else None
        y, V, ML = ops.afm_fwd(X, W, h, pv, p=p, rng=rng, drawn=drawn)
        ctx.p, ctx.rng, ctx.drawn = p, rng, drawn
        ctx.save_for_backward(X, W, h, pv, V, ML)
        return y

    @staticmethod
    def backward(ctx, gy):
        X, W, h, pv, V, ML = ctx.saved_tensors
        dX, dW, dh, dpv = ops.afm_bwd(X, W, h, pv, V, ML, gy.contiguous(), p=ctx.p, rng=ctx.rng,
                                      drawn=ctx.drawn)
        return dX, dW, dh, dpv, None, None


class AFM(ContextRecommender):

    graph_step_safe = False

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.attention_size = config['attention_size']
        self.dropout_prob = config['dropout_prob']
        self.reg_weight = config['reg_weight']
        self.afm_kernel = self._kernel_choice(config, 'afm_kernel')
        self.num_pair = self.num_feature_field * (self.num_feature_field - 1) / 2
        self.attlayer = AttLayer(self.embedding_size, self.attention_size)
        self.p = nn.Parameter(torch.randn(self.embedding_size), requires_grad=True)
        self.dropout_layer = nn.Dropout(p=self.dropout_prob)
        self.sigmoid = nn.Sigmoid()
        self.loss = nn.BCELoss()
        self._rng = None
        self.apply(self._init_weights)

    def afm_fused_applies(self, X):
        """K20 runs when asked for, on the GPU, in fp32, at a built shape."""
        if self.afm_kernel != 'fused' or not X.is_cuda or X.dtype != torch.float32:
            return False
        return X.dim() == 3 and ops.afm_shape_ok(X.shape[1], X.shape[2], self.attention_size)

    def _drop_rng(self, dev):
        """(seed, device draw counter) of K20a's dropout site."""
        if self._rng is None or self._rng[1].device != dev:
            self._rng = (site_seed(dev, AFM_SITE), torch.zeros(1, dtype=torch.int64, device=dev))
        return self._rng

    def afm_layer(self, infeature):
        """The attention-pooled pair score [B, 1] (afm.py:77-99)."""
        if self.afm_fused_applies(infeature):
            p = float(self.dropout_prob) if self.training else 0.0
            rng = self._drop_rng(infeature.device) if p else None
            return _AFMFn.apply(infeature, self.attlayer.w.weight, self.attlayer.h, self.p, p,
                                rng).unsqueeze(1)
        return afm_library(infeature, self.attlayer, self.p, self.dropout_layer)

    def _logits(self, interaction):
        """(first-order term [B], y_afm [B, 1], whether K20 ran)."""
        X, y_first = self.first_order_fields(interaction)
        return y_first, self.afm_layer(X), self.afm_fused_applies(X)

    def forward(self, interaction):
        y_first, y_afm, fused = self._logits(interaction)
        if fused:
            return sigmoid_prob(y_first, y_afm)
        return self.sigmoid(y_first + y_afm.squeeze(1))

    def calculate_loss(self, interaction):
        """BCE + reg_weight * ||attlayer.w.weight||_2 (afm.py:107-112)."""
        label = interaction[self.LABEL]
        y_first, y_afm, fused = self._logits(interaction)
        if fused:
            loss = _SigmoidBCEFn.apply(y_first, y_afm, label)
        else:
            loss = self.loss(self.sigmoid(y_first + y_afm.squeeze(1)), label.to(y_first.dtype))
        if self.reg_weight:
            loss = loss + self.reg_weight * torch.norm(self.attlayer.w.weight, p=2)
        return loss

    def predict(self, interaction):
        return self.forward(interaction)

    def deferred_tables(self):
        """The [V, d] token table and the [V, 1] first-order token weights, read by the same
        rows (as DeepFM), at a width the deferred kernels take."""
        return self._deferred_token_tables(with_first_order=True)
