"""Shared parts of the autoencoder models (MultiDAE, MultiVAE): the first encoder layer over
sparse user rows (BagLinear, K15a / K15b), the multinomial log-likelihood over the stored
logits (K15c), the evaluation scorer (K15d ranks its matrices) and the models' common base.

A batch row is the SET of a user's distinct history items (Dataset.history_item_csr), which
is what the reference's get_rating_matrix builds with a non-accumulating index_put_ of ones
(multivae.py:54-69): F.normalize then gives every nonzero 1 / sqrt(n_b), dropout acts on the
nonzeros only, and the loss of row b is n_b logsumexp(z_b) - sum_{i in S_b} z_b[i].

On the GPU (fp32) a training step is K15a -> the remaining torch layers -> addmm for the
logits -> K15c; the backward overwrites the logits with their gradient, the decoder's
gradients come from library mm on it, and K15b writes the first layer's weight gradient. No
[B, n_items] tensor other than the logits exists at any point. One host read per step (the
batch's nonzero count, in the backward) sizes the K15b launches. On a CPU device every step
is the reference's dense torch op sequence.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from recbole_amd import ops
from recbole_amd.model.abstract_recommender import GeneralRecommender
from recbole_amd.utils import InputType

BAG_SITE = 0x3000                 # dropout site words of the K15a draws: + position (< 0x1000)
BAG_MAX_WIDTH = 1024


class _BagLinearFn(torch.autograd.Function):
    """K15a forward / K15b backward around (weight_t [n_items, N], bias [N]). rng = (seed,
    device counter) of the calling module; the backward recomputes the draw and advances the
    counter."""

    @staticmethod
    def forward(ctx, users, weight_t, bias, hist_ptr, hist_cols, p, rng, train, tanh):
        users = users.contiguous()
        drop = bool(train) and p > 0
        drawn = torch.empty(1, dtype=torch.int64, device=users.device) if drop else None
        y = ops.bag_linear_fwd(users, hist_ptr, hist_cols, weight_t.detach(), bias.detach(),
                               p=p, rng=rng, train=train, tanh=tanh, drawn=drawn)
        ctx.save_for_backward(users, hist_ptr, hist_cols, y)
        ctx.drawn, ctx.p, ctx.rng, ctx.train, ctx.tanh = drawn, p, rng, train, tanh
        ctx.n_items = weight_t.shape[0]
        return y

    @staticmethod
    def backward(ctx, gy):
        users, hist_ptr, hist_cols, y = ctx.saved_tensors
        G = (gy * (1.0 - y * y) if ctx.tanh else gy).contiguous()
        dWt = ops.bag_linear_bwd(G, users, hist_ptr, hist_cols, ctx.n_items, p=ctx.p,
                                 rng=ctx.rng, train=ctx.train, drawn=ctx.drawn)
        return None, dWt, ops.colsum(G), None, None, None, None, None, None


class BagLinear(nn.Module):
    """nn.Linear(n_items, out) whose input is a batch of sparse user rows. The weight is kept
    item-major (weight_t [n_items, out]) so a row's nonzeros gather whole rows; state_dict()
    holds it as the reference's `weight` [out, n_items] (hooks both ways). Built FROM an
    initialised nn.Linear, so the seeded initial weights are the reference's."""

    def __init__(self, linear, site=BAG_SITE):
        super().__init__()
        self.in_features, self.out_features = linear.in_features, linear.out_features
        self.weight_t = nn.Parameter(linear.weight.detach().t().contiguous())
        self.bias = nn.Parameter(linear.bias.detach().clone())
        self._site = site
        self._rng = None
        self._register_state_dict_hook(self._save_hook)
        self._register_load_state_dict_pre_hook(self._load_hook)

    @staticmethod
    def _save_hook(module, state, prefix, local_metadata):
        bias = state.pop(prefix + 'bias')
        state[prefix + 'weight'] = state.pop(prefix + 'weight_t').t().contiguous()
        state[prefix + 'bias'] = bias
        return state

    @staticmethod
    def _load_hook(state, prefix, local_metadata, strict, missing, unexpected, errors):
        if prefix + 'weight' in state:
            state[prefix + 'weight_t'] = state.pop(prefix + 'weight').t().contiguous()

    def extra_repr(self):
        return f'in_features={self.in_features}, out_features={self.out_features}, sparse rows'

    def kernels_apply(self, users):
        W = self.weight_t
        return (users.is_cuda and W.is_cuda and W.dtype == torch.float32
                and self.out_features % 4 == 0 and 4 <= self.out_features <= BAG_MAX_WIDTH)

    def drop_rng(self, dev):
        """(seed, device draw counter) of this layer's dropout site."""
        if self._rng is None or self._rng[1].device != dev:
            from recbole_amd.model.layers import site_seed
            self._rng = (site_seed(dev, self._site), torch.zeros(1, dtype=torch.int64, device=dev))
        return self._rng

    def forward(self, x):
        """The dense form: x [B, n_items]."""
        return torch.addmm(self.bias, x, self.weight_t)

    def bag(self, users, hist_ptr, hist_cols, p=0.0, train=False, tanh=False):
        """act(bias + the normalised, dropped-out rows of `users` times the weight) on K15a."""
        drop = bool(train) and 0 < p < 1
        rng = self.drop_rng(users.device) if drop else None
        y = _BagLinearFn.apply(users, self.weight_t, self.bias, hist_ptr, hist_cols,
                               float(p) if drop else 0.0, rng, drop, bool(tanh))
        if drop and not y.requires_grad:          # no backward will advance the draw counter
            rng[1].add_(1)
        return y


class _MultinomialNLLFn(torch.autograd.Function):
    """mean_b (n_b logsumexp(z_b) - sum_{i in S_b} z_b[i]) + extra (K15c). The backward
    overwrites z with its gradient IN PLACE, so z must have no other use; its version is
    bumped then, which makes autograd refuse any other saved use instead of reading it."""

    @staticmethod
    def forward(ctx, z, users, hist_ptr, hist_cols, extra):
        users = users.contiguous()
        _, rows, stat = ops.multinomial_nll_fwd(z, users, hist_ptr, hist_cols)
        ctx.save_for_backward(z, users, hist_ptr, hist_cols, stat)
        ctx.has_extra = extra is not None
        loss = (ops.fixed_sum(rows) / z.shape[0]).view(())
        return loss + extra.detach() if extra is not None else loss

    @staticmethod
    def backward(ctx, g):
        z, users, hist_ptr, hist_cols, stat = ctx.saved_tensors
        g1 = g.detach().reshape(1).to(torch.float32).contiguous()
        ops.multinomial_nll_bwd_(z, users, hist_ptr, hist_cols, stat, g1)
        bump = getattr(torch.autograd.graph, 'increment_version', None)
        if bump is not None:
            bump(z)
        return z, None, None, None, (g if ctx.has_extra else None)


class MatrixScorer(object):
    """One evaluation's scorer of a model whose scores are a matrix: scores(uids) is the
    [len(uids), n_items] logits in evaluation mode (K15a, the layers, addmm)."""

    def __init__(self, model):
        self.model = model
        self.device = model.out_layer().weight.device

    @torch.no_grad()
    def scores(self, uids):
        m = self.model
        was = m.training
        m.eval()
        try:
            return m.score_matrix(uids)
        finally:
            m.train(was)


class AutoEncoderRecommender(GeneralRecommender):
    """What MultiDAE and MultiVAE share; a subclass builds `encoder` / `decoder` as the
    reference does, calls _finish_init, and provides _bag_position, _latent and the loss."""
    input_type = InputType.PAIRWISE

    # not offered to the trainer's HIP-graph capture: the step reads the batch's nonzero
    # count on the host
    graph_step_safe = False

    def _load_history(self, dataset):
        ptr, cols = dataset.history_item_csr()
        self.register_buffer('hist_ptr', ptr, persistent=False)
        self.register_buffer('hist_cols', cols, persistent=False)

    def _finish_init(self, container, index):
        """Replace the initialised nn.Linear at container[index] by its BagLinear."""
        container[index] = BagLinear(container[index])
        self.bag_layer = [container[index]]          # a list: not registered twice

    def mlp_layers(self, layer_dims):
        mods = []
        for i, (d_in, d_out) in enumerate(zip(layer_dims[:-1], layer_dims[1:])):
            mods.append(nn.Linear(d_in, d_out))
            if i != len(layer_dims[:-1]) - 1:
                mods.append(nn.Tanh())
        return nn.Sequential(*mods)

    # ------------------------------------------------------------------ the dense API
    def get_rating_matrix(self, user):
        """[len(user), n_items] 0 / 1 rows (multivae.py:54-69); dense, for the API and the
        CPU path."""
        ptr = self.hist_ptr
        lens = ptr[user + 1] - ptr[user]
        total = int(lens.sum())
        rows = torch.repeat_interleave(torch.arange(user.shape[0], device=user.device), lens)
        start = torch.repeat_interleave(ptr[user] - (torch.cumsum(lens, 0) - lens), lens)
        cols = self.hist_cols[start + torch.arange(total, device=user.device)].long()
        R = torch.zeros(user.shape[0], self.n_items, device=user.device)
        R[rows, cols] = 1.0
        return R

    def _dropout(self, h):
        return F.dropout(h, self.drop_out, training=self.training)

    def out_layer(self):
        return self.decoder[-1]

    # ------------------------------------------------------------------ both devices
    def _first(self, user):
        """The first encoder layer's output (after its Tanh, if one follows) and the modules
        that come after it."""
        bag = self.bag_layer[0]
        seq, i = self._bag_position()
        tanh = i + 1 < len(seq) and isinstance(seq[i + 1], nn.Tanh)
        rest = seq[i + (2 if tanh else 1):]
        if bag.kernels_apply(user):
            h = bag.bag(user, self.hist_ptr, self.hist_cols, p=self.drop_out,
                        train=self.training, tanh=tanh)
        else:
            h = bag(self._dropout(F.normalize(self.get_rating_matrix(user))))
            if tanh:
                h = torch.tanh(h)
        return h, rest

    def _hidden(self, user):
        """(input of the output layer [B, width], whatever the loss needs besides)."""
        h, rest = self._first(user)
        lat, aux = self._latent(rest(h))
        return self.decoder[:-1](lat), aux

    def score_matrix(self, user):
        h, _ = self._hidden(user)
        out = self.out_layer()
        return torch.addmm(out.bias, h, out.weight.t())

    def _nll(self, z, user, extra=None):
        if z.is_cuda and z.dtype == torch.float32:
            return _MultinomialNLLFn.apply(z, user, self.hist_ptr, self.hist_cols, extra)
        ce = -(F.log_softmax(z, 1) * self.get_rating_matrix(user)).sum(1).mean()
        return ce if extra is None else ce + extra

    def predict(self, interaction):
        """One network pass per DISTINCT user, never a [pairs, n_items] matrix. A pair's score
        is <h_u, W_out[item]> + b_out[item]; where the distinct users' score rows are fewer
        numbers than the pairs' gathered weight rows (a sampled evaluation: a thousand pairs
        per user), the rows are formed once and the pairs read from them."""
        user, item = interaction[self.USER_ID], interaction[self.ITEM_ID]
        uniq, inv = torch.unique(user, return_inverse=True)
        h, _ = self._hidden(uniq)
        out = self.out_layer()
        if uniq.numel() * self.n_items <= user.numel() * h.shape[1]:
            return torch.addmm(out.bias, h, out.weight.t())[inv, item]
        return (h[inv] * out.weight[item]).sum(-1) + out.bias[item]

    def full_sort_predict(self, interaction):
        return self.score_matrix(interaction[self.USER_ID]).view(-1)

    # ------------------------------------------------------------------ trainer hooks
    def deferred_tables(self):
        """None: the two catalogue-sized weights get dense gradients and dense Adam, which
        is what the reference runs."""
        return []

    def fused_matrix_scorer(self):
        """A MatrixScorer over the current weights, or None where the kernels do not apply
        (a CPU device, a first width K15a does not take)."""
        W = self.out_layer().weight
        if not (W.is_cuda and W.dtype == torch.float32 and self.hist_ptr.is_cuda):
            return None
        return MatrixScorer(self)
