"""xDeepFM (mirror of recbole/model/context_aware_recommender/xdeepfm.py:31-194).

y = sigmoid(first_order + cin_linear(CIN(X0)) + mlp_layers(X0.view(B, -1))), nn.BCELoss plus
reg_weight * sum ||w||_2 over the `*weight` parameters of mlp_layers, first_order_linear and
the CIN convolutions. Same class name, config keys, module names, construction order and
init as the reference.

Where things run on the GPU:
  field rows + first-order term   K8's first-order form (ContextRecommender.linear_fields)
  CIN (cin_kernel: 'fused')       K18 (csrc/cin.hip): one autograd Function from X0 and the
                                  layers' weights to pooled [B, final_len]; it saves X0 and
                                  the X_{k+1} only — z = einsum('bmd,bhd->bhmd') [B, H m, D]
                                  never exists, nor does direct_k at [B, ., D]
  cin_linear, the three-term sum  torch ops on [B, final_len] and [B]
  DNN tower                       the reference applies Dropout before and ReLU after every
                                  Linear, the last 1-wide one included. K10 (model/mlp.py,
                                  unchanged) has no dropout in front of its head, so it runs
                                  the whole tower (head = the 1-wide Linear, then one
                                  torch.relu on [B, 1]) only when no dropout is drawn (eval,
                                  or dropout_prob 0) and its widths fit; a training step with
                                  dropout_prob > 0 runs the modules' torch path
  sigmoid + BCE                   _SigmoidBCEFn (first_order + cin | dnn)
  regularisation                  torch norms

cin_kernel: 'library', a CPU device and shapes K18 is not built for (mirec_cin_shape_ok) run
the reference's op sequence (einsum, view, conv1d, split, cat, sum).

One departure: the reference keeps its Conv1d layers in a plain Python list (:57-61), so
their weights are in no state_dict and no optimizer and never train. Here conv1d_list is an
nn.ModuleList (as upstream later made it): the CIN weights train and are saved. The
construction draws from the generator in the same order and _init_weights does not touch
Conv1d, so the seeded initial values are the reference's.

With reg_weight != 0 the norm of the [V, 1] first-order token table has a dense gradient
every step, so only the [V, d] token table runs on the deferred Adam schedule (and, as for
every model, only at an embedding_size the deferred kernels take: 4, 16, 32, ...; at the
default 10 every table takes the dense step).

The step runs eagerly (graph_step_safe = False: no capture around K18 was built) on one GPU.
"""
import torch
import torch.nn as nn

from recbole_amd import ops
from recbole_amd.model.abstract_recommender import ContextRecommender
from recbole_amd.model.context import _SigmoidBCEFn, sigmoid_prob
from recbole_amd.model.layers import MLPLayers
from recbole_amd.model.mlp import fused_deep_tensors, tensors_supported


def cin_plan(num_field, cin_layer_size, direct):
    """Per layer (H, N, n_hid, dir0, pool_off) and final_len (xdeepfm.py:57-75, 155-166):
    channels [0, n_hid) of a layer's output go on as X_{k+1}, channels [dir0, N) are pooled
    into columns [pool_off, pool_off + N - dir0) of the result."""
    plan, H, off = [], num_field, 0
    last = len(cin_layer_size) - 1
    for k, N in enumerate(cin_layer_size):
        if direct:
            n_hid, dir0 = (N if k < last else 0), 0
            nxt = N
        else:
            n_hid, dir0 = (N // 2, N // 2) if k < last else (0, 0)
            nxt = N // 2
        plan.append((H, N, n_hid, dir0, off))
        off += N - dir0
        H = nxt
    return plan, off


def cin_library(X0, weights, biases, plan):
    """The reference's op sequence (xdeepfm.py:136-169, identity activation): per layer the
    outer product z [B, H m, D], a 1x1 Conv1d, the split; the direct parts concatenated and
    summed over the embedding axis."""
    B, m, D = X0.shape
    Xk, direct = X0, []
    for (H, N, n_hid, dir0, _), W, b in zip(plan, weights, biases):
        z = torch.einsum('bmd,bhd->bhmd', X0, Xk).view(B, H * m, D)
        out = torch.nn.functional.conv1d(z, W, b)
        direct.append(out[:, dir0:])
        Xk = out[:, :n_hid]
    return torch.cat(direct, dim=1).sum(-1)


class _CINFn(torch.autograd.Function):
    """pooled [B, final_len] = CIN(X0; W_k, b_k) through K18. Saves X0 and the X_{k+1}."""

    @staticmethod
    def forward(ctx, plan, final_len, X0, *params):
        X0 = X0.contiguous()
        Ws = [w.detach().reshape(w.shape[0], -1).contiguous() for w in params[0::2]]
        bs = [b.detach().contiguous() for b in params[1::2]]
        pooled = torch.empty(X0.shape[0], final_len, dtype=torch.float32, device=X0.device)
        Xs = [X0]
        for (H, N, n_hid, dir0, off), W, b in zip(plan, Ws, bs):
            Xs.append(ops.cin_layer_fwd(X0, Xs[-1], W, b, n_hid, dir0, pooled, off))
        ctx.plan = plan
        ctx.w_shapes = [w.shape for w in params[0::2]]
        ctx.save_for_backward(*Xs[:-1], *Ws)       # the last layer has no X_{k+1}
        return pooled

    @staticmethod
    def backward(ctx, g_pooled):
        L = len(ctx.plan)
        Xs, Ws = ctx.saved_tensors[:L], ctx.saved_tensors[L:]
        X0 = Xs[0]
        gp = g_pooled.contiguous()
        dX0 = torch.empty_like(X0)
        grads = [None] * (2 * L)
        dXn = None
        for k in range(L - 1, -1, -1):             # dX0 takes the layers' terms in this order
            H, N, n_hid, dir0, off = ctx.plan[k]
            if ctx.needs_input_grad[3 + 2 * k] or ctx.needs_input_grad[4 + 2 * k]:
                dW, db = ops.cin_wgrad(X0, Xs[k], N, n_hid, dir0, dXn, gp, off)
                grads[2 * k], grads[2 * k + 1] = dW.view(ctx.w_shapes[k]), db
            dXn = ops.cin_layer_bwd(X0, Xs[k], Ws[k], n_hid, dir0, dXn, gp, off, dX0,
                                    accumulate=k < L - 1, layer0=k == 0)
        return (None, None, dX0, *grads)


class xDeepFM(ContextRecommender):

    graph_step_safe = False

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.mlp_hidden_size = config['mlp_hidden_size']
        self.reg_weight = config['reg_weight']
        self.dropout_prob = config['dropout_prob']
        self.direct = config['direct']
        self.cin_kernel = self._kernel_choice(config, 'cin_kernel')
        asked = list(config['cin_layer_size'])
        self.cin_layer_size = asked
        if not self.direct:                        # halves go on: even sizes (:48-54)
            self.cin_layer_size = [int(x // 2 * 2) for x in asked]
            if self.cin_layer_size[:-1] != asked[:-1]:
                self.logger.warning(
                    'Layer size of CIN should be even except for the last layer when direct is '
                    'True. It is changed to {}'.format(self.cin_layer_size))
        self.conv1d_list = nn.ModuleList()
        self.field_nums = [self.num_feature_field]
        for layer_size in self.cin_layer_size:
            self.conv1d_list.append(
                nn.Conv1d(self.field_nums[-1] * self.field_nums[0], layer_size, 1))
            self.field_nums.append(layer_size if self.direct else layer_size // 2)
        size_list = [self.embedding_size * self.num_feature_field] + self.mlp_hidden_size + [1]
        self.mlp_layers = MLPLayers(size_list, dropout=self.dropout_prob)
        if self.direct:
            self.final_len = sum(self.cin_layer_size)
        else:
            self.final_len = sum(self.cin_layer_size[:-1]) // 2 + self.cin_layer_size[-1]
        self.cin_plan, plan_len = cin_plan(self.num_feature_field, self.cin_layer_size,
                                           self.direct)
        assert plan_len == self.final_len
        self.cin_linear = nn.Linear(self.final_len, 1, bias=False)
        self.sigmoid = nn.Sigmoid()
        self.loss = nn.BCELoss()
        self.apply(self._init_weights)

    def reg_loss(self, parameters):
        """Sum of the 2-norms of the parameters named *weight (:90-100)."""
        reg_loss = 0
        for name, parm in parameters:
            if name.endswith('weight'):
                reg_loss = reg_loss + parm.norm(2)
        return reg_loss

    def calculate_reg_loss(self):
        """mlp_layers, first_order_linear and the CIN convolutions (:102-114)."""
        l2_reg = self.reg_loss(self.mlp_layers.named_parameters())
        l2_reg = l2_reg + self.reg_loss(self.first_order_linear.named_parameters())
        for conv1d in self.conv1d_list:
            l2_reg = l2_reg + self.reg_loss(conv1d.named_parameters())
        return l2_reg

    def cin_fused_applies(self, X0):
        """K18 runs when asked for, on the GPU, and every layer's shape is built."""
        if self.cin_kernel != 'fused' or not X0.is_cuda or X0.dtype != torch.float32:
            return False
        _, m, D = X0.shape
        return all(ops.cin_shape_ok(m, H, D, N) for H, N, _, _, _ in self.cin_plan)

    def compressed_interaction_network(self, input_features, activation='identity'):
        """pooled [B, final_len] (:116-169); identity is the only activation forward asks for."""
        if activation.lower() != 'identity':
            raise NotImplementedError('CIN activations other than identity are not built')
        params = []
        for conv in self.conv1d_list:
            params += [conv.weight, conv.bias]
        if self.cin_fused_applies(input_features):
            return _CINFn.apply(self.cin_plan, self.final_len, input_features, *params)
        return cin_library(input_features, params[0::2], params[1::2], self.cin_plan)

    def _dnn(self, x):
        """mlp_layers(x) [B, 1]: K10 + one ReLU when no dropout is drawn, else the modules."""
        lins = [mod for mod in self.mlp_layers.mlp_layers if isinstance(mod, nn.Linear)]
        weights = [mod.weight for mod in lins]
        draws = self.mlp_layers.training and self.dropout_prob > 0
        if x.is_cuda and not draws and tensors_supported(self.mlp_layers, weights, x):
            return torch.relu(fused_deep_tensors(self.mlp_layers, x, weights,
                                                 [mod.bias for mod in lins]))
        return self.mlp_layers(x)

    def _logits(self, interaction):
        """(first_order + cin [B], dnn [B, 1])."""
        X0, y_first = self.first_order_fields(interaction)
        cin = self.cin_linear(self.compressed_interaction_network(X0))
        dnn = self._dnn(X0.view(X0.shape[0], -1))
        return y_first + cin.squeeze(1), dnn

    def forward(self, interaction):
        y, dnn = self._logits(interaction)
        if y.is_cuda:
            return sigmoid_prob(y, dnn)
        return self.sigmoid(y + dnn.squeeze(1))

    def calculate_loss(self, interaction):
        label = interaction[self.LABEL]
        y, dnn = self._logits(interaction)
        if y.is_cuda:
            loss = _SigmoidBCEFn.apply(y, dnn, label)
        else:
            loss = self.loss(self.sigmoid(y + dnn.squeeze(1)), label.to(y.dtype))
        if self.reg_weight:
            loss = loss + self.reg_weight * self.calculate_reg_loss()
        return loss

    def predict(self, interaction):
        return self.forward(interaction)

    def deferred_tables(self):
        """The token table [V, d]; the first-order token weights [V, 1] too when no
        regularisation term gives them a dense gradient. K8 catches the [V, 1] rows up beside
        the [V, d] ones, so it is offered only with a [V, d] table the optimizer takes."""
        return self._deferred_token_tables(with_first_order=not self.reg_weight)
