"""BERT4Rec (mirror of recbole/model/sequential_recommender/bert4rec.py:28-256).

Same modules, names, init and config keys as the reference (item_embedding with
n_items + 1 rows — the last is the mask token —, position_embedding with
max_seq_length + 1 rows, trm_encoder, LayerNorm, dropout). On the GPU:

* reconstruct_train_data (:111-156, a host copy and a Python loop over every position)
  -> K17a cloze_mask: one launch, counter-based draws (csrc/cloze.hip). On a CPU device
  the same rule from numpy (cloze_mask_host), so the two devices mask alike;
* item gather + position add + LayerNorm (:168-175) -> K9a (_SeqEmbedLNFn), the
  embedding dropout folded in while training;
* get_attention_mask (:90-97) -> mirec_seq_attn_mask_bidir_f32, the bidirectional mask
  in the [B, 1, L, L] layout K9e takes;
* loss_type 'CE' with ce_kernel 'fused' (:203-233) -> K17b compaction of the masked
  slots, K12 over the gathered encoder rows (no multi-hot bmm, no [B, M, n_items]
  logits), K17c placement of the row gradients; loss = sum of the row losses / n_act on
  the device (0 / 0 = NaN for a batch without a loss row, as the reference). Otherwise
  'CE', and 'BPR' on the device-drawn negatives, take the reference's op sequence;
* reconstruct_test_data (:158-166, a Python loop over the batch) -> one scatter_;
* predict -> K1 dot_rows; full_sort_predict -> the FP32-MFMA score matrix; the
  trainer's fused evaluator ranks the sequence outputs with K6.

As the reference, evaluation reads the encoder output at item_seq_len - 1 — the LAST REAL
ITEM's position, not the appended mask token's (which sits at item_seq_len).
The step runs eagerly (graph_step_safe = False) on one GPU.
"""
import numpy as np
import torch
import torch.nn as nn

from recbole_amd import ops
from recbole_amd._native import check, lib, ptr, stream_handle
from recbole_amd.model.abstract_recommender import SequentialRecommender
from recbole_amd.model.layers import LN_SITE, TransformerEncoder, _drop_rng, site_seed
from recbole_amd.model.sequential_recommender.sasrec import CE_WIDTHS, _SeqEmbedLNFn

CLOZE_SITE = 0x3000          # the Cloze draw's site word (LN sites 0x1000+, K9e 0x2000+)
CLOZE_ATTEMPTS = 4096        # csrc/cloze.hip kClozeAttempts
_M64 = (1 << 64) - 1
_U = np.uint64


def _mix64(z):
    """The splitmix64 finaliser (csrc/drop.h mix64) on uint64 arrays."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def cloze_mask_host(item_seq, M, n_items, mask_ratio, seed, c, negatives=True):
    """K17a's rule on the host (csrc/cloze.hip header): numpy int64 [B, L] in, (masked_seq,
    pos_items, neg_items or None, masked_index) out."""
    seq = np.asarray(item_seq, dtype=np.int64)
    B, L = seq.shape
    key = _mix64(_mix64(_U(seed & _M64)) ^ _U(c & _M64))
    thr = _U(min(4294967295, int(np.ldexp(1.0 - mask_ratio, 32))))
    e = np.arange(B * L, dtype=np.uint64).reshape(B, L)
    h = _mix64(key ^ (e >> _U(1)))
    draw = np.where((e & _U(1)) == 1, h >> _U(32), h & _U(0xFFFFFFFF))
    masked = (seq > 0) & ~(draw < thr)
    masked_seq = np.where(masked, np.int64(n_items), seq)
    pos = np.zeros((B, M), dtype=np.int64)
    idx = np.zeros((B, M), dtype=np.int64)
    neg = np.zeros((B, M), dtype=np.int64) if negatives else None
    span = _U(n_items - 1)
    for b in range(B):
        ts = np.flatnonzero(masked[b])[-M:]
        n = len(ts)
        if n == 0:
            continue
        pos[b, M - n:] = seq[b, ts]
        idx[b, M - n:] = ts
        if not negatives:
            continue
        row = set(seq[b].tolist())
        for s, t in enumerate(ts):
            base = _mix64(key ^ _U(1 << 63) ^ _U(b * L + int(t)))
            with np.errstate(over='ignore'):
                w = _mix64(base + np.arange(64, dtype=np.uint64))
            cand, k = None, 0
            while cand is None and k < CLOZE_ATTEMPTS:
                if k and k % 64 == 0:
                    with np.errstate(over='ignore'):
                        w = _mix64(base + np.arange(k, k + 64, dtype=np.uint64))
                v = 1 + int(((w[k % 64] >> _U(32)) * span) >> _U(32))
                cand = v if v not in row else None
                k += 1
            if cand is None:
                cand = next(v for v in range(1, n_items) if v not in row)
            neg[b, M - n + s] = cand
    return masked_seq, pos, neg, idx


class _ClozeCEFn(torch.autograd.Function):
    """sum_r [logsumexp_i <x_r, E_i> - <x_r, E_target_r>] / n_act over the n_act compact loss
    rows x_r = X[act_row[r]] (K12 over gathered rows), E = the first n_items rows of the item
    table; the backward places the compact row gradients with K17c and leaves the mask
    token's row of the table gradient zero."""

    @staticmethod
    def forward(ctx, X, W, act_row, act_target, n_act, slot_of, n_items):
        Xd = X.detach().contiguous()
        E = W.detach()[:n_items]
        lse, loss_rows = ops.full_ce_rows_fwd(Xd, act_row, act_target, E, n_act)
        ctx.save_for_backward(Xd, W, act_row, act_target, n_act, slot_of, lse)
        ctx.n_items = n_items
        return ops.fixed_sum(loss_rows).view(()) / n_act.to(torch.float32).view(())

    @staticmethod
    def backward(ctx, g):
        Xd, W, act_row, act_target, n_act, slot_of, lse = ctx.saved_tensors
        # g / n_act on the device (no host sync); K12's backward takes it as it stands
        gs = (g.detach().to(torch.float32).reshape(1) / n_act.to(torch.float32)).contiguous()
        dW = torch.empty_like(W)
        dW[ctx.n_items:].zero_()
        gS, _ = ops.full_ce_rows_bwd(Xd, act_row, act_target, W.detach()[:ctx.n_items], lse, gs,
                                     n_act, dE=dW[:ctx.n_items])
        return ops.rows_from_slots(gS, slot_of), dW, None, None, None, None, None


class BERT4Rec(SequentialRecommender):

    # the step is not offered to the trainer's HIP-graph capture (trainer/graph_step.py)
    graph_step_safe = False

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.n_layers = config['n_layers']
        self.n_heads = config['n_heads']
        self.hidden_size = config['hidden_size']
        self.inner_size = config['inner_size']
        self.hidden_dropout_prob = config['hidden_dropout_prob']
        self.attn_dropout_prob = config['attn_dropout_prob']
        self.hidden_act = config['hidden_act']
        self.layer_norm_eps = config['layer_norm_eps']
        self.mask_ratio = config['mask_ratio']
        self.loss_type = config['loss_type']
        self.initializer_range = config['initializer_range']
        # 'CE' only, as SASRec: 'library' (default) or 'fused' = K17b + K12 over rows + K17c
        self.ce_kernel = config['ce_kernel'] if config['ce_kernel'] is not None else 'library'
        if self.ce_kernel not in ('library', 'fused'):
            raise ValueError(f"ce_kernel must be 'library' or 'fused', got {self.ce_kernel!r}")
        self.mask_token = self.n_items
        self.mask_item_length = int(self.mask_ratio * self.max_seq_length)
        if self.mask_item_length < 1 or not 0 < self.mask_ratio < 1:
            raise ValueError(f'mask_ratio {self.mask_ratio} with MAX_ITEM_LIST_LENGTH '
                             f'{self.max_seq_length} leaves no masked slot '
                             f'(int(mask_ratio * length) = {self.mask_item_length})')
        if self.n_items - 1 <= self.max_seq_length:
            raise ValueError(f'{self.n_items - 1} items <= MAX_ITEM_LIST_LENGTH '
                             f'{self.max_seq_length}: a negative outside a full sequence '
                             f'could not be drawn')
        self.item_embedding = nn.Embedding(self.n_items + 1, self.hidden_size, padding_idx=0)
        self.position_embedding = nn.Embedding(self.max_seq_length + 1, self.hidden_size)
        self.trm_encoder = TransformerEncoder(
            n_layers=self.n_layers, n_heads=self.n_heads, hidden_size=self.hidden_size,
            inner_size=self.inner_size, hidden_dropout_prob=self.hidden_dropout_prob,
            attn_dropout_prob=self.attn_dropout_prob, hidden_act=self.hidden_act,
            layer_norm_eps=self.layer_norm_eps)
        self.LayerNorm = nn.LayerNorm(self.hidden_size, eps=self.layer_norm_eps)
        self.dropout = nn.Dropout(self.hidden_dropout_prob)
        self.dropout._ln_drop_site = LN_SITE            # LN site 0, as SASRec
        if self.loss_type not in ('BPR', 'CE'):
            raise NotImplementedError("Make sure 'loss_type' in ['BPR', 'CE']!")
        self._cloze_rng = None                          # (seed, counter) of the Cloze draws
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.initializer_range)
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    def _on_kernels(self, t):
        return t.is_cuda and self.item_embedding.weight.dtype == torch.float32

    def get_attention_mask(self, item_seq):
        """(1 - [item_seq > 0]) * -10000 over the key index (bert4rec.py:90-97): on the GPU one
        launch in K9e's [B, 1, L, L] layout, the reference's [B, 1, 1, L] otherwise."""
        if self._on_kernels(item_seq) and item_seq.dtype == torch.int64 and item_seq.dim() == 2:
            B, L = item_seq.shape
            mask = torch.empty(B, 1, L, L, dtype=torch.float32, device=item_seq.device)
            check(lib().mirec_seq_attn_mask_bidir_f32(ptr(item_seq.contiguous()), B, L, ptr(mask),
                                                      stream_handle()),
                  'mirec_seq_attn_mask_bidir_f32')
            return mask
        attention_mask = (item_seq > 0).long()
        extended = attention_mask.unsqueeze(1).unsqueeze(2)
        extended = extended.to(dtype=self.item_embedding.weight.dtype)
        return (1.0 - extended) * -10000.0

    # ------------------------------------------------------------------ the Cloze task
    def _cloze_state(self, dev):
        """(seed, draw counter) of this model's Cloze site on `dev`: the counter a device
        tensor on the GPU (K17a reads it there), a one-element list on the CPU."""
        st = self._cloze_rng
        if st is None or st[2] != dev:
            if dev.type == 'cuda':
                st = (site_seed(dev, CLOZE_SITE),
                      torch.zeros(1, dtype=torch.int64, device=dev), dev)
            else:
                st = ((torch.initial_seed() * 0x85EBCA6B + CLOZE_SITE) & _M64, [0], dev)
            self._cloze_rng = st
        return st

    def reconstruct_train_data(self, item_seq, negatives=True):
        """Mask item sequences for training: (masked_item_seq [B, L], pos_items, neg_items,
        masked_index [B, mask_item_length]); neg_items is None when not asked for."""
        B, L = item_seq.shape
        if self.n_items - 1 <= L:
            raise ValueError(f'{self.n_items - 1} items <= sequence length {L}: a negative '
                             f'outside a full sequence could not be drawn')
        M = self.mask_item_length
        seed, counter, dev = self._cloze_state(item_seq.device)
        if item_seq.is_cuda:
            out = ops.cloze_mask(item_seq.contiguous(), M, self.n_items, self.mask_ratio, seed,
                                 counter, negatives)
            counter.add_(1)                    # a forward without a backward: ours to advance
            return out
        res = cloze_mask_host(item_seq.numpy(), M, self.n_items, self.mask_ratio, seed,
                              counter[0], negatives)
        counter[0] += 1
        return tuple(None if a is None else torch.as_tensor(a, dtype=torch.long) for a in res)

    def reconstruct_test_data(self, item_seq, item_seq_len):
        """Append the mask token after each sequence's last item (one scatter_)."""
        padding = torch.zeros(item_seq.size(0), 1, dtype=torch.long, device=item_seq.device)
        item_seq = torch.cat((item_seq, padding), dim=-1)
        return item_seq.scatter_(1, item_seq_len.view(-1, 1).long(), self.mask_token)

    def forward(self, item_seq):
        if self._on_kernels(item_seq):
            p = self.dropout.p if (self.dropout.training and 0 < self.dropout.p < 1) else 0.0
            rng = _drop_rng(self.dropout, item_seq.device) if p > 0 else None
            input_emb = _SeqEmbedLNFn.apply(self.item_embedding.weight,
                                            self.position_embedding.weight,
                                            self.LayerNorm.weight, self.LayerNorm.bias, item_seq,
                                            self.layer_norm_eps, p, rng)
            if p == 0:
                input_emb = self.dropout(input_emb)
            elif not input_emb.requires_grad:     # no backward to advance the draw counter
                rng[1].add_(1)
        else:
            position_ids = torch.arange(item_seq.size(1), dtype=torch.long,
                                        device=item_seq.device)
            position_ids = position_ids.unsqueeze(0).expand_as(item_seq)
            input_emb = self.item_embedding(item_seq) + self.position_embedding(position_ids)
            input_emb = self.dropout(self.LayerNorm(input_emb))
        mask = self.get_attention_mask(item_seq)
        return self.trm_encoder(input_emb, mask, output_all_encoded_layers=True)[-1]

    def multi_hot_embed(self, masked_index, max_length):
        masked_index = masked_index.view(-1)
        multi_hot = torch.zeros(masked_index.size(0), max_length, device=masked_index.device)
        multi_hot[torch.arange(masked_index.size(0)), masked_index] = 1
        return multi_hot

    def _fused_ce(self, seq_output):
        return (self.loss_type == 'CE' and self.ce_kernel == 'fused' and seq_output.is_cuda
                and seq_output.dtype == torch.float32
                and self.item_embedding.weight.dtype == torch.float32
                and self.hidden_size in CE_WIDTHS)

    def calculate_loss(self, interaction):
        item_seq = interaction[self.ITEM_SEQ]
        masked_item_seq, pos_items, neg_items, masked_index = self.reconstruct_train_data(
            item_seq, negatives=self.loss_type == 'BPR')
        seq_output = self.forward(masked_item_seq)                 # [B, L, H]
        B, L, H = seq_output.shape
        if self._fused_ce(seq_output):
            act_row, act_target, n_act, slot_of = ops.cloze_compact(masked_index, pos_items, L)
            return _ClozeCEFn.apply(seq_output.reshape(B * L, H), self.item_embedding.weight,
                                    act_row, act_target, n_act, slot_of, self.n_items)
        # the reference's op sequence (bert4rec.py:208-233)
        pred_index_map = self.multi_hot_embed(masked_index, L).view(B, masked_index.size(1), -1)
        seq_output = torch.bmm(pred_index_map, seq_output)         # [B, M, H]
        targets = (masked_index > 0).float()
        if self.loss_type == 'BPR':
            pos_score = torch.sum(seq_output * self.item_embedding(pos_items), dim=-1)
            neg_score = torch.sum(seq_output * self.item_embedding(neg_items), dim=-1)
            return -torch.sum(torch.log(1e-14 + torch.sigmoid(pos_score - neg_score))
                              * targets) / torch.sum(targets)
        loss_fct = nn.CrossEntropyLoss(reduction='none')
        test_item_emb = self.item_embedding.weight[:self.n_items]
        logits = torch.matmul(seq_output, test_item_emb.transpose(0, 1))
        return torch.sum(loss_fct(logits.view(-1, test_item_emb.size(0)), pos_items.view(-1))
                         * targets.view(-1)) / torch.sum(targets)

    def _eval_output(self, interaction):
        item_seq_len = interaction[self.ITEM_SEQ_LEN]
        item_seq = self.reconstruct_test_data(interaction[self.ITEM_SEQ], item_seq_len)
        # as the reference: the last real item's position, not the mask token's
        return self.gather_indexes(self.forward(item_seq), item_seq_len - 1)

    def predict(self, interaction):
        seq_output = self._eval_output(interaction)
        test_item = interaction[self.ITEM_ID]
        if not seq_output.is_cuda:
            return torch.mul(seq_output, self.item_embedding(test_item)).sum(dim=1)
        return ops.dot_rows(seq_output.contiguous(), self.item_embedding.weight.detach(),
                            torch.arange(seq_output.shape[0], device=seq_output.device),
                            test_item)

    def full_sort_predict(self, interaction):
        seq_output = self._eval_output(interaction)
        test_items_emb = self.item_embedding.weight[:self.n_items]     # without the mask token
        if not seq_output.is_cuda:
            return torch.matmul(seq_output, test_items_emb.transpose(0, 1))
        return ops.score_matrix(seq_output.detach().contiguous(), test_items_emb.detach())

    def deferred_tables(self):
        """None: the loss reads the whole item table every step (dense Adam)."""
        return []

    # ------------------------------------------------------------------ fused eval hooks
    def fused_query_vectors(self, interaction):
        """Query vectors ranked by K6 (the sequence representations)."""
        return self._eval_output(interaction)

    def fused_item_table(self):
        return self.item_embedding.weight.detach()[:self.n_items]
