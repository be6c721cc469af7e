"""GRU4Rec (mirror of recbole/model/sequential_recommender/gru4rec.py:28-119).

Same modules, names, construction order and init as the reference (item_embedding,
emb_dropout, gru_layers — an nn.GRU kept as the parameter container, so state-dict keys
and checkpoints match — and dense). On the GPU:

* the item gather (:77) -> K1 gather_rows, its gradient grouped by item (K2 segment_sort +
  segment_scatter_add: fixed order, padding positions contribute nothing, as padding_idx=0);
* the GRU (:79) is the library's nn.GRU on the device (a fused recurrence kernel is not
  part of this build);
* dense (:80) on the B gathered last positions (the reference applies it to all B x L
  and then gathers: the same value per row);
* loss_type 'BPR' -> K3 (_SeqBPRFn); 'CE' -> the library matmul + CrossEntropyLoss, or K12
  (_FullCEFn) under ce_kernel 'fused';
* predict -> K1 dot_rows; full_sort_predict -> the FP32-MFMA score matrix; the trainer's
  fused evaluator ranks the sequence outputs with K6.
On a CPU device every step is the reference's torch op sequence.
"""
import torch
import torch.nn as nn
from torch.nn.init import xavier_normal_, xavier_uniform_

from recbole_amd import ops
from recbole_amd.model.abstract_recommender import SequentialRecommender
from recbole_amd.model.loss import BPRLoss
from recbole_amd.model.sequential_recommender.sasrec import CE_WIDTHS, _FullCEFn, _SeqBPRFn


class _ItemGatherFn(torch.autograd.Function):
    """item_embedding(item_seq) with padding_idx 0: K1 forward; backward the rows grouped by
    item id (K2) and summed in a fixed order, the padding positions' rows zeroed first."""

    @staticmethod
    def forward(ctx, E, item_seq):
        seq = item_seq.contiguous()
        ctx.save_for_backward(seq)
        ctx.nI = E.shape[0]
        return ops.gather_rows(E.detach(), seq.view(-1)).view(*seq.shape, E.shape[1])

    @staticmethod
    def backward(ctx, g):
        (seq,) = ctx.saved_tensors
        keys = seq.view(-1)
        rows = (g.reshape(keys.numel(), -1) * (keys != 0).unsqueeze(1)).contiguous()
        dE = ops.segment_scatter_add(rows, ops.segment_sort(keys, ctx.nI),
                                     torch.zeros(ctx.nI, rows.shape[1], dtype=rows.dtype,
                                                 device=rows.device))
        return dE, None


class GRU4Rec(SequentialRecommender):

    # the recurrence is the library's GRU, whose launches this project does not own: the
    # step is not offered to the trainer's HIP-graph capture (trainer/graph_step.py) and
    # runs eagerly, whatever train_graph says
    graph_step_safe = False

    def __init__(self, config, dataset):
        super().__init__(config, dataset)
        self.embedding_size = config['embedding_size']
        self.hidden_size = config['hidden_size']
        self.loss_type = config['loss_type']
        self.num_layers = config['num_layers']
        self.dropout_prob = config['dropout_prob']
        # 'CE' only, as SASRec: 'library' (default) or 'fused' = K12 where it applies
        self.ce_kernel = config['ce_kernel'] if config['ce_kernel'] is not None else 'library'
        if self.ce_kernel not in ('library', 'fused'):
            raise ValueError(f"ce_kernel must be 'library' or 'fused', got {self.ce_kernel!r}")
        self.item_embedding = nn.Embedding(self.n_items, self.embedding_size, padding_idx=0)
        self.emb_dropout = nn.Dropout(self.dropout_prob)
        self.gru_layers = nn.GRU(input_size=self.embedding_size, hidden_size=self.hidden_size,
                                 num_layers=self.num_layers, bias=False, batch_first=True)
        self.dense = nn.Linear(self.hidden_size, self.embedding_size)
        if self.loss_type == 'BPR':
            self.loss_fct = BPRLoss()
        elif self.loss_type == 'CE':
            self.loss_fct = nn.CrossEntropyLoss()
        else:
            raise NotImplementedError("Make sure 'loss_type' in ['BPR', 'CE']!")
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Embedding):
            xavier_normal_(module.weight)
        elif isinstance(module, nn.GRU):
            xavier_uniform_(module.weight_hh_l0)
            xavier_uniform_(module.weight_ih_l0)

    def forward(self, item_seq, item_seq_len):
        W = self.item_embedding.weight
        if item_seq.is_cuda and W.dtype == torch.float32:
            item_seq_emb = _ItemGatherFn.apply(W, item_seq)
        else:
            item_seq_emb = self.item_embedding(item_seq)
        item_seq_emb_dropout = self.emb_dropout(item_seq_emb)
        gru_output, _ = self.gru_layers(item_seq_emb_dropout)
        # dense on the B last positions (per row the value of dense over all, gathered)
        return self.dense(self.gather_indexes(gru_output, item_seq_len - 1))

    def calculate_loss(self, interaction):
        item_seq = interaction[self.ITEM_SEQ]
        item_seq_len = interaction[self.ITEM_SEQ_LEN]
        seq_output = self.forward(item_seq, item_seq_len)
        pos_items = interaction[self.POS_ITEM_ID]
        W = self.item_embedding.weight
        gpu = seq_output.is_cuda and seq_output.dtype == torch.float32 and W.dtype == torch.float32
        if self.loss_type == 'BPR':
            neg_items = interaction[self.NEG_ITEM_ID]
            if gpu:
                return _SeqBPRFn.apply(seq_output, W, pos_items, neg_items)
            pos_score = torch.sum(seq_output * self.item_embedding(pos_items), dim=-1)
            neg_score = torch.sum(seq_output * self.item_embedding(neg_items), dim=-1)
            return self.loss_fct(pos_score, neg_score)
        if self.ce_kernel == 'fused' and gpu and self.embedding_size in CE_WIDTHS:
            return _FullCEFn.apply(seq_output, W, pos_items)
        logits = torch.matmul(seq_output, W.transpose(0, 1))
        return self.loss_fct(logits, pos_items)

    def predict(self, interaction):
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        test_item = interaction[self.ITEM_ID]
        if not seq_output.is_cuda:
            return torch.mul(seq_output, self.item_embedding(test_item)).sum(dim=1)
        return ops.dot_rows(seq_output.contiguous(), self.item_embedding.weight.detach(),
                            torch.arange(seq_output.shape[0], device=seq_output.device),
                            test_item)

    def full_sort_predict(self, interaction):
        seq_output = self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])
        if not seq_output.is_cuda:
            return torch.matmul(seq_output, self.item_embedding.weight.transpose(0, 1))
        return ops.score_matrix(seq_output.detach().contiguous(),
                                self.item_embedding.weight.detach())

    def deferred_tables(self):
        """None yet: the item table takes the dense Adam path."""
        return []

    # ------------------------------------------------------------------ fused eval hooks
    def fused_query_vectors(self, interaction):
        """Query vectors ranked by K6 (the sequence representations)."""
        return self.forward(interaction[self.ITEM_SEQ], interaction[self.ITEM_SEQ_LEN])

    def fused_item_table(self):
        return self.item_embedding.weight.detach()

