"""GRU4Rec as the reference writes it (recbole/model/sequential_recommender/gru4rec.py:38-102),
restated on plain torch for the GRU4Rec tests — test infrastructure, no kernels: the same
modules in the same construction order with the same init, dense over all B x L positions
and then the gather, the BPR / CE losses on torch ops. Dropout is left out of the forward
(the tests run with dropout_prob 0); the module is there so the state-dict keys match."""
import torch
import torch.nn as nn
from torch.nn.init import xavier_normal_, xavier_uniform_


class GRU4RecRef(nn.Module):

    def __init__(self, n_items, embedding_size, hidden_size, num_layers=1, loss_type='CE'):
        super().__init__()
        self.loss_type = loss_type
        self.item_embedding = nn.Embedding(n_items, embedding_size, padding_idx=0)
        self.emb_dropout = nn.Dropout(0.0)
        self.gru_layers = nn.GRU(input_size=embedding_size, hidden_size=hidden_size,
                                 num_layers=num_layers, bias=False, batch_first=True)
        self.dense = nn.Linear(hidden_size, embedding_size)
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Embedding):
            xavier_normal_(module.weight)
        elif isinstance(module, nn.GRU):
            xavier_uniform_(module.weight_hh_l0)
            xavier_uniform_(module.weight_ih_l0)

    def forward(self, item_seq, item_seq_len):
        out, _ = self.gru_layers(self.item_embedding(item_seq))
        out = self.dense(out)
        idx = (item_seq_len - 1).view(-1, 1, 1).expand(-1, -1, out.shape[-1])
        return out.gather(dim=1, index=idx).squeeze(1)

    def calculate_loss(self, item_seq, item_seq_len, pos, neg=None):
        s = self.forward(item_seq, item_seq_len)
        if self.loss_type == 'BPR':
            ps = torch.sum(s * self.item_embedding(pos), dim=-1)
            ns = torch.sum(s * self.item_embedding(neg), dim=-1)
            return -torch.log(1e-10 + torch.sigmoid(ps - ns)).mean()
        logits = torch.matmul(s, self.item_embedding.weight.transpose(0, 1))
        return nn.functional.cross_entropy(logits, pos)

    def predict(self, item_seq, item_seq_len, item):
        return torch.mul(self.forward(item_seq, item_seq_len), self.item_embedding(item)).sum(1)

    def full_sort_predict(self, item_seq, item_seq_len):
        return torch.matmul(self.forward(item_seq, item_seq_len),
                            self.item_embedding.weight.transpose(0, 1))


def ref_of(model, dtype=torch.float64):
    """The restatement carrying `model`'s weights (loaded through its state_dict), in `dtype`
    on the CPU."""
    ref = GRU4RecRef(model.n_items, model.embedding_size, model.hidden_size, model.num_layers,
                     model.loss_type).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()})
    return ref
