"""numpy restatement of K17a / K17b (csrc/cloze.hip) — BERT4Rec's Cloze masking and the
compaction of its loss rows — plus a float64 torch restatement of the loss over masked
positions (reference bert4rec.py:203-233), given the masked tensors. Test infrastructure
only; the draws come from tests/drop_spec.py.

    key     = drop_spec.key(seed, c)                 c: the site's counter at the call
    masked  = item > 0 and not ln_keep(element e = b*L + t, p = mask_ratio)
    layout  = the reference's: masked positions -> mask_token = n_items; pos_items /
              masked_index / neg_items [B, M] left padded with 0, the LAST M of a longer row
    negative of masked element e, attempts k = 0, 1, ...:
              w_k  = splitmix64(splitmix64(key ^ 2^63 ^ e) + k)
              cand = 1 + (((w_k >> 32) * (n_items - 1)) >> 32)
              the first cand not among the row's L original entries; after ATTEMPTS
              rejections the smallest id >= 1 not in the row
    compact = the [B, M] slots with masked_index > 0 in ascending (b, slot) order
"""
import numpy as np
import torch

from tests import drop_spec

_U = np.uint64
ATTEMPTS = 4096


def mask_decisions(seq, mask_ratio, seed, c):
    """[B, L] bool: the positions K17a masks."""
    seq = np.asarray(seq, dtype=np.int64)
    keep = drop_spec.ln_keep(seed, c, seq.size, mask_ratio).reshape(seq.shape)
    return (seq > 0) & ~keep


def negative(key, e, row_items, n_items):
    base = drop_spec.splitmix64(key ^ _U(1 << 63) ^ _U(e))
    row = set(int(x) for x in row_items)
    for k in range(ATTEMPTS):
        with np.errstate(over='ignore'):
            w = int(drop_spec.splitmix64(base + _U(k)))
        cand = 1 + (((w >> 32) * (n_items - 1)) >> 32)
        if cand not in row:
            return cand
    return next(v for v in range(1, n_items) if v not in row)


def cloze_mask(seq, M, n_items, mask_ratio, seed, c, negatives=True):
    """(masked_seq [B, L], pos_items, neg_items or None, masked_index [B, M]) of K17a."""
    seq = np.asarray(seq, dtype=np.int64)
    B, L = seq.shape
    masked = mask_decisions(seq, mask_ratio, seed, c)
    key = drop_spec.key(seed, c)
    masked_seq = seq.copy()
    masked_seq[masked] = n_items
    pos = np.zeros((B, M), dtype=np.int64)
    idx = np.zeros((B, M), dtype=np.int64)
    neg = np.zeros((B, M), dtype=np.int64) if negatives else None
    for b in range(B):
        ts = [t for t in range(L) if masked[b, t]][-M:]
        for s, t in enumerate(ts, start=M - len(ts)):
            pos[b, s], idx[b, s] = seq[b, t], t
            if negatives:
                neg[b, s] = negative(key, b * L + t, seq[b], n_items)
    return masked_seq, pos, neg, idx


def reference_loop(seq, masked, M, mask_token, neg_of=None):
    """BERT4Rec.reconstruct_train_data (bert4rec.py:111-156) restated literally — Python
    lists, the break at the first padding item, _padding_sequence — with the mask decision
    masked[b][t] in place of `random.random() < mask_ratio` and neg_of(b, t) in place of
    _neg_sample."""
    def pad(sequence, max_length):
        sequence = [0] * (max_length - len(sequence)) + sequence
        return sequence[-max_length:]
    out_seq, out_pos, out_neg, out_idx = [], [], [], []
    for b, instance in enumerate(np.asarray(seq).tolist()):
        masked_sequence = instance.copy()
        pos_item, neg_item, index_ids = [], [], []
        for index_id, item in enumerate(instance):
            if item == 0:
                break
            if masked[b][index_id]:
                pos_item.append(item)
                neg_item.append(neg_of(b, index_id) if neg_of else 0)
                masked_sequence[index_id] = mask_token
                index_ids.append(index_id)
        out_seq.append(masked_sequence)
        out_pos.append(pad(pos_item, M))
        out_neg.append(pad(neg_item, M))
        out_idx.append(pad(index_ids, M))
    as_ = lambda x: np.asarray(x, dtype=np.int64).reshape(len(out_seq), -1)
    return as_(out_seq), as_(out_pos), as_(out_neg), as_(out_idx)


def compact(masked_index, pos_items, L):
    """(act_row [B*M], act_target [B*M], n_act, slot_of [B*L]) of K17b."""
    idx = np.asarray(masked_index, dtype=np.int64)
    pos = np.asarray(pos_items, dtype=np.int64)
    B, M = idx.shape
    act_row = np.zeros(B * M, dtype=np.int64)
    act_target = np.zeros(B * M, dtype=np.int64)
    slot_of = np.full(B * L, -1, dtype=np.int32)
    n = 0
    for b in range(B):
        for s in range(M):
            if idx[b, s] > 0:
                act_row[n] = b * L + idx[b, s]
                act_target[n] = pos[b, s]
                slot_of[b * L + idx[b, s]] = n
                n += 1
    return act_row, act_target, n, slot_of


def ce_loss64(seq_output, item_weight, pos_items, masked_index, n_items):
    """The reference's 'CE' loss (bert4rec.py:208-213, 225-233) in float64 torch ops:
    seq_output [B, L, H] and item_weight [n_items + 1, H] double (autograd flows to both)."""
    B, L, _ = seq_output.shape
    M = masked_index.shape[1]
    flat = masked_index.reshape(-1)
    multi_hot = torch.zeros(flat.numel(), L, dtype=torch.float64)
    multi_hot[torch.arange(flat.numel()), flat] = 1
    rows = torch.bmm(multi_hot.view(B, M, L), seq_output)
    test_item_emb = item_weight[:n_items]
    logits = torch.matmul(rows, test_item_emb.transpose(0, 1))
    targets = (masked_index > 0).double().view(-1)
    ce = torch.nn.functional.cross_entropy(logits.view(-1, n_items), pos_items.reshape(-1),
                                           reduction='none')
    return torch.sum(ce * targets) / torch.sum(targets)


def rows_ce64(X, row, target, E, n_act, g=1.0):
    """float64 (loss_rows [R], gS [R, d], dE [I, d]) of K12 over gathered rows with the
    backward's factor g as it stands: rows past n_act are zero."""
    X64, E64 = X.double(), E.double().requires_grad_()
    R = row.numel()
    S = X64[row[:n_act]].clone().requires_grad_()
    loss_rows = torch.zeros(R, dtype=torch.float64)
    gS = torch.zeros(R, X.shape[1], dtype=torch.float64)
    dE = torch.zeros_like(E64)
    if n_act:
        lr = torch.nn.functional.cross_entropy(S @ E64.T, target[:n_act], reduction='none')
        (lr.sum() * g).backward()
        loss_rows[:n_act] = lr.detach()
        gS[:n_act] = S.grad
        dE = E64.grad
    return loss_rows, gS, dE
