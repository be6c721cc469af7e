"""Evaluation on the fused kernels: full-sort top-K (K6) for general and sequential
models, K14c / K15d for models scored by an MLP or a matrix, and the sampled (uni-N / pop-N) evaluations, for Trainer.evaluate."""
from __future__ import annotations

import numpy as np
import torch

from recbole_amd import ops


def fused_full_sort_eval(model, eval_data, topk_evaluator, user_batch=1 << 20, dp=None,
                         round_users=None):
    """Trainer.evaluate for a FULL loader (trainer.py:355-412) on K6: scores,
    pad/history mask, top-K and positive flags in one kernel per user batch; only
    the [n_users, K] positive matrix returns to the host for the metric
    reduction (evaluators.py:122-141). With a DataParallelStep `dp` every rank ranks
    its contiguous block of users and one all-gather assembles the flags in user
    order (trainer/dist.py) — the metrics of one GPU."""
    dev = model.fused_item_table().device
    K = max(topk_evaluator.topk)
    uids, hist_ptr, hist_cols, pos_ptr, pos_cols = eval_data.device_csr(dev)
    EI = model.fused_item_table().contiguous()
    n = uids.numel()
    lo, hi, blk = dp.user_block(n) if dp is not None else (0, n, n)
    flags = torch.empty(max(hi - lo, 0), K, dtype=torch.uint8, device=dev)
    rnd = round_users or _fullsort_round_users(dev, EI.shape[1])
    if dp is None and n > rnd and user_batch >= n and round_users != 0 and K >= 2:
        return _fullsort_overlapped(model, eval_data, topk_evaluator, uids, hist_ptr, hist_cols,
                                    pos_ptr, pos_cols, EI, K, flags, rnd)
    for s in range(lo, hi, user_batch):
        e = min(hi, s + user_batch)
        Uq = model.fused_user_vectors(uids[s:e]).contiguous()
        o = {'pos_flags': flags[s - lo:e - lo]}
        ops.fullsort_topk(Uq, EI, K, hist_ptr=hist_ptr[s:e + 1], hist_cols=hist_cols,
                          pos_ptr=pos_ptr[s:e + 1], pos_cols=pos_cols, out=o)
    if dp is not None:
        flags = dp.gather_rows(flags, n, blk)
    pos_idx = flags.cpu().numpy().astype(bool)
    return topk_evaluator.evaluate_pos_idx(pos_idx, eval_data.get_pos_len_list())


def fused_pair_full_sort_eval(model, eval_data, topk_evaluator, user_batch=1 << 16):
    """Trainer.evaluate for a FULL loader and a model whose score is not a dot product but a
    per-pair MLP (NeuMF): model.fused_pair_scorer() forms the item part of the first layer
    once, then per user batch the user part and K14c — the layers 2..L, the MF dot, the
    pad / history mask, the top-K and the positive flags in one kernel. One GPU."""
    scorer = model.fused_pair_scorer()
    dev = scorer.device
    K = max(topk_evaluator.topk)
    uids, hist_ptr, hist_cols, pos_ptr, pos_cols = eval_data.device_csr(dev)
    n = uids.numel()
    flags = torch.empty(n, K, dtype=torch.uint8, device=dev)
    for s in range(0, n, user_batch):
        e = min(n, s + user_batch)
        scorer.topk(uids[s:e], K, hist_ptr=hist_ptr[s:e + 1], hist_cols=hist_cols,
                    pos_ptr=pos_ptr[s:e + 1], pos_cols=pos_cols,
                    out={'pos_flags': flags[s:e]})
    pos_idx = flags.cpu().numpy().astype(bool)
    return topk_evaluator.evaluate_pos_idx(pos_idx, eval_data.get_pos_len_list())


MATRIX_EVAL_BYTES = 256 << 20      # budget of one user block's score matrix


def fused_matrix_full_sort_eval(model, eval_data, topk_evaluator, user_batch=None):
    """Trainer.evaluate for a FULL loader and a model whose scores are a matrix and not a dot
    product of two tables (MultiDAE, MultiVAE): per user block, model.fused_matrix_scorer()
    forms the [block, n_items] logits and K15d (ops.matrix_topk) applies the pad / history
    mask, takes the top-K and tests the positives; only the [n_users, K] flags go to the
    host. user_batch defaults to the largest block whose score matrix stays within
    MATRIX_EVAL_BYTES = 256 MiB (2,509 users at 26,745 items). One GPU."""
    scorer = model.fused_matrix_scorer()
    dev = scorer.device
    K = max(topk_evaluator.topk)
    uids, hist_ptr, hist_cols, pos_ptr, pos_cols = eval_data.device_csr(dev)
    n = uids.numel()
    if user_batch is None:
        user_batch = max(1, MATRIX_EVAL_BYTES // (4 * model.n_items))
    flags = torch.empty(n, K, dtype=torch.uint8, device=dev)
    for s in range(0, n, user_batch):
        e = min(n, s + user_batch)
        ops.matrix_topk(scorer.scores(uids[s:e]), K, hist_ptr=hist_ptr[s:e + 1],
                        hist_cols=hist_cols, pos_ptr=pos_ptr[s:e + 1], pos_cols=pos_cols,
                        out={'pos_flags': flags[s:e]})
    pos_idx = flags.cpu().numpy().astype(bool)
    return topk_evaluator.evaluate_pos_idx(pos_idx, eval_data.get_pos_len_list())


def _fullsort_round_users(dev, d):
    """Users of one full round of K6 workgroups (128 users each; two resident per
    CU for d <= 128, one for d = 256): launches of this size fill the chip."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return 128 * cus * (2 if d <= 128 else 1)


def _fullsort_overlapped(model, eval_data, topk_evaluator, uids, hist_ptr, hist_cols, pos_ptr,
                         pos_cols, EI, K, flags, chunk):
    """fused_full_sort_eval in round-sized K6 launches: each launch's flags go to the
    host on a copy stream and its metric rows are reduced while the next launches
    run (TopKEvaluator.evaluate_pos_idx_chunks: the same values as one block)."""
    dev = flags.device
    n = uids.numel()
    host = torch.empty(flags.shape, dtype=torch.uint8, pin_memory=True)
    copy_stream = torch.cuda.Stream(device=dev)
    done = []
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        Uq = model.fused_user_vectors(uids[s:e]).contiguous()
        # a launch far below a round (the last one) splits the item range instead,
        # so it does not take a full round's time for a few workgroups
        wgs, full = -(-(e - s) // 128), chunk // 128
        split = min(16, full // wgs) if 2 * wgs <= full else 1
        ops.fullsort_topk(Uq, EI, K, hist_ptr=hist_ptr[s:e + 1], hist_cols=hist_cols,
                          pos_ptr=pos_ptr[s:e + 1], pos_cols=pos_cols,
                          out={'pos_flags': flags[s:e]}, n_split=split)
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ready)
            host[s:e].copy_(flags[s:e], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(copy_stream)
        done.append((s, e, copied, Uq))
    pl = np.asarray(eval_data.get_pos_len_list())

    def blocks():
        for s, e, copied, _ in done:
            copied.synchronize()
            yield host[s:e].numpy().astype(bool), pl[s:e]
    out = topk_evaluator.evaluate_pos_idx_chunks(blocks(), n)
    torch.cuda.current_stream(dev).wait_stream(copy_stream)
    return out


def fused_seq_full_sort_eval(model, eval_data, topk_evaluator):
    """Trainer.evaluate for SequentialFullDataLoader (trainer.py:328-353 with
    sequential_dataloader.py:318-345: pad column masked, the target swapped to
    the front, no history mask) on K6: per batch, the sequence representations
    are ranked against every item with the target as the only positive."""
    dev = model.fused_item_table().device
    K = max(topk_evaluator.topk)
    EI = model.fused_item_table().contiguous()
    flags = []
    for interaction, _, _, _, _ in eval_data:
        inter = interaction.to(dev)
        Uq = model.fused_query_vectors(inter).detach().contiguous()
        n = Uq.shape[0]
        pos_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev)
        pos_cols = inter[eval_data.iid_field].to(torch.int32).contiguous()
        o = ops.fullsort_topk(Uq, EI, K, pos_ptr=pos_ptr, pos_cols=pos_cols)
        flags.append(o['pos_flags'])
    pos_idx = torch.cat(flags).cpu().numpy().astype(bool)
    return topk_evaluator.evaluate_pos_idx(pos_idx, eval_data.get_pos_len_list())


def fused_seq_sampled_eval(model, eval_data, topk_evaluator):
    """Trainer.evaluate for SequentialNegSampleDataLoader in evaluation (uni-N, this
    fork's validation, data/utils.py:86-88): the reference repeats every sequence
    1+N times through the whole model (predict on each copy) and ranks the padded
    score rows with topk (trainer.py:384-409, abstract_evaluator.py:65-75). Here each
    sequence is encoded once and K9c counts the sampled items that beat the
    positive; pos_idx[q, r] = (rank[q] == r). The negatives are the ones the
    RepeatableSampler's per-row walk would draw (sample_by_user_ids(uid, N) for row
    after row, no rejection): the next N values of the walk, row by row, taken with
    one device gather; the walk pointer advances by rows x N exactly as it would."""
    from recbole_amd._native import check, lib, ptr, stream_handle
    sampler = eval_data.sampler
    dev = model.fused_item_table().device
    EI = model.fused_item_table().contiguous()
    K = max(topk_evaluator.topk)
    m = eval_data.neg_sample_by
    sampler.to_device(dev)
    L = sampler.random_list_length
    ranks = []
    for start in range(0, eval_data.pr_end, eval_data.step):
        inter = eval_data.augmentation(slice(start, start + eval_data.step)).to(dev)
        uids = inter[eval_data.uid_field]
        n = uids.numel()
        if n == 0:
            continue
        mn, mx = int(uids.min()), int(uids.max())
        if mn < 0 or mx >= sampler.n_users:
            raise ValueError(f'user_id [{mn if mn < 0 else mx}] not exist.')
        idx = (sampler._pr_dev + torch.arange(n * m, device=dev)) % L
        neg = sampler._rl_dev[idx].to(torch.int64)
        sampler._pr_dev.copy_((sampler._pr_dev + n * m) % L)
        S = model.fused_query_vectors(inter).detach().contiguous()
        pos = inter[eval_data.iid_field].to(torch.int64).contiguous()
        rank = torch.empty(n, dtype=torch.int32, device=dev)
        rc = lib().mirec_rank_of_pos_f32(ptr(S), ptr(EI), EI.shape[0], EI.shape[1], ptr(pos),
                                         ptr(neg), n, m, ptr(rank), stream_handle())
        check(rc, 'mirec_rank_of_pos_f32')
        ranks.append(rank)
    rank = torch.cat(ranks) if ranks else torch.zeros(0, dtype=torch.int32, device=dev)
    pos_idx = (rank.unsqueeze(1) == torch.arange(K, device=dev).unsqueeze(0)).cpu().numpy()
    return topk_evaluator.evaluate_pos_idx(pos_idx, eval_data.get_pos_len_list())


def fused_general_sampled_eval(model, eval_data, evaluator):
    """Trainer.evaluate for a GeneralNegSampleDataLoader in evaluation (uni-N /
    pop-N, point-wise, one batch = whole users: this fork's uni1000 validation,
    data/utils.py:86-88) with every batch built on the device.

    The reference builds each batch on the host (general_dataloader.py:210-221):
    per user, slice its rows, sample_by_user_ids(uids, N) (one sampler call per
    user), repeat them 1+N times with the negatives written after the positives
    (_neg_sample_by_point_wise_sampling, :243-251), join every user/item feature
    (unused by the general models' predict), concatenate the users, then
    predict + evaluator.collect (trainer.py:384-409). Here one K4 launch walks the
    batch's per-user calls in order (mirec_sample_walk_segments: the same walk,
    the same values, the pointer advanced exactly as the calls would), the
    [pos | negs] layout is assembled with two device scatters, and the model's
    own predict and the evaluator's collect run on the same layout — so the
    collected matrices are the ones the reference sequence produces on this
    device, without the per-user host loop and the feature joins."""
    sampler = eval_data.sampler
    dev = model.fused_item_table().device
    sampler.to_device(dev)
    ds = eval_data.dataset
    uid_f, iid_f = eval_data.uid_field, eval_data.iid_field
    items_all = ds.inter_feat[iid_f].to(dev)
    N = int(eval_data.neg_sample_by)
    times = eval_data.times
    test_bs = eval_data.config['eval_batch_size']
    out = []
    for start in range(0, eval_data.pr_end, eval_data.step):
        ul = eval_data.uid_list[start:start + eval_data.step]
        n_u = eval_data.uid2items_num[ul].astype(np.int64)
        s_u = eval_data.uid2start[ul].astype(np.int64)
        P = int(n_u.sum())
        if P == 0:
            continue
        seg = np.r_[0, np.cumsum(n_u)]
        # positive rows of the batch's users, user after user (dataset sorted by user)
        rows = np.repeat(s_u - seg[:-1], n_u) + np.arange(P)
        keys = torch.as_tensor(np.repeat(ul, n_u), dtype=torch.int64).to(dev)
        negs = sampler.launch_segments(keys, torch.as_tensor(seg).to(dev), int(n_u.max()), N)
        # block of user b: [its n_b positives | its n_b * N negatives], blocks in order
        blk = np.repeat(seg[:-1] * times, n_u)                  # block start per positive
        within = np.arange(P) - np.repeat(seg[:-1], n_u)        # positive's index in its block
        pos_at = torch.as_tensor(blk + within).to(dev)
        neg_blk = np.repeat(seg[:-1] * times + n_u, n_u * N)    # negatives' region start
        neg_at = torch.as_tensor(neg_blk + np.arange(P * N) - np.repeat(seg[:-1] * N, n_u * N))
        items = torch.empty(P * times, dtype=torch.int64, device=dev)
        items[pos_at] = items_all[torch.as_tensor(rows).to(dev)]
        items[neg_at.to(dev)] = negs
        users = torch.as_tensor(np.repeat(ul, n_u * times), dtype=torch.int64).to(dev)
        from recbole_amd.data.interaction import Interaction
        inter = Interaction({uid_f: users, iid_f: items})
        inter.set_additional_info(list(n_u), list(n_u * times))
        bs = inter.length
        if bs <= test_bs:
            scores = model.predict(inter)
        else:                                   # trainer.py _spilt_predict
            scores = torch.cat([model.predict(Interaction({uid_f: users[i:i + test_bs],
                                                           iid_f: items[i:i + test_bs]}))
                                for i in range(0, bs, test_bs)])
        out.append(evaluator.collect(inter, scores))
    sampler.check_status()
    return evaluator.evaluate(out, eval_data)
