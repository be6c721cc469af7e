"""Data-parallel generic trainer path on the GPU (trainer/dist.py): 2 ranks (gloo,
both on cuda:0) each with half of every global batch vs ONE process on the global
batch, for DeepFM (dense MLP all-reduce + deferred token-table stash gather) and
SASRec with the sampled-softmax loss (two stashed sources), plus the sharded K6
full-sort evaluation of LightGCN (identical metrics). Dense gradients are summed in
a different order across ranks, so weights agree to fp32 tolerance, not bitwise."""
import os
import pathlib

import numpy as np
import pytest
import torch
from conftest import free_port
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CASES = {
    'DeepFM': dict(train_batch_size=256),
    'SASRec': dict(loss_type='SSM', training_neg_sample_num=8, train_batch_size=128),
    'LightGCN': dict(training_neg_sample_num=1, train_batch_size=512),
}


def _pipe(name, root, shard=True):
    kw = dict(CASES[name])
    kw['shard_tables'] = shard
    if name == 'DeepFM':
        from tests.test_gpu_deepfm import _pipeline
    elif name == 'SASRec':
        from tests.test_gpu_sasrec import _pipeline
    else:
        from tests.test_gpu_e2e import _pipeline
        kw['model'] = 'LightGCN'
    return _pipeline(pathlib.Path(root), **kw)


def _grads(model, opt):
    """Dense view of this step's gradients: p.grad, or the deferred stash scattered
    (row-sharded tables: each owner's rows, summed over the ranks)."""
    import torch.distributed as tdist
    from recbole_amd import ops
    out = {}
    for n, p in model.named_parameters():
        if p.grad is not None:
            out[n] = p.grad.detach().cpu().numpy().copy()
        elif p in getattr(opt, '_deferred', {}):
            ds = opt._deferred[p]
            dense = torch.zeros_like(p)
            for rows, keys, tag in ds['stash']:
                if tag == 'owned':             # local row ids of this rank's shard
                    keys = keys * ds['shard']['G'] + ds['shard']['r']
                ops.segment_scatter_add(rows, ops.segment_sort(keys, p.shape[0]), dense)
            if 'shard' in ds:
                tdist.all_reduce(dense, group=ds['shard']['group'])
            out[n] = dense.cpu().numpy()
    return out


def _run(name, root, shard=True):
    """The Trainer's generic loop (trainer.py _train_epoch) with the first step's
    exchanged gradients captured."""
    from recbole_amd.trainer import Trainer
    config, train, valid, test, model = _pipe(name, root, shard)
    tr = Trainer(config, model)
    dp = tr._dp
    model.train()
    total, first = 0.0, None
    for inter in train:
        inter = inter.to(config['device'])
        shard = False
        if dp is not None:
            inter, shard = dp.local_slice(inter)
        tr.optimizer.zero_grad()
        loss = model.calculate_loss(inter)
        total += (dp.global_loss(loss) if shard else loss).item()
        (loss * dp.loss_scale() if shard else loss).backward()
        if shard:
            dp.exchange(model, tr.optimizer)
        if first is None:
            first = _grads(model, tr.optimizer)
        tr.optimizer.step()
    tr.optimizer.flush()
    metrics = tr.evaluate(test, load_best_model=False) if name == 'LightGCN' else None
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    osd = tr.optimizer.state_dict()          # full moments (sharded: gathered)
    sd.update({f'opt.{i}.{k}': st[k].detach().cpu().numpy() for i, st in osd['state'].items()
               for k in ('exp_avg', 'exp_avg_sq')})
    sharded = any('shard' in ds for ds in getattr(tr.optimizer, '_deferred', {}).values())
    return total, first, sd, metrics, (dp is not None, sharded)


def _worker(rank, port, name, root, q, shard=True):
    import torch.distributed as tdist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    tdist.init_process_group('gloo', rank=rank, world_size=2)
    try:
        torch.cuda.set_device(0)
        q.put((rank,) + _run(name, root, shard))
    except Exception as e:                      # report instead of hanging the parent
        q.put((rank, repr(e), None, None, None, None))
        raise
    finally:
        tdist.destroy_process_group()


def _two_ranks(tmp_path, name, shard, tag):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, name, str(tmp_path / f'{tag}{r}'), q,
                                               shard))
             for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=240) for _ in range(2)], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
    return outs


@pytest.mark.parametrize('name', ['DeepFM', 'SASRec', 'LightGCN'])
def test_two_ranks_match_one_process(tmp_path, name):
    ref_loss, ref_g, ref_sd, ref_metrics, (dp, _) = _run(name, str(tmp_path / 'one'))
    assert not dp
    outs = _two_ranks(tmp_path, name, True, 'r')
    for rank, loss, g, sd, metrics, flags in outs:
        assert g is not None, loss
        assert flags[0]
        assert flags[1] == (name != 'LightGCN')     # deferred tables row-sharded
        np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
        # the exchanged gradient of the first global batch = the one-process gradient
        assert g.keys() == ref_g.keys()
        for k in ref_g:
            # (rounding-level gradients, e.g. the key bias under softmax, compare
            # against an absolute floor)
            scale = float(np.abs(ref_g[k]).max())
            np.testing.assert_allclose(g[k], ref_g[k], rtol=1e-4, atol=max(1e-5 * scale, 1e-8),
                                       err_msg=k)
        # after an epoch: the deferred tables' sums match one process's (the reduction's
        # pieces count from each row's own first contribution); what differs is the
        # dense parameters' gradient all-reduce (another summation order than one
        # process's autograd), rounding-level, which the trajectory carries into every
        # table: measured ≤ 1e-5 after the epoch (was 5e-3 with array-position chunks)
        for k in ref_sd:
            np.testing.assert_allclose(sd[k], ref_sd[k], rtol=0, atol=5e-5, err_msg=k)
        if name == 'LightGCN':
            assert metrics == ref_metrics


@pytest.mark.parametrize('name', ['DeepFM', 'SASRec'])
def test_row_sharded_tables_match_replicated(tmp_path, name):
    """Row-sharded deferred tables (owner-only K5, rows fetched from owners, contribution
    rows all-to-all'd to owners in global order) against the replicated layout after
    an epoch, on both ranks: bit for bit. Each row's contributions arrive in the same
    order, and the fixed-order reduction cuts them into pieces counted from the row's
    own first contribution (csrc/segreduce.hip scatter_chunks_kernel), so the owner's
    shorter array gives the same sums as the replicated one."""
    sharded = _two_ranks(tmp_path, name, True, 's')
    replicated = _two_ranks(tmp_path, name, False, 'p')
    for (rs, ls, _, sds, _, fs), (rp, lp, _, sdp, _, fp) in zip(sharded, replicated):
        assert fs == (True, True) and fp == (True, False), (ls, lp)
        assert ls == lp
        assert sds.keys() == sdp.keys()
        for k in sdp:
            np.testing.assert_array_equal(sds[k], sdp[k], err_msg=k)
