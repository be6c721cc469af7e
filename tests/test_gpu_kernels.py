"""Parity of every HIP kernel against the oracle (CPU restatement of the
reference) on seeded inputs, through the C-ABI. Bit-exact for integer / index
work; float kernels within the stated tolerance (north_star: 1e-4 fp32)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

# fp32 tolerance for losses / scores / gradients (north_star: "within 1e-4 fp32")
RTOL, ATOL = 1e-4, 1e-6


def _walk_dev(rl, ptr, cols, dev):
    return (torch.as_tensor(np.asarray(rl, np.int32), device=dev),
            torch.as_tensor(np.asarray(ptr, np.int64), device=dev),
            torch.as_tensor(np.asarray(cols if len(cols) else [0], np.int32), device=dev))


def _membership(up, uc, n_users, n_bits, bits):
    """Sampler membership argument: the CSR alone, or the bitmap built from it."""
    from recbole_amd import ops
    if not bits:
        return {}
    return dict(used_bits=ops.used_bitmap(up, uc, n_users, n_bits), n_bits=n_bits)


# ---------------------------------------------------------------- K4 sampler
@pytest.mark.parametrize('bits', [False, True])
def test_sampler_golden_vectors(dev, bits):
    from recbole_amd import ops
    for c in json.load(open(os.path.join(GOLDEN, 'sampler_walk.json'))):
        rl, up, uc = _walk_dev(c['random_list'], c['used_ptr'], c['used_cols'], dev)
        mem = _membership(up, uc, c['n_users'], int(max(c['random_list'])) + 1, bits)
        pr = torch.zeros(1, dtype=torch.int64, device=dev)
        for b in c['batches']:
            keys = torch.as_tensor(b['keys'], dtype=torch.int64, device=dev)
            out = ops.sample_walk(rl, pr, keys, b['num'], up, uc, c['n_users'], True, **mem)
            assert out.cpu().tolist() == b['out']
            assert int(pr.item()) == b['pr']


@pytest.mark.parametrize('bits', [False, True])
@pytest.mark.parametrize('n_items,n_users,K,num', [(1683, 944, 2048, 1), (26745, 3000, 512, 4),
                                                   (50, 20, 3000, 7), (7, 3, 5, 9),
                                                   (300, 100, 5000, 1), (70, 10, 700, 3)])
def test_sampler_random_vs_c_oracle(dev, n_items, n_users, K, num, bits):
    from recbole_amd import ops
    rng = np.random.default_rng(n_items + K)
    deg = np.minimum(rng.integers(0, max(2, n_items // 2), n_users), n_items // 2)
    u = np.repeat(np.arange(n_users), deg)
    i = rng.integers(1, n_items, len(u))
    ptr, cols = cpu_ref.used_csr(n_users, u, i)
    rl = rng.permutation(np.arange(1, n_items))
    drl, dup, duc = _walk_dev(rl, ptr, cols, dev)
    mem = _membership(dup, duc, n_users, n_items, bits)
    pr_d = torch.zeros(1, dtype=torch.int64, device=dev)
    pr = 0
    for b in range(5):
        keys = rng.integers(0, n_users, K)
        if b == 3:
            keys[:] = keys[0]                       # single-key branch
        exp, pr = cpu_ref.c_sample_walk(rl, pr, keys, num, ptr, cols, n_users, True)
        got = ops.sample_walk(drl, pr_d, torch.as_tensor(keys, device=dev), num, dup, duc,
                              n_users, True, **mem)
        assert np.array_equal(got.cpu().numpy(), exp)
        assert int(pr_d.item()) == pr


@pytest.mark.parametrize('bits', [False, True])
@pytest.mark.parametrize('B', [256, 1536])      # 1536 x 4 slots: the wide (multi-CU round 0) path
def test_sampler_multi_batch_launch_equals_sequential(dev, bits, B):
    from recbole_amd import ops
    rng = np.random.default_rng(11)
    n_users, n_items, T, nb = 500, 3000, 4, 7
    u = rng.integers(0, n_users, 40000)
    i = rng.integers(1, n_items, 40000)
    ptr, cols = cpu_ref.used_csr(n_users, u, i)
    rl = rng.permutation(np.arange(1, n_items))
    keys = rng.integers(0, n_users, B * nb - 100)          # last batch ragged
    exp, pr = [], 0
    for b in range(nb):
        kb = keys[b * B:(b + 1) * B]
        o, pr = cpu_ref.c_sample_walk(rl, pr, kb, T, ptr, cols, n_users, True)
        exp.append(o)
    drl, dup, duc = _walk_dev(rl, ptr, cols, dev)
    pr_d = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty(len(keys) * T, dtype=torch.int64, device=dev)
    ops.sample_walk(drl, pr_d, torch.as_tensor(keys, device=dev), T, dup, duc, n_users, True,
                    batch_keys=B, n_batches=nb, out=out,
                    **_membership(dup, duc, n_users, n_items, bits))
    assert np.array_equal(out.cpu().numpy(), np.concatenate(exp))
    assert int(pr_d.item()) == pr


def test_repeatable_sampler_no_rejection(dev):
    from recbole_amd import ops
    rng = np.random.default_rng(5)
    rl = rng.permutation(np.arange(1, 1000))
    keys = rng.integers(0, 50, 333)
    exp, pr = cpu_ref.c_sample_walk(rl, 990, keys, 100, None, None, 50, False)
    drl = torch.as_tensor(rl.astype(np.int32), device=dev)
    pr_d = torch.tensor([990], dtype=torch.int64, device=dev)
    got = ops.sample_walk(drl, pr_d, torch.as_tensor(keys, device=dev), 100, None, None, 50, False)
    assert np.array_equal(got.cpu().numpy(), exp) and int(pr_d.item()) == pr


@pytest.mark.parametrize('bits', [False, True])
@pytest.mark.parametrize('reps', [1, 2500])     # 2 slots (single block) / 5,000 (wide path)
def test_sampler_livelock_reports_status(dev, bits, reps):
    from recbole_amd import ops
    rl = np.array([1, 2, 3, 4])
    ptr, cols = cpu_ref.used_csr(2, np.array([0, 0, 0, 1, 1, 1]), np.array([1, 3, 4, 2, 3, 4]))
    drl, dup, duc = _walk_dev(rl, ptr, cols, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.sample_walk(drl, torch.zeros(1, dtype=torch.int64, device=dev),
                    torch.tensor([0, 1] * reps, device=dev), 1, dup, duc, 2, True, status=status,
                    **_membership(dup, duc, 2, 5, bits))
    assert int(status.item()) == -3


@pytest.mark.parametrize('reps', [1, 2500])
def test_sampler_bad_key_status(dev, reps):
    from recbole_amd import ops
    rl = np.arange(1, 20)
    ptr, cols = cpu_ref.used_csr(3, np.array([0, 1]), np.array([1, 2]))
    drl, dup, duc = _walk_dev(rl, ptr, cols, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.sample_walk(drl, torch.zeros(1, dtype=torch.int64, device=dev),
                    torch.tensor([0, 7] * reps, device=dev), 2, dup, duc, 3, True, status=status)
    assert int(status.item()) == -2


def test_used_bitmap_matches_csr(dev):
    from recbole_amd import ops
    rng = np.random.default_rng(3)
    n_users, n_items = 37, 1000
    u = rng.integers(0, n_users, 5000)
    i = rng.integers(0, n_items, 5000)
    ptr, cols = cpu_ref.used_csr(n_users, u, i)
    _, dup, duc = _walk_dev([1], ptr, cols, dev)
    bits = ops.used_bitmap(dup, duc, n_users, n_items).cpu().numpy().view(np.uint32)
    words = (n_items + 31) // 32
    dense = np.unpackbits(bits.reshape(n_users, words).view(np.uint8), axis=1,
                          bitorder='little')[:, :n_items].astype(bool)
    exp = np.zeros((n_users, n_items), bool)
    exp[u, i] = True
    assert np.array_equal(dense, exp)


def test_sampler_api_mirror(dev):
    """Sampler(phases, datasets) / set_phase / sample_by_user_ids like the reference."""
    from recbole_amd.sampler import Sampler

    class _DS:
        uid_field, iid_field = 'user_id', 'item_id'

        def __init__(self, u, i, nu, ni):
            from recbole_amd.data.interaction import Interaction
            self.inter_feat = Interaction({'user_id': torch.as_tensor(u),
                                           'item_id': torch.as_tensor(i)})
            self.user_num, self.item_num = nu, ni

    rng = np.random.default_rng(9)
    nu, ni = 40, 300
    parts = [(rng.integers(0, nu, n), rng.integers(1, ni, n)) for n in (800, 100, 100)]
    np.random.seed(2020)
    s = Sampler(['train', 'valid', 'test'], [_DS(u, i, nu, ni) for u, i in parts])
    np.random.seed(2020)
    rl = cpu_ref.random_list_uniform(ni)
    assert s.random_list.tolist() == rl.tolist()
    tr = s.set_phase('train')
    ptr, cols = cpu_ref.used_csr(nu, parts[0][0], parts[0][1])
    pr = 0
    for _ in range(3):
        keys = rng.integers(0, nu, 64)
        exp, pr = cpu_ref.c_sample_walk(rl, pr, keys, 2, ptr, cols, nu, True)
        got = tr.sample_by_user_ids(torch.as_tensor(keys), 2)
        assert np.array_equal(got.cpu().numpy(), exp)
    assert tr.random_pr == pr
    assert s.set_phase('test').random_pr == 0          # independent pointer per phase copy
    assert tr.sample_by_user_ids([], 3) is None
    with pytest.raises(ValueError):
        tr.sample_by_user_ids([0, nu], 1)


# ---------------------------------------------------------------- K1 gather / dot
@pytest.mark.parametrize('shape,dtype', [((1000, 64), torch.float32), ((777,), torch.int64),
                                         ((50, 3), torch.float32), ((300, 7), torch.int8)])
def test_gather_rows_exact(dev, shape, dtype):
    from recbole_amd import ops
    g = torch.Generator().manual_seed(0)
    t = (torch.randn(shape, generator=g) * 100).to(dtype)
    idx = torch.randint(0, shape[0], (4097,), generator=g)
    got = ops.gather_rows(t.to(dev), idx.to(dev))
    assert torch.equal(got.cpu(), t[idx])
    got32 = ops.gather_rows(t.to(dev), idx.to(torch.int32).to(dev))
    assert torch.equal(got32.cpu(), t[idx])


@pytest.mark.parametrize('d', [32, 64, 128, 256])
def test_dot_rows(dev, d):
    from recbole_amd import ops
    g = torch.Generator().manual_seed(d)
    EU, EI = torch.randn(300, d, generator=g), torch.randn(500, d, generator=g)
    u, i = torch.randint(0, 300, (1001,), generator=g), torch.randint(0, 500, (1001,), generator=g)
    got = ops.dot_rows(EU.to(dev), EI.to(dev), u.to(dev), i.to(dev)).cpu()
    exp = (EU[u].double() * EI[i].double()).sum(1).float()
    torch.testing.assert_close(got, exp, rtol=RTOL, atol=1e-5)


# ---------------------------------------------------------------- K3 BPR
@pytest.mark.parametrize('d,times,B', [(64, 1, 2048), (128, 4, 512), (32, 3, 100),
                                       (256, 2, 333), (128, 1, 1)])
def test_bpr_fwd_bwd_vs_torch_autograd(dev, d, times, B):
    from recbole_amd import ops
    g = torch.Generator().manual_seed(d * 7 + times)
    nU, nI = 400, 900
    EU = torch.randn(nU, d, generator=g) * 0.1
    EI = torch.randn(nI, d, generator=g) * 0.1
    user = torch.randint(0, nU, (B,), generator=g)
    pos = torch.randint(1, nI, (B,), generator=g)
    neg = torch.randint(1, nI, (B * times,), generator=g)
    # reference: rows r = j*B + k, torch CPU autograd (bpr.py:74-83, loss.py:47-49)
    m = cpu_ref.BPRCPU(nU, nI, d, init=False)
    m.user_embedding.weight.data.copy_(EU)
    m.item_embedding.weight.data.copy_(EI)
    ur, pr_, nr = cpu_ref.pairwise_rows(user, pos, neg, times)
    loss = m.calculate_loss(ur, pr_, nr)
    loss.backward()
    o = ops.bpr_fwd_bwd(EU.to(dev), EI.to(dev), user.to(dev), pos.to(dev), neg.to(dev), times,
                        grads=True, scores=True)
    got_loss = o['loss_k'].sum().item() / (B * times)
    assert got_loss == pytest.approx(loss.item(), rel=RTOL)
    ps = (EU[user] * EI[pos]).sum(1)
    torch.testing.assert_close(o['pos_score'].cpu(), ps, rtol=RTOL, atol=ATOL)
    # group row gradients into dense table gradients with K2 + scatter
    dEU = torch.zeros(nU, d, device=dev)
    dEI = torch.zeros(nI, d, device=dev)
    ops.segment_scatter_add(o['gU'], ops.segment_sort(user.to(dev), nU), dEU)
    ops.segment_scatter_add(o['gI'], ops.segment_sort(torch.cat([pos, neg]).to(dev), nI), dEI)
    torch.testing.assert_close(dEU.cpu(), m.user_embedding.weight.grad, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(dEI.cpu(), m.item_embedding.weight.grad, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('d,times', [(32, 1), (128, 4), (256, 7)])
def test_bpr_coef_exchange_rebuild_bitwise(dev, d, times):
    """Data-parallel K3: per-rank forward (losses + coefficients) on slices of a
    global batch, the coefficient blocks concatenated as the all-gather leaves them,
    and the rebuild of the global batch's gradient rows must equal — bit for bit —
    the fused K3 on the global batch (losses too)."""
    from recbole_amd import ops
    g = torch.Generator().manual_seed(d + times)
    G, B, nU, nI = 4, 37, 50, 90
    EU = (torch.randn(nU, d, generator=g) * 0.1).to(dev)
    EI = (torch.randn(nI, d, generator=g) * 0.1).to(dev)
    users = torch.randint(0, nU, (G * B,), generator=g).to(dev)
    items = torch.randint(0, nI, ((1 + times) * G * B,), generator=g).to(dev)
    gs = 1.0 / (G * B * times)
    ref = ops.bpr_fwd_bwd(EU, EI, users, items[:G * B], items[G * B:], times, grad_scale=gs)
    W = (1 + times) * B
    buf = torch.empty(G, W, device=dev)
    it = items.view(1 + times, G, B)
    for r in range(G):
        lu = users.view(G, B)[r].contiguous()
        li = it[:, r, :].contiguous()
        loss, coef = ops.bpr_fwd_coef(EU, EI, lu, li[0].contiguous(),
                                      li[1:].reshape(-1).contiguous(), times, gs)
        buf[r, :B] = loss
        buf[r, B:] = coef
    gU, gI = ops.bpr_contrib(EU, EI, users, items[:G * B].contiguous(),
                             items[G * B:].contiguous(), times, buf.view(-1)[B:], B, W)
    assert torch.equal(gU, ref['gU']) and torch.equal(gI, ref['gI'])
    assert torch.equal(buf[:, :B].reshape(-1), ref['loss_k'])


def test_bpr_extreme_scores_no_nan(dev):
    from recbole_amd import ops
    d = 64
    EU = torch.full((2, d), 3.0)
    EI = torch.zeros(3, d)
    EI[1] = -3.0          # pos score -576 -> sigmoid underflows; loss = -log(1e-10)
    EI[2] = 3.0
    o = ops.bpr_fwd_bwd(EU.to(dev), EI.to(dev), torch.tensor([0], device=dev),
                        torch.tensor([1], device=dev), torch.tensor([2], device=dev), 1)
    assert o['loss_k'].item() == pytest.approx(-np.log(1e-10), rel=1e-5)
    assert torch.isfinite(o['gU']).all() and torch.isfinite(o['gI']).all()


# ---------------------------------------------------------------- K2 segment sort
@pytest.mark.parametrize('n,key_space', [(0, 10), (1, 1), (100, 7), (2560, 26745),
                                         (8192, 138494), (20000, 5000), (513, 2 ** 22)])
def test_segment_sort_exact(dev, n, key_space):
    from recbole_amd import ops
    rng = np.random.default_rng(n + key_space)
    keys = rng.integers(0, key_space, n).astype(np.int64)
    segs = ops.segment_sort(torch.as_tensor(keys, device=dev), key_space)
    nu = int(segs.n_uniq.item())
    perm = np.argsort(keys, kind='stable')
    uniq, starts = np.unique(keys[perm], return_index=True)
    assert nu == len(uniq)
    assert np.array_equal(segs.perm[:n].cpu().numpy(), perm)
    assert np.array_equal(segs.uniq[:nu].cpu().numpy(), uniq)
    assert np.array_equal(segs.seg[:nu + 1].cpu().numpy(), np.r_[starts, n])


def _check_sort_batched(dev, keys, batch_n, key_space):
    """ops.segment_sort_batched (its own workspace sizing) against numpy's stable argsort
    and np.unique per batch, at the batched layout: perm / uniq at b * batch_n, seg at
    b * (batch_n + 1), n_uniq[b]."""
    from recbole_amd import ops
    n = len(keys)
    nb = -(-n // batch_n)
    perm = torch.full((nb * batch_n,), -1, dtype=torch.int32, device=dev)
    uniq = torch.full((nb * batch_n,), -1, dtype=torch.int32, device=dev)
    seg = torch.full((nb * (batch_n + 1),), -1, dtype=torch.int32, device=dev)
    n_uniq = torch.full((nb,), -1, dtype=torch.int32, device=dev)
    ops.segment_sort_batched(torch.as_tensor(keys, device=dev), batch_n, key_space, perm, uniq,
                             seg, n_uniq)
    perm, uniq, seg, n_uniq = (t.cpu().numpy() for t in (perm, uniq, seg, n_uniq))
    for b in range(nb):
        kb = keys[b * batch_n:(b + 1) * batch_n]
        order = np.argsort(kb, kind='stable')
        u, first = np.unique(kb[order], return_index=True)
        nu = int(n_uniq[b])
        assert nu == len(u), b
        assert np.array_equal(perm[b * batch_n:b * batch_n + len(kb)], order), b
        assert np.array_equal(uniq[b * batch_n:b * batch_n + nu], u), b
        assert np.array_equal(seg[b * (batch_n + 1):b * (batch_n + 1) + nu + 1],
                              np.r_[first, len(kb)]), b


@pytest.mark.parametrize('key_space', [1, 33, 5000])
@pytest.mark.parametrize('n', [8193, 20000])
def test_segment_sort_large_single_batch_without_status(dev, n, key_space):
    """One batch past the LDS path with no status buffer (the sort a graph capture takes
    before one exists): the 5-bit upsweep / scan / downsweep sort. 8,193 keys are 5 tiles
    of 2,048, the last holding one key; 20,000 leave a ragged last tile. Key space 1: no
    pass, the permutation is the index column; 33: two passes, the second with one live
    bit; 5,000: Zipf-hot keys."""
    rng = np.random.default_rng(n + key_space)
    keys = (np.minimum(rng.zipf(1.1, n), key_space) - 1).astype(np.int64)
    _check_sort_batched(dev, keys, n, key_space)


@pytest.mark.parametrize('key_space', [7, 5000])
def test_segment_sort_large_batches_global_kernel(dev, key_space):
    """Several batches of more than 8,192 keys (a sharded chunk's item keys): one
    workgroup per batch over global ping-pong buffers, 1-bit splits. Three batches of
    8,193, the last ragged (100 keys); the first quarter of batch 0 is one key."""
    batch_n = 8193
    n = 2 * batch_n + 100
    rng = np.random.default_rng(n + key_space)
    keys = rng.integers(0, key_space, n).astype(np.int64)
    keys[:batch_n // 4] = key_space - 1
    _check_sort_batched(dev, keys, batch_n, key_space)


# ---------------------------------------------------------------- K5 Adam
@pytest.mark.parametrize('d,wd', [(64, 0.0), (128, 0.0), (32, 0.01)])
def test_adam_compact_vs_torch_dense_adam(dev, d, wd):
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(d)
    n, R = 700, 300
    p0 = torch.randn(n, d, generator=g) * 0.1
    ref = torch.nn.Parameter(p0.clone())
    topt = torch.optim.Adam([ref], lr=1e-3, weight_decay=wd)
    mine = torch.nn.Parameter(p0.clone().to(dev))
    fopt = FusedAdam([mine], lr=1e-3, weight_decay=wd)
    consts, idx = fopt.prepare_window(6, dev)
    for step in range(6):
        keys = torch.randint(0, n, (R,), generator=g)
        rows = torch.randn(R, d, generator=g) * 0.01
        dense = torch.zeros(n, d).index_add_(0, keys, rows)
        ref.grad = dense
        topt.step()
        segs = ops.segment_sort(keys.to(dev), n)
        fopt.step_compact(mine, rows.to(dev), segs, consts, idx)
        idx += 1                                       # step_finish's job in the trainer
    fopt.advance(6)
    torch.testing.assert_close(mine.detach().cpu(), ref.detach(), rtol=RTOL, atol=1e-6)
    st = fopt.state_dict()['state'][0]
    torch.testing.assert_close(st['exp_avg'].cpu(), topt.state[ref]['exp_avg'], rtol=RTOL,
                               atol=1e-8)
    torch.testing.assert_close(st['exp_avg_sq'].cpu(), topt.state[ref]['exp_avg_sq'],
                               rtol=RTOL, atol=1e-10)
    assert float(st['step']) == float(topt.state[ref]['step'])


def test_fused_adam_dense_step_matches_torch(dev):
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(3)
    shapes = [(50, 64), (13, 4), (7,)]          # 2-D table, flat view, odd 1-D (numel%4!=0)
    ps = [torch.randn(s, generator=g) for s in shapes[:2]]
    ref = [torch.nn.Parameter(p.clone()) for p in ps]
    mine = [torch.nn.Parameter(p.clone().to(dev)) for p in ps]
    topt = torch.optim.Adam(ref, lr=1e-2)
    fopt = FusedAdam(mine, lr=1e-2)
    for _ in range(4):
        gr = [torch.randn(p.shape, generator=g) for p in ps]
        for r, m, x in zip(ref, mine, gr):
            r.grad, m.grad = x.clone(), x.clone().to(dev)
        topt.step()
        fopt.step()
    for r, m in zip(ref, mine):
        torch.testing.assert_close(m.detach().cpu(), r.detach(), rtol=RTOL, atol=1e-6)


@pytest.mark.parametrize('d,beta1,wd', [(128, 0.9, 0.0), (32, 0.3, 0.01), (64, 0.9, 0.0),
                                         (16, 0.9, 0.0), (4, 0.9, 0.0)])
@pytest.mark.parametrize('wide', [False, True])    # True: a row bound that selects float2 columns
@pytest.mark.parametrize('marks', [False, True])   # True: zero-state marks (MIREC_ADAM_ZERO_STATE)
def test_adam_deferred_bitwise_equals_streamed(dev, d, beta1, wd, wide, marks):
    """The deferred schedule (touch + replay, flushes at irregular steps) leaves
    p, m, v bit-identical to the streamed dense Adam over every row. With marks,
    half the rows start from a nonzero (m, v) and the rest from +0 marked as a
    zero-gradient fixed point (skipped by look-aheads and flushes until their
    first gradient step). d = 16 / 4: tables over several 1,024-row blocks of the
    narrow flush (adam_flush_list_kernel), the last one partial."""
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(d)
    sizes, R, steps = ((2500, 1031), (300, 200), 37) if d < 32 else ((300, 517), (40, 200), 37)
    init = [torch.randn(n, d, generator=g) * 0.1 for n in sizes]
    # a hot set touched often plus a cold tail touched rarely, as in a Zipf stream
    batches = []
    for s in range(steps):
        ks = []
        for n, r in zip(sizes, R):
            hot = torch.randint(0, n // 10, (r // 2,), generator=g)
            cold = torch.randint(0, n, (r - r // 2,), generator=g)
            ks.append(torch.cat([hot, cold]))
        batches.append([(k, torch.randn(k.numel(), d, generator=g) * 0.05) for k in ks])
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2, betas=(beta1, 0.999),
                    weight_decay=wd)
    consts = torch.from_numpy(opt.step_constants(1, steps).reshape(-1)).to(dev)

    segs = [[ops.segment_sort(k.to(dev), sizes[q]) for q, (k, _) in enumerate(b)]
            for b in batches]
    aheads = []                      # rows batch s+1 reads that batch s does not touch
    for s in range(steps - 1):
        row = []
        for q in range(2):
            a = np.setdiff1d(batches[s + 1][q][0].numpy(), batches[s][q][0].numpy())
            row.append((torch.as_tensor(a.astype(np.int32) if len(a) else np.zeros(1, np.int32),
                                        device=dev),
                        torch.tensor([len(a)], dtype=torch.int32, device=dev)))
        aheads.append(row)
    snaps = []

    m0 = [torch.zeros(n, d) for n in sizes]
    v0 = [torch.zeros(n, d) for n in sizes]
    if marks:                        # rows 0, 2, 4, ... carry optimizer state
        for q, n in enumerate(sizes):
            m0[q][::2] = torch.randn(len(range(0, n, 2)), d, generator=g) * 1e-3
            v0[q][::2] = torch.rand(len(range(0, n, 2)), d, generator=g) * 1e-6

    def run(schedule, flush_at=(), check_ahead=False):
        P = [x.clone().to(dev) for x in init]
        M = [x.clone().to(dev) for x in m0]
        V = [x.clone().to(dev) for x in v0]
        last = [torch.zeros(x.shape[0], dtype=torch.int32, device=dev) for x in P]
        if marks and schedule == 'deferred':
            for q in range(2):
                ops.zero_state_marks(M[q], V[q], last[q], wd)
                if wd == 0:
                    assert int((last[q] == ops.ADAM_ZERO_STATE).sum()) == sizes[q] // 2
        base = torch.zeros(1, dtype=torch.int32, device=dev)
        for s, batch in enumerate(batches):
            specs = []
            for q, (k, rows) in enumerate(batch):
                specs.append(dict(p=P[q], m=M[q], v=V[q], rows=rows.to(dev), segs=segs[s][q],
                                  last=last[q],
                                  ahead=aheads[s][q] if s + 1 < steps else None))
            tabs = ops.adam_tables(specs)
            ops.adam_multi(tabs, d, consts, base, 0, schedule,
                           n_max_uniq=[max(b[0].numel(), 40000 if wide else 0) for b in batch],
                           beta1=beta1, weight_decay=wd)
            base += 1
            if s in flush_at:
                ops.adam_multi(tabs, d, consts, base, 0, 'flush', beta1=beta1, weight_decay=wd)
            if schedule == 'streamed':
                snaps.append([x.cpu() for x in P])
            elif check_ahead and s + 1 < steps:       # next forward reads complete rows
                for q in range(2):
                    k = batches[s + 1][q][0]
                    assert torch.equal(P[q].cpu()[k], snaps[s][q][k]), (s, q)
        if schedule == 'deferred':
            ops.adam_multi(tabs, d, consts, base, 0, 'flush', beta1=beta1, weight_decay=wd)
            assert all(bool(((x == steps) | (x == ops.ADAM_ZERO_STATE)).all()) for x in last)
            if marks and wd == 0:    # some rows were never touched: still marked
                assert any(bool((x == ops.ADAM_ZERO_STATE).any()) for x in last)
        return [t.cpu() for t in P + M + V]

    ref = run('streamed')
    for flush_at, chk in (((), True), ((5, 6, 20), False)):
        got = run('deferred', flush_at, chk)
        for a, b in zip(ref, got):
            assert torch.equal(a, b), (a - b).abs().max()


@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('rows', [(8, 1), (2, 64), (5, 3)])
@pytest.mark.parametrize('target', [24, 25])        # even / odd: parity-buffer publishing
def test_adam_flush_rows_equals_flush(dev, d, rows, target):
    """mirec_adam_flush_rows_f32 (R rows per wave) leaves every buffer bit-identical to
    the one-wave-per-row flush: rows in the zero state, rows current at the target
    (held in p_alt at an odd target), rows lagging by 1..target steps with their state
    in either parity buffer, and table sizes that are not multiples of 4R."""
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(d + target)
    sizes = (1037, 301)
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    consts = torch.from_numpy(opt.step_constants(1, 64).reshape(-1)).to(dev)
    base = torch.full((1,), target, dtype=torch.int32, device=dev)
    state = []
    for n in sizes:
        P = torch.randn(n, d, generator=g) * 0.1
        A = torch.randn(n, d, generator=g) * 0.1
        M = torch.randn(n, d, generator=g) * 1e-3
        V = torch.rand(n, d, generator=g) * 1e-6
        last = torch.randint(0, target + 1, (n,), generator=g, dtype=torch.int32)
        kind = torch.randint(0, 4, (n,), generator=g)
        last[kind == 0] = ops.ADAM_ZERO_STATE           # zero state: identical buffers
        zs = kind == 0
        M[zs] = 0
        V[zs] = 0
        A[zs] = P[zs]
        last[kind == 1] = target                         # current
        state.append((P, A, M, V, last))

    def run(flush_rows):
        bufs = [[x.clone().to(dev) for x in st] for st in state]
        tabs = ops.adam_tables([dict(p=P, p_alt=A, m=M, v=V, last=L) for P, A, M, V, L in bufs])
        ops.adam_multi(tabs, d, consts, base, 0, 'flush', flush_rows=flush_rows)
        return [x.cpu() for b in bufs for x in b]

    ref, got = run(None), run(rows)
    for a, b in zip(ref, got):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()


@pytest.mark.parametrize('d,wide', [(16, False), (16, True), (4, False), (128, False)])
def test_adam_deferred_pair_equals_two_launches(dev, d, wide):
    """mirec_adam_deferred_pair_f32 ([V, d] + [V, 1] tables, one launch) leaves every
    buffer bit-identical to two mirec_adam_deferred_f32 launches: touched rows with
    grouped gradients, look-ahead rows, rows in the zero state and lagging rows."""
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(d + wide)
    n, nk, st = 3001, 900, 9
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    consts = torch.from_numpy(opt.step_constants(1, 64).reshape(-1)).to(dev)
    base = torch.full((1,), st, dtype=torch.int32, device=dev)
    keys = torch.randint(0, n // 3, (nk,), generator=g)
    segs = ops.segment_sort(keys.to(dev), n)
    ah = np.setdiff1d(torch.randint(0, n, (400,), generator=g).numpy(), keys.numpy())
    ahead = (torch.as_tensor(ah.astype(np.int32), device=dev),
             torch.tensor([len(ah)], dtype=torch.int32, device=dev))
    state = []
    for w in (d, 1):
        P = torch.randn(n, w, generator=g) * 0.1
        M = torch.randn(n, w, generator=g) * 1e-3
        V = torch.rand(n, w, generator=g) * 1e-6
        last = torch.randint(0, st + 1, (n,), generator=g, dtype=torch.int32)
        zs = torch.rand(n, generator=g) < 0.3
        last[zs] = ops.ADAM_ZERO_STATE
        M[zs] = 0
        V[zs] = 0
        rows = torch.randn(nk, w, generator=g) * 0.05
        state.append((P, M, V, last, rows))
    nmax = [max(nk, 40000 if wide else 0)] * 2

    def specs(bufs):
        return [dict(p=P, m=M, v=V, last=L, rows=R, segs=segs, ahead=ahead)
                for P, M, V, L, R in bufs]

    def run(paired):
        bufs = [[x.clone().to(dev) for x in s] for s in state]
        sp = specs(bufs)
        if paired:
            ops.adam_multi(ops.adam_tables(sp), d, consts, base, 0, 'deferred_pair',
                           n_max_uniq=nmax)
        else:
            for s, w in zip(sp, (d, 1)):
                ops.adam_multi(ops.adam_tables([s]), w, consts, base, 0, 'deferred',
                               n_max_uniq=nmax[:1])
        return [x.cpu() for b in bufs for x in b[:4]]

    ref, got = run(False), run(True)
    for a, b in zip(ref, got):
        assert torch.equal(a, b), (a.float() - b.float()).abs().max()
    assert bool((ref[3] == st + 1).any()) and bool((ref[7] == st + 1).any())


@pytest.mark.parametrize('target', [7, 40])
def test_adam_flush_width1_equals_columns(dev, target):
    """The d = 1 flush (DeepFM's first-order [V, 1] table) replays each row exactly as
    the d = 4 flush replays each column: a [n, 1] table flushed alone equals column 0
    of the same values repeated over four columns (d = 4 is pinned to the streamed
    Adam above). Rows lag by 0..target steps, sit in the zero state, or are current;
    n spans several 1,024-row blocks with a partial last one."""
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(target)
    n = 3077
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    consts = torch.from_numpy(opt.step_constants(1, 64).reshape(-1)).to(dev)
    base = torch.full((1,), target, dtype=torch.int32, device=dev)
    P = torch.randn(n, 1, generator=g) * 0.1
    M = torch.randn(n, 1, generator=g) * 1e-3
    V = torch.rand(n, 1, generator=g) * 1e-6
    last = torch.randint(0, target + 1, (n,), generator=g, dtype=torch.int32)
    kind = torch.randint(0, 4, (n,), generator=g)
    last[kind == 0] = ops.ADAM_ZERO_STATE
    M[kind == 0] = 0
    V[kind == 0] = 0
    out = {}
    for d in (1, 4):
        bufs = [x.repeat(1, d).contiguous().to(dev) for x in (P, M, V)] + [last.clone().to(dev)]
        tabs = ops.adam_tables([dict(p=bufs[0], m=bufs[1], v=bufs[2], last=bufs[3])])
        ops.adam_multi(tabs, d, consts, base, 0, 'flush')
        out[d] = [x.cpu() for x in bufs]
    for a, b in zip(out[1][:3], out[4][:3]):
        assert torch.equal(a[:, 0], b[:, 0]), (a[:, 0] - b[:, 0]).abs().max()
        assert torch.equal(b, b[:, :1].repeat(1, 4))
    assert torch.equal(out[1][3], out[4][3])
    assert bool(((out[1][3] == target) | (out[1][3] == ops.ADAM_ZERO_STATE)).all())
    lag = (kind != 0) & (last < target)
    assert bool((out[1][0][lag] != P[lag]).any())          # lagging rows did move


@pytest.mark.parametrize('lr', [1e-3, 3e-2])
@pytest.mark.parametrize('wide', [False, True])
def test_adam_deferred_long_idle_rows_bitwise(dev, lr, wide):
    """Rows idle for hundreds of steps (where the deferred replay stops updating p
    once its increments provably round away) end bit-identical to the streamed
    dense Adam that updates them every step."""
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(11)
    d, sizes, steps = 128, (40, 72), 420
    init = [(torch.randn(n, d, generator=g) * s) for n, s in zip(sizes, (0.1, 3e-3))]
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    consts = torch.from_numpy(opt.step_constants(1, steps).reshape(-1)).to(dev)
    hot = 6
    keys = []
    for s in range(steps):
        ks = [torch.arange(n) if s == 0 else torch.randint(0, hot, (5,), generator=g)
              for n in sizes]
        keys.append([(k, torch.randn(k.numel(), d, generator=g) * 1e-2) for k in ks])
    segs = [[ops.segment_sort(k.to(dev), sizes[q]) for q, (k, _) in enumerate(b)] for b in keys]

    def run(schedule):
        P = [x.clone().to(dev) for x in init]
        M = [torch.zeros_like(x) for x in P]
        V = [torch.zeros_like(x) for x in P]
        last = [torch.zeros(x.shape[0], dtype=torch.int32, device=dev) for x in P]
        base = torch.zeros(1, dtype=torch.int32, device=dev)
        for s in range(steps):
            tabs = ops.adam_tables([dict(p=P[q], m=M[q], v=V[q], rows=keys[s][q][1].to(dev),
                                         segs=segs[s][q], last=last[q]) for q in range(2)])
            ops.adam_multi(tabs, d, consts, base, 0, schedule,
                           n_max_uniq=[max(k.numel(), 40000 if wide else 0) for k, _ in keys[s]])
            base += 1
        if schedule == 'deferred':
            ops.adam_multi(tabs, d, consts, base, 0, 'flush')
        return [t.cpu() for t in P + M + V]

    ref, got = run('streamed'), run('deferred')
    for a, b in zip(ref, got):
        assert torch.equal(a, b), (a - b).abs().max()


def test_adam_matches_torch_cpu_rounding(dev):
    """m and v agree with torch CPU's Adam to the bit (same fma pattern); p to
    the ulp the CPU's vector sqrt may differ by."""
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    g = torch.Generator().manual_seed(7)
    n, d = 256, 64
    p0 = torch.randn(n, d, generator=g) * 0.1
    ref = torch.nn.Parameter(p0.clone())
    topt = torch.optim.Adam([ref], lr=1e-3, weight_decay=0.01)
    mine = torch.nn.Parameter(p0.clone().to(dev))
    fopt = FusedAdam([mine], lr=1e-3, weight_decay=0.01)
    consts, idx = fopt.prepare_window(1, dev)
    grad = torch.randn(n, d, generator=g) * 0.01
    ref.grad = grad
    topt.step()
    fopt._ensure_state(mine)
    st = fopt.state[mine]
    ops.adam_step(mine.data, st['exp_avg'], st['exp_avg_sq'], consts, idx,
                  dense_grad=grad.to(dev), weight_decay=0.01)
    assert torch.equal(st['exp_avg'].cpu(), topt.state[ref]['exp_avg'])
    torch.testing.assert_close(st['exp_avg_sq'].cpu(), topt.state[ref]['exp_avg_sq'],
                               rtol=0, atol=0)
    torch.testing.assert_close(mine.detach().cpu(), ref.detach(), rtol=3e-7, atol=1e-9)


@pytest.mark.parametrize('stride,nb', [(2560, 9), (20000, 3)])
def test_uniq_ahead_diff(dev, stride, nb):
    from recbole_amd import ops
    rng = np.random.default_rng(stride)
    uniq = np.zeros(nb * stride, np.int32)
    nu = np.zeros(nb, np.int32)
    sets = []
    for b in range(nb):
        k = np.unique(rng.integers(0, stride, int(rng.integers(0, stride))))
        sets.append(k)
        uniq[b * stride:b * stride + len(k)] = k
        nu[b] = len(k)
    out = torch.full((nb * stride,), -7, dtype=torch.int32, device=dev)
    n_out = torch.full((nb,), -7, dtype=torch.int32, device=dev)
    ops.uniq_ahead_diff(torch.as_tensor(uniq, device=dev), torch.as_tensor(nu, device=dev),
                        stride, nb, out, n_out)
    o, n = out.cpu().numpy(), n_out.cpu().numpy()
    for b in range(nb - 1):
        exp = np.setdiff1d(sets[b + 1], sets[b])
        assert n[b] == len(exp) and np.array_equal(o[b * stride:b * stride + n[b]], exp)
    assert n[nb - 1] == 0


def test_chunk_finish_matches_step_finish(dev):
    from recbole_amd import ops
    g = torch.Generator().manual_seed(1)
    C, B = 5, 300
    loss = (torch.rand(C * 512, generator=g)).to(dev)
    h1 = torch.zeros(8, device=dev)
    h2 = torch.zeros(8, device=dev)
    i1 = torch.full((1,), 2, dtype=torch.int32, device=dev)
    i2 = i1.clone()
    for c in range(C):
        ops.step_finish(loss[c * 512:c * 512 + B].contiguous(), 1200.0, h1, i1)
    ops.chunk_finish(loss, B, 512, C, 1200.0, h2, i2)
    assert torch.equal(h1, h2) and int(i1) == int(i2) == 2 + C


# ---------------------------------------------------------------- K6 full sort
def _fullsort_case(rng, nq, I, d, K, max_hist=30, max_pos=8):
    U = rng.standard_normal((nq, d)).astype(np.float32)
    E = rng.standard_normal((I, d)).astype(np.float32)
    hist, pos = [], []
    for q in range(nq):
        perm = rng.permutation(np.arange(1, I))
        npos = int(rng.integers(1, min(max_pos, I - 2) + 1))
        nh = int(rng.integers(0, min(max_hist, I - 1 - npos) + 1))
        pos.append(sorted(perm[:npos].tolist()))
        hist.append(sorted(perm[npos:npos + nh].tolist()))
    return U, E, hist, pos


def _csr(lists):
    ptr = np.r_[0, np.cumsum([len(x) for x in lists])].astype(np.int64)
    cols = np.concatenate([np.asarray(x, np.int32) for x in lists]) if ptr[-1] else \
        np.zeros(1, np.int32)
    return ptr, cols


def _check_topk(U, E, hist, pos, K, got_ids, got_flags, got_scores):
    """Exact ids unless two scores tie within fp32 rounding (then either order)."""
    scores = torch.as_tensor(U) @ torch.as_tensor(E).T
    exp_flags, exp_ids = cpu_ref.full_sort_pos_idx(scores, hist, pos, K)
    s64 = U.astype(np.float64) @ E.astype(np.float64).T
    for q in range(len(U)):
        for r in range(K):
            if got_ids[q, r] == exp_ids[q, r]:
                assert bool(got_flags[q, r]) == bool(exp_flags[q, r])
                continue
            a, b = got_ids[q, r], exp_ids[q, r]
            assert a >= 0 and abs(s64[q, a] - s64[q, b]) <= 1e-4 * max(1.0, abs(s64[q, b])), \
                (q, r, a, b)
        valid = got_ids[q] >= 0
        np.testing.assert_allclose(got_scores[q][valid], s64[q, got_ids[q][valid]],
                                   rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('nq,I,d,K', [(300, 1682, 64, 10), (129, 2000, 128, 20),
                                      (64, 517, 256, 10), (40, 300, 32, 50), (5, 33, 64, 1)])
def test_fullsort_topk_vs_oracle(dev, nq, I, d, K):
    from recbole_amd import ops
    rng = np.random.default_rng(nq * I + d)
    U, E, hist, pos = _fullsort_case(rng, nq, I, d, K)
    hp, hc = _csr(hist)
    pp, pc = _csr(pos)
    T = lambda x: torch.as_tensor(x, device=dev)
    o = ops.fullsort_topk(T(U), T(E), K, hist_ptr=T(hp), hist_cols=T(hc), pos_ptr=T(pp),
                          pos_cols=T(pc))
    _check_topk(U, E, hist, pos, K, o['ids'].cpu().numpy(), o['pos_flags'].cpu().numpy(),
                o['scores'].cpu().numpy())


@pytest.mark.parametrize('n_split,d,K', [(1, 64, 10), (2, 64, 10), (3, 64, 10), (8, 64, 10),
                                          (8, 32, 20), (3, 256, 50), (8, 256, 20)])
def test_fullsort_item_split_identical(dev, n_split, d, K):
    """K6 with the item range split over workgroups + the per-user merge returns
    the same scores, ids and positive flags as one sweep (history masked, ties),
    for the K = 20 / 50 merges, d = 32 / 256, and users whose history spans several
    split ranges (the split's history cursor starts by a binary search)."""
    from recbole_amd import ops
    g = torch.Generator().manual_seed(n_split * 1000 + d + K)
    nq, I = 300, 1000
    Uq = torch.randn(nq, d, generator=g).to(dev)
    EI = torch.randn(I, d, generator=g).round().to(dev)       # many tied scores
    EI[500:520] = EI[10:30]                                     # exact duplicates
    hp, hc, pp, pc = [0], [], [0], []
    for q in range(nq):
        n_h = 400 if q % 10 == 0 else q % 37                    # some longer than a split span
        h = sorted(set(torch.randint(1, I, (n_h,), generator=g).tolist()))
        hc += h
        hp.append(len(hc))
        p = sorted(set(torch.randint(1, I, (3,), generator=g).tolist()) - set(h))
        pc += p
        pp.append(len(pc))
    T64 = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)
    T32 = lambda a: torch.tensor(a if a else [0], dtype=torch.int32, device=dev)
    args = dict(hist_ptr=T64(hp), hist_cols=T32(hc), pos_ptr=T64(pp), pos_cols=T32(pc))
    ref = ops.fullsort_topk(Uq, EI, K, **args)
    got = ops.fullsort_topk(Uq, EI, K, n_split=n_split, **args)
    for key in ('scores', 'ids', 'pos_flags'):
        assert torch.equal(got[key], ref[key]), key


def test_fullsort_fewer_items_than_k(dev):
    from recbole_amd import ops
    rng = np.random.default_rng(1)
    U = rng.standard_normal((3, 64)).astype(np.float32)
    E = rng.standard_normal((9, 64)).astype(np.float32)
    hist = [[1, 2, 3, 4, 5, 6], [], [2, 4, 6, 8]]
    pos = [[7], [1, 2], [3]]
    hp, hc = _csr(hist)
    pp, pc = _csr(pos)
    T = lambda x: torch.as_tensor(x, device=dev)
    o = ops.fullsort_topk(T(U), T(E), 10, hist_ptr=T(hp), hist_cols=T(hc), pos_ptr=T(pp),
                          pos_cols=T(pc))
    ids = o['ids'].cpu().numpy()
    assert sorted(ids[0][ids[0] >= 0].tolist()) == [7, 8]           # items 1..8 minus history
    assert (ids[0][2:] == -1).all() and np.isneginf(o['scores'].cpu().numpy()[0][2:]).all()
    assert sorted(ids[1][ids[1] >= 0].tolist()) == list(range(1, 9))
    assert o['pos_flags'].cpu().numpy()[0][ids[0] == 7].all()


@pytest.mark.parametrize('nq,I,d', [(130, 1000, 64), (33, 70, 128), (1, 5, 32), (200, 257, 256)])
def test_score_matrix(dev, nq, I, d):
    from recbole_amd import ops
    rng = np.random.default_rng(I)
    U = rng.standard_normal((nq, d)).astype(np.float32)
    E = rng.standard_normal((I, d)).astype(np.float32)
    got = ops.score_matrix(torch.as_tensor(U, device=dev), torch.as_tensor(E, device=dev)).cpu()
    exp = torch.as_tensor(U.astype(np.float64) @ E.astype(np.float64).T).float()
    torch.testing.assert_close(got, exp, rtol=RTOL, atol=1e-4)


@pytest.mark.parametrize('n,key_space,d', [(9000, 50, 16), (206_000, 3_000_001, 128),
                                           (53_248, 33_000_026, 1), (100_000, 7, 64),
                                           (30_000, 1 << 24, 10)])
def test_large_segment_sort_and_hot_row_scatter(dev, n, key_space, d):
    """Onesweep sort of K2 (n > 8,192 through ops.segment_sort) and the chunked scatter: stable
    grouping identical to numpy's stable argsort; dense sums vs index_add with
    Zipf-hot rows (one row owns a large share of the contributions)."""
    from recbole_amd import ops
    rng = np.random.default_rng(n)
    keys = np.minimum(rng.zipf(1.1, n), key_space) - 1
    keys = keys.astype(np.int64)
    segs = ops.segment_sort(torch.as_tensor(keys, device=dev), key_space)
    nu = int(segs.n_uniq.item())
    order = np.argsort(keys, kind='stable')
    u, first = np.unique(keys[order], return_index=True)
    assert nu == len(u)
    assert np.array_equal(segs.perm[:n].cpu().numpy(), order)
    assert np.array_equal(segs.uniq[:nu].cpu().numpy(), u)
    assert np.array_equal(segs.seg[:nu + 1].cpu().numpy(), np.r_[first, n])
    if segs.pos_seg is not None:
        assert np.array_equal(segs.pos_seg[:n].cpu().numpy(), np.repeat(np.arange(nu),
                                                                     np.diff(np.r_[first, n])))
    rows = torch.randn(n, d, generator=torch.Generator().manual_seed(1))
    n_rows = int(keys.max()) + 1
    exp = torch.zeros(n_rows, d, dtype=torch.float64).index_add_(
        0, torch.as_tensor(keys), rows.double())
    got = ops.segment_scatter_add(rows.to(dev), segs, torch.zeros(n_rows, d, device=dev))
    torch.testing.assert_close(got.cpu().double(), exp, rtol=1e-4, atol=2e-3)


@pytest.mark.parametrize('n,key_space,kind', [(8193, 1, 'zero'), (8193, 2, 'bits'),
                                               (2048 * 7, 3_000_001, 'zipf'),
                                               (309_248, 3_000_001, 'zipf'),
                                               (100_001, (1 << 30) + 5, 'uniform'),
                                               (50_000, 300, 'uniform')])
def test_onesweep_sort_exact(dev, n, key_space, kind):
    """The device-wide onesweep sort (8-bit passes, look-back offsets, look-back segment
    scan) equals numpy's stable argsort for every pass count (0-4 digit bits over 1 to
    31-bit key spaces), exact tile multiples and a ragged last tile, Zipf heads; pos_seg
    is each sorted position's segment; its status words are zero after every call."""
    from recbole_amd import ops
    rng = np.random.default_rng(n + key_space)
    if kind == 'zero':
        keys = np.zeros(n, np.int64)
    elif kind == 'zipf':
        keys = (np.minimum(rng.zipf(1.1, n), key_space) - 1).astype(np.int64)
    else:
        keys = rng.integers(0, key_space, n).astype(np.int64)
    kd = torch.as_tensor(keys, device=dev)
    order = np.argsort(keys, kind='stable')
    u, first = np.unique(keys[order], return_index=True)
    for _ in range(2):                                  # the status buffer is reused
        segs = ops.segment_sort(kd, key_space)
        assert segs.pos_seg is not None
        nu = int(segs.n_uniq.item())
        assert nu == len(u)
        assert np.array_equal(segs.perm[:n].cpu().numpy(), order)
        assert np.array_equal(segs.uniq[:nu].cpu().numpy(), u)
        assert np.array_equal(segs.seg[:nu + 1].cpu().numpy(), np.r_[first, n])
        assert np.array_equal(segs.pos_seg[:n].cpu().numpy(),
                              np.repeat(np.arange(nu), np.diff(np.r_[first, n])))
    torch.cuda.synchronize()
    for buf in ops._SORT_STATUS.values():
        assert int(buf.abs().sum().item()) == 0


@pytest.mark.parametrize('d', [1, 4, 16, 64, 100, 128, 256])
def test_segment_reduce_pos_seg_equals_search(dev, d):
    """segment_reduce over the onesweep grouping, which gives pos_seg (window kernels, no
    search) equals the searching chunk kernel bit for bit: Zipf-hot rows of thousands of
    contributions (fixup), one-piece rows, -0.0 terms, d not a multiple of 64."""
    from recbole_amd import ops
    rng = np.random.default_rng(d)
    n = 60_000
    keys = (np.minimum(rng.zipf(1.1, n), 3_000_000) - 1).astype(np.int64)
    kd = torch.as_tensor(keys, device=dev)
    rows = torch.randn(n, d, generator=torch.Generator().manual_seed(d))
    rows[::11] = -0.0
    rows = rows.to(dev)
    sg = ops.segment_sort(kd, 3_000_000)
    assert sg.pos_seg is not None
    plain = ops.Segments(n, dev)
    for f in ('perm', 'uniq', 'seg', 'n_uniq'):
        setattr(plain, f, getattr(sg, f))
    a, _ = ops.segment_reduce(rows, plain)
    b, _ = ops.segment_reduce(rows, sg)
    nu = int(sg.n_uniq.item())
    assert torch.equal(a[:nu].view(torch.int32), b[:nu].view(torch.int32))


def _second_level_sort_reduce(parts, n_rows, dev):
    """The deferred optimizer's second level as a sort of the concatenated keys + a reduce
    (optim.py before segment_merge2): the reference the merges must equal bit for bit."""
    from recbole_amd import ops
    keys, rows = [], []
    for cr, cs in parts:
        idx = torch.arange(cs.n, device=dev)
        keys.append(torch.where(idx < cs.n_uniq.long(), cs.uniq[:cs.n].long(),
                                torch.full_like(idx, n_rows)))
        rows.append(cr[:cs.n])
    keys, rows = torch.cat(keys), torch.cat(rows)
    segs = ops.segment_sort(keys, n_rows + 1)
    last = segs.uniq.gather(0, (segs.n_uniq.long() - 1).clamp(min=0))
    segs.n_uniq.sub_((last == n_rows).to(torch.int32))
    return ops.segment_reduce(rows, segs)


@pytest.mark.parametrize('d,n_parts', [(128, 2), (16, 3), (100, 2), (1, 2)])
def test_segment_merge_equals_sort_reduce(dev, d, n_parts):
    """The second level as merges of the sources' reduced row lists equals sorting the
    concatenated keys and reducing, bit for bit: rows in one, two or all sources, -0.0
    partial sums, sources of different lengths, a source with no rows at all."""
    from recbole_amd import ops
    rng = np.random.default_rng(d * 10 + n_parts)
    n_rows = 3_000_001
    parts = []
    for k in range(n_parts):
        n = [60_000, 9_000, 0][k] if n_parts == 3 else [40_000, 90_000][k]
        if n == 0:
            n = 1
            keys = np.array([5], np.int64)
        else:
            keys = (np.minimum(rng.zipf(1.1 + 0.1 * k, n), n_rows) - 1).astype(np.int64)
        rows = torch.randn(n, d, generator=torch.Generator().manual_seed(k))
        rows[::7] = -0.0
        segs = ops.segment_sort(torch.as_tensor(keys, device=dev), n_rows)
        parts.append(ops.segment_reduce(rows.to(dev), segs))
    ref_rows, ref_segs = _second_level_sort_reduce(parts, n_rows, dev)
    acc = parts[0]
    for k, part in enumerate(parts[1:]):
        acc = ops.segment_merge2(acc, part, a_pre=k > 0)
    rows, segs = acc
    nu = int(ref_segs.n_uniq.item())
    assert int(segs.n_uniq.item()) == nu
    assert torch.equal(segs.uniq[:nu], ref_segs.uniq[:nu])
    assert torch.equal(rows[:nu].view(torch.int32), ref_rows[:nu].view(torch.int32))


@pytest.mark.parametrize('d', [1, 16, 128])
def test_segment_reduce_independent_of_position(dev, d):
    """The chunked fixed-order reduction cuts each row's contributions into pieces
    counted from the row's own first contribution, so a row's sum does not depend on
    where its contributions sit in the sorted array: the same rows behind 0..63 extra
    contributions of smaller keys (a row-sharded owner's shorter or longer array)
    give bit-identical sums, rows of 1..700 contributions included."""
    from recbole_amd import ops
    rng = np.random.default_rng(d)
    lens = np.r_[1, 2, 31, 32, 33, 64, 65, 97, 300, 700, rng.integers(1, 90, 40)]
    keys = np.repeat(np.arange(100, 100 + len(lens)), lens).astype(np.int64)
    rows = torch.randn(len(keys), d, generator=torch.Generator().manual_seed(d))
    ref = None
    for shift in (0, 1, 5, 17, 31, 32, 63):
        k = np.r_[rng.integers(0, 100, shift), keys].astype(np.int64)
        r = torch.cat([torch.randn(shift, d), rows])
        segs = ops.segment_sort(torch.as_tensor(k, device=dev), 100 + len(lens))
        out, osegs = ops.segment_reduce(r.to(dev), segs)
        nu = int(osegs.n_uniq.item())
        uniq = osegs.uniq[:nu].cpu().numpy()
        got = out[:nu].cpu()[uniq >= 100]
        assert got.shape[0] == len(lens)
        if ref is None:
            ref = got
            exp = torch.zeros(len(lens), d, dtype=torch.float64).index_add_(
                0, torch.as_tensor(keys - 100), rows.double())
            torch.testing.assert_close(got.double(), exp, rtol=1e-5, atol=1e-4)
        assert torch.equal(got, ref), shift


def test_adam_fast_math_selftest(dev):
    """The K5 replay's fast sqrt / division (csrc/adam_math.h) equal sqrtf and IEEE
    division bit for bit on this GPU: every 64th float of the fast sqrt range plus
    the floats around each power of two, and 2^26 random division pairs of the fast
    range (tools/check_adam_math.hip runs the exhaustive / 2^34-pair version)."""
    from recbole_amd._native import check, lib
    out = torch.zeros(4, dtype=torch.int64, device=dev)
    check(lib().mirec_selftest_adam_math(64, 1 << 26, 2024, out.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream),
          'mirec_selftest_adam_math')
    sq_bad, sq_n, dv_bad, dv_n = out.cpu().tolist()
    assert sq_n > 2 ** 24 and dv_n > 2 ** 24
    assert sq_bad == 0 and dv_bad == 0, (sq_bad, dv_bad)


@pytest.mark.parametrize('block_n,n_blocks,space', [(2048, 26, 1 << 25), (100, 7, 1000), (8192, 3, 1 << 20), (513, 4, 2100),
                                                   (4096, 5, 1 << 30), (64, 3, 64 * 3)])
@pytest.mark.parametrize('chained', [False, True])
def test_segment_sort_blocks_equals_global(dev, block_n, n_blocks, space, chained):
    """mirec_segment_sort_blocks on keys in blocks of increasing key ranges (DeepFM's
    field-major token keys) gives exactly the device-wide segment_sort's outputs,
    incl. a ragged last block; chained (one launch, block_n <= 4,096): the same, and
    the status words are zero again after each of two calls."""
    from recbole_amd import ops
    g = torch.Generator(device='cpu').manual_seed(block_n)
    edges = torch.linspace(0, space, n_blocks + 1).long()
    parts = []
    n = block_n * n_blocks - block_n // 3
    for b in range(n_blocks):
        m = min(block_n, n - b * block_n)
        lo, hi = int(edges[b]), int(edges[b + 1])
        parts.append(lo + torch.randint(0, max(1, min(hi - lo, 50 + b * 997)), (m,), generator=g))
    keys = torch.cat(parts).to(dev)
    a = ops.segment_sort(keys, space)
    status = torch.zeros(300, dtype=torch.int32, device=dev) if chained else None
    for _ in range(2 if chained else 1):
        b = ops.segment_sort_blocks(keys, block_n, space, status=status)
        if chained:
            assert int(status.abs().sum().item()) == 0
    nu = int(a.n_uniq.item())
    assert int(b.n_uniq.item()) == nu
    assert torch.equal(a.perm[:n], b.perm[:n])
    assert torch.equal(a.uniq[:nu], b.uniq[:nu])
    assert torch.equal(a.seg[:nu + 1], b.seg[:nu + 1])


def test_segment_sort_fields_equals_offset_keys_then_blocks(dev):
    """The fields form of the chained block sort (keys formed from the columns + offsets
    inside the sort launch) gives mirec_offset_keys' keys and the block sort's grouping."""
    from recbole_amd import ops
    from recbole_amd._native import lib, ptr, stream_handle, check
    import ctypes
    rng = np.random.default_rng(3)
    B, F = 2048, 26
    vocab = [10_000_000 // (j + 1) + 3 for j in range(F)]
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).tolist()
    cols = [torch.as_tensor(np.minimum(rng.zipf(1.1, B), vocab[j] - 1).astype(np.int64),
                            device=dev) for j in range(F)]
    space = int(sum(vocab))
    status = torch.zeros(F + 1, dtype=torch.int32, device=dev)
    keys, sf = ops.segment_sort_fields(cols, offs, B, space, status)
    ref_keys = torch.empty(F * B, dtype=torch.int64, device=dev)
    check(lib().mirec_offset_keys((ctypes.c_void_p * F)(*[ptr(c) for c in cols]),
                                  (ctypes.c_int64 * F)(*offs), F, B, ptr(ref_keys),
                                  stream_handle()), 'mirec_offset_keys')
    assert torch.equal(keys, ref_keys)
    sb = ops.segment_sort_blocks(ref_keys, B, space, status=status)
    nu = int(sb.n_uniq.item())
    assert int(sf.n_uniq.item()) == nu
    for f in ('perm', 'uniq'):
        assert torch.equal(getattr(sf, f)[:F * B if f == 'perm' else nu],
                           getattr(sb, f)[:F * B if f == 'perm' else nu])
    assert torch.equal(sf.seg[:nu + 1], sb.seg[:nu + 1])
    assert torch.equal(sf.pos_seg, sb.pos_seg)
    assert int(status.abs().sum().item()) == 0


def test_segment_sort_blocks_spans(dev):
    """Block sort across key spans: a constant block (no digit pass), a two-key block,
    a Zipf-headed block and blocks spanning 20 and 30 bits (3 and 4 digit passes), ragged
    last block — equal to the device-wide sort."""
    from recbole_amd import ops
    g = torch.Generator(device='cpu').manual_seed(7)
    bn, space = 4096, (1 << 31) - 1
    base = [0, 1 << 26, 1 << 27, 1 << 28, 1 << 29, 1 << 30]
    parts = [torch.full((bn,), base[0] + 5, dtype=torch.int64),
             base[1] + 3 * torch.randint(0, 2, (bn,), generator=g),
             base[2] + torch.minimum(torch.distributions.Geometric(0.05).sample((bn,)).long(),
                                     torch.tensor(999)),
             base[3] + torch.randint(0, 1 << 20, (bn,), generator=g),
             base[4] + torch.randint(0, 1 << 29, (bn,), generator=g),
             base[5] + torch.randint(0, (1 << 30) - 1, (bn - 1000,), generator=g)]
    keys = torch.cat(parts).to(dev)
    n = keys.numel()
    a = ops.segment_sort(keys, space)
    nu = int(a.n_uniq.item())
    status = torch.zeros(8, dtype=torch.int32, device=dev)
    for st in (None, status, status):
        b = ops.segment_sort_blocks(keys, bn, space, status=st)
        assert int(b.n_uniq.item()) == nu
        assert torch.equal(a.perm[:n], b.perm[:n])
        assert torch.equal(a.uniq[:nu], b.uniq[:nu])
        assert torch.equal(a.seg[:nu + 1], b.seg[:nu + 1])
    assert int(status.abs().sum().item()) == 0


@pytest.mark.parametrize('d', [4, 16])
def test_segment_reduce2_equals_two_reductions(dev, d):
    """mirec_segment_reduce2_f32 (the [V, d] token rows and the [V, 1] first-order rows
    of DeepFM reduced in one pass) equals two segment_reduce calls bit for bit, incl.
    hot rows cut into many pieces (fixup path) and one-piece rows."""
    from recbole_amd import ops
    g = torch.Generator().manual_seed(d)
    n = 53_248
    keys = torch.cat([torch.zeros(3000, dtype=torch.int64),                 # one very hot row
                      torch.randint(1, 40, (10_000,), generator=g),         # hot rows
                      torch.randint(40, 5_000_000, (n - 13_000,), generator=g)])
    keys = keys[torch.randperm(n, generator=g)].to(dev)
    rows = (torch.randn(n, d, generator=g)).to(dev)
    rows1 = (torch.randn(n, 1, generator=g)).to(dev)
    segs = ops.segment_sort(keys, 5_000_000)
    a, sa = ops.segment_reduce(rows, segs)
    a1, _ = ops.segment_reduce(rows1, segs)
    b, b1, sb = ops.segment_reduce2(rows, rows1, segs)
    nu = int(segs.n_uniq.item())
    assert torch.equal(a[:nu], b[:nu])
    assert torch.equal(a1[:nu], b1[:nu])
    assert torch.equal(sa.perm, sb.perm) and torch.equal(sa.seg, sb.seg)


@pytest.mark.parametrize('d', [4, 16])
def test_segment_reduce2_pos_seg_equals_search(dev, d):
    """C4's grouping: 26 field blocks of 2,048 Zipf ids sorted by the chained block sort,
    which also gives each sorted position's segment (pos_seg). The window reduction that
    reads pos_seg (no search) equals the searching one and two single reductions bit for
    bit — one-piece rows, hot rows of hundreds of pieces (fixup), -0.0 contributions —
    and pos_seg agrees with seg."""
    from recbole_amd import ops
    rng = np.random.default_rng(d)
    B, F = 2048, 26
    vocab = [10_000_000 // (j + 1) + 3 for j in range(F)]
    off = np.concatenate([[0], np.cumsum(vocab)[:-1]])
    keys = np.concatenate([off[j] + np.minimum(rng.zipf(1.1, B), vocab[j] - 1) for j in range(F)])
    kd = torch.as_tensor(keys.astype(np.int64), device=dev)
    n = kd.numel()
    g = torch.Generator().manual_seed(d)
    rows = torch.randn(n, d, generator=g)
    rows[::7] = -0.0
    rows1 = torch.randn(n, 1, generator=g)
    rows1[::5] = -0.0
    rows, rows1 = rows.to(dev), rows1.to(dev)
    status = torch.zeros(F + 1, dtype=torch.int32, device=dev)
    sc = ops.segment_sort_blocks(kd, B, int(sum(vocab)), status=status)
    assert sc.pos_seg is not None
    nu = int(sc.n_uniq.item())
    seg = sc.seg[:nu + 1].cpu().numpy()
    assert np.array_equal(sc.pos_seg.cpu().numpy(), np.repeat(np.arange(nu), np.diff(seg)))
    plain = ops.Segments(n, dev)
    for f in ('perm', 'uniq', 'seg', 'n_uniq'):
        setattr(plain, f, getattr(sc, f))
    a, a1, _ = ops.segment_reduce2(rows, rows1, plain)          # searching kernel
    b, b1, _ = ops.segment_reduce2(rows, rows1, sc)             # pos_seg window kernel
    c, _ = ops.segment_reduce(rows, plain)
    c1, _ = ops.segment_reduce(rows1, plain)
    for x, y in ((a, b), (a1, b1), (a, c), (a1, c1)):
        assert torch.equal(x[:nu].view(torch.int32), y[:nu].view(torch.int32))
    exp = torch.zeros(nu, d, dtype=torch.float64).index_add_(
        0, sc.pos_seg.cpu().long(), rows.cpu().double()[sc.perm[:n].cpu().long()])
    torch.testing.assert_close(b[:nu].cpu().double(), exp, rtol=1e-5, atol=1e-4)
