"""xDeepFM on the GPU: K18 (csrc/cin.hip) against the float64 restatement
(tests/xdeepfm_spec.py), K8's first-order form, and the model against its 'library' path run
in float64 on the CPU with the same state. Tolerances are the project's: rtol 1e-4, atol 1e-6
for values and data gradients; a weight gradient (a sum over all B D rows) that misses atol
1e-6 is held to twice the fp32 torch op sequence's own largest error against float64 on the
same inputs, both figures printed (as tests/test_gpu_ngcf.py does)."""
import numpy as np
import pytest
import torch

from tests.ctx_data import write_ctx_dataset
from tests.xdeepfm_spec import cin_grads64

pytestmark = pytest.mark.gpu

SHAPES = [(37, 5, 10, [20, 12, 18], False), (37, 5, 16, [20, 12, 18], True),
          (33, 2, 1, [2], True), (19, 7, 64, [34, 6], False)]


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda', 0)


def _inputs(B, m, D, sizes, direct, seed=7):
    """float64 CPU operands: X0 and the upstream gradient uniform in [-1, 1], weights and
    biases uniform within +-1/sqrt(K) (Conv1d's own bound)."""
    from recbole_amd.model.context_aware_recommender.xdeepfm import cin_plan
    plan, final_len = cin_plan(m, sizes, direct)
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    X0 = u(B, m, D)
    Ws = [u(N, H * m) / (H * m) ** 0.5 for H, N, _, _, _ in plan]
    bs = [u(N) / (H * m) ** 0.5 for H, N, _, _, _ in plan]
    return plan, final_len, X0, Ws, bs, u(B, final_len)


def _fused(dev, plan, final_len, X0, Ws, bs, gp):
    """pooled, the hidden X_k, dX0, dW_k, db_k through K18 (fp32 on the device)."""
    from recbole_amd import ops
    from recbole_amd.model.context_aware_recommender.xdeepfm import _CINFn
    f = lambda t: t.to(dev, torch.float32).contiguous()
    x = f(X0).requires_grad_(True)
    params = []
    for W, b in zip(Ws, bs):
        params += [f(W).unsqueeze(2).requires_grad_(True), f(b).requires_grad_(True)]
    pooled = _CINFn.apply(plan, final_len, x, *params)
    pooled.backward(f(gp))
    # the hidden layers, as the forward hands them on
    scratch = torch.empty_like(pooled)
    hidden, Xk = [], x.detach()
    for (H, N, n_hid, dir0, off), W, b in zip(plan[:-1], params[0::2], params[1::2]):
        Xk = ops.cin_layer_fwd(x.detach(), Xk, W.detach()[:, :, 0].contiguous(), b.detach(),
                               n_hid, dir0, scratch, off)
        hidden.append(Xk)
    return (pooled.detach(), hidden, x.grad, [w.grad[:, :, 0] for w in params[0::2]],
            [b.grad for b in params[1::2]])


def _library32(dev, plan, X0, Ws, bs, gp):
    """The fp32 torch op sequence's weight gradients on the device."""
    from recbole_amd.model.context_aware_recommender.xdeepfm import cin_library
    f = lambda t: t.to(dev, torch.float32)
    x = f(X0)
    W = [f(w).unsqueeze(2).requires_grad_(True) for w in Ws]
    b = [f(v).requires_grad_(True) for v in bs]
    cin_library(x, W, b, plan).backward(f(gp))
    return [w.grad[:, :, 0] for w in W], [v.grad for v in b]


def _check(tag, got, want, lib32=None, vals32=None):
    """vals32 (the wide shapes only, where every output is a sum of thousands of terms): fp32
    torch values (pooled, hidden, dX0) on the same inputs; a value that misses atol 1e-6 is
    then held to twice their own largest error against float64, as the weight gradients
    are."""
    pooled, hidden, dX0, dWs, dbs = got
    wp, wh, wx, wW, wb = want

    def close(a, b, n, t=None):
        a = a.cpu().double()
        if t is None:
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6,
                                       msg=lambda s: f'{tag} {n}: {s}')
            return
        excess = ((a - b).abs() - 1e-4 * b.abs()).max().item()
        t_err = (t.cpu().double() - b).abs().max().item()
        atol = 1e-6 if excess <= 1e-6 else max(1e-6, 2 * t_err)
        print(f'{tag} {n}: max err {(a - b).abs().max():.3e} max (err - 1e-4 |w|) {excess:.3e}; '
              f'torch fp32 max err {t_err:.3e} -> atol {atol:.3e}')
        assert excess <= atol, (tag, n)

    v = vals32 or (None, [None] * len(wh), None)
    close(pooled, wp, 'pooled', v[0])
    assert len(hidden) == len(wh)
    for k, (a, b) in enumerate(zip(hidden, wh)):
        close(a, b, f'X_{k + 1}', v[1][k])
    close(dX0, wx, 'dX0', v[2])
    bad = []
    for k in range(len(wW)):
        for name, g, w, t in (('dW', dWs[k], wW[k], lib32 and lib32[0][k]),
                              ('db', dbs[k], wb[k], lib32 and lib32[1][k])):
            g = g.cpu().double()
            err = (g - w).abs()
            excess = (err - 1e-4 * w.abs()).max().item()
            line = (f'{tag} {name}_{k}: max |w| {w.abs().max():.3e} max err {err.max():.3e} '
                    f'max (err - 1e-4 |w|) {excess:.3e}')
            atol = 1e-6
            if t is not None:
                t_err = (t.cpu().double() - w).abs().max().item()
                line += f'; torch fp32 max err {t_err:.3e}'
                if excess > atol:
                    atol = max(atol, 2 * t_err)
                    line += f' -> atol {atol:.3e}'
            print(line)
            if excess > atol:
                bad.append(f'{name}_{k}')
    assert not bad, (tag, bad)


@pytest.mark.parametrize('B,m,D,sizes,direct', SHAPES)
def test_kernels_match_float64(dev, B, m, D, sizes, direct):
    """Slabs straddling samples (D = 10), a ragged last slab, N and K off the 16 / 4 grid, an
    odd N / 2 (34 -> 17), more than one column tile, D = 1 and D = 64."""
    plan, final_len, X0, Ws, bs, gp = _inputs(B, m, D, sizes, direct)
    want = cin_grads64(X0, Ws, bs, direct, gp)
    got = _fused(dev, plan, final_len, X0, Ws, bs, gp)
    _check(f'B={B} m={m} D={D} {sizes} direct={direct}', got, want,
           _library32(dev, plan, X0, Ws, bs, gp))


@pytest.mark.parametrize('B,m,D,sizes,direct', [(5, 64, 3, [256, 130], True),
                                                (9, 20, 4, [40, 24], False)])
def test_wide_forms_match_float64(dev, B, m, D, sizes, direct):
    """The widest built shapes at a small B: m = 64 (four 16-wide tiles of j), N = 256 and
    H = 256 (K = 16,384; 16 and 12 column tiles, the backward forms that spill), and a middle
    one (two tiles of j, N = 40 on four column tiles). Every output here is an fp32 sum of
    4,096 to 16,384 products; an fp32 sum of K terms of size t carries about sqrt(K) 6e-8 t
    of rounding (1e-6 at K = 4,096, partial sums near 0.3), so where the plain atol is missed
    the bound is twice what the same formulas give in fp32 torch ops on the same inputs."""
    plan, final_len, X0, Ws, bs, gp = _inputs(B, m, D, sizes, direct, seed=11)
    want = cin_grads64(X0, Ws, bs, direct, gp)
    got = _fused(dev, plan, final_len, X0, Ws, bs, gp)
    # the same formulas in fp32 torch ops on the device: the yardstick for sums this long
    f = lambda t: t.to(dev, torch.float32)
    t32 = cin_grads64(f(X0), [f(w) for w in Ws], [f(b) for b in bs], direct, f(gp))
    _check(f'B={B} m={m} D={D} {sizes} direct={direct}', got, want,
           _library32(dev, plan, X0, Ws, bs, gp), vals32=t32[:3])


@pytest.fixture
def capped_grid():
    """K18a / K18b launch 3 workgroups at most for the test, then as before."""
    from recbole_amd import ops
    before = ops.cin_grid_cap(3)
    yield 3
    ops.cin_grid_cap(before)


def test_waves_walk_many_slabs(dev, capped_grid):
    """B = 300, D = 10: 50 forward chunks of 6 samples and 47 backward passes of 64 rows on 3
    workgroups; the same bounds, and the same bits as the uncapped run."""
    from recbole_amd import ops
    assert ops.cin_grid_cap(-1) == 3
    plan, final_len, X0, Ws, bs, gp = _inputs(300, 5, 10, [20, 12], False)
    want = cin_grads64(X0, Ws, bs, False, gp)
    got = _fused(dev, plan, final_len, X0, Ws, bs, gp)
    _check('B=300 capped', got, want, _library32(dev, plan, X0, Ws, bs, gp))
    ops.cin_grid_cap(0)
    free = _fused(dev, plan, final_len, X0, Ws, bs, gp)
    for a, b in zip(got, free):
        for x, y in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
            assert torch.equal(x, y)


def test_two_runs_same_bits(dev):
    plan, final_len, X0, Ws, bs, gp = _inputs(300, 5, 10, [20, 12, 18], False, seed=9)
    one = _fused(dev, plan, final_len, X0, Ws, bs, gp)
    two = _fused(dev, plan, final_len, X0, Ws, bs, gp)
    for a, b in zip(one, two):
        for x, y in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
            assert torch.equal(x, y)


def test_no_outer_product_in_memory(dev):
    """B = 2048, m = 20, D = 16, [64, 64], direct False: the fused forward + backward never
    holds B m m D floats (52 MB, the smaller layer's z) above its inputs; the library path,
    probed the same way, does."""
    from recbole_amd.model.context_aware_recommender.xdeepfm import _CINFn, cin_library, cin_plan
    B, m, D, sizes = 2048, 20, 16, [64, 64]
    bound = B * m * m * D * 4
    plan, final_len = cin_plan(m, sizes, False)
    g = torch.Generator().manual_seed(1)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)
    X0 = u(B, m, D).requires_grad_(True)
    params = []
    for H, N, _, _, _ in plan:
        params += [(u(N, H * m, 1) / (H * m) ** 0.5).requires_grad_(True),
                   (u(N) / (H * m) ** 0.5).requires_grad_(True)]
    gp = u(B, final_len)

    def peak(fn):
        for p in [X0] + params:
            p.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn().backward(gp)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = peak(lambda: _CINFn.apply(plan, final_len, X0, *params))
    library = peak(lambda: cin_library(X0, params[0::2], params[1::2], plan))
    print(f'peak above the inputs: fused {fused / 2**20:.1f} MiB, library '
          f'{library / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB')
    assert fused < bound
    assert library > bound


# ---------------------------------------------------------------------------- K8, first order
def _pipeline(tmp_path, use_gpu=True, **over):
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.utils import get_model, init_seed
    root = write_ctx_dataset(str(tmp_path), seq=over.pop('seq', True))
    cd = {'model': 'xDeepFM', 'dataset': 'ctx', 'data_path': root, 'embedding_size': 10,
          'cin_layer_size': [20, 12, 18], 'dropout_prob': 0.0, 'load_col': None, 'epochs': 1,
          'train_batch_size': 512, 'state': 'ERROR', 'use_gpu': use_gpu,
          # float fields scaled to [0, 1]: with raw values up to 20 the CIN's fourth-order
          # products give logits near 200, where a float32 sigmoid is exactly 0 or 1 (and
          # BCELoss clamps its log at -100) while the float64 one is not
          'normalize_all': True,
          'checkpoint_dir': str(tmp_path / 'saved')}
    cd.update(over)
    config = Config(config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    ds = create_dataset(config)
    train, valid, test = data_preparation(config, ds)
    model = get_model('xDeepFM')(config, train).to(config['device'])
    return config, train, model


def _library64(tmp_path, model, **over):
    """The 'library' path on the CPU in float64 with `model`'s state."""
    _, _, ref = _pipeline(tmp_path / 'ref', use_gpu=False, cin_kernel='library', **over)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.double()


def _cpu(b):
    from recbole_amd.data.interaction import Interaction
    return Interaction({k: v.cpu() for k, v in b.interaction.items()})


@pytest.mark.parametrize('seq', [True, False])
def test_first_order_fields(tmp_path, seq):
    """linear_fields: concat bit-identical to fm_fields', y_first_order against a float64 sum,
    the table gradients against torch (the CPU float64 field ops) for an upstream gradient
    on both outputs."""
    config, train, model = _pipeline(tmp_path, seq=seq)
    ref = _library64(tmp_path, model, seq=seq)
    b = next(iter(train)).to(config['device'])
    concat_fm, _ = model.fm_fields(b)
    concat, y1 = model.linear_fields(b)
    assert torch.equal(concat, concat_fm)
    want_c, want_y = ref.linear_fields_torch(_cpu(b))
    torch.testing.assert_close(y1.cpu().double(), want_y, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(concat.cpu().double(), want_c, rtol=1e-4, atol=1e-6)
    g = torch.Generator().manual_seed(2)
    gc = torch.rand(concat.shape, generator=g) * 2 - 1
    gy = torch.rand(y1.shape, generator=g) * 2 - 1
    torch.autograd.backward([concat, y1], [gc.to(concat.device), gy.to(concat.device)])
    torch.autograd.backward([want_c, want_y], [gc.double(), gy.double()])
    refp = dict(ref.named_parameters())
    n = 0
    for name, p in model.named_parameters():
        if 'embedding_table' in name or name == 'first_order_linear.bias':
            torch.testing.assert_close(p.grad.cpu().double(), refp[name].grad, rtol=1e-4,
                                       atol=1e-6, msg=lambda s, k=name: f'{k}: {s}')
            n += 1
    assert n == (7 if seq else 5)


# ---------------------------------------------------------------------------- whole model
@pytest.mark.parametrize('reg', [5e-4, 0.0])
def test_loss_grads_predictions_match_library_float64(tmp_path, reg):
    config, train, model = _pipeline(tmp_path, reg_weight=reg)
    b = next(iter(train)).to(config['device'])
    assert model.cin_fused_applies(model.linear_fields(b)[0])
    ref = _library64(tmp_path, model, reg_weight=reg)
    loss = model.calculate_loss(b)
    loss.backward()
    want = ref.calculate_loss(_cpu(b))
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        torch.testing.assert_close(p.grad.cpu().double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda s, k=name: f'{k}: {s}')
    model.eval()
    ref.eval()
    with torch.no_grad():
        torch.testing.assert_close(model.predict(b).cpu().double(), ref.predict(_cpu(b)),
                                   rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('d,reg', [(10, 5e-4), (10, 0.0), (16, 5e-4), (16, 0.0)])
def test_train_steps_match_library_float64(tmp_path, d, reg):
    """Five Adam steps through Trainer against torch.optim.Adam on the float64 copy. Which
    tables ran deferred: none at embedding_size 10 (not a width of the deferred kernels); at
    16 the [V, d] token table, and the [V, 1] first-order one only without a regularisation
    term (whose norm gives it a dense gradient)."""
    from recbole_amd.trainer import Trainer
    config, train, model = _pipeline(tmp_path, reg_weight=reg, embedding_size=d)
    ref = _library64(tmp_path, model, reg_weight=reg, embedding_size=d)
    opt = torch.optim.Adam(ref.parameters(), lr=config['learning_rate'])
    trainer = Trainer(config, model)
    T = model.token_embedding_table.embedding.weight
    T1 = model.first_order_linear.token_embedding_table.embedding.weight
    deferred = list(getattr(trainer.optimizer, '_deferred', {}))
    want = [] if d == 10 else ([T] if reg else [T, T1])
    assert len(deferred) == len(want) and all(a is b for a, b in zip(deferred, want))
    for b in list(train)[:5]:
        bd = b.to(config['device'])
        trainer.optimizer.zero_grad()
        loss = model.calculate_loss(bd)
        loss.backward()
        trainer.optimizer.step()
        opt.zero_grad()
        want = ref.calculate_loss(_cpu(b))
        want.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    trainer.optimizer.flush()
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.detach().cpu().double(), refp[name].detach(), rtol=1e-3,
                                   atol=2e-5, msg=lambda s, k=name: f'{k}: {s}')


def test_unbuilt_shape_runs_through_torch(tmp_path):
    """cin_layer_size [300] (N > 256) is not built: the model takes the op sequence."""
    config, train, model = _pipeline(tmp_path, cin_layer_size=[300])
    b = next(iter(train)).to(config['device'])
    assert not model.cin_fused_applies(model.linear_fields(b)[0])
    ref = _library64(tmp_path, model, cin_layer_size=[300])
    loss = model.calculate_loss(b)
    loss.backward()
    want = ref.calculate_loss(_cpu(b))
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    torch.testing.assert_close(model.conv1d_list[0].weight.grad.cpu().double(),
                               ref.conv1d_list[0].weight.grad, rtol=1e-4, atol=1e-6)


def test_ops_refuse_cpu_tensors_and_unbuilt_shapes(dev):
    from recbole_amd import ops
    from recbole_amd._native import NativeError
    z = lambda *s, d='cpu': torch.zeros(*s, device=d)
    assert ops.cin_shape_ok(39, 50, 16, 100) and ops.cin_shape_ok(2, 1, 1, 2)
    assert ops.cin_shape_ok(64, 256, 64, 256)
    for bad in ((1, 4, 8, 8), (65, 4, 8, 8), (4, 257, 8, 8), (4, 4, 65, 8), (4, 4, 8, 258),
                (4, 4, 8, 1), (4, 4, 0, 8)):
        assert not ops.cin_shape_ok(*bad), bad
    with pytest.raises(NativeError):
        ops.cin_layer_fwd(z(4, 3, 8), z(4, 3, 8), z(6, 9), z(6), 3, 3, z(4, 3), 0)
    with pytest.raises(NativeError):
        ops.cin_layer_bwd(z(4, 3, 8), z(4, 3, 8), z(6, 9), 3, 3, None, z(4, 3), 0, z(4, 3, 8),
                          False, True)
    with pytest.raises(NativeError):
        ops.cin_wgrad(z(4, 3, 8), z(4, 3, 8), 6, 3, 3, None, z(4, 3), 0)
    x = z(4, 3, 8, d=dev)
    with pytest.raises(NativeError, match='not in the built set'):
        ops.cin_layer_fwd(x, x, z(300, 9, d=dev), z(300, d=dev), 0, 0, z(4, 300, d=dev), 0)
    with pytest.raises(NativeError, match='not in the built set'):
        ops.cin_wgrad(x, x, 300, 0, 0, None, z(4, 300, d=dev), 0)
    xw = z(4, 3, 65, d=dev)
    with pytest.raises(NativeError, match='not in the built set'):
        ops.cin_layer_bwd(xw, xw, z(6, 9, d=dev), 0, 0, None, z(4, 6, d=dev), 0,
                          torch.empty_like(xw), False, True)


def test_run_recbole_xdeepfm(tmp_path):
    from recbole_amd.quick_start import run_recbole
    root = write_ctx_dataset(str(tmp_path))
    res = run_recbole(model='xDeepFM', dataset='ctx', config_dict={
        'data_path': root, 'epochs': 2, 'load_col': None, 'state': 'ERROR',
        'checkpoint_dir': str(tmp_path / 'saved'), 'show_progress': False})
    r = {k.lower(): v for k, v in res['test_result'].items()}
    assert set(r) == {'auc', 'logloss'}
    assert 0.0 <= r['auc'] <= 1.0 and np.isfinite(r['logloss'])
