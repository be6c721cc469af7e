"""DCN on the GPU: K19 (csrc/cross.hip) in both modes against the float64 restatement
(tests/dcn_spec.py), and the model against its 'library' path run in float64 on the CPU with
the same state. Tolerances are the project's: rtol 1e-4, atol 1e-6; a quantity that misses
atol 1e-6 is held to twice the fp32 torch op sequence's own largest error against float64 on
the same inputs, both figures printed (as tests/test_gpu_xdeepfm.py and test_gpu_ngcf.py do).
The fp32 op sequence itself stays inside 1e-4 / 1e-6 at these inputs except at (5, 1024, 8)
and at B = 300, where its own excess is about 2e-6 to 6e-6."""
import numpy as np
import pytest
import torch

from tests.ctx_data import write_ctx_dataset
from tests.dcn_spec import cross_grads64, cross_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(33, 2, 1), (37, 50, 3), (3, 65, 2), (19, 390, 6), (5, 1024, 8), (2065, 20, 4)]
NAMES = ('y', 'xL', 'S', 'dx0', 'dW', 'dB', 'dwp')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda', 0)


def _fused(dev, inp, head):
    """dict of K19's outputs (fp32 on the device) in head or plain mode."""
    from recbole_amd import ops
    f = lambda t: t.to(dev, torch.float32).contiguous()
    x0, W, Bv = f(inp['x0']), f(inp['W']), f(inp['Bv'])
    if head:
        wp, gy = f(inp['wp']), f(inp['gy'])
        S, y, xL = ops.cross_fwd(x0, W, Bv, wp=wp)
        assert xL is None
        dx0, dW, dB, dwp = ops.cross_bwd(x0, W, Bv, S, wp=wp, gy=gy)
        return {'y': y, 'S': S, 'dx0': dx0, 'dW': dW, 'dB': dB, 'dwp': dwp}
    S, y, xL = ops.cross_fwd(x0, W, Bv)
    assert y is None
    dx0, dW, dB, dwp = ops.cross_bwd(x0, W, Bv, S, gL=f(inp['gL']))
    assert not dwp.any()
    return {'xL': xL, 'S': S, 'dx0': dx0, 'dW': dW, 'dB': dB}


def _library32(dev, inp, head):
    """The same quantities from the fp32 torch op sequence (autograd) on the device."""
    from recbole_amd.model.context_aware_recommender.dcn import cross_library
    f = lambda t: t.to(dev, torch.float32)
    L = inp['W'].shape[0]
    x0 = f(inp['x0']).requires_grad_(True)
    ws = [f(inp['W'][l]).requires_grad_(True) for l in range(L)]
    bs = [f(inp['Bv'][l]).requires_grad_(True) for l in range(L)]
    with torch.no_grad():                    # S: the op sequence's own tensordots
        S = [torch.tensordot(cross_library(x0, ws[:l], bs[:l]), ws[l], dims=([1], [0]))
             for l in range(L)]
    xL = cross_library(x0, ws, bs)
    out = {'S': torch.stack(S, dim=1)}
    if head:
        wp = f(inp['wp']).requires_grad_(True)
        y = torch.tensordot(xL, wp, dims=([1], [0]))
        y.backward(f(inp['gy']))
        out.update(y=y.detach(), dwp=wp.grad)
    else:
        xL.backward(f(inp['gL']))
        out['xL'] = xL.detach()
    out.update(dx0=x0.grad, dW=torch.stack([w.grad for w in ws]),
               dB=torch.stack([b.grad for b in bs]))
    return out


def _want(inp, head):
    if head:
        return cross_grads64(inp['x0'], inp['W'], inp['Bv'], wp=inp['wp'], gy=inp['gy'])
    return cross_grads64(inp['x0'], inp['W'], inp['Bv'], gL=inp['gL'])


def _check(tag, got, want, lib32):
    bad = []
    for name in NAMES:
        if name not in got:
            continue
        a, w = got[name].cpu().double(), want[name]
        assert a.shape == w.shape, (tag, name, a.shape, w.shape)
        err = (a - w).abs()
        excess = (err - 1e-4 * w.abs()).max().item()
        t_err = (lib32[name].cpu().double() - w).abs().max().item()
        atol = 1e-6 if excess <= 1e-6 else max(1e-6, 2 * t_err)
        print(f'{tag} {name}: max |w| {w.abs().max():.3e} max err {err.max():.3e} '
              f'max (err - 1e-4 |w|) {excess:.3e}; torch fp32 max err {t_err:.3e} '
              f'-> atol {atol:.3e}')
        if not excess <= atol:
            bad.append(name)
    assert not bad, (tag, bad)


@pytest.mark.parametrize('head', [True, False])
@pytest.mark.parametrize('B,n,L', SHAPES)
def test_kernels_match_float64(dev, B, n, L, head):
    """n = 2 and L = 1, rows off the 64-lane grid (50, 65), 8-byte aligned rows (390), the
    widest built shape (1024, 8: the four-wave backward), more than one split with a ragged
    last one (2065 rows: 28 splits of 72 and one of 49)."""
    from recbole_amd._native import lib
    inp = cross_inputs(B, n, L)
    _check(f'B={B} n={n} L={L} head={head}', _fused(dev, inp, head), _want(inp, head),
           _library32(dev, inp, head))
    splits = lib().mirec_cross_bwd_splits(B, n, L)
    assert 1 <= splits <= 32
    if B == 2065:
        assert splits == 29
    assert lib().mirec_cross_bwd_stride(n, L) == ((2 * L + 1) * n + 3) // 4 * 4


@pytest.fixture
def capped_grid():
    """K19a / K19b launch 3 workgroups at most for the test, then as before."""
    from recbole_amd import ops
    before = ops.cross_grid_cap(3)
    yield 3
    ops.cross_grid_cap(before)


def _same_bits(one, two):
    assert set(one) == set(two)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@pytest.mark.parametrize('head', [True, False])
def test_waves_walk_many_rows(dev, capped_grid, head):
    """B = 300, n = 100, L = 6: 75 forward row groups and 19 splits on 3 workgroups; the same
    bounds, and the same bits as the uncapped run."""
    from recbole_amd import ops
    assert ops.cross_grid_cap(-1) == 3
    inp = cross_inputs(300, 100, 6)
    got = _fused(dev, inp, head)
    _check(f'B=300 capped head={head}', got, _want(inp, head), _library32(dev, inp, head))
    ops.cross_grid_cap(0)
    _same_bits(got, _fused(dev, inp, head))


@pytest.mark.parametrize('head', [True, False])
def test_two_runs_same_bits(dev, head):
    inp = cross_inputs(300, 100, 6, seed=9)
    _same_bits(_fused(dev, inp, head), _fused(dev, inp, head))


def test_no_layer_outputs_in_memory(dev):
    """B = 2048, n = 390, L = 6, head mode: the fused forward + backward holds dx0, S and at
    most 32 partial rows above its inputs, under 3 B n floats; the library path, probed the
    same way, keeps the six x_l and is over it."""
    from recbole_amd.model.context_aware_recommender.dcn import _CrossHeadFn, cross_library
    B, n, L = 2048, 390, 6
    bound = 3 * B * n * 4
    g = torch.Generator().manual_seed(1)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)
    x0 = u(B, n).requires_grad_(True)
    ws = [(u(n) / n ** 0.5).requires_grad_(True) for _ in range(L)]
    bs = [(u(n) * 0.1).requires_grad_(True) for _ in range(L)]
    wp = (u(n) / n ** 0.5).requires_grad_(True)
    gy = u(B)

    def peak(fn):
        for p in [x0, wp] + ws + bs:
            p.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn().backward(gy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = peak(lambda: _CrossHeadFn.apply(x0, wp, torch.stack(ws), torch.stack(bs)))
    library = peak(lambda: torch.tensordot(cross_library(x0, ws, bs), wp, dims=([1], [0])))
    print(f'peak above the inputs: fused {fused / 2**20:.2f} MiB, library '
          f'{library / 2**20:.2f} MiB, bound {bound / 2**20:.2f} MiB')
    assert fused < bound
    assert library > bound


# ---------------------------------------------------------------------------- whole model
def _pipeline(tmp_path, use_gpu=True, **over):
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.utils import get_model, init_seed
    root = write_ctx_dataset(str(tmp_path), seq=over.pop('seq', True))
    cd = {'model': 'DCN', 'dataset': 'ctx', 'data_path': root, 'embedding_size': 10,
          'mlp_hidden_size': [32, 16], 'cross_layer_num': 3, 'dropout_prob': 0.0,
          'load_col': None, 'epochs': 1, 'train_batch_size': 512, 'state': 'ERROR',
          'use_gpu': use_gpu, 'normalize_all': True,
          'checkpoint_dir': str(tmp_path / 'saved')}
    cd.update(over)
    config = Config(config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    ds = create_dataset(config)
    train, valid, test = data_preparation(config, ds)
    model = get_model('DCN')(config, train).to(config['device'])
    return config, train, model


def _library64(tmp_path, model, **over):
    """The 'library' path on the CPU in float64 with `model`'s state."""
    _, _, ref = _pipeline(tmp_path / 'ref', use_gpu=False, cross_kernel='library', **over)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.double()


def _cpu(b):
    from recbole_amd.data.interaction import Interaction
    return Interaction({k: v.cpu() for k, v in b.interaction.items()})


def _x0(model, b):
    return model.linear_fields(b)[0].view(b.length, -1)


def _compare_step(model, ref, b, dev_b):
    loss = model.calculate_loss(dev_b)
    loss.backward()
    want = ref.calculate_loss(_cpu(b))
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        if name.startswith('first_order_linear'):       # unused: zero gradients or none
            assert p.grad is None or not p.grad.any(), name
            assert refp[name].grad is None, name
            continue
        assert p.grad is not None, name
        torch.testing.assert_close(p.grad.cpu().double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda s, k=name: f'{k}: {s}')


@pytest.mark.parametrize('seq,reg', [(True, 2), (True, 0.0), (False, 2), (False, 0.0)])
def test_loss_grads_predictions_match_library_float64(tmp_path, seq, reg):
    """n = 100 (seq: True) and 90; train-mode BatchNorm over the 512-row batch on both sides,
    then predict in eval mode (the running statistics of that one step)."""
    config, train, model = _pipeline(tmp_path, reg_weight=reg, seq=seq)
    b = next(iter(train))
    dev_b = b.to(config['device'])
    x0 = _x0(model, dev_b)
    assert x0.shape[1] == (100 if seq else 90) and model.cross_fused_applies(x0)
    ref = _library64(tmp_path, model, reg_weight=reg, seq=seq)
    _compare_step(model, ref, b, dev_b)
    model.eval()
    ref.eval()
    with torch.no_grad():
        torch.testing.assert_close(model.predict(dev_b).cpu().double(), ref.predict(_cpu(b)),
                                   rtol=1e-4, atol=1e-6)
        xL = model.cross_network(x0.detach())
        assert xL.shape == x0.shape
        torch.testing.assert_close(xL.cpu().double(),
                                   ref.cross_network(x0.detach().cpu().double()),
                                   rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('d', [10, 16])
def test_train_steps_match_library_float64(tmp_path, d):
    """Five Adam steps through Trainer against torch.optim.Adam on the float64 copy. Deferred:
    nothing at embedding_size 10 (not a width of the deferred kernels), the [V, d] token table
    at 16. first_order_linear, which DCN does not use, stays bit-equal to its initial values.

    One kind of parameter has no trained value to compare: the bias of a Linear that feeds a
    train-mode BatchNorm1d. The batch mean is subtracted right after it, so its exact gradient
    is identically zero and what backward returns is rounding residue (about 1e-9 in fp32,
    1e-18 in float64). Adam divides that residue by its own size: against eps = 1e-8 the fp32
    residue moves the bias by a fraction of lr a step in a direction rounding decides, the
    float64 one by nothing. That holds for any fp32 run, the library path's included, and no
    train-mode output depends on the value (the per-step losses above are compared at rtol
    1e-4). These biases (zero at construction) are held to Adam's bound on five steps,
    5 lr (1 - beta1) / sqrt(1 - beta2), and their step-one gradients to the residue's size;
    every other parameter to the 1e-3 / 2e-5 of the xDeepFM test."""
    from recbole_amd.trainer import Trainer
    config, train, model = _pipeline(tmp_path, embedding_size=d, reg_weight=2)
    ref = _library64(tmp_path, model, embedding_size=d, reg_weight=2)
    opt = torch.optim.Adam(ref.parameters(), lr=config['learning_rate'])
    trainer = Trainer(config, model)
    T = model.token_embedding_table.embedding.weight
    deferred = list(getattr(trainer.optimizer, '_deferred', {}))
    want = [] if d == 10 else [T]
    assert len(deferred) == len(want) and all(a is b for a, b in zip(deferred, want))
    first0 = {k: v.detach().clone() for k, v in model.first_order_linear.named_parameters()}
    assert first0
    mods = list(model.mlp_layers.mlp_layers)
    pre_bn = [f'mlp_layers.mlp_layers.{i}.bias' for i, m in enumerate(mods[:-1])
              if isinstance(m, torch.nn.Linear) and isinstance(mods[i + 1], torch.nn.BatchNorm1d)]
    assert len(pre_bn) == 2
    params = dict(model.named_parameters())
    for step, b in enumerate(list(train)[:5]):
        bd = b.to(config['device'])
        trainer.optimizer.zero_grad()
        loss = model.calculate_loss(bd)
        loss.backward()
        if step == 0:
            for name in pre_bn:
                g = params[name].grad.abs().max().item()
                print(f'{name}: max |grad| {g:.3e} (exact value 0)')
                assert g <= 1e-6, name
        trainer.optimizer.step()
        opt.zero_grad()
        want = ref.calculate_loss(_cpu(b))
        want.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    trainer.optimizer.flush()
    refp = dict(ref.named_parameters())
    adam_bound = 5 * config['learning_rate'] * (1 - 0.9) / (1 - 0.999) ** 0.5
    for name, p in model.named_parameters():
        if name in pre_bn:
            drift = p.detach().abs().max().item()
            print(f'{name}: max |value| {drift:.3e}, float64 copy '
                  f'{refp[name].detach().abs().max().item():.3e}, bound {adam_bound:.3e}')
            assert drift <= adam_bound, name
            continue
        torch.testing.assert_close(p.detach().cpu().double(), refp[name].detach(), rtol=1e-3,
                                   atol=2e-5, msg=lambda s, k=name: f'{k}: {s}')
    for k, v in model.first_order_linear.named_parameters():
        assert torch.equal(v.detach(), first0[k]), k


def test_unbuilt_shape_runs_through_torch(tmp_path):
    """cross_layer_num 9 (L > 8) is not built: the model takes the op sequence."""
    config, train, model = _pipeline(tmp_path, cross_layer_num=9, reg_weight=2)
    b = next(iter(train))
    dev_b = b.to(config['device'])
    assert not model.cross_fused_applies(_x0(model, dev_b))
    ref = _library64(tmp_path, model, cross_layer_num=9, reg_weight=2)
    _compare_step(model, ref, b, dev_b)


def test_ops_refuse_cpu_tensors_and_unbuilt_shapes(dev):
    from recbole_amd import ops
    from recbole_amd._native import NativeError, lib
    z = lambda *s, d='cpu': torch.zeros(*s, device=d)
    assert ops.cross_shape_ok(2, 1) and ops.cross_shape_ok(1024, 8) and ops.cross_shape_ok(390, 6)
    for bad in ((1, 3), (1025, 3), (50, 0), (50, 9)):
        assert not ops.cross_shape_ok(*bad), bad
    with pytest.raises(NativeError):
        ops.cross_fwd(z(4, 8), z(2, 8), z(2, 8))
    with pytest.raises(NativeError):
        ops.cross_bwd(z(4, 8), z(2, 8), z(2, 8), z(4, 2), gL=z(4, 8))
    x = z(4, 8, d=dev)
    with pytest.raises(NativeError, match='not in the built set'):
        ops.cross_fwd(x, z(9, 8, d=dev), z(9, 8, d=dev))
    with pytest.raises(NativeError, match='not in the built set'):
        ops.cross_bwd(x, z(9, 8, d=dev), z(9, 8, d=dev), z(4, 9, d=dev), gL=x)
    xw = z(4, 1025, d=dev)
    with pytest.raises(NativeError, match='not in the built set'):
        ops.cross_fwd(xw, z(2, 1025, d=dev), z(2, 1025, d=dev))
    # the library itself refuses too, with the same words
    S = z(4, 9, d=dev)
    rc = lib().mirec_cross_fwd_f32(x.data_ptr(), 4, 8, x.data_ptr(), x.data_ptr(), 9, None,
                                   S.data_ptr(), None, x.data_ptr(), None)
    assert rc == -1 and b'not in the built set' in lib().mirec_last_error()
    with pytest.raises(ValueError, match='neither gy nor gL'):
        ops.cross_bwd(x, z(2, 8, d=dev), z(2, 8, d=dev), z(4, 2, d=dev))
    with pytest.raises(ValueError):
        ops.cross_bwd(x, z(2, 8, d=dev), z(2, 8, d=dev), z(4, 2, d=dev), wp=z(8, d=dev))
    with pytest.raises(ValueError):
        ops.cross_fwd(x, z(2, 7, d=dev), z(2, 7, d=dev))


def test_run_recbole_dcn(tmp_path):
    from recbole_amd.quick_start import run_recbole
    root = write_ctx_dataset(str(tmp_path))
    res = run_recbole(model='DCN', dataset='ctx', config_dict={
        'data_path': root, 'epochs': 2, 'load_col': None, 'state': 'ERROR',
        'checkpoint_dir': str(tmp_path / 'saved'), 'show_progress': False})
    r = {k.lower(): v for k, v in res['test_result'].items()}
    assert set(r) == {'auc', 'logloss'}
    assert 0.0 <= r['auc'] <= 1.0 and np.isfinite(r['logloss'])
