"""AFM on the GPU: K20 (csrc/afm.hip) against the float64 restatement (tests/afm_spec.py),
and the model against its 'library' path run in float64 on the CPU with the same state.
Tolerances are the project's: rtol 1e-4, atol 1e-6; a quantity that misses atol 1e-6 is held
to twice the fp32 torch op sequence's own largest error against float64 on the same inputs,
both figures printed (as tests/test_gpu_dcn.py does)."""
import functools

import numpy as np
import pytest
import torch

from tests import drop_spec
from tests.afm_spec import afm_grads64, afm_inputs
from tests.ctx_data import write_ctx_dataset

pytestmark = pytest.mark.gpu

SHAPES = [(5, 2, 4, 4), (33, 3, 10, 25), (7, 39, 16, 25), (1, 64, 64, 64), (130, 17, 10, 25),
          (2065, 4, 8, 16), (9, 20, 20, 40), (3, 64, 32, 16)]
NAMES = ('y', 'v', 'dX', 'dW', 'dh', 'dpv')


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _case(B, F, d, A, seed=0):
    """(inputs, float64 results) of a shape, computed once and shared."""
    inp = afm_inputs(B, F, d, A, seed)
    assert inp['seed'] - seed < 64
    want = dict(zip(NAMES, afm_grads64(inp['X'], inp['W'], inp['h'], inp['pv'], inp['gy'])))
    return inp, want


def _fused(dev, inp, p=0.0, rng=None):
    """dict of K20's outputs (fp32 on the device)."""
    from recbole_amd import ops
    f = lambda t: t.to(dev, torch.float32).contiguous()
    X, W, h, pv, gy = (f(inp[k]) for k in ('X', 'W', 'h', 'pv', 'gy'))
    drawn = torch.full((1,), -1, dtype=torch.int64, device=dev) if p else None
    y, V, ML = ops.afm_fwd(X, W, h, pv, p=p, rng=rng, drawn=drawn)
    assert V.shape == (X.shape[0], X.shape[2]) and ML.shape == (X.shape[0], 2)
    dX, dW, dh, dpv = ops.afm_bwd(X, W, h, pv, V, ML, gy, p=p, rng=rng, drawn=drawn)
    out = {'y': y, 'v': V, 'dX': dX, 'dW': dW, 'dh': dh, 'dpv': dpv}
    if p:
        out['drawn'] = drawn
    return out


def _library32(dev, inp, keep=None):
    """The same quantities from the fp32 torch op sequence (autograd) on the device."""
    from recbole_amd.model.context_aware_recommender.afm import afm_library
    from recbole_amd.model.layers import AttLayer
    f = lambda t: t.to(dev, torch.float32)
    A, d = inp['W'].shape
    att = AttLayer(d, A).to(dev)
    with torch.no_grad():
        att.w.weight.copy_(f(inp['W']))
        att.h.copy_(f(inp['h']))
    X = f(inp['X']).requires_grad_(True)
    pv = f(inp['pv']).requires_grad_(True)
    seen = []

    def drop(t):
        seen.append(t.detach())
        return t if keep is None else t * f(keep)
    y = afm_library(X, att, pv, drop)[:, 0]
    y.backward(f(inp['gy']))
    return {'y': y.detach(), 'v': seen[0], 'dX': X.grad, 'dW': att.w.weight.grad,
            'dh': att.h.grad, 'dpv': pv.grad}


def _check(tag, got, want, lib32):
    bad = []
    for name in NAMES:
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


@pytest.mark.parametrize('B,F,d,A', SHAPES)
def test_kernels_match_float64(dev, B, F, d, A):
    """One pair with alpha = 1 and the smallest of every dimension; d and A off every tile
    edge with 3 pairs; the Criteo field shape (66 slabs, the last of most fields ragged); the
    widest built shape (2,016 pairs, the largest LDS and register form); many samples per
    workgroup walk; 32 splits of 65 rows with a ragged last one of 50. K20b runs 16 waves a
    workgroup at all of those but the widest (4 waves); the last two take its 8-wave form, by
    registers (d and A in 2 x 3 tiles) and by LDS (16 copies of a 64 x 32 dX do not fit)."""
    from recbole_amd._native import lib
    inp, want = _case(B, F, d, A)
    _check(f'B={B} F={F} d={d} A={A}', _fused(dev, inp), want, _library32(dev, inp))
    splits = lib().mirec_afm_bwd_splits(B, F, d, A)
    rows = -(-B // 32)
    assert splits == -(-B // rows) and 1 <= splits <= 32
    if B == 2065:
        assert rows == 65 and splits == 32
    assert lib().mirec_afm_bwd_stride(d, A) == (A * d + A + d + 3) // 4 * 4


def test_one_pair_has_no_attention_gradient(dev):
    """F = 2: alpha = 1 whatever W and h are, so dW and dh are zero up to the rounding of
    t - c (two fp32 dots of the same numbers in different orders)."""
    inp, want = _case(5, 2, 4, 4)
    got = _fused(dev, inp)
    assert float(want['dW'].abs().max()) < 1e-12 and float(want['dh'].abs().max()) < 1e-12
    assert float(got['dW'].abs().max()) <= 1e-6 and float(got['dh'].abs().max()) <= 1e-6
    torch.testing.assert_close(got['v'].cpu().double(), inp['X'][:, 0] * inp['X'][:, 1],
                               rtol=1e-6, atol=1e-7)


def test_dropout_follows_the_counter_rule(dev):
    """(33, 5, 10, 25), p = 0.3: the float64 side takes its mask from
    drop_spec.ln_keep(site seed, counter, B d, p); y and all gradients match, the counter
    advances by one a step, and the second step draws another mask."""
    from recbole_amd.model.layers import AFM_SITE, site_seed
    B, F, d, A, p = 33, 5, 10, 25, 0.3
    inp, _ = _case(B, F, d, A)
    seed = site_seed(dev, AFM_SITE)
    assert seed == drop_spec.site_seed(torch.cuda.default_generators[0].initial_seed(), 0x5000)
    counter = torch.full((1,), 7, dtype=torch.int64, device=dev)
    masks = []
    for step in range(2):
        c = 7 + step
        flags = drop_spec.ln_keep(seed, c, B * d, p).reshape(B, d)
        masks.append(flags)
        keep = torch.as_tensor(flags).double() / (1 - p)
        want = dict(zip(NAMES, afm_grads64(inp['X'], inp['W'], inp['h'], inp['pv'], inp['gy'],
                                           keep=keep)))
        got = _fused(dev, inp, p=p, rng=(seed, counter))
        assert int(got['drawn'].item()) == c
        assert int(counter.item()) == c + 1
        _check(f'dropout step {step}', got, want, _library32(dev, inp, keep=keep))
    assert 0.5 < masks[0].mean() < 0.9
    assert not np.array_equal(masks[0], masks[1])
    # a probability outside (0, 1) is refused
    from recbole_amd import ops
    from recbole_amd._native import NativeError
    with pytest.raises(NativeError):
        ops.afm_fwd(*(inp[k].to(dev, torch.float32) for k in ('X', 'W', 'h', 'pv')), p=1.5,
                    rng=(seed, counter), drawn=counter.clone())
    assert int(counter.item()) == 9


@pytest.fixture
def capped_grid():
    """K20a / K20b launch 3 workgroups at most for the test, then as before."""
    from recbole_amd import ops
    before = ops.afm_grid_cap(3)
    yield 3
    ops.afm_grid_cap(before)


def _same_bits(one, two):
    assert set(one) == set(two)
    for k in one:
        assert torch.equal(one[k], two[k]), k


def test_waves_walk_many_samples(dev, capped_grid):
    """(300, 12, 16, 32): 300 samples and 30 splits on 3 workgroups; the same bounds, and the
    same bits as the uncapped run."""
    from recbole_amd import ops
    assert ops.afm_grid_cap(-1) == 3
    inp, want = _case(300, 12, 16, 32)
    got = _fused(dev, inp)
    _check('B=300 capped', got, want, _library32(dev, inp))
    ops.afm_grid_cap(0)
    _same_bits(got, _fused(dev, inp))


def test_two_runs_same_bits(dev):
    inp, _ = _case(300, 12, 16, 32)
    _same_bits(_fused(dev, inp), _fused(dev, inp))


def test_no_pair_tensors_in_memory(dev):
    """B = 2048, F = 39, d = 16, A = 25: the fused forward + backward holds dX, the saved
    state and at most 32 partial rows above its inputs, under 3 B F d floats; the library
    path, probed the same way, keeps the pair tensors (one [B, P, d] alone is 19 B F d) and
    is over it."""
    from recbole_amd.model.context_aware_recommender.afm import _AFMFn, afm_library
    from recbole_amd.model.layers import AttLayer
    B, F, d, A = 2048, 39, 16, 25
    bound = 3 * B * F * d * 4
    g = torch.Generator().manual_seed(1)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)
    X = u(B, F, d).requires_grad_(True)
    att = AttLayer(d, A).to(dev)
    pv = u(d).requires_grad_(True)
    gy = u(B)

    def peak(fn):
        for p in [X, pv] + list(att.parameters()):
            p.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn().backward(gy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = peak(lambda: _AFMFn.apply(X, att.w.weight, att.h, pv, 0.0, None))
    library = peak(lambda: afm_library(X, att, pv, lambda t: t)[:, 0])
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
    cd = {'model': 'AFM', 'dataset': 'ctx', 'data_path': root, 'embedding_size': 10,
          'attention_size': 25, 'dropout_prob': 0.0, 'load_col': None, 'epochs': 1,
          'train_batch_size': 512, 'state': 'ERROR', 'use_gpu': use_gpu, 'normalize_all': True,
          'checkpoint_dir': str(tmp_path / 'saved')}
    cd.update(over)
    config = Config(config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    ds = create_dataset(config)
    train, valid, test = data_preparation(config, ds)
    model = get_model('AFM')(config, train).to(config['device'])
    return config, train, model


def _library64(tmp_path, model, **over):
    """The 'library' path on the CPU in float64 with `model`'s state."""
    _, _, ref = _pipeline(tmp_path / 'ref', use_gpu=False, afm_kernel='library', **over)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.double()


def _cpu(b):
    from recbole_amd.data.interaction import Interaction
    return Interaction({k: v.cpu() for k, v in b.interaction.items()})


def _compare_step(model, ref, b, dev_b):
    loss = model.calculate_loss(dev_b)
    loss.backward()
    want = ref.calculate_loss(_cpu(b))
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        torch.testing.assert_close(p.grad.cpu().double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda s, k=name: f'{k}: {s}')


@pytest.mark.parametrize('seq,reg', [(True, 2), (True, 0.0), (False, 2), (False, 0.0)])
def test_loss_grads_predictions_match_library_float64(tmp_path, seq, reg):
    """F = 10 (seq: True) and 9; then predict in eval mode."""
    config, train, model = _pipeline(tmp_path, reg_weight=reg, seq=seq)
    b = next(iter(train))
    dev_b = b.to(config['device'])
    X = model.linear_fields(dev_b)[0]
    assert X.shape[1] == (10 if seq else 9) and model.afm_fused_applies(X)
    ref = _library64(tmp_path, model, reg_weight=reg, seq=seq)
    assert not ref.afm_fused_applies(X.cpu().double())
    _compare_step(model, ref, b, dev_b)
    model.eval()
    ref.eval()
    with torch.no_grad():
        out = model.predict(dev_b)
        assert out.shape == (b.length,)
        torch.testing.assert_close(out.cpu().double(), ref.predict(_cpu(b)), rtol=1e-4,
                                   atol=1e-6)


@pytest.mark.parametrize('d', [10, 16])
def test_train_steps_match_library_float64(tmp_path, d):
    """Four Adam steps through Trainer against torch.optim.Adam on the float64 copy, dropout
    0. Deferred: nothing at embedding_size 10 (not a width of the deferred kernels), the
    [V, d] token table and the [V, 1] first-order table at 16."""
    from recbole_amd.trainer import Trainer
    config, train, model = _pipeline(tmp_path, embedding_size=d, reg_weight=2)
    ref = _library64(tmp_path, model, embedding_size=d, reg_weight=2)
    opt = torch.optim.Adam(ref.parameters(), lr=config['learning_rate'])
    trainer = Trainer(config, model)
    deferred = list(getattr(trainer.optimizer, '_deferred', {}))
    want = [] if d == 10 else [model.token_embedding_table.embedding.weight,
                               model.first_order_linear.token_embedding_table.embedding.weight]
    assert len(deferred) == len(want) and all(a is b for a, b in zip(deferred, want))
    for step, b in enumerate(list(train)[:4]):
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


def test_model_dropout_draws_per_step(tmp_path):
    """Training mode at dropout_prob 0.3 draws through K20a's site and advances its counter
    by one a step; eval mode draws nothing."""
    config, train, model = _pipeline(tmp_path, dropout_prob=0.3)
    b = next(iter(train)).to(config['device'])
    for step in range(2):
        model.calculate_loss(b).backward()
        assert int(model._rng[1].item()) == step + 1
    model.eval()
    with torch.no_grad():
        one, two = model.predict(b), model.predict(b)
    assert torch.equal(one, two) and int(model._rng[1].item()) == 2


def test_unbuilt_shape_runs_through_torch(tmp_path):
    """attention_size 65 is not built: the model takes the op sequence."""
    config, train, model = _pipeline(tmp_path, attention_size=65, reg_weight=2)
    b = next(iter(train))
    dev_b = b.to(config['device'])
    assert not model.afm_fused_applies(model.linear_fields(dev_b)[0])
    ref = _library64(tmp_path, model, attention_size=65, reg_weight=2)
    _compare_step(model, ref, b, dev_b)


def test_ops_refuse_cpu_tensors_and_unbuilt_shapes(dev):
    from recbole_amd import ops
    from recbole_amd._native import NativeError, lib
    z = lambda *s, d='cpu': torch.zeros(*s, device=d)
    assert ops.afm_shape_ok(2, 2, 1) and ops.afm_shape_ok(64, 64, 64)
    assert ops.afm_shape_ok(39, 16, 25)
    for bad in ((1, 10, 25), (65, 10, 25), (10, 1, 25), (10, 65, 25), (10, 10, 0), (10, 10, 65)):
        assert not ops.afm_shape_ok(*bad), bad
    with pytest.raises(NativeError):
        ops.afm_fwd(z(4, 3, 8), z(5, 8), z(5), z(8))
    with pytest.raises(NativeError):
        ops.afm_bwd(z(4, 3, 8), z(5, 8), z(5), z(8), z(4, 8), z(4, 2), z(4))
    X = z(4, 3, 8, d=dev)
    with pytest.raises(NativeError, match='not in the built set'):
        ops.afm_fwd(X, z(65, 8, d=dev), z(65, d=dev), z(8, d=dev))
    with pytest.raises(NativeError, match='not in the built set'):
        ops.afm_bwd(X, z(65, 8, d=dev), z(65, d=dev), z(8, d=dev), z(4, 8, d=dev),
                    z(4, 2, d=dev), z(4, d=dev))
    with pytest.raises(NativeError, match='not in the built set'):
        ops.afm_fwd(z(4, 65, 8, d=dev), z(5, 8, d=dev), z(5, d=dev), z(8, d=dev))
    # the library itself refuses too, with the same words
    p = X.data_ptr()
    rc = lib().mirec_afm_fwd_f32(p, 4, 3, 8, p, p, 65, p, p, p, p, 0.0, 0, None, None, None)
    assert rc == -1 and b'not in the built set' in lib().mirec_last_error()
    with pytest.raises(ValueError):
        ops.afm_fwd(X, z(5, 7, d=dev), z(5, d=dev), z(8, d=dev))
    with pytest.raises(ValueError):
        ops.afm_bwd(X, z(5, 8, d=dev), z(5, d=dev), z(8, d=dev), z(4, 8, d=dev),
                    z(4, 2, d=dev), z(3, d=dev))
    assert ops.afm_grid_cap(-1) == 0


def test_run_recbole_afm(tmp_path):
    from recbole_amd.quick_start import run_recbole
    root = write_ctx_dataset(str(tmp_path))
    res = run_recbole(model='AFM', dataset='ctx', config_dict={
        'data_path': root, 'epochs': 2, 'load_col': None, 'state': 'ERROR',
        'checkpoint_dir': str(tmp_path / 'saved'), 'show_progress': False})
    r = {k.lower(): v for k, v in res['test_result'].items()}
    assert set(r) == {'auc', 'logloss'}
    assert 0.0 <= r['auc'] <= 1.0 and np.isfinite(r['logloss'])
