"""AFM without a GPU: plugin lookup and alias, yaml defaults, state-dict keys, seeded
construction against a locally built module with the reference's draw order, the float64
closed forms (tests/afm_spec.py) against torch autograd of the op sequence, the CPU model
against the restatement, deferred_tables, the afm_kernel key, and a two-epoch CPU run."""
import importlib

import numpy as np
import pytest
import torch

from tests.afm_spec import AFMRef, afm_grads64, afm_inputs, ref_of
from tests.ctx_data import write_ctx_dataset


def _model(tmp_path, build=True, **over):
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.utils import get_model, init_seed
    root = write_ctx_dataset(str(tmp_path), seq=over.pop('seq', True))
    cd = {'model': 'AFM', 'dataset': 'ctx', 'data_path': root, 'use_gpu': False,
          'embedding_size': 10, 'attention_size': 25, 'dropout_prob': 0.0, 'load_col': None,
          'train_batch_size': 256, 'state': 'ERROR', 'normalize_all': True,
          'checkpoint_dir': str(tmp_path / 'saved')}
    cd.update(over)
    config = Config(config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    ds = create_dataset(config)
    train, _, _ = data_preparation(config, ds)
    model = get_model('AFM')(config, train) if build else None
    return config, train, model


def test_plugin_lookup_and_alias():
    from recbole_amd.model.context_aware_recommender import AFM
    from recbole_amd.model.layers import AFM_SITE, NGCF_SITE, AttLayer
    from recbole_amd.utils import InputType, get_model
    assert get_model('AFM') is AFM
    mod = importlib.import_module('recbole.model.context_aware_recommender.afm')
    assert mod is importlib.import_module('recbole_amd.model.context_aware_recommender.afm')
    assert mod.AFM is AFM
    from recbole.model.context_aware_recommender import AFM as aliased
    assert aliased is AFM
    assert AFM.input_type == InputType.POINTWISE
    assert AFM.graph_step_safe is False
    assert AFM_SITE == 0x5000 and AFM_SITE != NGCF_SITE
    att = AttLayer(4, 3)
    assert list(dict(att.named_parameters())) == ['h', 'w.weight']
    w = att(torch.rand(2, 6, 4))
    assert w.shape == (2, 6)
    torch.testing.assert_close(w.sum(dim=1), torch.ones(2))


def test_defaults_are_the_reference_yaml():
    from recbole_amd.config.defaults import MODEL_DEFAULTS
    d = dict(MODEL_DEFAULTS['AFM'])
    assert d.pop('afm_kernel') in ('fused', 'library')      # the build's key
    assert d == dict(embedding_size=10, attention_size=25, dropout_prob=0.3, reg_weight=2)


def test_state_dict_keys(tmp_path):
    _, _, model = _model(tmp_path)
    keys = list(model.state_dict())
    assert keys == [
        'p', 'token_embedding_table.embedding.weight', 'float_embedding_table.weight',
        'token_seq_embedding_table.0.weight', 'first_order_linear.bias',
        'first_order_linear.token_embedding_table.embedding.weight',
        'first_order_linear.float_embedding_table.weight',
        'first_order_linear.token_seq_embedding_table.0.weight', 'attlayer.h',
        'attlayer.w.weight']
    assert model.attlayer.w.weight.shape == (25, 10) and model.attlayer.w.bias is None
    assert model.attlayer.h.shape == (25,) and model.p.shape == (10,)
    assert model.num_pair == model.num_feature_field * (model.num_feature_field - 1) / 2


@pytest.mark.parametrize('seed', [0, 2020])
def test_seeded_construction_matches_the_reference_sequence(tmp_path, seed):
    """The base's tables, then attlayer.w (Linear's own init, overwritten later), attlayer.h =
    randn, p = randn; _init_weights touches Embedding and Linear only."""
    from recbole_amd.utils import get_model, init_seed
    config, train, _ = _model(tmp_path, build=False)
    init_seed(seed, True)
    model = get_model('AFM')(config, train)
    init_seed(seed, True)
    ref = AFMRef(model.token_field_names, list(model.token_field_dims),
                 model.token_seq_field_names, list(model.token_seq_field_dims),
                 model.float_field_names, 10, 25, 2)
    got, want = model.state_dict(), ref.state_dict()
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert float(got['attlayer.h'].abs().max()) > 1.0            # randn, not xavier
    assert float(got['p'].abs().max()) > 0.5
    assert not torch.equal(got['p'], got['attlayer.h'][:10])


@pytest.mark.parametrize('B,F,d,A', [(33, 3, 10, 25), (5, 2, 4, 4)])
def test_closed_forms_match_autograd_of_the_op_sequence(B, F, d, A):
    """The spec's written-out gradients against torch autograd of afm_library in float64,
    without and with a keep mask."""
    from recbole_amd.model.context_aware_recommender.afm import afm_library
    from recbole_amd.model.layers import AttLayer
    inp = afm_inputs(B, F, d, A)
    assert inp['seed'] < 64
    g = torch.Generator().manual_seed(3)
    keep = (torch.rand(B, d, generator=g) < 0.7).double() / 0.7
    for k in (None, keep):
        att = AttLayer(d, A).double()
        with torch.no_grad():
            att.w.weight.copy_(inp['W'])
            att.h.copy_(inp['h'])
        X = inp['X'].clone().requires_grad_(True)
        pv = inp['pv'].clone().requires_grad_(True)
        drop = (lambda t: t) if k is None else (lambda t: t * k)
        y = afm_library(X, att, pv, drop)
        assert y.shape == (B, 1)
        y[:, 0].backward(inp['gy'])
        wy, wv, dX, dW, dh, dpv = afm_grads64(inp['X'], inp['W'], inp['h'], inp['pv'], inp['gy'],
                                              keep=k)
        torch.testing.assert_close(y.detach()[:, 0], wy, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(X.grad, dX, rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(att.w.weight.grad, dW, rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(att.h.grad, dh, rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(pv.grad, dpv, rtol=1e-11, atol=1e-12)
        assert wv.shape == (B, d)
    if F == 2:                                # one pair: alpha = 1, v = z, no attention gradient
        torch.testing.assert_close(wv, inp['X'][:, 0] * inp['X'][:, 1], rtol=1e-12, atol=1e-12)
        assert float(dW.abs().max()) < 1e-12 and float(dh.abs().max()) < 1e-12


@pytest.mark.parametrize('reg', [2, 0.0])
def test_cpu_model_matches_the_restatement(tmp_path, reg):
    """Loss, every parameter gradient and predict of a CPU-device model against float64,
    dropout 0."""
    _, train, model = _model(tmp_path, reg_weight=reg)
    ref = ref_of(model)
    b = next(iter(train))
    inter = {k: v for k, v in b.interaction.items()}
    X, _ = model.linear_fields_torch(b)
    assert not model.afm_fused_applies(X)
    loss = model.calculate_loss(b)
    loss.backward()
    want = ref.calculate_loss(inter, b['label'])
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    assert set(refp) == {n for n, _ in model.named_parameters()}
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        torch.testing.assert_close(p.grad.double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda s, n=name: f'{n}: {s}')
    model.eval()
    with torch.no_grad():
        out = model.predict(b)
        assert out.shape == (b.length,)
        torch.testing.assert_close(out.double(), ref.forward(inter), rtol=1e-4, atol=1e-6)
        assert model.afm_layer(X).shape == (b.length, 1)


@pytest.mark.parametrize('d', [10, 16])
def test_deferred_tables(tmp_path, d):
    """The [V, d] token table and the [V, 1] first-order table, at a width the deferred Adam
    kernels take."""
    _, _, model = _model(tmp_path, embedding_size=d)
    tables = model.deferred_tables()
    if d == 10:
        assert tables == []
    else:
        assert len(tables) == 2
        assert tables[0] is model.token_embedding_table.embedding.weight
        assert tables[1] is model.first_order_linear.token_embedding_table.embedding.weight


def test_afm_kernel_key(tmp_path):
    _, _, model = _model(tmp_path, afm_kernel='library')
    assert model.afm_kernel == 'library'
    assert not model.afm_fused_applies(torch.zeros(4, 10, 10))
    _, _, model = _model(tmp_path)
    assert model.afm_kernel == 'fused'
    with pytest.raises(ValueError, match='afm_kernel'):
        _model(tmp_path, afm_kernel='triton')


def test_run_recbole_afm_cpu(tmp_path):
    from recbole_amd.quick_start import run_recbole
    root = write_ctx_dataset(str(tmp_path))
    res = run_recbole(model='AFM', dataset='ctx', config_dict={
        'data_path': root, 'use_gpu': False, 'epochs': 2, 'state': 'ERROR',
        'show_progress': False, 'load_col': None, 'attention_size': 8,
        'checkpoint_dir': str(tmp_path / 'saved')})
    r = {k.lower(): v for k, v in res['test_result'].items()}
    assert set(r) == {'auc', 'logloss'}
    assert np.isfinite(r['auc']) and 0.0 <= r['auc'] <= 1.0
    assert np.isfinite(r['logloss']) and r['logloss'] > 0.0
