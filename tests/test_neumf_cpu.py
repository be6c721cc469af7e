"""NeuMF without a GPU: plugin lookup and alias, yaml defaults, state-dict keys and seeded
construction against a locally built module with the reference's construction order, the
CPU path against the float64 restatement (tests/neumf_spec.py), the mf_train / mlp_train
forms and errors, one CPU epoch on ml-100k, and the CPU check of the weight draw the GPU
scorer tests rank (tests/test_gpu_neumf.py)."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests.neumf_spec import (NeuMFRef, draw_weights, logits32_split, logits64, make_history,
                              masked_topk, ref_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, nq, I, dmf, dm, hidden): the cases test_gpu_neumf.py runs K14c on
SCORER_CASES = [(0, 70, 301, 16, 32, [64, 32, 16]), (1, 1, 33, 8, 8, [16, 16]),
                (2, 130, 1000, 64, 64, [128, 64, 32]), (0, 70, 301, 0, 12, [32, 16, 48, 16])]
GAP = 2e-4


def _model(tmp_path, build=True, **over):
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.utils import get_model, init_seed
    root = _write_dataset(str(tmp_path), 'synth', n_users=40, n_items=60, n_inter=900)
    cd = {'model': 'NeuMF', 'dataset': 'synth', 'data_path': root, 'use_gpu': False,
          'train_batch_size': 64, 'mf_embedding_size': 8, 'mlp_embedding_size': 12,
          'mlp_hidden_size': [16, 8], 'state': 'ERROR'}
    cd.update(over)
    config = Config(config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    ds = create_dataset(config)
    train, _, test = data_preparation(config, ds)
    model = get_model('NeuMF')(config, train) if build else None
    return config, train, test, model


def _batch(model, B=37, seed=3):
    g = torch.Generator().manual_seed(seed)
    user = torch.randint(1, model.n_users, (B,), generator=g)
    item = torch.randint(1, model.n_items, (B,), generator=g)
    user[5:9] = user[0]                              # repeated users and items
    item[20:23] = item[1]
    label = (torch.rand(B, generator=g) < 0.5).float()
    return {'user_id': user, 'item_id': item, 'label': label}


def test_plugin_lookup_and_alias():
    from recbole_amd.model.general_recommender import NeuMF
    from recbole_amd.utils import InputType, get_model
    assert get_model('NeuMF') is NeuMF
    mod = importlib.import_module('recbole.model.general_recommender.neumf')
    assert mod is importlib.import_module('recbole_amd.model.general_recommender.neumf')
    assert mod.NeuMF is NeuMF
    from recbole.model.general_recommender import NeuMF as aliased
    assert aliased is NeuMF
    assert NeuMF.input_type == InputType.POINTWISE
    assert not hasattr(NeuMF, 'fused_user_vectors')      # that hook means "a dot product"


def test_defaults_are_the_reference_yaml():
    from recbole_amd.config.defaults import MODEL_DEFAULTS
    assert MODEL_DEFAULTS['NeuMF'] == dict(
        mf_embedding_size=64, mlp_embedding_size=64, mlp_hidden_size=[128, 64, 32],
        dropout_prob=0.0, weight_decay=1e-08, mf_train=True, mlp_train=True,
        valid_metric='HIT@10', use_pretrain=False, mf_pretrain_path=None,
        mlp_pretrain_path=None)


def test_state_dict_keys(tmp_path):
    _, _, _, model = _model(tmp_path)
    assert list(model.state_dict()) == [
        'user_mf_embedding.weight', 'item_mf_embedding.weight', 'user_mlp_embedding.weight',
        'item_mlp_embedding.weight', 'mlp_layers.mlp_layers.1.weight',
        'mlp_layers.mlp_layers.1.bias', 'mlp_layers.mlp_layers.4.weight',
        'mlp_layers.mlp_layers.4.bias', 'predict_layer.weight', 'predict_layer.bias']
    assert [n for n, _ in model.named_children()] == [
        'user_mf_embedding', 'item_mf_embedding', 'user_mlp_embedding', 'item_mlp_embedding',
        'mlp_layers', 'predict_layer', 'sigmoid', 'loss']
    assert model.graph_step_safe is False


@pytest.mark.parametrize('seed', [0, 2020])
def test_seeded_construction_matches_the_reference_sequence(tmp_path, seed):
    from recbole_amd.utils import get_model
    config, train, _, _ = _model(tmp_path, build=False)
    torch.manual_seed(seed)
    model = get_model('NeuMF')(config, train)
    torch.manual_seed(seed)
    ref = NeuMFRef(model.n_users, model.n_items, 8, 12, [16, 8])
    want, got = ref.state_dict(), model.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert float(got['user_mf_embedding.weight'].std()) == pytest.approx(0.01, rel=0.2)
    # Linears keep torch's default init: not the embeddings' normal(0, 0.01)
    assert float(got['predict_layer.weight'].abs().max()) > 0.05


@pytest.mark.parametrize('mf,mlp', [(True, True), (True, False), (False, True)])
def test_cpu_model_matches_the_restatement(tmp_path, mf, mlp):
    """Loss, every parameter gradient and predict of a CPU-device model against float64,
    for the three predict_layer shapes."""
    from recbole_amd.utils import get_model
    config, train, _, _ = _model(tmp_path, build=False)
    config['mf_train'], config['mlp_train'] = mf, mlp
    model = get_model('NeuMF')(config, train)
    assert model.predict_layer.in_features == (8 if mf else 0) + (8 if mlp else 0)
    ref = ref_of(model)
    b = _batch(model)
    loss = model.calculate_loss(b)
    loss.backward()
    want = ref.calculate_loss(b['user_id'], b['item_id'], b['label'])
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        if refp[name].grad is None:                  # the half that is off
            assert p.grad is None, name
            continue
        torch.testing.assert_close(p.grad.double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda m, n=name: f'{n}: {m}')
    with torch.no_grad():
        got = model.predict(b)
        torch.testing.assert_close(got.double(), ref(b['user_id'], b['item_id']), rtol=1e-4,
                                   atol=1e-6)
    assert got.shape == (37,)
    with pytest.raises(NotImplementedError):         # a CPU device: the trainer's generic path
        model.full_sort_predict(b)
    assert model.fused_pair_scorer() is None


def test_both_halves_off_raises(tmp_path):
    _, _, _, model = _model(tmp_path, mf_train=False, mlp_train=False)
    with pytest.raises(RuntimeError, match='mf_train and mlp_train can not be False'):
        model.calculate_loss(_batch(model))


def test_use_pretrain_raises(tmp_path):
    with pytest.raises(NotImplementedError, match='use_pretrain'):
        _model(tmp_path, use_pretrain=True)


def test_run_recbole_neumf_cpu(tmp_path):
    """One epoch on ml-100k on the CPU: the pointwise sampling loader, the torch op sequence
    and the generic full-sort evaluation (no full_sort_predict on a CPU device)."""
    from recbole_amd.quick_start import run_recbole
    res = run_recbole(model='NeuMF', dataset='ml-100k', config_dict={
        'data_path': os.path.join(ROOT, 'dataset'), 'use_gpu': False, 'epochs': 1,
        'state': 'ERROR', 'show_progress': False, 'mf_embedding_size': 8,
        'mlp_embedding_size': 8, 'mlp_hidden_size': [16, 8],
        # the interaction columns alone: the sampled validation joins every loaded feature
        # onto its ~10^7 candidate rows on the host
        'load_col': {'inter': ['user_id', 'item_id']},
        'checkpoint_dir': str(tmp_path / 'saved')})
    assert res['valid_score_bigger'] is True
    for part in ('best_valid_result', 'test_result'):
        assert 'hit@10' in {k.lower() for k in res[part]}
        for k, v in res[part].items():
            assert 0.0 <= v <= 1.0, (part, k, v)


@pytest.mark.parametrize('seed,nq,I,dmf,dm,hidden', SCORER_CASES)
def test_scorer_draw_ranks_in_fp32(seed, nq, I, dmf, dm, hidden):
    """The draw the GPU tests rank: the fp32 split-layer form stays within 1e-4 of float64,
    agrees with the float64 top-10 wherever the float64 gap to both neighbours exceeds
    2e-4, and at most 3 % of the positions fall under that gap."""
    w = draw_weights(seed, nq, I, dmf, dm, hidden)
    users = np.arange(nq)
    z64, z32 = logits64(w, users), logits32_split(w, users)
    assert np.abs(z32 - z64).max() < 1e-4
    assert 0.3 < z64.std() < 10                      # spread to O(1)
    hist = make_history(seed, nq, I, nearly_all=0 if nq > 1 else None)
    want, gap = masked_topk(z64, hist, 10)
    got, _ = masked_topk(z32.astype(np.float64), hist, 10)
    clear = gap > GAP
    assert np.array_equal(got[clear], want[clear])
    assert (~clear).mean() <= 0.03
    assert (want[:, :3] > 0).all() and not (want == 0).any()
