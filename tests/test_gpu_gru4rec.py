"""GRU4Rec on the GPU (K1 gather with the grouped gradient, the library GRU, dense on the last
positions, K3 BPR / library or K12 cross entropy, K6 evaluation) against the float64 CPU
restatement of the reference's op sequence (tests/gru4rec_spec.py) carrying the model's
weights. The synthetic data set of the SASRec tests: 80 users, 120 items,
MAX_ITEM_LIST_LENGTH 12; dropout_prob 0 wherever values are compared. Tolerances are those
of test_gpu_sasrec.py: loss rtol 1e-4; gradients rtol 1e-4, atol 1e-6; parameters after
four Adam steps rtol 1e-3, atol 2e-5."""
import numpy as np
import pytest
import torch

from tests.gru4rec_spec import ref_of

pytestmark = pytest.mark.gpu


def _pipeline(tmp_path, **over):
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.utils import get_model, init_seed
    root = _write_dataset(str(tmp_path), 'synth', n_users=80, n_items=120, n_inter=3000)
    cd = {'model': 'GRU4Rec', 'dataset': 'synth', 'data_path': root, 'epochs': 1,
          'load_col': {'inter': ['user_id', 'item_id', 'timestamp']}, 'MAX_ITEM_LIST_LENGTH': 12,
          'dropout_prob': 0.0, 'train_batch_size': 256,
          'checkpoint_dir': str(tmp_path / 'saved'), 'loss_type': 'CE',
          'training_neg_sample_num': 0}
    cd.update(over)
    config = Config(config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    ds = create_dataset(config)
    train, valid, test = data_preparation(config, ds)
    model = get_model('GRU4Rec')(config, train).to(config['device'])
    return config, train, valid, test, model


def _ref_loss(ref, b):
    c = {k: v.cpu() for k, v in b.interaction.items()}
    return ref.calculate_loss(c['item_id_list'], c['item_length'], c['item_id'],
                              c.get('neg_item_id'))


def _check_grads(model, ref, loss, ref_loss):
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.grad.cpu().double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda m, n=name: f'{n}: {m}')


@pytest.mark.parametrize('loss_type,neg,ce_kernel', [('CE', 0, 'library'), ('BPR', 1, 'library'),
                                                     ('CE', 0, 'fused')])
def test_gru4rec_loss_grads_match_restatement(tmp_path, loss_type, neg, ce_kernel):
    config, train, valid, test, model = _pipeline(tmp_path, loss_type=loss_type,
                                                  training_neg_sample_num=neg,
                                                  ce_kernel=ce_kernel)
    assert model.hidden_size == 128 and model.embedding_size == 64
    ref = ref_of(model)
    b = next(iter(train))
    loss = model.calculate_loss(b)
    loss.backward()
    if loss_type == 'CE':
        want = '_FullCEFnBackward' if ce_kernel == 'fused' else 'NllLossBackward0'
        assert type(loss.grad_fn).__name__ == want
    ref_loss = _ref_loss(ref, b)
    ref_loss.backward()
    _check_grads(model, ref, loss, ref_loss)


def test_gru4rec_train_and_eval(tmp_path):
    """Four Adam steps through the Trainer vs torch Adam on the restatement; fused K6
    sequential full-sort evaluation vs the generic full_sort_predict sequence; the sampled
    (uni1000) validation runs."""
    from recbole_amd.trainer import Trainer
    config, train, valid, test, model = _pipeline(tmp_path)
    ref = ref_of(model)
    opt = torch.optim.Adam(ref.parameters(), lr=config['learning_rate'])
    trainer = Trainer(config, model)
    for b in list(train)[:4]:
        trainer.optimizer.zero_grad()
        loss = model.calculate_loss(b)
        loss.backward()
        trainer.optimizer.step()
        opt.zero_grad()
        ref_loss = _ref_loss(ref, b)
        ref_loss.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    trainer.optimizer.flush()
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.detach().cpu().double(), refp[name].detach(), rtol=1e-3,
                                   atol=2e-5, msg=lambda m, n=name: f'{n}: {m}')
    fused = trainer.evaluate(test, load_best_model=False)
    config['fused_eval'] = False
    generic = trainer.evaluate(test, load_best_model=False)
    for k in fused:
        assert fused[k] == pytest.approx(generic[k], abs=2e-4), k
    config['fused_eval'] = True
    res = trainer.evaluate(valid, load_best_model=False)
    assert 0.0 <= res['hit@10'] <= 1.0


@pytest.mark.parametrize('train_graph', [True, False])
def test_run_recbole_gru4rec(tmp_path, train_graph):
    """One epoch end to end with the default dropout_prob, train_graph on and off (the
    model does not offer its step for capture, so both train eagerly)."""
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.quick_start import run_recbole
    root = _write_dataset(str(tmp_path), 'synth', n_users=80, n_items=120, n_inter=3000)
    cd = {'data_path': root, 'epochs': 1, 'checkpoint_dir': str(tmp_path / 'saved'),
          'load_col': {'inter': ['user_id', 'item_id', 'timestamp']}, 'show_progress': False,
          'MAX_ITEM_LIST_LENGTH': 12, 'training_neg_sample_num': 0, 'train_graph': train_graph}
    res = run_recbole(model='GRU4Rec', dataset='synth', config_dict=cd)
    for part in ('best_valid_result', 'test_result'):
        for k, v in res[part].items():
            assert 0.0 <= v <= 1.0, (part, k, v)
