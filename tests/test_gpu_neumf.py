"""NeuMF on the GPU against the float64 restatement (tests/neumf_spec.py): the training
path (K14a gather, K10 MLP + head slice, sigmoid + BCE, K14b backward, K2 scatter, dense /
deferred / streamed Adam), dropout, the fused pair-MLP full-sort scorer K14c (scores and
top-K modes), the trainer's evaluator wiring and one epoch end to end.

Tolerances: loss rtol 1e-4; gradients rtol 1e-4, atol 1e-6; parameters after four Adam
steps rtol 1e-3, atol 2e-5 (those of test_gpu_gru4rec.py). K14c: every logit within 1e-4
of float64; top-K ids equal the float64 ranking wherever the float64 gap to both neighbours
exceeds 2e-4, at most 3 % of the positions excused (tests/test_neumf_cpu.py checks the same
draw in fp32 on the CPU)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.neumf_spec import draw_weights, logits64, make_history, masked_topk, ref_of
from tests.test_neumf_cpu import GAP, SCORER_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_USERS, N_ITEMS, B = 70, 301, 37
WIDTHS = [(8, 8, [16, 8]), (16, 32, [64, 32, 16])]


class _DS:
    def num(self, field):
        return {'user_id': N_USERS, 'item_id': N_ITEMS}[field]


def _build(tmp_path, dmf, dm, hidden, emb_std=0.5, **over):
    """A NeuMF on cuda:0 over 70 users x 301 items with its embeddings re-drawn at emb_std
    (the 0.01 of the init leaves gradients at the absolute tolerance)."""
    from recbole_amd.config import Config
    from recbole_amd.model.general_recommender import NeuMF
    cd = {'mf_embedding_size': dmf, 'mlp_embedding_size': dm, 'mlp_hidden_size': hidden,
          'load_col': None, 'state': 'ERROR', 'checkpoint_dir': str(tmp_path / 'saved')}
    cd.update(over)
    config = Config(model='NeuMF', dataset='neumf_test', config_dict=cd)
    torch.manual_seed(11)
    model = NeuMF(config, _DS()).to(config['device'])
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'embedding' in name:
                p.normal_(0.0, emb_std)
    return config, model


def _batch(seed, dev):
    g = torch.Generator().manual_seed(seed)
    user = torch.randint(1, N_USERS, (B,), generator=g)
    item = torch.randint(1, N_ITEMS, (B,), generator=g)
    user[5:9] = user[0]                              # repeated users and items in the batch
    item[20:23] = item[1]
    user[30] = user[12]
    label = (torch.rand(B, generator=g) < 0.5).float()
    return {'user_id': user.to(dev), 'item_id': item.to(dev), 'label': label.to(dev)}


def _ref_loss(ref, b):
    return ref.calculate_loss(b['user_id'].cpu(), b['item_id'].cpu(), b['label'].cpu())


def _check_loss_grads(model, ref, b):
    loss = model.calculate_loss(b)
    loss.backward()
    assert type(loss.grad_fn).__name__ == '_SigmoidBCEFnBackward'
    want = _ref_loss(ref, b)
    want.backward()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        if refp[name].grad is None:
            assert p.grad is None, name
            continue
        assert float(refp[name].grad.abs().max()) > 1e-5, name      # above the absolute tolerance
        torch.testing.assert_close(p.grad.cpu().double(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda m, n=name: f'{n}: {m}')


@pytest.mark.parametrize('dmf,dm,hidden', WIDTHS)
def test_loss_and_gradients_match_the_restatement(tmp_path, dmf, dm, hidden):
    config, model = _build(tmp_path, dmf, dm, hidden)
    _check_loss_grads(model, ref_of(model), _batch(3, config['device']))
    with torch.no_grad():
        b = _batch(4, config['device'])
        torch.testing.assert_close(model.predict(b).cpu().double(),
                                   ref_of(model)(b['user_id'].cpu(), b['item_id'].cpu()),
                                   rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize('mf,mlp', [(True, False), (False, True)])
def test_single_half_forms(tmp_path, mf, mlp):
    config, model = _build(tmp_path, 16, 32, [64, 32, 16], mf_train=mf, mlp_train=mlp)
    assert model.predict_layer.in_features == 16       # dmf alone, or the last hidden width
    _check_loss_grads(model, ref_of(model), _batch(5, config['device']))


@pytest.mark.parametrize('adam_mode', ['deferred', 'streamed'])
@pytest.mark.parametrize('dmf,dm,hidden', WIDTHS)
def test_four_adam_steps(tmp_path, dmf, dm, hidden, adam_mode):
    """Through the Trainer's optimizer (weight_decay 1e-8, the yaml default) against
    torch.optim.Adam on the restatement; widths 16 / 32 run the deferred tables, 8 is
    outside enable_deferred's list and takes dense gradients."""
    from recbole_amd.trainer import Trainer
    config, model = _build(tmp_path, dmf, dm, hidden, adam_mode=adam_mode)
    assert config['weight_decay'] == 1e-8
    ref = ref_of(model)
    opt = torch.optim.Adam(ref.parameters(), lr=config['learning_rate'], weight_decay=1e-8)
    trainer = Trainer(config, model)
    deferred = getattr(trainer.optimizer, '_deferred', {})
    assert len(deferred) == (4 if adam_mode == 'deferred' and dmf == 16 else 0)
    for s in range(4):
        b = _batch(20 + s, config['device'])
        trainer.optimizer.zero_grad()
        loss = model.calculate_loss(b)
        loss.backward()
        trainer.optimizer.step()
        opt.zero_grad()
        want = _ref_loss(ref, b)
        want.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), want.item(), rtol=1e-4)
    trainer.optimizer.flush()
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.detach().cpu().double(), refp[name].detach(), rtol=1e-3,
                                   atol=2e-5, msg=lambda m, n=name: f'{n}: {m}')


def test_dropout_draws_in_training_only(tmp_path):
    config, model = _build(tmp_path, 16, 32, [64, 32, 16], dropout_prob=0.2)
    b = _batch(6, config['device'])
    model.train()
    a1, a2 = model.calculate_loss(b).item(), model.calculate_loss(b).item()
    assert a1 != a2
    model.eval()
    with torch.no_grad():
        e1, e2 = model.calculate_loss(b).item(), model.calculate_loss(b).item()
        p1, p2 = model.predict(b), model.predict(b)
    assert e1 == e2 and torch.equal(p1, p2)
    np.testing.assert_allclose(e1, _ref_loss(ref_of(model).eval(), b).item(), rtol=1e-4)


# ------------------------------------------------------------------ K14c against the spec
@functools.lru_cache(maxsize=None)
def _scorer_case(idx):
    """Weights, float64 logits, histories, positives and the expected rankings of one case,
    computed once."""
    seed, nq, I, dmf, dm, hidden = SCORER_CASES[idx]
    w = draw_weights(seed, nq, I, dmf, dm, hidden)
    z = logits64(w, np.arange(nq))
    hist = make_history(seed, nq, I, nearly_all=0 if nq > 1 else None)
    rng = np.random.default_rng(seed + 100)
    pos = [sorted(set(rng.integers(1, I, 3).tolist()) - set(h)) for h in hist]
    want = {(K, m): masked_topk(z, hist if m else None, K) for K in (10, 1) for m in (True, False)}
    return w, z, hist, pos, want


def _device_side(w, dev):
    """The host side of K14c for every user of a drawn case: A, Pq, Bm and the descriptor."""
    from recbole_amd import ops
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    dmf, dm = w['U_mf'].shape[1], w['U_mlp'].shape[1]
    Ws, bs = [T(x) for x in w['W']], [T(x) for x in w['b']]
    A = ops.neumf_project(T(w['U_mlp']), Ws[0], 0, bias=bs[0],
                          idx=torch.arange(w['U_mlp'].shape[0], device=dev))
    Bm = ops.neumf_project(T(w['I_mlp']), Ws[0], dm)
    Pq = T(w['U_mf'] * w['predict'][:dmf]) if dmf else None
    I_mf = T(w['I_mf']) if dmf else None
    desc, keep = ops.pair_mlp_desc(Ws, bs, T(w['predict'][dmf:]), T(w['bias']), dmf)
    return desc, keep, A, Pq, Bm, I_mf


def _csr(lists, dev):
    ptr = np.r_[0, np.cumsum([len(x) for x in lists])].astype(np.int64)
    cols = np.asarray([c for x in lists for c in x] or [0], dtype=np.int32)
    return torch.as_tensor(ptr, device=dev), torch.as_tensor(cols, device=dev)


@pytest.mark.parametrize('idx', range(len(SCORER_CASES)))
def test_pair_scorer_supported_shapes(idx):
    from recbole_amd import ops
    _, _, _, dmf, _, hidden = SCORER_CASES[idx]
    assert ops.pair_mlp_supported(hidden, dmf)
    assert ops.pair_mlp_supported([256, 256, 256, 256], 128)
    assert not ops.pair_mlp_supported([16, 8], 8) and not ops.pair_mlp_supported([64], 8)


@pytest.mark.parametrize('idx', range(len(SCORER_CASES)))
def test_k14c_scores_mode(idx):
    from recbole_amd import ops
    dev = torch.device('cuda', 0)
    w, z, _, _, _ = _scorer_case(idx)
    desc, keep, A, Pq, Bm, I_mf = _device_side(w, dev)
    got = ops.pair_mlp_scores(desc, A, Pq, Bm, I_mf).cpu().numpy().astype(np.float64)
    err = np.abs(got - z).max()
    print(f'case {idx}: max |logit - float64| = {err:.3g}')
    assert got.shape == z.shape and err < 1e-4


@pytest.mark.parametrize('mask', [True, False])
@pytest.mark.parametrize('K', [10, 1])
@pytest.mark.parametrize('idx', range(len(SCORER_CASES)))
def test_k14c_topk_mode(idx, K, mask):
    from recbole_amd import ops
    dev = torch.device('cuda', 0)
    w, z, hist, pos, want = _scorer_case(idx)
    desc, keep, A, Pq, Bm, I_mf = _device_side(w, dev)
    hp, hc = _csr(hist, dev) if mask else (None, None)
    pp, pc = _csr(pos, dev)
    o = ops.pair_mlp_topk(desc, A, Pq, Bm, I_mf, K, hist_ptr=hp, hist_cols=hc, pos_ptr=pp,
                          pos_cols=pc)
    ids = o['ids'].cpu().numpy().astype(np.int64)
    scores = o['scores'].cpu().numpy().astype(np.float64)
    flags = o['pos_flags'].cpu().numpy().astype(bool)
    exp_ids, gap = want[(K, mask)]
    assert not (ids == 0).any()                          # the pad item is never returned
    clear = gap > GAP
    excused = (~clear).mean()
    print(f'case {idx} K={K} mask={mask}: {excused:.4f} of the positions under the gap, '
          f'{(ids != exp_ids).mean():.4f} differ')
    assert np.array_equal(ids[clear], exp_ids[clear])
    assert excused <= 0.03
    nq = z.shape[0]
    for q in range(nq):
        for r in range(K):
            i = ids[q, r]
            if i < 0:
                assert scores[q, r] == -np.inf and not flags[q, r]
                continue
            assert abs(scores[q, r] - z[q, i]) < 1e-4, (q, r, i)
            assert flags[q, r] == (i in pos[q]), (q, r, i)
            if mask:
                assert i not in hist[q], (q, r, i)
    if mask and nq > 1:                                  # all but 3 items masked for user 0
        assert (ids[0, :min(K, 3)] > 0).all() and (ids[0, 3:] == -1).all()


# ------------------------------------------------------------------ the trainer
def _ml100k(tmp_path, **over):
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.utils import get_model, init_seed
    cd = {'data_path': os.path.join(ROOT, 'dataset'), 'state': 'ERROR', 'show_progress': False,
          'checkpoint_dir': str(tmp_path / 'saved')}
    cd.update(over)
    config = Config(model='NeuMF', dataset='ml-100k', config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    train, valid, test = data_preparation(config, create_dataset(config))
    model = get_model('NeuMF')(config, train).to(config['device'])
    return config, train, valid, test, model


def test_evaluate_goes_through_the_pair_scorer(tmp_path, monkeypatch):
    """Trainer.evaluate with fused_eval on takes fused_pair_full_sort_eval; its per-user
    positive-flag rows equal the generic path's (repeat_interleave over the catalogue +
    predict, ranked by sigmoid outputs) except where scores tie: at most 3 % of the users."""
    import recbole_amd.trainer.trainer as tt
    from recbole_amd.trainer import Trainer
    # 64 users per generic batch (the FULL loader takes eval_batch_size // n_items users)
    config, train, valid, test, model = _ml100k(tmp_path, eval_batch_size=64 * 1682)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'embedding' in name:
                p.normal_(0.0, 1.0)
    trainer = Trainer(config, model)
    calls, rows = [], []
    real = tt.fused_pair_full_sort_eval
    monkeypatch.setattr(tt, 'fused_pair_full_sort_eval',
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    topk = trainer.evaluator.topk_evaluator
    real_eval = topk.evaluate_pos_idx
    monkeypatch.setattr(topk, 'evaluate_pos_idx',
                        lambda pos_idx, pl: (rows.append(np.array(pos_idx)), real_eval(pos_idx, pl))[1])
    fused = trainer.evaluate(test, load_best_model=False)
    assert len(calls) == 1
    config['fused_eval'] = False
    generic = trainer.evaluate(test, load_best_model=False)
    assert len(calls) == 1 and len(rows) == 2
    differ = (rows[0] != rows[1]).any(axis=1).mean()
    print(f'users whose flag rows differ: {differ:.4f}; fused {fused} generic {generic}')
    assert rows[0].shape == rows[1].shape and rows[0].any() and differ <= 0.03
    config['fused_eval'] = True
    with torch.no_grad():                                # full_sort_predict = predict's values
        u = torch.arange(1, 4, device=config['device'])
        full = model.full_sort_predict({'user_id': u}).view(3, -1)
        it = torch.arange(model.n_items, device=config['device'])
        one = model.predict({'user_id': u[1:2].expand(model.n_items), 'item_id': it})
    torch.testing.assert_close(full[1], one, rtol=1e-4, atol=1e-6)


def test_run_recbole_neumf(tmp_path):
    """One epoch end to end at the default widths on the small synthetic data set: the
    pointwise loader, the deferred tables, the sampled (uni-N) validation through predict,
    the fused full-sort test evaluation."""
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.quick_start import run_recbole
    root = _write_dataset(str(tmp_path), 'synth', n_users=80, n_items=120, n_inter=3000)
    res = run_recbole(model='NeuMF', dataset='synth', config_dict={
        'data_path': root, 'epochs': 1, 'state': 'ERROR', 'train_batch_size': 512,
        'show_progress': False, 'checkpoint_dir': str(tmp_path / 'saved')})
    for part in ('best_valid_result', 'test_result'):
        assert res[part]
        for k, v in res[part].items():
            assert np.isfinite(v) and 0.0 <= v <= 1.0, (part, k, v)
