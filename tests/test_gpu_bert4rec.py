"""BERT4Rec on the GPU (K17, csrc/cloze.hip; K12 over gathered rows, csrc/xent.hip; the
bidirectional mask, csrc/seq.hip; model/sequential_recommender/bert4rec.py).

K17a / K17b / K17c and the mask are checked bit for bit against their restatements
(tests/cloze_spec.py, torch.where, the reference's mask formula). K12 over rows is checked
against float64 torch with K12's tolerances (tests/test_gpu_full_ce.py): loss rtol 1e-4;
gradients rtol 1e-4, atol 1e-6 — and against K12 itself on the identity row list: forward
bit for bit, backward bit for bit for K12's incoming gradient g = B (its factor g / B is then
exactly 1, the rows entry's factor for g = 1), and for a power-of-two B also K12's g = 1
outputs times B. The model is compared with a float64 CPU copy of itself (the reference's
op sequence) fed the same masked tensors."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import cloze_spec

pytestmark = pytest.mark.gpu

SEED = 0x5EED0BE27


def _sequences(rng, B, L, n_items):
    """Right-padded rows; lengths 0, 1 and L among the first three."""
    seq = np.zeros((B, L), dtype=np.int64)
    lens = rng.integers(0, L + 1, B)
    lens[:3] = (0, 1, L)[:min(3, B)]
    if B == 1:
        lens[0] = L
    for b, n in enumerate(lens):
        seq[b, :n] = rng.integers(1, n_items, n)
    return seq


# ------------------------------------------------------------------ K17a / K17b
@pytest.mark.parametrize('ratio', [0.2, 0.9])
@pytest.mark.parametrize('B,L,M', [(1, 1, 1), (3, 7, 1), (5, 50, 10), (130, 64, 12)])
def test_cloze_mask_and_compact_match_the_spec(dev, B, L, M, ratio):
    from recbole_amd import ops
    n_items = 90
    rng = np.random.default_rng(1000 * B + L)
    seq = _sequences(rng, B, L, n_items)
    c0 = 5
    want = cloze_spec.cloze_mask(seq, M, n_items, ratio, SEED, c0)
    if B == 130:            # the cases the issue names occur in the spec's own output
        masked = cloze_spec.mask_decisions(seq, ratio, SEED, c0)
        live = (seq > 0).sum(1) > 0
        assert masked[:, 0].any()
        if ratio == 0.9:
            assert (masked.sum(1) > M).any()
        else:
            assert (masked[live].sum(1) == 0).any()
    seq_d = torch.as_tensor(seq, device=dev)
    counter = torch.full((1,), c0, dtype=torch.int64, device=dev)
    got = ops.cloze_mask(seq_d, M, n_items, ratio, SEED, counter)
    assert int(counter.item()) == c0                      # the kernel only reads it
    for g, w, name in zip(got, want, ('masked_seq', 'pos_items', 'neg_items', 'masked_index')):
        assert np.array_equal(g.cpu().numpy(), w), name
    # without negatives: the other three unchanged
    got3 = ops.cloze_mask(seq_d, M, n_items, ratio, SEED, counter, negatives=False)
    assert got3[2] is None
    for k in (0, 1, 3):
        assert torch.equal(got3[k], got[k])
    # the next draw differs (where anything can be masked at all)
    counter.add_(1)
    nxt = ops.cloze_mask(seq_d, M, n_items, ratio, SEED, counter)
    want_nxt = cloze_spec.cloze_mask(seq, M, n_items, ratio, SEED, c0 + 1)
    for g, w in zip(nxt, want_nxt):
        assert np.array_equal(g.cpu().numpy(), w)
    if B >= 5:
        assert not torch.equal(nxt[0], got[0])
    # K17b
    act_row, act_target, n_act, slot_of = ops.cloze_compact(got[3], got[1], L)
    w_row, w_target, w_n, w_slot = cloze_spec.compact(want[3], want[1], L)
    assert int(n_act.item()) == w_n
    assert np.array_equal(act_row.cpu().numpy(), w_row)
    assert np.array_equal(act_target.cpu().numpy(), w_target)
    assert np.array_equal(slot_of.cpu().numpy(), w_slot)


def test_cloze_host_checks(dev):
    from recbole_amd import ops
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    seq = torch.ones(2, 7, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match='negative'):
        ops.cloze_mask(seq, 2, 8, 0.2, 1, counter)         # n_items - 1 = 7 <= L
    with pytest.raises(ValueError, match='M'):
        ops.cloze_mask(seq, 0, 90, 0.2, 1, counter)


# ------------------------------------------------------------------ K17c
@pytest.mark.parametrize('n_pos,d,R', [(1, 32, 1), (250, 64, 37), (333, 128, 50), (77, 256, 5)])
def test_rows_from_slots_is_torch_where(dev, n_pos, d, R):
    from recbole_amd import ops
    g = torch.Generator().manual_seed(n_pos)
    gS = torch.randn(R, d, generator=g).to(dev)
    slot_of = torch.full((n_pos,), -1, dtype=torch.int32)
    pick = torch.randperm(n_pos, generator=g)[:min(R, n_pos)]
    slot_of[pick] = torch.randperm(R, generator=g)[:len(pick)].to(torch.int32)
    slot_of = slot_of.to(dev)
    got = ops.rows_from_slots(gS, slot_of)
    want = torch.where((slot_of >= 0).unsqueeze(1), gS[slot_of.clamp_min(0).long()],
                       torch.zeros((), device=dev))
    assert got.shape == (n_pos, d) and torch.equal(got, want)
    assert not torch.signbit(got[slot_of < 0]).any()       # exact +0


# ------------------------------------------------------------------ the bidirectional mask
@pytest.mark.parametrize('L', [1, 50, 51, 64])
def test_bidirectional_mask_is_the_reference_formula(dev, L):
    from recbole_amd._native import check, lib, ptr, stream_handle
    B = 7
    rng = np.random.default_rng(L)
    seq = torch.as_tensor(_sequences(rng, B, L, 50), device=dev)
    seq[B - 1, L // 2] = 0                                 # an interior padding item too
    got = torch.empty(B, 1, L, L, dtype=torch.float32, device=dev)
    check(lib().mirec_seq_attn_mask_bidir_f32(ptr(seq), B, L, ptr(got), stream_handle()),
          'mirec_seq_attn_mask_bidir_f32')
    ext = (seq > 0).long().unsqueeze(1).unsqueeze(2).to(dtype=torch.float32)
    want = ((1.0 - ext) * -10000.0).expand(B, 1, L, L)
    assert torch.equal(got, want)
    assert torch.equal(torch.signbit(got), torch.signbit(want))     # -0.0 where allowed


# ------------------------------------------------------------------ K12 over gathered rows
ROW_SHAPES = ((1, 1, 31), (1, 0, 31), (33, 33, 65), (257, 129, 1000), (257, 130, 2049),
              (257, 257, 2049))
WIDTHS = (32, 64, 128, 256)


@functools.lru_cache(maxsize=None)
def _rows_case(R, n_act, I, d):
    """Inputs (CPU) and the float64 reference, computed once per shape, read-only."""
    g = torch.Generator().manual_seed(1000 * d + 7 * R + n_act + I)
    n_x = R + 9
    X = torch.randn(n_x, d, generator=g) * 0.3
    E = torch.randn(I, d, generator=g) * 0.3
    row = torch.randint(0, n_x, (R,), generator=g)
    row[0] = n_x - 1                                       # the last row of X
    if R > 2:
        row[2] = row[0]                                    # a repeat
        row[R - 1] = row[1]
    target = torch.randint(0, I, (R,), generator=g)
    target[0] = I - 1
    if R > 1:
        target[1] = 0
    gscale = 1.0 / max(n_act, 1)
    return X, E, row, target, gscale, cloze_spec.rows_ce64(X, row, target, E, n_act, gscale)


@pytest.mark.parametrize('splits', [1, 2, 7])
@pytest.mark.parametrize('R,n_act,I', ROW_SHAPES)
@pytest.mark.parametrize('d', WIDTHS)
def test_rows_ce_matches_float64(dev, d, R, n_act, I, splits):
    from recbole_amd import ops
    X, E, row, target, gscale, (w_loss, w_gS, w_dE) = _rows_case(R, n_act, I, d)
    Xd, Ed, rd, td = X.to(dev), E.to(dev), row.to(dev), target.to(dev)
    n_dev = torch.full((1,), n_act, dtype=torch.int32, device=dev)
    lse, loss_rows = ops.full_ce_rows_fwd(Xd, rd, td, Ed, n_dev, splits)
    g = torch.full((1,), gscale, dtype=torch.float32, device=dev)
    gS, dE = ops.full_ce_rows_bwd(Xd, rd, td, Ed, lse, g, n_dev, splits)
    for t in (lse, loss_rows, gS, dE):
        assert torch.isfinite(t).all()
    print(f'd={d} R={R} n_act={n_act} I={I} splits={splits}: '
          f'loss err {(loss_rows.cpu().double() - w_loss).abs().max():.3e} '
          f'gS err {(gS.cpu().double() - w_gS).abs().max():.3e} '
          f'dE err {(dE.cpu().double() - w_dE).abs().max():.3e}')
    assert (loss_rows[n_act:] == 0).all() and (lse[n_act:] == 0).all()
    assert (gS[n_act:] == 0).all()
    torch.testing.assert_close(loss_rows.cpu().double(), w_loss, rtol=1e-4, atol=0)
    torch.testing.assert_close(gS.cpu().double(), w_gS, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dE.cpu().double(), w_dE, rtol=1e-4, atol=1e-6)
    if n_act == R:                 # a null count means all R
        lse2, loss2 = ops.full_ce_rows_fwd(Xd, rd, td, Ed, None, splits)
        gS2, dE2 = ops.full_ce_rows_bwd(Xd, rd, td, Ed, lse2, g, None, splits)
        for a, b in ((lse2, lse), (loss2, loss_rows), (gS2, gS), (dE2, dE)):
            assert torch.equal(a, b)


@pytest.mark.parametrize('splits', [1, 2, 7])
@pytest.mark.parametrize('B,I', [(33, 65), (128, 1000), (257, 2049)])
@pytest.mark.parametrize('d', WIDTHS)
def test_identity_rows_reproduce_k12(dev, d, B, I, splits):
    """row = arange(B), no count: K12's lse and loss_rows bit for bit; its gS and dE bit for
    bit where K12's own factor g / B is exactly 1 (g = B), which is the rows entry's factor
    for g = 1; for a power-of-two B also K12(g = 1) * B; otherwise K12(g = 1) * B within
    K12's tolerances (K12 rounds each softmax weight times fl(1 / B) once more)."""
    from recbole_amd import ops
    g_ = torch.Generator().manual_seed(d + B + I)
    S = (torch.randn(B, d, generator=g_) * 0.3).to(dev)
    E = (torch.randn(I, d, generator=g_) * 0.3).to(dev)
    t = torch.randint(0, I, (B,), generator=g_).to(dev)
    row = torch.arange(B, device=dev)
    one = torch.ones(1, device=dev)
    lse, loss_rows = ops.full_ce_fwd(S, E, t, splits)
    lse_r, loss_r = ops.full_ce_rows_fwd(S, row, t, E, None, splits)
    assert torch.equal(lse_r, lse) and torch.equal(loss_r, loss_rows)
    gS_r, dE_r = ops.full_ce_rows_bwd(S, row, t, E, lse, one, None, splits)
    gS_b, dE_b = ops.full_ce_bwd(S, E, t, lse, one * B, splits)
    assert torch.equal(gS_r, gS_b) and torch.equal(dE_r, dE_b)
    gS_1, dE_1 = ops.full_ce_bwd(S, E, t, lse, one, splits)
    if B & (B - 1) == 0:
        assert torch.equal(gS_r, gS_1 * B) and torch.equal(dE_r, dE_1 * B)
    else:
        torch.testing.assert_close(gS_r, gS_1 * B, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(dE_r, dE_1 * B, rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------ the model
def _stub_model(dev, hidden, heads, ce_kernel='fused', n_items=300, L=50, drop=0.0,
                loss_type='CE', seed=2020):
    from recbole_amd.config import Config
    from recbole_amd.model.sequential_recommender import BERT4Rec
    from recbole_amd.utils import FeatureType

    class _DS:
        field2type = {'item_id': FeatureType.TOKEN}

        def fields(self, *a, **k):
            return list(self.field2type)

        def num(self, f):
            return n_items
    config = Config(model='BERT4Rec', dataset='stub', config_dict={
        'hidden_size': hidden, 'n_heads': heads, 'inner_size': 2 * hidden,
        'MAX_ITEM_LIST_LENGTH': L, 'hidden_dropout_prob': drop, 'attn_dropout_prob': drop,
        'loss_type': loss_type, 'ce_kernel': ce_kernel, 'state': 'ERROR', 'load_col': None,
        'training_neg_sample_num': 0})
    config['device'] = dev
    torch.manual_seed(seed)
    return BERT4Rec(config, _DS()).to(dev)


@functools.lru_cache(maxsize=None)
def _model_case(hidden, heads):
    """Batch (CPU), the masked tensors of draw 0 from the spec, and the float64 reference
    (loss and the compared gradients) of a CPU double copy of the seeded model."""
    B, L, n_items = 5, 50, 300
    rng = np.random.default_rng(hidden)
    seq = _sequences(rng, B, L, n_items)
    seq[3] = rng.integers(1, n_items, L)
    model = _stub_model(torch.device('cpu'), hidden, heads, 'library')
    state = copy.deepcopy(model.state_dict())
    ref = model.double()
    from tests import drop_spec
    from recbole_amd.model.sequential_recommender.bert4rec import CLOZE_SITE
    seed = drop_spec.site_seed(2020, CLOZE_SITE)       # layers.site_seed after manual_seed(2020)
    masked_seq, pos, _, idx = cloze_spec.cloze_mask(seq, ref.mask_item_length, n_items,
                                                    ref.mask_ratio, seed, 0, negatives=False)
    assert (idx > 0).sum() > 0 and (masked_seq[:, 0] == n_items).any()
    out = ref.forward(torch.as_tensor(masked_seq))
    loss = cloze_spec.ce_loss64(out, ref.item_embedding.weight, torch.as_tensor(pos),
                                torch.as_tensor(idx), n_items)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in ref.named_parameters()}
    return seq, state, loss.item(), grads


COMPARED = ('item_embedding.weight', 'position_embedding.weight',
            'trm_encoder.layer.0.feed_forward.dense_1.weight')


@pytest.mark.parametrize('hidden,heads', [(64, 1), (128, 2)])
def test_model_loss_and_gradients(dev, hidden, heads):
    seq, state, w_loss, w_grads = _model_case(hidden, heads)
    inter = {'item_id_list': torch.as_tensor(seq, device=dev)}
    res = {}
    for kernel in ('fused', 'library'):
        torch.manual_seed(2020)                 # the Cloze seed comes from the device generator
        model = _stub_model(dev, hidden, heads, kernel)
        model.load_state_dict(state)
        from tests import drop_spec
        assert model._cloze_state(dev)[0] == drop_spec.site_seed(2020, 0x3000)
        loss = model.calculate_loss(inter)
        want_fn = '_ClozeCEFnBackward' if kernel == 'fused' else 'DivBackward0'
        assert type(loss.grad_fn).__name__ == want_fn
        loss.backward()
        res[kernel] = (loss.item(), {n: p.grad for n, p in model.named_parameters()})
        print(f'{kernel}: loss {loss.item():.7f} (float64 {w_loss:.7f})')
        np.testing.assert_allclose(loss.item(), w_loss, rtol=1e-4)
        for n in COMPARED:
            torch.testing.assert_close(res[kernel][1][n].cpu().double(), w_grads[n], rtol=1e-4,
                                       atol=1e-6, msg=lambda m, n=n: f'{kernel} {n}: {m}')
    np.testing.assert_allclose(res['fused'][0], res['library'][0], rtol=1e-4)
    for n in COMPARED:
        torch.testing.assert_close(res['fused'][1][n], res['library'][1][n], rtol=1e-4,
                                   atol=1e-6, msg=lambda m, n=n: f'fused vs library {n}: {m}')
    # the CE side gives the mask token's row nothing: its gradient is the embedding side's,
    # which the float64 reference holds; the loss rows never see row n_items as an item
    from recbole_amd import ops
    from recbole_amd.model.sequential_recommender.bert4rec import _ClozeCEFn
    model = _stub_model(dev, hidden, heads, 'fused')
    X = torch.randn(5 * 50, hidden, device=dev).requires_grad_()
    W = model.item_embedding.weight
    idx = torch.zeros(5, 10, dtype=torch.int64, device=dev)
    idx[:, -3:] = torch.tensor([4, 9, 30], device=dev)
    pos = torch.randint(1, 300, (5, 10), device=dev)
    _ClozeCEFn.apply(X, W, *ops.cloze_compact(idx, pos, 50), 300).backward()
    assert (W.grad[300] == 0).all() and W.grad[:300].abs().sum() > 0


def test_full_sort_predict_matches_torch(dev):
    """L + 1 = 51 positions through K9a / K9e / the MFMA score matrix against the float64
    CPU copy's torch path; predict reads the same scores."""
    model = _stub_model(dev, 64, 1).eval()
    ref = copy.deepcopy(model).cpu().double().eval()
    rng = np.random.default_rng(3)
    seq = _sequences(rng, 6, 50, 300)
    lens = np.maximum((seq > 0).sum(1), 1)
    seq[0, 0] = 7                                # the empty row gets one item (length >= 1)
    inter = {'item_id_list': torch.as_tensor(seq), 'item_length': torch.as_tensor(lens),
             'item_id': torch.as_tensor(rng.integers(1, 300, 6))}
    with torch.no_grad():
        want = ref.full_sort_predict(inter)
        on = {k: v.to(dev) for k, v in inter.items()}
        got = model.full_sort_predict(on)
        one = model.predict(on)
    assert got.shape == (6, 300)
    torch.testing.assert_close(got.cpu().double(), want, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(one.cpu().double(), want.gather(1, inter['item_id'].view(-1, 1))
                               .view(-1), rtol=1e-4, atol=1e-5)


def test_no_loss_row_gives_nan(dev):
    model = _stub_model(dev, 64, 1)
    inter = {'item_id_list': torch.zeros(3, 50, dtype=torch.int64, device=dev)}
    loss = model.calculate_loss(inter)
    assert torch.isnan(loss)


# ------------------------------------------------------------------ training and evaluation
def test_training_step_with_dropout_and_fused_evaluation(tmp_path):
    """Adam steps with both dropouts at 0.5 stay finite and advance the Cloze counter; one
    pass of the fused K6 evaluator returns the generic full_sort_predict sequence's top-K
    metrics on an ml-100k-sized synthetic data set."""
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.trainer import Trainer
    from recbole_amd.utils import get_model, init_seed
    root = _write_dataset(str(tmp_path), 'synth', n_users=943, n_items=1682, n_inter=20000)
    config = Config(config_dict={
        'model': 'BERT4Rec', 'dataset': 'synth', 'data_path': root, 'epochs': 1,
        'load_col': {'inter': ['user_id', 'item_id', 'timestamp']}, 'ce_kernel': 'fused',
        'train_batch_size': 512, 'checkpoint_dir': str(tmp_path / 'saved'),
        'training_neg_sample_num': 0})
    init_seed(config['seed'], config['reproducibility'])
    train, valid, test = data_preparation(config, create_dataset(config))
    model = get_model('BERT4Rec')(config, train).to(config['device'])
    assert model.hidden_dropout_prob == 0.5 and model.attn_dropout_prob == 0.5
    trainer = Trainer(config, model)
    assert not trainer._graph_step_applicable()
    model.train()
    losses = []
    for b in list(train)[:3]:
        trainer.optimizer.zero_grad()
        loss = model.calculate_loss(b.to(config['device']))
        assert type(loss.grad_fn).__name__ == '_ClozeCEFnBackward'
        loss.backward()
        trainer.optimizer.step()
        losses.append(loss.item())
    assert np.isfinite(losses).all()
    assert int(model._cloze_rng[1].item()) == 3
    for p in model.parameters():
        assert torch.isfinite(p).all()
    fused = trainer.evaluate(test, load_best_model=False)
    config['fused_eval'] = False
    generic = trainer.evaluate(test, load_best_model=False)
    assert set(fused) == set(generic)
    for k in fused:
        assert fused[k] == pytest.approx(generic[k], abs=2e-4), k


@pytest.mark.parametrize('ce_kernel', ['fused', 'library'])
def test_run_recbole_bert4rec(tmp_path, ce_kernel):
    """One epoch end to end through run_recbole with the default dropouts (the model does
    not offer its step for capture: train_graph's default changes nothing)."""
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.quick_start import run_recbole
    root = _write_dataset(str(tmp_path), 'synth', n_users=80, n_items=120, n_inter=3000)
    cd = {'data_path': root, 'epochs': 1, 'checkpoint_dir': str(tmp_path / 'saved'),
          'load_col': {'inter': ['user_id', 'item_id', 'timestamp']}, 'show_progress': False,
          'MAX_ITEM_LIST_LENGTH': 12, 'training_neg_sample_num': 0, 'ce_kernel': ce_kernel}
    res = run_recbole(model='BERT4Rec', dataset='synth', config_dict=cd)
    for part in ('best_valid_result', 'test_result'):
        for k, v in res[part].items():
            assert 0.0 <= v <= 1.0, (part, k, v)
