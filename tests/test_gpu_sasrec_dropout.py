"""SASRec training with dropout on (the C3 path: K9a with the embedding dropout, K9e with
the attention dropout, K9d with the hidden dropouts) against the oracle's torch-CPU
restatement with the same masks: each site's keep mask is built from the numpy restatement
of the draw rule (tests/drop_spec.py) and the (seed, counter) read from the GPU model
before the step, and the oracle applies it where the reference applies dropout
(sasrec.py:107-114, layers.py:338-461). Head size 64 (K9e applies), odd L = 13, p = 0.5 at
every site. Tolerances are those of the dropout-0 tests (test_gpu_sasrec.py): loss 1e-4
relative, gradients 1e-4 relative + 1e-6 absolute, parameters after Adam steps 1e-3
relative + 2e-5 absolute."""
import numpy as np
import pytest
import torch

from tests import drop_spec
from tests.test_gpu_sasrec import _oracle, _pipeline

pytestmark = pytest.mark.gpu

P_HIDDEN = P_ATTN = 0.5
SHAPE = dict(hidden_size=128, n_heads=2, inner_size=256, n_layers=2, MAX_ITEM_LIST_LENGTH=13,
             hidden_dropout_prob=P_HIDDEN, attn_dropout_prob=P_ATTN, train_batch_size=96)


def _sites(model):
    """{site name: (seed, device counter, ...)} of the model's dropout sites, the names of
    the oracle's keeps."""
    from recbole_amd.model import layers
    dev = model.item_embedding.weight.device
    s = {'emb': layers._drop_rng(model.dropout, dev)}
    for l, lm in enumerate(model.trm_encoder.layer):
        mha = lm.multi_head_attention
        s[f'attn{l}'] = mha._k9e_rng(dev)
        s[f'out{l}'] = layers._drop_rng(mha.out_dropout, dev)
        s[f'ffn{l}'] = layers._drop_rng(lm.feed_forward.dropout, dev)
    return s


def _keeps(model, sites, B):
    """The specification's masks for the draw each site makes next."""
    L, d, H = model.max_seq_length, model.hidden_size, model.n_heads
    keeps = {}
    for name, rng in sites.items():
        seed, c = rng[0], int(rng[1].item())
        if name.startswith('attn'):
            keeps[name] = drop_spec.attn_keep(seed, c, B, H, L, P_ATTN)
        else:
            keeps[name] = drop_spec.ln_keep(seed, c, B * L * d, P_HIDDEN).reshape(B, L, d)
    return keeps


def _counters(sites):
    return {name: int(rng[1].item()) for name, rng in sites.items()}


def _ref_loss(ref, b, keeps, loss_type='CE'):
    c = {k: v.cpu() for k, v in b.interaction.items()}
    return ref.calculate_loss(c['item_id_list'], c['item_length'], c['item_id'],
                              c.get('neg_item_id'), loss_type, keeps=keeps,
                              p_hidden=P_HIDDEN, p_attn=P_ATTN)


def test_site_seeds_follow_the_spec(tmp_path):
    """The model's per-site seeds are drop_spec's seed rule of the device generator's
    initial seed (the configured seed), all seven distinct (LN sites against K9e sites
    included)."""
    config, train, valid, test, model = _pipeline(tmp_path, **SHAPE)
    sites = _sites(model)
    dev = model.item_embedding.weight.device
    initial = torch.cuda.default_generators[dev.index or 0].initial_seed()
    assert initial == config['seed']
    assert {k: v[0] for k, v in sites.items()} == drop_spec.model_sites(initial, 2)
    assert len({v[0] for v in sites.values()}) == 7


@pytest.mark.parametrize('loss_type,neg', [('CE', 0), ('BPR', 1), ('SSM', 20)])
def test_loss_and_grads_match_oracle_with_dropout(tmp_path, loss_type, neg):
    config, train, valid, test, model = _pipeline(tmp_path, loss_type=loss_type,
                                                  training_neg_sample_num=neg, **SHAPE)
    model.train()
    ref = _oracle(model)
    sites = _sites(model)
    b = next(iter(train))
    assert b['item_id_list'].shape == (96, 13)
    keeps = _keeps(model, sites, 96)
    assert set(_counters(sites).values()) == {0}
    loss = model.calculate_loss(b)
    loss.backward()
    # every dropout ran folded into its kernel: one draw per site, advanced by the backward
    assert set(_counters(sites).values()) == {1}, _counters(sites)
    lr_ = _ref_loss(ref, b, keeps, loss_type)
    lr_.backward()
    print(f'loss gpu {loss.item():.8f} oracle {lr_.item():.8f}')
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        print(f'{name}: max |grad diff| {(p.grad.cpu() - refp[name].grad).abs().max().item():.3e}'
              f' of max |grad| {refp[name].grad.abs().max().item():.3e}')
    np.testing.assert_allclose(loss.item(), lr_.item(), rtol=1e-4)
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.grad.cpu(), refp[name].grad, rtol=1e-4, atol=1e-6,
                                   msg=name)


def test_three_adam_steps_match_oracle_with_dropout(tmp_path):
    """Three steps through the Trainer's optimizer against torch optim.Adam on the oracle
    with the masks of counters 0, 1 and 2: every site's counter advances by one per real
    training step, and the parameters agree afterwards."""
    from recbole_amd.trainer import Trainer
    config, train, valid, test, model = _pipeline(tmp_path, **SHAPE)
    model.train()
    ref = _oracle(model)
    opt = torch.optim.Adam(ref.parameters(), lr=config['learning_rate'])
    trainer = Trainer(config, model)
    sites = _sites(model)
    for step, b in enumerate(list(train)[:3]):
        assert set(_counters(sites).values()) == {step}, (step, _counters(sites))
        keeps = _keeps(model, sites, b['item_id_list'].shape[0])
        trainer.optimizer.zero_grad()
        loss = model.calculate_loss(b)
        loss.backward()
        trainer.optimizer.step()
        opt.zero_grad()
        lr_ = _ref_loss(ref, b, keeps)
        lr_.backward()
        opt.step()
        print(f'step {step}: loss gpu {loss.item():.8f} oracle {lr_.item():.8f}')
        np.testing.assert_allclose(loss.item(), lr_.item(), rtol=1e-4)
    trainer.optimizer.flush()
    assert set(_counters(sites).values()) == {3}
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        torch.testing.assert_close(p.detach().cpu(), refp[name].detach(), rtol=1e-3, atol=2e-5,
                                   msg=name)


def test_same_seed_same_masks_in_one_process(tmp_path):
    """Two models built one after the other from the same seed draw the same masks: their
    first training losses are bitwise equal (site words come from the position in the
    model, not from how many modules the process has built)."""
    losses = []
    for sub in ('a', 'b'):
        config, train, valid, test, model = _pipeline(tmp_path / sub, **SHAPE)
        model.train()
        loss = model.calculate_loss(next(iter(train)))
        losses.append(loss.detach().cpu())
    assert torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32)), losses
