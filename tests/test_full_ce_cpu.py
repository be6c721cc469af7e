"""CPU guards for the fused full-catalogue cross entropy (K12): the `ce_kernel` config
key of SASRec (validation, and the library path everywhere K12 does not apply: a CPU
tensor never reaches a kernel) and the ctypes signature table against the prototypes of
include/mirec.h."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CE_SYMBOLS = ('mirec_full_ce_splits', 'mirec_full_ce_workspace_size', 'mirec_full_ce_fwd_f32',
              'mirec_full_ce_bwd_f32')


def _model(tmp_path, **over):
    from tests.test_gpu_e2e import _write_dataset
    from recbole_amd.config import Config
    from recbole_amd.data import create_dataset, data_preparation
    from recbole_amd.utils import get_model, init_seed
    root = _write_dataset(str(tmp_path), 'synth', n_users=40, n_items=60, n_inter=900)
    cd = {'model': 'SASRec', 'dataset': 'synth', 'data_path': root, 'use_gpu': False,
          'MAX_ITEM_LIST_LENGTH': 7, 'training_neg_sample_num': 0, 'loss_type': 'CE',
          'hidden_dropout_prob': 0.0, 'attn_dropout_prob': 0.0, 'train_batch_size': 64,
          'load_col': {'inter': ['user_id', 'item_id', 'timestamp']}}
    cd.update(over)
    config = Config(config_dict=cd)
    init_seed(config['seed'], config['reproducibility'])
    ds = create_dataset(config)
    train, _, _ = data_preparation(config, ds)
    return get_model('SASRec')(config, train), train


def test_bogus_ce_kernel_raises(tmp_path):
    with pytest.raises(ValueError, match='ce_kernel'):
        _model(tmp_path, ce_kernel='bogus')


def test_cpu_model_takes_the_library_path_for_every_setting(tmp_path):
    """Key absent, 'library' and 'fused' on a CPU-device SASRec: the same CE loss on one
    batch, exactly (K12 is GPU-only, so all three are the library matmul + CrossEntropyLoss).
    The model's encoder starts with a GPU-only kernel (K9a), so the sequence
    representation comes from a torch stand-in (the mean of the sequence's item rows):
    what is under test is the loss path calculate_loss takes behind it."""
    losses, grads = [], []
    for k, over in enumerate(({}, {'ce_kernel': 'library'}, {'ce_kernel': 'fused'})):
        model, train = _model(tmp_path / str(k), **over)
        assert model.ce_kernel == over.get('ce_kernel', 'library')
        assert model.graph_step_safe
        assert model.deferred_tables() == []
        model.forward = lambda seq, n, m=model: m.item_embedding(seq).mean(1)
        loss = model.calculate_loss(next(iter(train)))
        loss.backward()
        assert type(loss.grad_fn).__name__ == 'NllLossBackward0'
        losses.append(loss.detach().clone())
        grads.append(model.item_embedding.weight.grad.clone())
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2])
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    assert torch.isfinite(losses[0]) and losses[0] > 0


def _header_prototypes():
    """{name: (return type, [argument declarations])} of every function include/mirec.h
    declares whose name is in CE_SYMBOLS, parsed from the header text."""
    text = open(os.path.join(ROOT, 'include', 'mirec.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    out = {}
    for m in re.finditer(r'([A-Za-z_0-9]+)\s+(mirec_full_ce_\w+)\s*\(([^)]*)\)\s*;', text):
        args = [a.strip() for a in m.group(3).split(',') if a.strip() and a.strip() != 'void']
        out[m.group(2)] = (m.group(1), args)
    return out


def test_signature_table_matches_the_header():
    import ctypes

    from recbole_amd import _native
    protos = _header_prototypes()
    assert set(protos) == set(CE_SYMBOLS)
    kinds = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'size_t': ctypes.c_size_t,
             'int': ctypes.c_int}
    for name in CE_SYMBOLS:
        res, args = _native.SIGNATURES[name]
        ret, decl = protos[name]
        assert len(args) == len(decl), name
        assert res is kinds[ret], name
        for a, dcl in zip(args, decl):
            if '*' in dcl:
                assert a is ctypes.c_void_p, (name, dcl)
            else:
                assert a is kinds[dcl.split()[-2]], (name, dcl)
