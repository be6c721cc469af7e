"""bench.py --dump-outputs (CPU): the arrays written are float32, stay inside the byte budget,
a table that does not fit is a fixed seeded sample of its rows (the same rows on every call),
a table that fits is whole, and the losses are those of the timed steps only."""
import os
import types

import numpy as np
import torch

import bench


def _step(nU=1000, nI=50, d=8, nb=40):
    g = torch.Generator().manual_seed(3)
    return types.SimpleNamespace(pU=torch.nn.Parameter(torch.randn(nU, d, generator=g)),
                                 pI=torch.nn.Parameter(torch.randn(nI, d, generator=g)),
                                 loss_hist=torch.rand(nb, generator=g))


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    step = _step()
    budget = 300 * 8 * 4                      # the item table (50 rows) + 250 user rows
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', budget)
    W, K = 5, 20
    bench.dump_outputs(str(tmp_path / 'a'), step, W, K)
    bench.dump_outputs(str(tmp_path / 'b'), step, W, K)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['item_embedding.npy', 'loss.npy', 'user_embedding.npy']
    got = {n: np.load(tmp_path / 'a' / n) for n in names}
    for n in names:
        assert got[n].dtype == np.float32
        assert np.array_equal(got[n], np.load(tmp_path / 'b' / n))
    assert got['item_embedding.npy'].nbytes + got['user_embedding.npy'].nbytes <= budget
    assert np.array_equal(got['item_embedding.npy'], step.pI.detach().numpy())
    assert np.array_equal(got['loss.npy'], step.loss_hist[W:W + K].numpy())
    # the sample: 250 distinct rows of the user table, ascending
    U = step.pU.detach().numpy()
    S = got['user_embedding.npy']
    assert S.shape == (250, 8)
    rows = [int(np.flatnonzero((U == r).all(axis=1))[0]) for r in S]
    assert rows == sorted(set(rows))


def test_dump_outputs_whole_tables_when_they_fit(tmp_path):
    step = _step()
    bench.dump_outputs(str(tmp_path), step, 0, 40)
    assert np.array_equal(np.load(tmp_path / 'user_embedding.npy'), step.pU.detach().numpy())
    assert np.array_equal(np.load(tmp_path / 'item_embedding.npy'), step.pI.detach().numpy())
    assert np.load(tmp_path / 'loss.npy').shape == (40,)
