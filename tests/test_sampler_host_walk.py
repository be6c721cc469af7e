"""The sampler's host walk (Sampler._host_walk: what a use_gpu: False run takes on a machine
without any GPU) against the oracle's C restatement of K4's rule: the same values, the same
walk pointer, over successive calls, with and without rejection."""
import numpy as np
import pytest

from oracle import cpu_ref


def _bare_sampler(rl, n_users, n_items, csr):
    from recbole_amd.sampler import Sampler
    s = Sampler.__new__(Sampler)
    s.random_list, s.random_list_length = rl, len(rl)
    s.n_users, s.n_items = n_users, n_items
    s.phase, s.used_csr = 'train', {'train': csr}
    s.device = s._rl_dev = s._pr_dev = None
    s._pr_host = 0
    return s


@pytest.mark.parametrize('reject', [True, False])
def test_host_walk_equals_the_c_walk(reject):
    rng = np.random.default_rng(7)
    nU, nI, T = 50, 90, 3
    u, i = rng.integers(0, nU, 1500), rng.integers(1, nI, 1500)
    ptr, cols = cpu_ref.used_csr(nU, u, i)
    rl = rng.permutation(np.arange(1, nI))
    s = _bare_sampler(rl, nU, nI, (ptr, cols))
    if not reject:
        s._used_host = lambda: None
    pr = 0
    for n_keys in (37, 1, 64):                       # the pointer carries over between calls
        keys = rng.integers(0, nU, n_keys)
        want, pr = cpu_ref.c_sample_walk(rl, pr, keys, T, ptr, cols, nU, reject)
        got = s._host_walk(keys, T)
        assert np.array_equal(got.numpy(), want)
        assert s.random_pr == pr
    with pytest.raises(ValueError, match='out of range'):
        s._host_walk(np.array([nU]), 1)
