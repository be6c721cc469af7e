"""The draw specification of the transformer dropouts (tests/drop_spec.py) on its own, in
numpy: the streams of a 2-layer model's sites are independent across sites and steps under
the key rule splitmix64(splitmix64(seed) ^ c), and were not under the earlier
splitmix64(seed + c) (site s at counter c + 1 = site s + 1 at counter c, agreement 1.0);
the oracle's keeps argument leaves the dropout-0 computation unchanged."""
import itertools

import numpy as np
import torch

from tests import drop_spec as ds

INITIAL_SEED = 2020


def _agreements(masks):
    return [float((a == b).mean()) for a, b in itertools.combinations(masks, 2)]


def test_ln_streams_independent_and_parent_rule_was_not():
    n = 257 * 64
    seeds = [ds.ln_site_seed(INITIAL_SEED, s) for s in range(5)]
    pairs = [(s, c) for s in seeds for c in range(4)]
    for p, bound in ((0.5, 0.0115), (0.1, 0.0091)):
        want = p * p + (1 - p) ** 2
        assert len({int(ds.key(s, c)) for s, c in pairs}) == 20
        ag = _agreements([ds.ln_keep(s, c, n, p) for s, c in pairs])
        assert len(ag) == 190 and max(abs(a - want) for a in ag) <= bound
        # the earlier rule: 8 keys for the 20 (site, counter) pairs, identical masks
        assert len({int(ds.key_parent(s, c)) for s, c in pairs}) == 8
        a = ds.ln_keep(seeds[0], 1, n, p, ds.key_parent)
        b = ds.ln_keep(seeds[1], 0, n, p, ds.key_parent)
        assert float((a == b).mean()) == 1.0


def test_k9e_streams_independent_and_rate():
    B, H, L = 3, 2, 50
    seeds = [ds.attn_site_seed(INITIAL_SEED, l) for l in range(2)]
    pairs = [(s, c) for s in seeds for c in range(3)]
    assert len({int(ds.key(s, c)) for s, c in pairs}) == 6
    ag = _agreements([ds.attn_keep(s, c, B, H, L, 0.5) for s, c in pairs])
    assert max(abs(a - 0.5) for a in ag) <= 0.0115
    a = ds.attn_keep(seeds[0], 1, B, H, L, 0.5, ds.key_parent)
    b = ds.attn_keep(seeds[1], 0, B, H, L, 0.5, ds.key_parent)
    assert float((a == b).mean()) == 1.0
    m = ds.attn_keep((1 << 33) + 987654321, 5, B, H, L, 0.3)
    assert m.shape == (B, H, L, L) and abs(m.mean() - 0.7) <= 0.02


def test_site_seeds_distinct():
    s = ds.model_sites(INITIAL_SEED, 2)
    assert len(s) == 7 and len(set(s.values())) == 7
    assert ds.threshold(0.0) == 4294967295 and ds.threshold(0.5) == 1 << 31


def test_oracle_keeps_none_is_dropout_zero():
    """SASRecCPU with all-true masks and p = 0 computes what it computes with keeps=None,
    and a dropped site changes the result."""
    from oracle import cpu_ref
    torch.manual_seed(0)
    B, L, d, H = 5, 7, 16, 2
    ref = cpu_ref.SASRecCPU(30, L, d, 2, H, 32, 1e-12)
    seq = torch.randint(1, 30, (B, L))
    lens = torch.full((B,), L)
    ones = {'emb': np.ones((B, L, d), bool)}
    for l in range(2):
        ones.update({f'attn{l}': np.ones((B, H, L, L), bool), f'out{l}': np.ones((B, L, d), bool),
                     f'ffn{l}': np.ones((B, L, d), bool)})
    with torch.no_grad():
        a = ref(seq, lens)
        b = ref(seq, lens, keeps=ones, p_hidden=0.0, p_attn=0.0)
        assert torch.equal(a, b)
        for name in ones:
            k = dict(ones)
            k[name] = ds.ln_keep(7, 0, ones[name].size, 0.5).reshape(ones[name].shape)
            c = ref(seq, lens, keeps=k, p_hidden=0.5, p_attn=0.5)
            assert not torch.equal(a, c), name
