"""numpy restatement of the transformer dropout draws — K9a / K9d (csrc/seq.hip header of
K9d) and K9e (csrc/attn.hip header) — and of the per-site seeds (model/layers.py
site_seed, assign_drop_sites; SASRec.__init__): the specification the GPU masks are
checked against. Test infrastructure only.

    key  = splitmix64(splitmix64(seed) ^ c)        c: the site's device counter at the forward
    thr  = min(2^32 - 1, ldexp(1 - p, 32))         keep iff the 32-bit draw < thr
    LN   element e = row * d + column: half e & 1 of splitmix64(key ^ (e >> 1))
    K9e  element (b, h, i, j): x = splitmix64(key ^ (((b H + h) 64 + (i & ~1)) 64 + j)),
         low 32 bits for an even row i, high 32 bits for an odd one
    seed = (initial_seed * 0x85EBCA6B + word) mod 2^64, word = 0x1000 + LN site or
         0x2000 + layer (K9e); LN sites of a model: 0 the embedding dropout, 1 + 2 l layer
         l's attention-output dropout, 2 + 2 l its feed-forward dropout
"""
import numpy as np

_M = (1 << 64) - 1
_U = np.uint64


def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def key(seed, c):
    """The key of the draw that read counter value c: the seed and the counter enter
    separately."""
    return splitmix64(splitmix64(_U(seed & _M)) ^ _U(c & _M))


def key_parent(seed, c):
    """The rule before the fix, splitmix64(seed + c): kept to show what it did (site s at
    counter c + 1 has the key of the site with seed + 1 at counter c)."""
    return splitmix64(_U((seed + c) & _M))


def threshold(p):
    return min(4294967295, int(np.ldexp(1.0 - p, 32)))


def ln_keep(seed, c, n_elems, p, key_fn=key):
    """[n_elems] bool keep flags of an LN site (K9a / K9d), element e = row * d + column."""
    k = key_fn(seed, c)
    e = np.arange(n_elems, dtype=np.uint64)
    h = splitmix64(k ^ (e >> _U(1)))
    half = np.where((e & _U(1)) == 1, h >> _U(32), h & _U(0xFFFFFFFF))
    return half < _U(threshold(p))


def attn_keep(seed, c, B, H, L, p, key_fn=key):
    """[B, H, L, L] bool keep flags of K9e's attention dropout."""
    k = key_fn(seed, c)
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    i = np.arange(L, dtype=np.uint64)[None, :, None]
    j = np.arange(L, dtype=np.uint64)[None, None, :]
    x = splitmix64(k ^ ((bh * _U(64) + (i & ~_U(1))) * _U(64) + j))
    half = np.where((i & _U(1)) == 1, x >> _U(32), x & _U(0xFFFFFFFF))
    return (half < _U(threshold(p))).reshape(B, H, L, L)


def site_seed(initial_seed, word):
    return (initial_seed * 0x85EBCA6B + word) & _M


LN_EMBEDDING = 0


def ln_attn_out(layer):
    return 1 + 2 * layer


def ln_ffn(layer):
    return 2 + 2 * layer


def ln_site_seed(initial_seed, site):
    """Seed of a model's LN site (LN_EMBEDDING, ln_attn_out(l), ln_ffn(l))."""
    return site_seed(initial_seed, 0x1000 + site)


def attn_site_seed(initial_seed, layer):
    """Seed of layer `layer`'s K9e attention dropout."""
    return site_seed(initial_seed, 0x2000 + layer)


def model_sites(initial_seed, n_layers):
    """{site name: seed} of an n_layers SASRec: 'emb', and per layer l 'attn{l}' (K9e),
    'out{l}' and 'ffn{l}' (LN sites)."""
    s = {'emb': ln_site_seed(initial_seed, LN_EMBEDDING)}
    for l in range(n_layers):
        s[f'attn{l}'] = attn_site_seed(initial_seed, l)
        s[f'out{l}'] = ln_site_seed(initial_seed, ln_attn_out(l))
        s[f'ffn{l}'] = ln_site_seed(initial_seed, ln_ffn(l))
    return s
