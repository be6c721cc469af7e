"""mirec_adam_flush_first_f32 (K5, csrc/adam.hip): the flush with a target per row — the
chunk's base step + the row's first read — leaves p, p_alt, m, v and last exactly as the
existing masked flush does when it is run once per distinct target on the rows sharing that
target, and leaves every row that is not read, in the zero state, or already at or past its
target bit-unchanged (the poisoned other parity buffer included).
mirec_first_read builds the first-read table the train step uses.

One exception is made in the reference's bitmaps, and checked on its own instead: a row that
is at or past an ODD target is kept out of its target's bitmap. The uniform flush copies such
a row p_alt -> p (it completes the parameter tensor); the per-row-target form must not load
it at all, which is what the bit-unchanged check asks of it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS = (70, 300)                   # no multiple of the rows per wave or of 32
NAMES = ('p', 'p_alt', 'm', 'v', 'last')
BASE, OFF = 7, 3                     # step_base_dev[0] and step_off: targets from 10 on
KINDS = ('lag1', 'lag5', 'lag40', 'at', 'past', 'zero', 'unread')
LAG = {'lag1': 1, 'lag5': 5, 'lag40': 40, 'at': 0, 'past': -3}
POISON = 1.0e30


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _state(d, n, g):
    """One table (CPU tensors): per row a kind (cycled, so every wave's rows mix them), a
    first read in [32, 62) — even and odd targets — and a `last` set by the kind; the row's
    p sits in the buffer of its last's parity, the other buffer is poisoned."""
    from recbole_amd import ops
    kind = np.array([KINDS[i % len(KINDS)] for i in range(n)])
    first = torch.randint(32, 62, (n,), generator=g, dtype=torch.int32)
    # successive rows of one kind alternate between even and odd targets
    first = (first & ~1) | ((torch.arange(n, dtype=torch.int32) // len(KINDS) + BASE + OFF) & 1)
    target = BASE + OFF + first
    last = target.clone()
    for name, lag in LAG.items():
        sel = torch.from_numpy(kind == name)
        last[sel] = target[sel] - lag
    unread = torch.from_numpy(kind == 'unread')
    last[unread] = target[unread] - 9            # lagging, but the chunk does not read it
    first[unread] = -1
    val = torch.randn(n, d, generator=g) * 0.1
    odd = (last & 1).bool().view(n, 1)
    poison = torch.full((n, d), POISON) + torch.arange(n, dtype=torch.float32).view(n, 1)
    P = torch.where(odd, poison, val)
    A = torch.where(odd, val, poison)
    M = torch.randn(n, d, generator=g) * 1e-3
    V = torch.rand(n, d, generator=g) * 1e-6
    zs = torch.from_numpy(kind == 'zero')
    last[zs] = ops.ADAM_ZERO_STATE               # zero state: identical buffers
    M[zs] = 0
    V[zs] = 0
    P[zs] = A[zs] = val[zs]
    assert int(last.min()) >= 0
    return (P, A, M, V, last), first, target, kind


def _device_tables(state, dev):
    from recbole_amd import ops
    bufs = [[x.clone().to(dev) for x in st] for st in state]
    tabs = ops.adam_tables([dict(p=P, p_alt=A, m=M, v=V, last=L) for P, A, M, V, L in bufs])
    return bufs, tabs


def _bitmap(bits, dev):
    n = len(bits)
    full = np.zeros(-(-n // 32) * 32, dtype=bool)
    full[:n] = bits
    words = np.packbits(full.reshape(-1, 32), axis=1, bitorder='little').view(np.uint32)
    return torch.from_numpy(words.reshape(-1).view(np.int32).copy()).to(dev)


@functools.lru_cache(maxsize=None)
def _case(d):
    """Initial state of the two tables, their first-read arrays, and the expected result:
    for each distinct target in turn, the masked scan-form flush on a copy with a bitmap of
    the rows sharing that target (see the module docstring for the one exception)."""
    from recbole_amd._native import check, lib
    from recbole_amd.ops import stream_handle
    from recbole_amd.trainer.optim import FusedAdam
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(77 * d)
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    consts = torch.from_numpy(opt.step_constants(1, 120).reshape(-1)).to(dev)
    made = [_state(d, n, g) for n in N_ROWS]
    state = [m[0] for m in made]
    firsts, targets, kinds = ([m[i] for m in made] for i in (1, 2, 3))
    for target, kind in zip(targets, kinds):     # even and odd targets in every kind
        for name in KINDS:
            par = set((target[torch.from_numpy(kind == name)] & 1).tolist())
            assert par == {0, 1}, (name, par)
    bufs, tabs = _device_tables(state, dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    skipped = [torch.from_numpy(np.isin(kind, ('at', 'past'))) & (target & 1).bool()
               for target, kind in zip(targets, kinds)]
    for t in sorted(set(torch.cat(targets).tolist())):
        masks = [_bitmap(((first >= 0) & (target == t) & ~skip).numpy(), dev)
                 for first, target, skip in zip(firsts, targets, skipped)]
        rc = lib().mirec_adam_flush_masked_f32(
            tabs, 2, d, (ctypes.c_void_p * 2)(*[m.data_ptr() for m in masks]),
            (ctypes.c_int32 * 2)(1, 1), (ctypes.c_int32 * 2)(4, 4), 0, consts.data_ptr(),
            zero.data_ptr(), int(t), 0.9, 0.999, 1e-8, 0.0, stream_handle())
        check(rc, 'mirec_adam_flush_masked_f32')
    ref = [[x.cpu() for x in b] for b in bufs]
    for q in range(2):                           # the reference did move the lagging rows
        moved = ref[q][4] != state[q][4]
        lag = torch.from_numpy(np.isin(kinds[q], ('lag1', 'lag5', 'lag40')))
        assert torch.equal(moved, lag)
        assert torch.equal(ref[q][4][lag], targets[q][lag])
    return state, firsts, kinds, ref, consts


@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('rows', [1, 8, 64])
def test_flush_to_first_read_equals_masked_flushes(dev, d, rows):
    from recbole_amd._native import check, lib
    from recbole_amd.ops import stream_handle
    state, firsts, kinds, ref, consts = _case(d)
    bufs, tabs = _device_tables(state, dev)
    first_d = [f.to(dev) for f in firsts]
    base = torch.full((1,), BASE, dtype=torch.int32, device=dev)
    rc = lib().mirec_adam_flush_first_f32(
        tabs, 2, d, (ctypes.c_void_p * 2)(*[f.data_ptr() for f in first_d]),
        (ctypes.c_int32 * 2)(rows, rows), consts.data_ptr(), base.data_ptr(), OFF,
        0.9, 0.999, 1e-8, 0.0, stream_handle())
    check(rc, 'mirec_adam_flush_first_f32')
    for q in range(2):
        still = torch.from_numpy(np.isin(kinds[q], ('at', 'past', 'zero', 'unread')))
        for name, x, x0, xr in zip(NAMES, bufs[q], state[q], ref[q]):
            got = _bits(x.cpu())
            assert torch.equal(got, _bits(xr)), (q, name)
            assert torch.equal(got[still], _bits(x0)[still]), (q, name)


def test_flush_to_first_read_leaves_a_table_out(dev):
    from recbole_amd._native import NativeError, check, lib
    from recbole_amd.ops import stream_handle
    state, firsts, _, ref, consts = _case(64)
    bufs, tabs = _device_tables(state, dev)
    first_d = firsts[1].to(dev)
    base = torch.full((1,), BASE + OFF, dtype=torch.int32, device=dev)
    args = (consts.data_ptr(), base.data_ptr(), 0, 0.9, 0.999, 1e-8, 0.0, stream_handle())
    check(lib().mirec_adam_flush_first_f32(
        tabs, 2, 64, (ctypes.c_void_p * 2)(None, first_d.data_ptr()),
        (ctypes.c_int32 * 2)(2, 3), *args), 'mirec_adam_flush_first_f32')
    for name, x, x0 in zip(NAMES, bufs[0], state[0]):        # NULL: the table is left out
        assert torch.equal(_bits(x.cpu()), _bits(x0)), name
    for name, x, xr in zip(NAMES, bufs[1], ref[1]):
        assert torch.equal(_bits(x.cpu()), _bits(xr)), name
    with pytest.raises(NativeError):                         # rows per wave out of range
        check(lib().mirec_adam_flush_first_f32(
            tabs, 2, 64, (ctypes.c_void_p * 2)(None, first_d.data_ptr()),
            (ctypes.c_int32 * 2)(1, 65), *args), 'mirec_adam_flush_first_f32')
    with pytest.raises(NativeError):
        check(lib().mirec_adam_flush_first_f32(tabs, 2, 64, None, None, *args),
              'mirec_adam_flush_first_f32')


@pytest.mark.parametrize('per,n_rows', [(7, 23), (12, 40)])   # users / items of 5 batches
def test_first_read_table(dev, per, n_rows):
    from recbole_amd._native import check, lib
    from recbole_amd.ops import stream_handle
    g = np.random.default_rng(per)
    nb = 5
    keys = g.integers(0, n_rows, (nb, per))
    keys[:, 1] = keys[:, 0]                      # repeats within a batch
    keys[1:, 2] = keys[:-1, 3]                   # and across batches
    keys[4, 4] = keys[0, 5]
    uniq = np.full((nb, per), -7, dtype=np.int32)            # past the count: not read
    nu = np.zeros(nb, dtype=np.int32)
    exp = np.full(n_rows, -1, dtype=np.int32)
    for c in range(nb):
        u = np.unique(keys[c])
        uniq[c, :len(u)] = u
        nu[c] = len(u)
        assert len(u) < per
        exp[u] = np.where(exp[u] < 0, c, exp[u])
    assert (exp < 0).any() and len(set(exp.tolist())) == nb + 1
    first = torch.from_numpy(g.integers(-5, 9, n_rows).astype(np.int32)).to(dev)   # stale
    uniq_d, nu_d = torch.from_numpy(uniq).to(dev), torch.from_numpy(nu).to(dev)
    check(lib().mirec_first_read(uniq_d.data_ptr(), nu_d.data_ptr(), nb, per, n_rows,
                                 first.data_ptr(), stream_handle()), 'mirec_first_read')
    assert np.array_equal(first.cpu().numpy(), exp)
    check(lib().mirec_first_read(None, None, 0, per, n_rows, first.data_ptr(), stream_handle()),
          'mirec_first_read')
    assert int((first != -1).sum()) == 0
