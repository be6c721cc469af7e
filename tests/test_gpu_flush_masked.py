"""mirec_adam_flush_masked_f32 (K5, csrc/adam.hip): a flush split over two launches by a
row bitmap leaves p, p_alt, m, v and last exactly as one mirec_adam_flush_f32 does, in
either order and in both dispatch forms (scan: R rows per wave; walk: a bounded grid of
one-wave workgroups), and a launch leaves the rows outside its selection untouched.
mirec_row_bitmap builds the bitmap the train step uses."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_MASKED, N_PLAIN = 301, 77          # rows: 301 = 9 bitmap words + 13 bits of a tenth
NAMES = ('p', 'p_alt', 'm', 'v', 'last')


@functools.lru_cache(maxsize=None)
def _case(d, target):
    """Initial state of two tables (CPU) and the one-launch flush's result: rows in the
    zero state, rows current at the target (at an odd target held in p_alt only: p
    differs), rows lagging by 1..70 steps with their state in either parity buffer."""
    from recbole_amd import ops
    from recbole_amd.trainer.optim import FusedAdam
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(1000 * d + target)
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    consts = torch.from_numpy(opt.step_constants(1, 80).reshape(-1)).to(dev)
    state = []
    for n in (N_MASKED, N_PLAIN):
        P = torch.randn(n, d, generator=g) * 0.1
        A = torch.randn(n, d, generator=g) * 0.1
        M = torch.randn(n, d, generator=g) * 1e-3
        V = torch.rand(n, d, generator=g) * 1e-6
        last = target - torch.randint(1, 71, (n,), generator=g, dtype=torch.int32)   # lag 1..70
        assert int(last.min()) >= 0
        kind = torch.randint(0, 5, (n,), generator=g)
        zs = kind == 0
        last[zs] = ops.ADAM_ZERO_STATE                   # zero state: identical buffers
        M[zs] = 0
        V[zs] = 0
        A[zs] = P[zs]
        last[kind == 1] = target                         # current
        state.append((P, A, M, V, last))
    bufs, tabs = _device_tables(state, dev)
    base = torch.full((1,), target, dtype=torch.int32, device=dev)
    ops.adam_multi(tabs, d, consts, base, 0, 'flush')
    ref = [[x.cpu() for x in b] for b in bufs]
    lag = ref[0][4] != state[0][4]
    assert int(lag.sum()) > N_MASKED // 2                # most rows do lag
    return state, ref, consts


def _device_tables(state, dev):
    from recbole_amd import ops
    bufs = [[x.clone().to(dev) for x in st] for st in state]
    tabs = ops.adam_tables([dict(p=P, p_alt=A, m=M, v=V, last=L) for P, A, M, V, L in bufs])
    return bufs, tabs


def _bitmap(bits, dev, pad):
    """uint32 words (as an int32 tensor) of a boolean row vector; the unused bits of the
    last word are set to `pad` (the kernels must not take them for rows)."""
    n = len(bits)
    full = np.full(-(-n // 32) * 32, pad, dtype=bool)
    full[:n] = bits
    words = np.packbits(full.reshape(-1, 32), axis=1, bitorder='little').view(np.uint32)
    return torch.from_numpy(words.reshape(-1).view(np.int32).copy()).to(dev)


def _masked(tabs, d, masks, want, consts, base, off, rows=None, waves=0):
    from recbole_amd._native import check, lib
    from recbole_amd.ops import stream_handle
    n = len(tabs)
    mp = (ctypes.c_void_p * n)(*[m.data_ptr() if m is not None else None for m in masks])
    rc = lib().mirec_adam_flush_masked_f32(
        tabs, n, d, mp, (ctypes.c_int32 * n)(*want),
        (ctypes.c_int32 * n)(*rows) if rows is not None else None, waves,
        consts.data_ptr(), base.data_ptr(), off, 0.9, 0.999, 1e-8, 0.0, stream_handle())
    check(rc, 'mirec_adam_flush_masked_f32')


# dispatch forms of one launch: the scan form's rows per wave, or the walk form's waves
# (2: many stride iterations per wave; 1,024: far more waves than 32-row groups)
FORMS = [dict(rows=(4, 1)), dict(rows=(64, 3)), dict(waves=2), dict(waves=1024)]


@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('target', [70, 71])             # even / odd: parity-buffer publishing
@pytest.mark.parametrize('mask_kind', ['random', 'zeros', 'ones'])
def test_two_masked_flushes_equal_one_flush(dev, d, target, mask_kind):
    state, ref, consts = _case(d, target)
    g = np.random.default_rng(d + target)
    bits = {'random': g.random(N_MASKED) < 0.4, 'zeros': np.zeros(N_MASKED, bool),
            'ones': np.ones(N_MASKED, bool)}[mask_kind]
    base = torch.full((1,), target, dtype=torch.int32, device=dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    sel = torch.from_numpy(bits)
    for fi, first_form in enumerate(FORMS):
        second_form = FORMS[(fi + 1) % len(FORMS)]
        for order in ((1, 0), (0, 1)):
            # the unused bits of the last word carry the value each launch selects
            bufs, tabs = _device_tables(state, dev)
            for step, (want, form) in enumerate(zip(order, (first_form, second_form))):
                mask = _bitmap(bits, dev, pad=bool(want))
                if want == 1:        # the chunk's rows and the whole second table, at step_idx
                    _masked(tabs, d, (mask, None), (1, 1), consts, base, 0, **form)
                else:                # the other rows, explicit target; second table left out
                    form0 = dict(form, rows=(form['rows'][0], 1)) if 'rows' in form else form
                    _masked(tabs, d, (mask, None), (0, -1), consts, zero, target, **form0)
                if step == 0:        # rows outside the first launch's selection: untouched
                    out = sel if want == 0 else ~sel
                    for name, x, x0, xr in zip(NAMES, bufs[0], state[0], ref[0]):
                        assert torch.equal(x.cpu()[out], x0[out]), (name, order, first_form)
                        assert torch.equal(x.cpu()[~out], xr[~out]), (name, order, first_form)
                    for name, x, x0, xr in zip(NAMES, bufs[1], state[1], ref[1]):
                        assert torch.equal(x.cpu(), xr if want == 1 else x0), (name, order)
            for q in range(2):
                for name, x, xr in zip(NAMES, bufs[q], ref[q]):
                    assert torch.equal(x.cpu(), xr), (q, name, order, first_form, second_form)


def test_masked_flush_rejects_bad_forms(dev):
    from recbole_amd._native import NativeError
    state, _, consts = _case(64, 70)
    bufs, tabs = _device_tables(state, dev)
    base = torch.full((1,), 70, dtype=torch.int32, device=dev)
    before = [x.clone() for b in bufs for x in b]
    with pytest.raises(NativeError):                     # neither form
        _masked(tabs, 64, (None, None), (1, 1), consts, base, 0)
    with pytest.raises(NativeError):                     # both forms
        _masked(tabs, 64, (None, None), (1, 1), consts, base, 0, rows=(1, 1), waves=8)
    with pytest.raises(NativeError):
        _masked(tabs, 64, (None, None), (2, 1), consts, base, 0, waves=8)
    _masked(tabs, 64, (None, None), (-1, -1), consts, base, 0, waves=8)   # no table: no launch
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, [x for b in bufs for x in b]))


def test_row_bitmap(dev):
    from recbole_amd._native import check, lib
    from recbole_amd.ops import stream_handle
    g = np.random.default_rng(5)
    n_rows = 1037
    keys = g.integers(0, n_rows, 700)
    keys[:4] = (-3, n_rows, n_rows + 99, n_rows - 1)     # clamped as the records clamp ids
    keys_d = torch.from_numpy(keys).to(dev)
    bitmap = torch.full((-(-n_rows // 32),), -1, dtype=torch.int32, device=dev)   # stale bits
    check(lib().mirec_row_bitmap(keys_d.data_ptr(), len(keys), n_rows, bitmap.data_ptr(),
                                 stream_handle()), 'mirec_row_bitmap')
    exp = np.zeros(n_rows, bool)
    exp[np.clip(keys, 0, n_rows - 1)] = True
    assert torch.equal(bitmap.cpu(), _bitmap(exp, 'cpu', pad=False))
    check(lib().mirec_row_bitmap(None, 0, n_rows, bitmap.data_ptr(), stream_handle()),
          'mirec_row_bitmap')
    assert int(bitmap.abs().sum()) == 0
