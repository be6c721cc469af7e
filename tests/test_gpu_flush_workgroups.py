"""Workgroup size of the flush forms with R rows per wave (K5, csrc/adam.hip): a launch of at
most 2^17 waves runs as one-wave workgroups, a larger one as four-wave workgroups, and the
kernels take their wave's rows from blockDim. On a table of 2^17 + 70 rows (no multiple of a
workgroup's rows in either shape) the scan form, its masked variant and the per-row-target
form, at 1 row per wave (more than 2^17 waves) and at 8 (fewer), leave p, p_alt, m, v and
last exactly as the one-wave-per-row flush does, the poisoned dead parity buffer included."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, D = (1 << 17) + 70, 64
NAMES = ('p', 'p_alt', 'm', 'v', 'last')
TARGET = 12                          # even: a current row has nothing to publish
POISON = 1.0e30


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


@functools.lru_cache(maxsize=None)
def _case():
    """Initial state (device tensors, never written) and the one-row flush's result: most
    rows in the zero state, every 5th lagging by 1 or 4 steps (both parities), every 7th
    current; the first and last rows of the table lag."""
    from recbole_amd import ops
    from recbole_amd._native import check, lib
    from recbole_amd.ops import stream_handle
    from recbole_amd.trainer.optim import FusedAdam
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(5)
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    consts = torch.from_numpy(opt.step_constants(1, 40).reshape(-1)).to(dev)
    r = torch.arange(N, device=dev)
    last = torch.full((N,), ops.ADAM_ZERO_STATE, dtype=torch.int32, device=dev)
    last[r % 7 == 0] = TARGET
    lag = (r % 5 == 0) | (r == N - 1)
    last[lag] = (TARGET - 1 - 3 * ((r // 5) & 1)).to(torch.int32)[lag]
    zs = (last == ops.ADAM_ZERO_STATE).view(N, 1)
    val = torch.randn(N, D, generator=g, device=dev) * 0.1
    odd = (last & 1).bool().view(N, 1) & ~zs
    poison = torch.full((N, D), POISON, device=dev)
    P = torch.where(odd, poison, val)
    A = torch.where(odd | zs, val, poison)
    M = torch.where(zs, torch.zeros((), device=dev),
                    torch.randn(N, D, generator=g, device=dev) * 1e-3)
    V = torch.where(zs, torch.zeros((), device=dev),
                    torch.rand(N, D, generator=g, device=dev) * 1e-6)
    state = (P, A, M, V, last)
    bufs = [x.clone() for x in state]
    tabs = ops.adam_tables([dict(zip(NAMES, bufs))])
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().mirec_adam_flush_f32(tabs, 1, D, consts.data_ptr(), zero.data_ptr(), TARGET,
                                     0.9, 0.999, 1e-8, 0.0, stream_handle()),
          'mirec_adam_flush_f32')
    assert int((bufs[4] != last).sum()) == int(lag.sum()) and bool(lag[0]) and bool(lag[-1])
    return state, bufs, consts, zero


@pytest.mark.parametrize('rows', [1, 8])
@pytest.mark.parametrize('form', ['scan', 'masked', 'first'])
def test_flush_forms_equal_the_one_row_flush_in_both_workgroup_shapes(dev, form, rows):
    from recbole_amd import ops
    from recbole_amd._native import check, lib
    from recbole_amd.ops import stream_handle
    state, ref, consts, zero = _case()
    assert (N + rows - 1) // rows > (1 << 17) if rows == 1 else (N + rows - 1) // rows < (1 << 17)
    bufs = [x.clone() for x in state]
    tabs = ops.adam_tables([dict(zip(NAMES, bufs))])
    step = (consts.data_ptr(), zero.data_ptr(), TARGET, 0.9, 0.999, 1e-8, 0.0, stream_handle())
    R = (ctypes.c_int32 * 1)(rows)
    if form == 'scan':
        rc = lib().mirec_adam_flush_rows_f32(tabs, 1, D, R, *step)
    elif form == 'masked':
        ones = torch.full(((N + 31) // 32,), -1, dtype=torch.int32, device=dev)
        rc = lib().mirec_adam_flush_masked_f32(tabs, 1, D, (ctypes.c_void_p * 1)(ones.data_ptr()),
                                               (ctypes.c_int32 * 1)(1), R, 0, *step)
    else:                                        # every row read, first read 5 after base 7
        first = torch.full((N,), 5, dtype=torch.int32, device=dev)
        rc = lib().mirec_adam_flush_first_f32(
            tabs, 1, D, (ctypes.c_void_p * 1)(first.data_ptr()), R, consts.data_ptr(),
            zero.data_ptr(), TARGET - 5, 0.9, 0.999, 1e-8, 0.0, stream_handle())
    check(rc, form)
    for name, x, xr in zip(NAMES, bufs, ref):
        assert torch.equal(_bits(x), _bits(xr)), name
