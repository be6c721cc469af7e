"""The fixed-order sums of csrc/context.hip and csrc/capi.hip against float64:
ops.colsum (mirec_colsum_f32: the tile forms CB = 1, 8, 64, each past its eight-deep
unrolled row stride and with a remainder), layers.colsums (mirec_colsum_multi_f32: the
block-to-job map, every job the one-launch form's bits), ops.fixed_sum (mirec_sum_f32)
and mirec_offset_keys. They produce every bias, LayerNorm, position-embedding and
float-field gradient of the models.

Each shape runs on integers in [-8, 8], asserted equal to the float64 sum (a dropped or
doubled row shows at any n), and on standard normals within (n - 1) 2^-24 sum|x|, the
bound of a float32 sum in any order."""
import ctypes

import pytest
import torch

from recbole_amd import ops
from recbole_amd._native import NativeError, check, lib, ptr, stream_handle

pytestmark = pytest.mark.gpu

COLSUM_SHAPES = [(0, 5), (1, 1),
                 (1023, 1), (1024, 1), (1025, 3), (8197, 3),        # CB = 1: stride 8 x 1024
                 (127, 8), (129, 9), (1030, 63),                    # CB = 8: stride 8 x 128
                 (15, 64), (17, 65), (130, 130), (300, 200)]        # CB = 64: stride 8 x 16


def _ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).to(torch.float32)


def _check_sum(got, x, n):
    """got against the float64 sum of x [n, ...] over dim 0: within (n - 1) 2^-24 sum|x|."""
    want = x.double().sum(0)
    bound = max(n - 1, 0) * 2.0 ** -24 * x.double().abs().sum(0)
    err = (got.double().cpu().reshape(want.shape) - want).abs()
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize('n,m', COLSUM_SHAPES)
def test_colsum(dev, n, m):
    g = torch.Generator().manual_seed(n * 1000 + m)
    x = _ints(g, n, m)
    got = ops.colsum(x.to(dev))
    assert got.shape == (m,) and torch.equal(got.double().cpu(), x.double().sum(0))
    x = torch.randn(n, m, generator=g)
    out = torch.full((m + 1,), -77., device=dev)
    got = ops.colsum(x.to(dev), out[:m])
    _check_sum(got, x, n)
    assert float(out[m]) == -77                        # nothing past column m


def _jobs(dev, shapes, g, integer):
    xs = [(_ints(g, n, m) if integer else torch.randn(n, m, generator=g)).to(dev)
          for n, m in shapes]
    outs = [torch.full((m,), -77., device=dev) for _, m in shapes]
    return xs, outs, [(x, n, m, o) for x, o, (n, m) in zip(xs, outs, shapes)]


@pytest.mark.parametrize('shapes', [[(257, 20)], [(1030, 1), (129, 20), (40, 130)],
                                    [(300, 130), (8197, 1), (17, 20), (1, 1)],
                                    [(50, 20), (33, 0), (2000, 1)],
                                    [(0, 9), (1025, 64)]],
                         ids=['1job', '3jobs', '4jobs', 'empty_job', 'no_rows'])
def test_colsums_is_colsum_per_job(dev, shapes):
    from recbole_amd.model.layers import colsums
    g = torch.Generator().manual_seed(len(shapes) + shapes[0][0])
    for integer in (True, False):
        xs, outs, jobs = _jobs(dev, shapes, g, integer)
        colsums(jobs)
        for x, o, (n, m) in zip(xs, outs, shapes):
            assert torch.equal(o, ops.colsum(x)), (n, m)          # bit for bit
            if integer:
                assert torch.equal(o.double(), x.double().sum(0))
            else:
                _check_sum(o, x.cpu(), n)


def test_colsums_refuses_a_fifth_job(dev):
    from recbole_amd.model.layers import colsums
    g = torch.Generator().manual_seed(0)
    xs, outs, jobs = _jobs(dev, [(9, 3)] * 5, g, True)
    with pytest.raises(NativeError):
        colsums(jobs)
    torch.cuda.synchronize()
    assert all(bool((o == -77).all()) for o in outs)


@pytest.mark.parametrize('n', [0, 1, 1023, 1024, 1025, 5000])
def test_fixed_sum(dev, n):
    g = torch.Generator().manual_seed(n)
    x = _ints(g, n)
    assert float(ops.fixed_sum(x.to(dev))) == float(x.double().sum())
    x = torch.randn(n, generator=g)
    _check_sum(ops.fixed_sum(x.to(dev))[0], x, n)


def _offset_keys(dev, cols, offsets, B):
    nf = len(cols)
    out = torch.full((nf * B + 1,), -77, dtype=torch.int64, device=dev)
    rc = lib().mirec_offset_keys((ctypes.c_void_p * nf)(*[ptr(c) for c in cols]),
                                 (ctypes.c_int64 * nf)(*offsets), nf, B, ptr(out),
                                 stream_handle())
    return rc, out


@pytest.mark.parametrize('B', [1, 257, 16385])
@pytest.mark.parametrize('nf', [1, 2, 64])
def test_offset_keys(dev, nf, B):
    g = torch.Generator().manual_seed(nf * B)
    ids = torch.randint(0, 2 ** 40, (nf, B), generator=g)
    offsets = [int(v) for v in torch.randint(0, 1000, (nf,), generator=g)]
    offsets[-1] = 2 ** 31 + 12345
    cols = [ids[f].to(dev) for f in range(nf)]
    rc, out = _offset_keys(dev, cols, offsets, B)
    check(rc, 'mirec_offset_keys')
    want = ids + torch.tensor(offsets).unsqueeze(1)           # field-major
    assert torch.equal(out[:-1].cpu().view(nf, B), want) and int(out[-1]) == -77


def test_offset_keys_refuses_65_fields(dev):
    cols = [torch.zeros(4, dtype=torch.int64, device=dev) for _ in range(65)]
    rc, out = _offset_keys(dev, cols, [0] * 65, 4)
    with pytest.raises(NativeError):
        check(rc, 'mirec_offset_keys')
    assert bool((out == -77).all())
