"""tests/ctx_spec.py (the float64 reference of the K8 GPU tests) against the oracle's
DeepFM restatement, the float32-restatement ratio behind test_gpu_context's tolerance,
and the sigmoid + BCE point sets as torch-float32 sees them on the CPU."""
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from tests import ctx_spec


def _close(got, ref, mag, name):
    """|got - ref| <= 1e-12 |ref| + 1e-14 mag (float64 against float64: the absolute part
    covers another summation order where the terms cancel)."""
    bad = (got - ref).abs() > 1e-12 * ref.abs() + 1e-14 * mag
    assert not bool(bad.any()), (name, float((got - ref).abs().max()))


@pytest.mark.parametrize('ns', [1, 0])
def test_spec_matches_oracle_deepfm(ns):
    d, B, nt, nf = 10, 67, 3, 2
    tables, cols, layout = ctx_spec.make_case(d, B, nt, ns, nf, seed=5 + ns)
    dims = [int(b - a) for a, b in zip(layout.token_offsets,
                                       layout.token_offsets[1:] + [tables['T'].shape[0]])]
    sdims = [t.shape[0] for t in tables['seq']]
    ref = cpu_ref.DeepFMCPU(layout.token_names, dims, layout.seq_names, sdims,
                            layout.float_names, d, [8, 4], 0.0).double()
    fo = ref.first_order_linear
    with torch.no_grad():
        for p in list(ref.mlp_layers.parameters()) + list(ref.deep_predict_layer.parameters()):
            p.zero_()                       # y_deep = 0: the output is sigmoid(first + fm)
        ref.token_embedding_table.embedding.weight.copy_(tables['T'])
        fo.token_embedding_table.embedding.weight.copy_(tables['T1'])
        ref.float_embedding_table.weight.copy_(tables['Ef'])
        fo.float_embedding_table.weight.copy_(tables['Ef1'])
        fo.bias.copy_(tables['bias'])
        for i in range(ns):
            ref.token_seq_embedding_table[i].weight.copy_(tables['seq'][i])
            fo.token_seq_embedding_table[i].weight.copy_(tables['seq1'][i])
    g_y = torch.randn(B, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    # .double() leaves the oracle's masked-mean epsilon a FloatTensor, and count + 1e-8
    # rounds to count in float32: as a DoubleTensor the whole forward is float64
    with mock.patch.object(torch, 'sigmoid', lambda x: x), \
            mock.patch.object(torch, 'FloatTensor', torch.DoubleTensor):   # the logit itself
        logit = ref.forward(cols)
    (logit * g_y).sum().backward()
    want, mag = ctx_spec.reference(tables, cols, layout, None, g_y, fm=True)
    _close(logit.detach(), want['y'], mag['y'], 'logit')
    got = {'dT': ref.token_embedding_table.embedding.weight.grad,
           'dT1': fo.token_embedding_table.embedding.weight.grad,
           'dEf': ref.float_embedding_table.weight.grad,
           'dEf1': fo.float_embedding_table.weight.grad, 'dbias': fo.bias.grad}
    for i in range(ns):
        got[f'dseq{i}'] = ref.token_seq_embedding_table[i].weight.grad
        got[f'dseq1_{i}'] = fo.token_seq_embedding_table[i].weight.grad
    assert set(got) == {k for k in want if k.startswith('d')}
    for k, g in got.items():
        assert float(want[k].abs().max()) > 0, k
        _close(g, want[k], mag[k], k)
    # the sigmoid output too, unpatched
    with mock.patch.object(torch, 'FloatTensor', torch.DoubleTensor):
        out = ref.forward(cols).detach()
    torch.testing.assert_close(out, torch.sigmoid(want['y']), rtol=1e-12, atol=1e-15)


def test_mag_bounds_reference_and_first_order_form():
    tables, cols, layout = ctx_spec.make_case(5, 37, 2, 2, 3, seed=11)
    g = torch.Generator().manual_seed(1)
    gc, gy = torch.randn(37, 7, 5, generator=g), torch.randn(37, generator=g)
    for fm in (True, False):
        ref, mag = ctx_spec.reference(tables, cols, layout, gc, gy, fm=fm)
        for k in ref:
            assert bool((mag[k] >= ref[k].abs() * (1 - 1e-12)).all()), k
    full, _ = ctx_spec.reference(tables, cols, layout, fm=True)
    lin, _ = ctx_spec.reference(tables, cols, layout, fm=False)
    assert torch.equal(full['concat'], lin['concat'])
    S, Q = full['concat'].sum(1), (full['concat'] ** 2).sum(1)
    torch.testing.assert_close(full['y'] - lin['y'], 0.5 * (S * S - Q).sum(1), rtol=1e-12,
                               atol=1e-12)
    # all-zero token_seq rows: e = 0
    assert bool((full['concat'][0::4, 2:4] == 0).all())


def test_float32_ratio_behind_the_gpu_tolerance():
    """c of tests/test_gpu_context.py is 16x the float32 restatement's worst error / mag
    over that module's own cases: the constant there is this measurement, neither looser
    (more than a rounding of 16x) nor tighter."""
    from tests.test_gpu_context import C_MAG, F32_RATIO
    ratio = ctx_spec.float32_ratio()
    assert ratio <= F32_RATIO <= 1.05 * ratio, ratio
    assert C_MAG == 16 * F32_RATIO


def test_integer_cases_are_exact_in_float32():
    """The exact cases' premise: with integers in [-3, 3] the float32 restatement of y is
    the float64 value, and every magnitude stays below 2^24."""
    for d in (3, 10, 33, 64):
        for fs in ((9, 0, 0), (5, 0, 10)):
            tables, cols, layout = ctx_spec.make_case(d, 257, *fs, seed=d, integer=True)
            g = torch.Generator().manual_seed(d)
            gc = torch.randint(-3, 4, (257, sum(fs), d), generator=g).float()
            gy = torch.randint(-3, 4, (257,), generator=g).float()
            ref, mag = ctx_spec.reference(tables, cols, layout, gc, gy)
            assert all(float(m.max()) < 2 ** 24 for m in mag.values())
            assert all(bool((r == r.round()).all()) for r in ref.values())
            y32 = ctx_spec.y_float32(tables, cols, layout)
            assert np.array_equal(y32.astype(np.float64), ref['y'].numpy())


# ------------------------------------------------------------------ sigmoid + BCE points
@pytest.mark.parametrize('grad_scale', [1.0, 1.0 / 3000])
def test_bce_moderate_set_float32_within_gpu_tolerance(grad_scale):
    z, t = ctx_spec.bce_moderate(3000, seed=2)
    assert float(z.abs().max()) <= 6 and set(t.tolist()) == {0.0, 1.0}
    p32, l32, dz32 = ctx_spec.bce_torch(z, t, torch.float32, grad_scale)
    p64, l64, dz64 = ctx_spec.bce_torch(z, t, torch.float64, grad_scale)
    torch.testing.assert_close(p32.double(), p64, rtol=1e-5, atol=0)
    torch.testing.assert_close(l32.double(), l64, rtol=ctx_spec.BCE_RTOL, atol=ctx_spec.BCE_ATOL)
    torch.testing.assert_close(dz32.double(), dz64, rtol=ctx_spec.BCE_RTOL,
                               atol=ctx_spec.BCE_ATOL * grad_scale)


def test_bce_saturated_set_float32_values():
    z, t = ctx_spec.bce_saturated()
    _, loss, dz = ctx_spec.bce_torch(z, t, torch.float32)
    at = lambda zv, tv: int(((z == zv) & (t == tv)).nonzero()[0, 0])
    for zv in (20., 30., 95., 200.):
        assert loss[at(zv, 0.)] == 100 and loss[at(zv, 1.)] == 0     # p rounds to 1
        assert dz[at(zv, 0.)] == 0 and dz[at(zv, 1.)] == 0
    for zv in (-95., -200.):
        assert loss[at(zv, 1.)] == 100 and loss[at(zv, 0.)] == 0     # p rounds to 0
        assert dz[at(zv, 0.)] == 0 and dz[at(zv, 1.)] == 0
    assert loss[at(-20., 1.)] == 20 and loss[at(-30., 1.)] == 30
    assert dz[at(-20., 1.)] == -1
    np.testing.assert_allclose(float(dz[at(-30., 1.)]), -0.0935762, rtol=1e-6)  # 1e-12 clamp
    np.testing.assert_allclose(float(dz[at(-30., 0.)]), 8.7565e-15, rtol=1e-4)
