"""K8 (csrc/context.hip: field gather, FM reduce, backward, the first-order-only form) and
the fused sigmoid + BCE against tests/ctx_spec.py's float64 restatement, kernel by kernel.

K8 is driven through model.context (build_fields, ctx_fm_forward, _CtxFMFn / _CtxLinearFn)
with plain tensors as tables, so the descriptor pointer arithmetic is under test too.
Shapes: every lanes-per-sample form at full width and with idle lanes (d = 1 .. 64),
B = 257 = 4 * 64 + 1 (a part block for each of the 64 / 32 / 16 / 8 / 4 samples per block)
and B = 1, 37; 1, 8, 9 and 17 fields (the reduce loads eight at a time), field sets that
lack a kind.

Tolerance against float64: |got - ref| <= 1e-4 |ref| + C_MAG * mag, mag = the sum of the
absolute values of the terms that enter the output (ctx_spec). C_MAG is not tuned to the
kernel: y restated in plain float32 numpy (one add at a time, field order) is off float64
by at most 1.77e-7 of mag over this module's own cases (ctx_spec.float32_ratio(),
re-measured by tests/test_ctx_spec_cpu.py; F32_RATIO = 1.8e-7), and
C_MAG = 16 x that = 2.88e-6; the 16x covers another summation order and FMA contraction.
A dropped field or lane moves y by about e^2 / mag, 1.5e-4 at 17 fields x d = 64. The
exact cases (integers in [-3, 3]: float32 is exact in any order) catch what a tolerance
could hide.

Sigmoid + BCE: a moderate set (|z| <= 6) against float64 and a saturated set against
torch-float32 on the CPU (tests/test_ctx_spec_cpu.py shows both sets behave so there)."""
import ctypes

import numpy as np
import pytest
import torch

from recbole_amd import ops
from recbole_amd._native import NativeError, check, lib, ptr, stream_handle
from tests import ctx_spec

pytestmark = pytest.mark.gpu

F32_RATIO = 1.8e-7
C_MAG = 16 * F32_RATIO


# ------------------------------------------------------------------ K8 plumbing
def _to_dev(tables, dev, grad=False):
    f = lambda t: None if t is None else t.to(dev).requires_grad_(grad)
    out = {k: f(tables[k]) for k in ctx_spec.TABLE_KEYS}
    out['seq'], out['seq1'] = [f(t) for t in tables['seq']], [f(t) for t in tables['seq1']]
    return out


def _gpu_inputs(tables, cols, layout, dev, grad=False):
    from recbole_amd.data.interaction import Interaction
    from recbole_amd.model.context import FieldLayout
    lay = FieldLayout(layout.token_names, layout.seq_names, layout.float_names,
                      layout.token_offsets)
    return _to_dev(tables, dev, grad), Interaction({k: v.to(dev) for k, v in cols.items()}), lay


def _width(tables):
    return next(t for t in (tables['T'], tables['Ef'], *tables['seq']) if t is not None).shape[1]


def _apply(fm, tables, cols, layout, dev, gc, gy):
    """(concat, y, gradients by ctx_spec's names) of _CtxFMFn / _CtxLinearFn."""
    from recbole_amd.model.context import _CtxFMFn, _CtxLinearFn
    tb, inter, lay = _gpu_inputs(tables, cols, layout, dev, grad=True)
    fn = _CtxFMFn if fm else _CtxLinearFn
    concat, y = fn.apply(lay, inter, tb['T'], tb['T1'], tb['Ef'], tb['Ef1'], tb['bias'],
                         *tb['seq'], *tb['seq1'])
    torch.autograd.backward([concat, y], [gc.to(dev), gy.to(dev)])
    got = {'d' + k: tb[k].grad for k in ctx_spec.TABLE_KEYS if tb[k] is not None}
    for i, (s, s1) in enumerate(zip(tb['seq'], tb['seq1'])):
        got[f'dseq{i}'], got[f'dseq1_{i}'] = s.grad, s1.grad
    return concat.detach(), y.detach(), got


def _close(got, ref, mag, name):
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = err > 1e-4 * ref.abs() + C_MAG * mag
    assert not bool(bad.any()), (name, int(bad.sum()), float((err / mag.clamp_min(1e-300)).max()))


def _upstream(B, F, d, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        return (torch.randint(-3, 4, (B, F, d), generator=g).float(),
                torch.randint(-3, 4, (B,), generator=g).float())
    return torch.randn(B, F, d, generator=g), torch.randn(B, generator=g)


def _raw_forward(fm, lay, inter, tb, B, d, work, grads=None, edit=None):
    """The forward through raw descriptors (build_fields + the C entry point) with the
    caller's work buffer; edit(arr) changes the descriptors before the upload."""
    from recbole_amd.model.context import _upload, build_fields
    arr, keep = build_fields(lay, inter, tb, grads)
    if edit is not None:
        edit(arr)
    fields_dev = _upload(arr, work.device)
    concat = torch.empty(B, lay.n_fields, d, device=work.device)
    y = torch.empty(B, device=work.device)
    fwd = lib().mirec_ctx_fm_fwd_f32 if fm else lib().mirec_ctx_linear_fwd_f32
    check(fwd(ptr(fields_dev), lay.n_fields, B, d, ptr(tb['bias']), ptr(concat), ptr(y),
              ptr(work), stream_handle()), 'ctx forward')
    return concat, y, fields_dev, keep


def _raw_backward(fm, lay, fields_dev, B, d, concat, gc, gy, work):
    bwd = lib().mirec_ctx_fm_bwd_f32 if fm else lib().mirec_ctx_linear_bwd_f32
    check(bwd(ptr(fields_dev), lay.n_fields, B, d, ptr(concat), ptr(gc), ptr(gy), ptr(work),
              stream_handle()), 'ctx backward')


# ------------------------------------------------------------------ K8 against float64
@pytest.mark.parametrize('d,B,fs', ctx_spec.tolerance_cases(),
                         ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_k8_matches_float64(dev, d, B, fs):
    tables, cols, layout = ctx_spec.make_case(d, B, *fs, seed=ctx_spec.case_seed(d, B, fs))
    gc, gy = _upstream(B, sum(fs), d, seed=B + d)
    concats = {}
    for fm in (True, False):
        ref, mag = ctx_spec.reference(tables, cols, layout, gc, gy, fm=fm)
        concat, y, got = _apply(fm, tables, cols, layout, dev, gc, gy)
        concats[fm] = concat
        _close(concat, ref['concat'], mag['concat'], 'concat')
        _close(y, ref['y'], mag['y'], 'y')
        assert set(got) == {k for k in ref if k.startswith('d')}
        for k, g in got.items():
            assert g is not None, k
            _close(g, ref[k], mag[k], f'{k} fm={fm}')
    assert torch.equal(concats[True], concats[False])     # bit for bit
    if fs[1]:                                             # count 0: e = 0 exactly
        assert bool((concats[True][0::4, fs[0]:fs[0] + fs[1]] == 0).all())


@pytest.mark.parametrize('d', [3, 10, 33, 64])
@pytest.mark.parametrize('fs', [(9, 0, 0), (5, 0, 10)], ids=['9-0-0', '5-0-10'])
def test_k8_exact_on_integers(dev, d, fs):
    """Every table entry, float value, bias and upstream gradient an integer in [-3, 3]:
    all sums stay below 2^24, so float32 equals float64 whatever the order."""
    B = 257
    tables, cols, layout = ctx_spec.make_case(d, B, *fs, seed=31 * d + fs[0], integer=True)
    gc, gy = _upstream(B, sum(fs), d, seed=d, integer=True)
    for fm in (True, False):
        ref, _ = ctx_spec.reference(tables, cols, layout, gc, gy, fm=fm)
        concat, y, got = _apply(fm, tables, cols, layout, dev, gc, gy)
        assert torch.equal(concat.double().cpu(), ref['concat'])
        assert torch.equal(y.double().cpu(), ref['y'])
        for k, g in got.items():
            assert torch.equal(g.double().cpu(), ref[k]), (k, fm)


@pytest.mark.parametrize('d', [5, 16, 33])
def test_linear_form_leaves_the_fm_sums_alone(dev, d):
    """fm=False neither writes nor reads the S part of work (mirec.h): a sentinel there
    survives the forward and the backward, and a NaN sentinel reaches no output."""
    from recbole_amd.model.context import _grad_buffers
    B, fs = 37, (3, 1, 2)
    tables, cols, layout = ctx_spec.make_case(d, B, *fs, seed=d)
    tb, inter, lay = _gpu_inputs(tables, cols, layout, dev)
    F = lay.n_fields
    assert lib().mirec_ctx_fm_work_floats(B, F, d) == B * (F + d)
    work = torch.full((B * (F + d),), float('nan'), device=dev)
    keys = torch.empty(fs[0] * B, dtype=torch.int64, device=dev)
    grads = _grad_buffers(lay, inter, B, d, keys, dev)
    concat, y, fields_dev, keep = _raw_forward(False, lay, inter, tb, B, d, work, grads)
    gc, gy = (t.to(dev) for t in _upstream(B, F, d, seed=2))
    _raw_backward(False, lay, fields_dev, B, d, concat, gc, gy, work)
    assert bool(torch.isnan(work[B * F:]).all()) and not bool(torch.isnan(work[:B * F]).any())
    ref, mag = ctx_spec.reference(tables, cols, layout, fm=False)
    _close(y, ref['y'], mag['y'], 'y')
    _close(concat, ref['concat'], mag['concat'], 'concat')
    # per-contribution rows: ge = g_concat alone
    assert torch.equal(grads['T'].view(fs[0], B, d), gc[:, :fs[0]].transpose(0, 1))
    x = torch.stack([inter[n] for n in lay.float_names], 1)
    assert torch.equal(grads['Ef'].view(B, fs[2], d), gc[:, fs[0] + fs[1]:] * x.unsqueeze(2))
    assert not bool(torch.isnan(grads['seq'][0]).any())
    # the FM form writes S there: the sum over fields of the concat rows
    work2 = torch.full_like(work, float('nan'))
    concat2, y2, _, keep2 = _raw_forward(True, lay, inter, tb, B, d, work2)
    assert torch.equal(concat2, concat)
    S = ctx_spec.reference(tables, cols, layout)[0]['concat'].sum(1)
    Smag = ctx_spec.reference(tables, cols, layout)[1]['concat'].sum(1)
    _close(work2[B * F:], S, Smag, 'S')


# ------------------------------------------------------------------ raw descriptors
def test_bwd_without_g_concat(dev):
    """g_concat = NULL is g_concat = 0: ge = g_fm * (S - e), exact on integers."""
    from recbole_amd.model.context import _grad_buffers
    d, B, fs = 10, 257, (5, 0, 10)
    tables, cols, layout = ctx_spec.make_case(d, B, *fs, seed=8, integer=True)
    tb, inter, lay = _gpu_inputs(tables, cols, layout, dev)
    F = lay.n_fields
    _, gy = _upstream(B, F, d, seed=4, integer=True)
    ge = ctx_spec.contribution_grad(tables, cols, layout, gy)
    work = torch.empty(B * (F + d), device=dev)
    keys = torch.empty(fs[0] * B, dtype=torch.int64, device=dev)
    grads = _grad_buffers(lay, inter, B, d, keys, dev)
    concat, y, fields_dev, keep = _raw_forward(True, lay, inter, tb, B, d, work, grads)
    gyd = gy.to(dev)
    _raw_backward(True, lay, fields_dev, B, d, concat, None, gyd, work)
    assert torch.equal(grads['T'].view(fs[0], B, d).double().cpu(), ge[:, :fs[0]].transpose(0, 1))
    x = torch.stack([cols[n] for n in layout.float_names], 1).double()
    assert torch.equal(grads['Ef'].view(B, fs[2], d).double().cpu(),
                       ge[:, fs[0]:] * x.unsqueeze(2))
    assert torch.equal(grads['T1'].view(fs[0], B).cpu(), gy.expand(fs[0], B))
    assert torch.equal(grads['Ef1'].double().cpu(), gy.double().unsqueeze(1) * x)
    rows = torch.stack([cols[n] + o for n, o in zip(layout.token_names, layout.token_offsets)])
    assert torch.equal(keys.view(fs[0], B).cpu(), rows)


def test_null_output_pointers_write_nothing(dev):
    """grad / grad1 / keys = NULL: that output is skipped, every other one is as before."""
    from recbole_amd.model.context import _grad_buffers
    d, B, fs = 10, 37, (3, 1, 2)
    tables, cols, layout = ctx_spec.make_case(d, B, *fs, seed=6)
    tb, inter, lay = _gpu_inputs(tables, cols, layout, dev)
    F = lay.n_fields
    gc, gy = (t.to(dev) for t in _upstream(B, F, d, seed=9))

    def run(edit):
        work = torch.empty(B * (F + d), device=dev)
        keys = torch.full((fs[0] * B,), -77, dtype=torch.int64, device=dev)
        grads = _grad_buffers(lay, inter, B, d, keys, dev)
        for k in ('T', 'T1', 'Ef', 'Ef1'):
            grads[k].fill_(-77.)
        for t in grads['seq'] + grads['seq1']:
            t.fill_(-77.)
        concat, y, fields_dev, keep = _raw_forward(True, lay, inter, tb, B, d, work, grads, edit)
        _raw_backward(True, lay, fields_dev, B, d, concat, gc, gy, work)
        torch.cuda.synchronize()
        return concat, y, grads

    def edit(arr):
        arr[0].grad = None              # token 0: no embedding gradient rows
        arr[0].keys = None
        arr[1].grad1 = None             # token 1: no first-order gradient
        arr[3].grad = None              # the token_seq field
        arr[3].grad1 = None
        arr[4].grad = None              # float 0: its columns of the [B, nf * d] buffer
        arr[5].grad1 = None             # float 1
    full = run(None)
    part = run(edit)
    assert torch.equal(full[0], part[0]) and torch.equal(full[1], part[1])
    f, p = full[2], part[2]
    s = lambda t: bool((t == -77).all())
    T, T1 = p['T'].view(3, B, d), p['T1'].view(3, B)
    assert s(T[0]) and torch.equal(T[1:], f['T'].view(3, B, d)[1:])
    assert s(T1[1]) and torch.equal(T1[[0, 2]], f['T1'].view(3, B)[[0, 2]])
    K = p['keys'].view(3, B)
    assert s(K[0]) and torch.equal(K[1:], f['keys'].view(3, B)[1:])
    assert not bool((f['keys'] == -77).any())
    assert s(p['seq'][0]) and s(p['seq1'][0])
    Ef, Ef1 = p['Ef'].view(B, 2, d), p['Ef1'].view(B, 2)
    assert s(Ef[:, 0]) and torch.equal(Ef[:, 1], f['Ef'].view(B, 2, d)[:, 1])
    assert s(Ef1[:, 1]) and torch.equal(Ef1[:, 0], f['Ef1'].view(B, 2)[:, 0])


def test_token_rows_are_clamped(dev):
    """id + offset below 0 or at / above n_rows: the row read and the key written are the
    clamped row's (clamp_row runs before any address is formed)."""
    from recbole_amd.model.context import ctx_fm_forward
    d, B, fs = 10, 37, (2, 0, 1)
    tables, cols, layout = ctx_spec.make_case(d, B, *fs, seed=12)
    V = tables['T'].shape[0]
    bad = {k: v.clone() for k, v in cols.items()}
    bad['tok0'][3], bad['tok0'][20] = -1, -(2 ** 40)
    bad['tok1'][5], bad['tok1'][6], bad['tok1'][30] = 50, 51, 2 ** 40
    good = {k: v.clone() for k, v in cols.items()}
    good['tok0'][3] = good['tok0'][20] = 0
    good['tok1'][5] = good['tok1'][6] = good['tok1'][30] = 49
    assert layout.token_offsets[1] + 49 == V - 1
    tb, inter, lay = _gpu_inputs(tables, bad, layout, dev)
    keys = torch.full((2 * B,), -77, dtype=torch.int64, device=dev)
    concat, y, keep = ctx_fm_forward(lay, inter, tb, B, d, tb['bias'], keys=keys)
    rows = torch.stack([good[n] + o for n, o in zip(layout.token_names, layout.token_offsets)])
    assert torch.equal(keys.view(2, B).cpu(), rows)
    assert torch.equal(concat[:, :2].cpu(), tables['T'][rows].transpose(0, 1))
    ref, mag = ctx_spec.reference(tables, good, layout)
    _close(y, ref['y'], mag['y'], 'y')


# ------------------------------------------------------------------ sigmoid + BCE
def _bce(dev, y_fm, y_deep, t, gs, mean):
    B = y_fm.numel()
    a, b, lab = y_fm.to(dev), None if y_deep is None else y_deep.to(dev), t.to(dev)
    loss_b, dz = torch.empty(B, device=dev), torch.empty(B, device=dev)
    if mean:
        m = torch.empty(1, device=dev)
        check(lib().mirec_sigmoid_bce_mean_f32(ptr(a), ptr(b), ptr(lab), B, gs, ptr(loss_b),
                                               ptr(m), ptr(dz), stream_handle()), 'bce mean')
        return None, loss_b, dz, m
    prob = torch.empty(B, device=dev)
    check(lib().mirec_sigmoid_bce_f32(ptr(a), ptr(b), ptr(lab), B, gs, ptr(prob), ptr(loss_b),
                                      ptr(dz), stream_handle()), 'bce')
    return prob, loss_b, dz, None


def _split(z, seed):
    """(y_fm, y_deep) on a 2^-10 grid whose float32 sum is exact and within [-6, 6]."""
    g = torch.Generator().manual_seed(seed)
    zq = torch.round(z * 1024) / 1024
    yd = torch.round((torch.rand(z.numel(), generator=g) * 2 - 1) * 1024) / 1024
    return zq - yd, yd, zq


def _scale(B, which):
    return 1.0 if which == 'one' else float(np.float32(1.0) / np.float32(B))


@pytest.mark.parametrize('which', ['one', 'inv_B'])
@pytest.mark.parametrize('deep', [False, True])
@pytest.mark.parametrize('B', [1, 1023, 1024, 1025, 3000, 4096 * 256 + 3])
def test_bce_moderate_matches_float64(dev, B, deep, which):
    z, t = ctx_spec.bce_moderate(B, seed=B)
    y_fm, y_deep = z, None
    if deep:
        y_fm, y_deep, z = _split(z, seed=B + 1)
        assert torch.equal(y_fm + y_deep, z) and float(z.abs().max()) <= 6
    gs = _scale(B, which)
    p64, l64, dz64 = ctx_spec.bce_torch(z, t, torch.float64, gs)
    prob, loss_b, dz, _ = _bce(dev, y_fm, y_deep, t, gs, mean=False)
    rt, at = ctx_spec.BCE_RTOL, ctx_spec.BCE_ATOL
    torch.testing.assert_close(prob.double().cpu(), p64, rtol=1e-5, atol=0)
    torch.testing.assert_close(loss_b.double().cpu(), l64, rtol=rt, atol=at)
    torch.testing.assert_close(dz.double().cpu(), dz64, rtol=rt, atol=at * gs)
    _, loss_m, dz_m, m = _bce(dev, y_fm, y_deep, t, gs, mean=True)
    assert torch.equal(loss_m, loss_b) and torch.equal(dz_m, dz)     # bit for bit
    np.testing.assert_allclose(float(m), float(l64.mean()), rtol=1e-4)
    # the one-launch mean = the per-sample kernel + the fixed sum + a float32 division
    want = ops.fixed_sum(loss_b).cpu().numpy()[0] / np.float32(B)
    assert m.cpu().numpy()[0] == want and want.dtype == np.float32
    # prob alone: no labels needed
    only = torch.empty(B, device=dev)
    a, b = y_fm.to(dev), None if y_deep is None else y_deep.to(dev)
    check(lib().mirec_sigmoid_bce_f32(ptr(a), ptr(b), None, B, 1.0, ptr(only), None, None,
                                      stream_handle()), 'prob')
    assert torch.equal(only, prob)


@pytest.mark.parametrize('deep', [False, True])
@pytest.mark.parametrize('mean', [False, True])
def test_bce_saturated_matches_torch_float32(dev, mean, deep):
    z, t = ctx_spec.bce_saturated()
    _, l32, dz32 = ctx_spec.bce_torch(z, t, torch.float32)
    y_fm, y_deep = (z * 0.5, z * 0.5) if deep else (z, None)
    _, loss_b, dz, m = _bce(dev, y_fm, y_deep, t, 1.0, mean)
    torch.testing.assert_close(loss_b.cpu(), l32, rtol=1e-5, atol=2.4e-7)
    torch.testing.assert_close(dz.cpu(), dz32, rtol=1e-5, atol=1e-30)
    at = lambda zv, tv: int(((z == zv) & (t == tv)).nonzero()[0, 0])
    assert float(loss_b[at(20., 0.)]) == 100 and float(loss_b[at(-200., 1.)]) == 100
    assert float(dz[at(-20., 1.)]) == -1 and float(dz[at(-95., 1.)]) == 0
    np.testing.assert_allclose(float(dz[at(-30., 1.)]), -0.0935762, rtol=1e-5)
    if mean:
        np.testing.assert_allclose(float(m), float(l32.double().mean()), rtol=1e-5)


def test_bce_refuses_bad_arguments(dev):
    x = torch.zeros(4, device=dev)
    with pytest.raises(NativeError):          # loss without labels
        check(lib().mirec_sigmoid_bce_f32(ptr(x), None, None, 4, 1.0, None, ptr(x), None,
                                          stream_handle()), 'bce')
    with pytest.raises(NativeError):          # the mean of nothing
        check(lib().mirec_sigmoid_bce_mean_f32(ptr(x), None, ptr(x), 0, 1.0, None, ptr(x),
                                               ptr(x), stream_handle()), 'bce mean')
