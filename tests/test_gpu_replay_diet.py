"""The deferred-Adam replay engine (csrc/adam_core.h adam_replay_row / incr_steps, csrc/adam_math.h)
after its instruction diet: the rsq-based correctly rounded sqrt for every float of its range,
and the flush forms bit for bit against the streamed schedule where the engine changes state —
rows that start to vanish at every phase of the coarser vanishing-test cadence, and waves that
leave the fast path's ranges inside a step group."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, TAKEN = 96, 40            # steps of the streamed run; optimizer steps before it
LAGS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 96)


def test_replay_sqrt_exhaustive(dev):
    """sqrt takes one fp32 argument, so this is a proof on the GPU that runs it: the sqrt the
    replay calls equals sqrtf for EVERY float of the fast range [2^-96, FLT_MAX] (stride 1,
    about 2^31 values), beside 2^20 division pairs."""
    from recbole_amd._native import check, lib
    out = torch.zeros(4, dtype=torch.int64, device=dev)
    check(lib().mirec_selftest_adam_math(1, 1 << 20, 2025, out.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream),
          'mirec_selftest_adam_math')
    sq_bad, sq_n, dv_bad, dv_n = out.cpu().tolist()
    print(f'sqrt: {sq_n} values, {sq_bad} mismatches; division: {dv_n} pairs, {dv_bad} mismatches')
    assert sq_n >= 0x7f7fffff - 0x0f800000 + 1          # every float of the range
    assert dv_n > 2 ** 19
    assert sq_bad == 0 and dv_bad == 0, (sq_bad, dv_bad)


def _consts(dev):
    from recbole_amd.trainer.optim import FusedAdam
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    table = opt.step_constants(TAKEN + 1, STEPS)
    return table, torch.from_numpy(table.reshape(-1)).to(dev)


def _streamed(dev, d, P, M, V, consts, steps):
    """Snapshots [steps + 1] of (p, m, v) on the device: `steps` zero-gradient steps of the
    streamed kernel (mirec_adam_multi_f32), state t = after t steps."""
    from recbole_amd import ops
    p, m, v = (x.clone().to(dev) for x in (P, M, V))
    zero = torch.zeros_like(p)
    tabs = ops.adam_tables([dict(p=p, m=m, v=v, dense_grad=zero)])
    base = torch.zeros(1, dtype=torch.int32, device=dev)
    snaps = [(p.clone(), m.clone(), v.clone())]
    for _ in range(steps):
        ops.adam_multi(tabs, d, consts, base, 0, 'streamed')
        base += 1
        snaps.append((p.clone(), m.clone(), v.clone()))
    return snaps


def _flush_equals_streamed(dev, d, snaps, consts, start, target, scan):
    """One deferred flush of every row from state `start` to `target`: the one-row flush or the
    scan form (R rows per wave); the state sits in the parity buffer of `start`, the other
    buffer holds NaN; p, m, v and the target's parity buffer must be the streamed state."""
    from recbole_amd import ops
    p0, m0, v0 = snaps[start]
    junk = torch.full_like(p0, float('nan'))
    p, alt = (junk, p0.clone()) if start & 1 else (p0.clone(), junk)
    m, v = m0.clone(), v0.clone()
    last = torch.full((p0.shape[0],), start, dtype=torch.int32, device=dev)
    base = torch.full((1,), target, dtype=torch.int32, device=dev)
    tabs = ops.adam_tables([dict(p=p, p_alt=alt, m=m, v=v, last=last)])
    ops.adam_multi(tabs, d, consts, base, 0, 'flush', flush_rows=(5,) if scan else None)
    where = (d, start, target, 'scan' if scan else 'row')
    for got, want, name in zip((p, m, v), snaps[target], 'pmv'):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name,) + where
    if target & 1:
        assert torch.equal(alt.view(torch.int32), snaps[target][0].view(torch.int32)), where
    assert bool((last == target).all()), where


@pytest.mark.parametrize('d', [64, 128, 256])
def test_replay_transitions_every_cadence_phase(dev, d):
    """1,024 rows whose p updates start to round away at steps spread over the run, so that the
    change into the skipping state falls on every phase of the 16-step test cadence: flushes
    from lags 1..96, from the start and to the end of the run, one-row and scan form, both
    parity buffers, even and odd targets, equal the streamed states bit for bit."""
    rng = np.random.default_rng(20250 + d)
    n = 1024
    table, consts = _consts(dev)
    ss, bc2s = float(table[0, 0]), float(table[0, 1])
    p = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-4, 5, n))[:, None] * np.ones((1, d))
    v = np.full((n, d), 1e-4)
    # |first increment| / |p| = 2^e: q = ss * (0.9 m) / (sqrt(0.999 v) / bc2s + eps)
    e = rng.uniform(-26, -13, n)[:, None]
    den = np.sqrt(0.999 * v) / bc2s + 1e-8
    m = 2.0 ** e * np.abs(p) * den / (ss * 0.9) * rng.uniform(1, 1.02, (1, d)) * \
        rng.choice([-1.0, 1.0], n)[:, None]
    P, M, V = (torch.as_tensor(x.astype(np.float32)) for x in (p, m, v))
    snaps = _streamed(dev, d, P, M, V, consts, STEPS)

    # from the streamed run alone: a row's transition step = the first step from which its p no
    # longer changes (the kernel's own predicate, a sufficient condition, fires at or after it)
    ps = torch.stack([s[0].view(torch.int32) for s in snaps])            # [STEPS + 1, n, d]
    changed = (ps[1:] != ps[:-1]).any(dim=2).cpu().numpy()               # [STEPS, n]: step t+1
    last_change = np.where(changed.any(0), STEPS - np.argmax(changed[::-1], axis=0), 0)
    inside = (last_change >= 1) & (last_change < STEPS - 1)             # stops inside the run
    per_residue = np.bincount((last_change[inside] + 1) % 16, minlength=16)
    print(f'd={d}: {int(inside.sum())} rows change state inside the run, steps '
          f'{int(last_change[inside].min()) + 1}-{int(last_change[inside].max()) + 1}; '
          f'rows per residue mod 16: {per_residue.tolist()}')
    assert per_residue.min() >= 8, per_residue

    for lag in LAGS:
        for start in sorted({0, 1, STEPS - lag, STEPS - 1 - lag}):
            if start < 0 or start + lag > STEPS:
                continue
            for scan in (False, True):
                _flush_equals_streamed(dev, d, snaps, consts, start, start + lag, scan)


@pytest.mark.parametrize('d', [64, 128, 256])
def test_replay_waves_leaving_fast_range(dev, d):
    """Ordinary rows with columns outside the fast path's ranges, or crossing a bound inside a
    step group: v = 0, 1e-30, a denormal, 3e38 (sqrt / denominator bounds), v just above 2^-96
    (below it after 1-4 steps), m = 0 and |m| around 2^-50 (the numerator's lower bound), and
    whole rows of m = 0. The wave vote sends such a group down the library path; deferred
    equals streamed bit for bit at lags 4, 7 and 64."""
    rng = np.random.default_rng(777 + d)
    n, steps = 256, 64
    table, consts = _consts(dev)
    p = rng.standard_normal((n, d)) * 0.1
    m = rng.standard_normal((n, d)) * 1e-3
    v = rng.uniform(0, 1, (n, d)) * 1e-6
    odd_v = np.array([0.0, 1e-30, 1e-41, 3e38] + [2.0 ** -96 * f for f in
                                                   (1.0005, 1.0015, 1.0025, 1.0035, 1.006)])
    odd_m = np.array([0.0] + [s * 2.0 ** -50 * f for s in (-1, 1) for f in (1.02, 1.15, 1.3, 1.6)])
    for r in range(n):
        kind = r % 4                                   # 0: an ordinary row
        cols = rng.choice(d, 1 + r % 7, replace=False)
        if kind == 1 or kind == 3:
            v[r, cols] = rng.choice(odd_v, cols.size)
        if kind == 2 or kind == 3:
            m[r, rng.permutation(cols)] = rng.choice(odd_m, cols.size)
    m[5::32] = 0.0                                     # whole rows that never move
    v[9::64] = rng.choice(odd_v, (len(v[9::64]), d))   # whole rows outside / at the bounds
    P, M, V = (torch.as_tensor(x.astype(np.float32)) for x in (p, m, v))
    assert bool((V[V > 0] < 1.2e-38).any())            # the denormal survived the cast
    snaps = _streamed(dev, d, P, M, V, consts, steps)
    for lag in (4, 7, 64):
        for start in sorted({0, 1, steps - lag, steps - 1 - lag}):
            if start < 0 or start + lag > steps:
                continue
            for scan in (False, True):
                _flush_equals_streamed(dev, d, snaps, consts, start, start + lag, scan)
