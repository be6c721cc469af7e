"""The chunk advance of the fused train step (trainer/fused.py CHUNK_ADVANCE): a captured
chunk graph is preceded by one flush launch that brings every row the chunk reads to the step
of its first read, in place of the entry catch-up and of K35's look-ahead replays of those
rows. FusedBPRTrainStep with the advance on, with it off, and on the streamed Adam schedule
leave the tables, the moments, the per-row step counts and the per-step losses bit-identical
— with the background flush on and off, over two epochs whose chunks are ramp chunks (a
short one without the advance, one with an entry catch-up), flushing chunks, a chunk entered
mid-way (eager: no advance) and a bench.py-shaped window, with users repeating inside every chunk (512 reads of 600 users).
After a chunk's advance launch every row it reads has last == b0 + first[row]."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = (600, 200, 4000)      # users, items, interactions asked of the generator
CHUNK = 8


def _build(dev, d, adam_mode='deferred', adv=True, bg=True):
    import bench
    _, _, _, _, opt, step = bench.build_workload(
        dev, d=d, batch_rows=256, adam_mode=adam_mode, chunk=CHUNK, source='memory', shape=SHAPE)
    assert step.Bg == 64 and step.times == 4
    assert step.fused_step == (adam_mode == 'deferred')
    step.FLUSH_EVERY = CHUNK
    step.BG_FLUSH = bg
    step.BG_MIN_STEPS = 4
    step.CHUNK_ADVANCE = adv
    step.ADV_MIN_STEPS = 3                       # the ramp's 2-step chunk is too short
    return opt, step


def _result(opt, step, losses):
    state = [step.pU.detach(), step.pI.detach()]
    for p in (step.pU, step.pI):
        state += [opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']]
    last = [step.lastU, step.lastI] if step.adam_mode == 'deferred' else []
    out = [x.cpu().clone() for x in state], [x.cpu().clone() for x in last], losses
    step.close()
    return out


@functools.lru_cache(maxsize=None)
def _run(d, scenario, adam_mode='deferred', adv=True, bg=True):
    dev = torch.device('cuda', 0)
    opt, step = _build(dev, d, adam_mode, adv, bg)
    step.RAMP = (2, 3) if scenario == 'ramp' else step.RAMP
    captured = []
    inner = step._advance
    step._advance = lambda slot, stream, nb: (captured.append(nb), inner(slot, stream, nb))
    losses = []
    if scenario == 'bench':                      # warm-up, held preparation, timed window
        W, K = 5, 20
        nb = step.begin_epoch(cuts=(W, W + K), hold_prep_from=W, flush_at=(W + K,))
        assert nb > W + K
        step.run_batches(0, W)
        torch.cuda.synchronize()
        step.release_prep(upto=W + K)
        step.run_batches(W, W + K)
        step.sync_params()
        losses += step.end_epoch(W + K)
    elif scenario == 'mid':                      # chunk [8, 16) cut short, then entered mid-way:
        nb = step.begin_epoch()                  # eager, entry catch-up and K35's look-ahead
        step.run_batches(0, 11)
        step.run_batches(11, nb)
        losses += step.end_epoch()
        assert step.n_eager_steps >= CHUNK
    else:
        losses += step.run_epoch()
    plan, flags = step._plan, step._flags
    if scenario == 'ramp':
        # a 2-step chunk that neither flushes nor advances, then a 3-step chunk that starts
        # with an entry catch-up — subsumed by its advance — and flushes
        assert plan[0][1] == 2 and not flags[0][1] and not step._adv[0]
        assert plan[1][1] == 3 and flags[1][0] and flags[1][1]
        assert step._adv[1] == (adv and adam_mode == 'deferred')
    losses += step.run_epoch()                   # a second epoch: the state carries over
    if adv and adam_mode == 'deferred':
        assert sum(step._adv) > 2 and CHUNK in captured
        if scenario == 'ramp':
            assert 3 in captured and 2 not in captured
    else:
        assert not captured and not any(step._adv)
    return _result(opt, step, losses)


@pytest.mark.parametrize('d,scenario', [(64, 'ramp'), (128, 'ramp'), (128, 'bench'),
                                        (64, 'mid')])
@pytest.mark.parametrize('bg', [True, False])
def test_chunk_advance_is_bitwise_neutral(dev, d, scenario, bg):
    on = _run(d, scenario, adv=True, bg=bg)
    off = _run(d, scenario, adv=False, bg=bg)
    streamed = _run(d, scenario, adam_mode='streamed')
    assert on[2] == off[2] == streamed[2] and len(on[2]) > 2 * CHUNK
    for a, b, c in zip(on[0], off[0], streamed[0]):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(on[1], off[1]):
        assert torch.equal(a, b)


def test_advance_brings_each_row_to_its_first_read(dev):
    from recbole_amd import ops
    d = 128
    ref = _run(d, 'plain', adv=True, bg=True)
    opt, step = _build(dev, d)
    losses = step.run_epoch()                    # epoch 1: most rows leave the zero state
    step.begin_epoch()
    torch.cuda.synchronize()
    slot = step.slots[0]
    b0, nb, Bc = step._plan[0]
    assert b0 == 0 and nb == CHUNK and step._adv[0] and slot.chunk == step._plan[0]
    before = [x.cpu().clone() for x in (step.lastU, step.lastI)]
    step._advance(slot, torch.cuda.current_stream(dev), nb)    # what run_batches starts with
    torch.cuda.synchronize()
    for l, per, n, first, was, now in zip(slot.tab, (Bc, 5 * Bc), (step.nU, step.nI), slot.first,
                                          before, (step.lastU, step.lastI)):
        uniq, nu = l.uniq.cpu().numpy(), l.nu.cpu().numpy()
        exp = np.full(n, -1, dtype=np.int32)
        for c in reversed(range(nb)):
            exp[uniq[c * per:c * per + nu[c]]] = c
        first = first.cpu().numpy()
        assert np.array_equal(first, exp)
        was, now = was.numpy(), now.cpu().numpy()
        read = (first >= 0) & (was != ops.ADAM_ZERO_STATE)
        assert read.sum() > nb and (first[read] > 0).any()
        assert np.array_equal(now[read], b0 + first[read])
        assert np.array_equal(now[~read], was[~read])
    step.run_batches(0, step.n_batches)          # the chunk's own advance finds nothing to do
    losses += step.end_epoch()
    got = _result(opt, step, losses)
    assert got[2] == ref[2]
    for a, b in zip(got[0] + got[1], ref[0] + ref[1]):
        assert torch.equal(a, b)
