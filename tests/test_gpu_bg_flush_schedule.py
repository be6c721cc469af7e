"""The background flush of the fused train step (trainer/fused.py BG_FLUSH): a flushing
chunk's idle user rows are flushed beside its steps and its closing flush takes the rest.
FusedBPRTrainStep with BG_FLUSH on, with it off, and on the streamed Adam schedule leave
the tables, the moments, the per-row step counts and the per-step losses bit-identical —
on whole-graph chunks, a bench.py-shaped window, a chunk entered mid-way (eager, full
flush) and ramp chunks that do not flush."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = (600, 200, 4000)      # users, items, interactions asked of the generator
CHUNK = 8


def _run(dev, d, scenario, adam_mode='deferred', bg=True):
    import bench
    _, train, _, _, opt, step = bench.build_workload(
        dev, d=d, batch_rows=256, adam_mode=adam_mode, chunk=CHUNK, source='memory', shape=SHAPE)
    assert step.Bg == 64 and step.times == 4
    assert step.fused_step == (adam_mode == 'deferred')
    step.FLUSH_EVERY = CHUNK
    step.BG_FLUSH = bg
    step.BG_MIN_STEPS = 4                        # the short chunks of this test qualify
    step.RAMP = (2, 3) if scenario == 'ramp' else step.RAMP
    launched = []
    inner = step._flush_background
    step._flush_background = lambda slot, t_end, stream: (launched.append(t_end),
                                                          inner(slot, t_end, stream))
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
    elif scenario == 'mid':                      # chunk [8, 16) cut short, then entered mid-way
        nb = step.begin_epoch()
        step.run_batches(0, 11)
        step.run_batches(11, nb)
        losses += step.end_epoch()
        assert step.n_eager_steps >= CHUNK
    else:
        losses += step.run_epoch()
    if scenario == 'ramp':                       # the ramp's first chunk does not flush
        assert step._plan[0][1] == 2 and not step._flags[0][1] and step._flags[1][1]
    n_first = len(launched)
    losses += step.run_epoch()                   # a second epoch: the state carries over
    planned = sum(step._bg)
    if bg and adam_mode == 'deferred':
        assert n_first > 0 and len(launched) - n_first == planned > 0
    else:
        assert not launched and planned == 0
    state = [step.pU.detach(), step.pI.detach()]
    for p in (step.pU, step.pI):
        state += [opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']]
    last = [step.lastU, step.lastI] if adam_mode == 'deferred' else []
    out = [x.cpu().clone() for x in state], [x.cpu().clone() for x in last], losses
    step.close()
    return out


@pytest.mark.parametrize('d,scenario', [(64, 'plain'), (128, 'plain'), (128, 'bench'),
                                        (64, 'mid'), (128, 'ramp')])
def test_background_flush_is_bitwise_neutral(dev, d, scenario):
    on = _run(dev, d, scenario, bg=True)
    off = _run(dev, d, scenario, bg=False)
    streamed = _run(dev, d, scenario, adam_mode='streamed')
    assert on[2] == off[2] == streamed[2] and len(on[2]) > 2 * CHUNK
    for a, b, c in zip(on[0], off[0], streamed[0]):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(on[1], off[1]):
        assert torch.equal(a, b)
