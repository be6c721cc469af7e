"""The background-flush part of the chunk plan (trainer/chunk_plan.py): which chunks
split their closing flush into a background half and a masked foreground half, that no
chunk does on the eager, streamed, replicated or sharded paths, and the rows per wave
of the masked foreground flush. CPU only: pure integer logic, loaded from its file."""
import importlib.util
import os

from conftest import ROOT

PATH = os.path.join(ROOT, 'recbole_amd', 'trainer', 'chunk_plan.py')
_spec = importlib.util.spec_from_file_location('_chunk_plan_bg_under_test', PATH)
cp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cp)

N_ROWS = (138494, 26745)


def _plan_flags(n, Bg, C, ramp, cuts=(), ramps=(0,), flush_at=(), adam_mode='deferred'):
    plan = cp.plan_chunks(n, Bg, C, ramp, cuts=cuts, ramps=ramps)
    flags = cp.chunk_flags(plan, Bg, 64, set(flush_at), 4, adam_mode, 128, N_ROWS, N_ROWS, 8)
    return plan, flags


def test_bench_window_chunks():
    # bench.py's default window: 64 warm-up steps, 256 timed, cut and flushed at both ends
    plan, flags = _plan_flags(20_000_000, 512, 64, (8, 16, 32), cuts=(64, 320, 384),
                              ramps=(0, 64), flush_at=(320, 384))
    bg = cp.bg_flush_chunks(plan, flags, 512, 'deferred', True, True, min_steps=32)
    assert len(bg) == len(plan)
    timed = [(c[1], bool(f[1]), b) for c, f, b in zip(plan, flags, bg) if 64 <= c[0] < 320]
    # the ramp's first chunks do not flush; its last one flushes 56 steps of lag beside 32
    # steps, and the window's closing chunk has 8 steps: neither covers a background flush
    assert timed == [(8, False, False), (16, False, False), (32, True, False), (64, True, True),
                     (64, True, True), (64, True, True), (8, True, False)]
    for (_, nb, Bc), (entry, flush), b in zip(plan, flags, bg):
        assert b == (bool(flush) and not entry and Bc == 512 and nb >= 32)
    # every flushing chunk of full batches that follows a flush, whatever its length
    every = cp.bg_flush_chunks(plan, flags, 512, 'deferred', True, True)
    assert [b for c, b in zip(plan, every) if 64 <= c[0] < 320] == \
        [False, False, False, True, True, True, True]
    # bench.py's driver window (warm-up 5, 20 steps): chunks of 8 and 12, no background
    plan, flags = _plan_flags(20_000_000, 512, 64, (8, 16, 32), cuts=(5, 25, 89),
                              ramps=(0, 5), flush_at=(25, 89))
    bg = cp.bg_flush_chunks(plan, flags, 512, 'deferred', True, True, min_steps=32)
    assert [c[1] for c in plan[:4]] == [5, 8, 12, 64] and bg[:4] == [False, False, False, True]
    # the ragged last batch flushes, but is not a chunk of full batches
    assert plan[-1][2] != 512 and flags[-1][1] and not bg[-1]


def test_no_background_off_the_fused_graph_path():
    plan, flags = _plan_flags(96 * 300, 96, 64, (8, 16, 32))
    assert any(cp.bg_flush_chunks(plan, flags, 96, 'deferred', True, True))
    # switched off; K3 + K5, replicated and sharded steps (fused_step False); no graphs
    assert not any(cp.bg_flush_chunks(plan, flags, 96, 'deferred', True, True, enabled=False))
    assert not any(cp.bg_flush_chunks(plan, flags, 96, 'deferred', True, True, min_steps=65))
    assert not any(cp.bg_flush_chunks(plan, flags, 96, 'deferred', False, True))
    assert not any(cp.bg_flush_chunks(plan, flags, 96, 'deferred', True, False))
    # the streamed schedule has nothing to flush
    splan, sflags = _plan_flags(96 * 300, 96, 64, (8, 16, 32), adam_mode='streamed')
    assert not any(cp.bg_flush_chunks(splan, sflags, 96, 'streamed', True, True))
    assert not any(cp.bg_flush_chunks(splan, sflags, 96, 'streamed', False, True))


def test_background_only_for_a_whole_graph_replay():
    assert cp.bg_flush_now(True, 0, 64, 64, True, False)
    assert not cp.bg_flush_now(False, 0, 64, 64, True, False)     # not planned
    assert not cp.bg_flush_now(True, 3, 64, 64, True, False)      # entered mid-way
    assert not cp.bg_flush_now(True, 0, 40, 64, True, False)      # cut short
    assert not cp.bg_flush_now(True, 0, 64, 64, False, False)     # no captured graph
    assert not cp.bg_flush_now(True, 0, 64, 64, True, True)       # per-kernel events: eager


def test_masked_flush_rows_bound():
    # the user table's R from min(1, nb * Bg / n_users); the item table's as planned
    assert cp.masked_flush_rows((1, 1), 64, 512, 138494, 8) == (4, 1)    # 0.237 of the rows
    assert cp.masked_flush_rows((1, 1), 8, 512, 138494, 8) == (8, 1)     # 0.030: capped at 8
    assert cp.masked_flush_rows((2, 4), 32, 512, 138494, 8) == (8, 4)    # 0.118
    assert cp.masked_flush_rows((1, 1), 32, 512, 138494, 64) == (8, 1)   # 16 x 0.118 > 1
    assert cp.masked_flush_rows((1, 2), 4, 64, 600, 8) == (2, 2)         # 0.427
    assert cp.masked_flush_rows((1, 1), 8, 64, 600, 8) == (1, 1)         # 0.853
    assert cp.masked_flush_rows((1, 1), 64, 512, 1000, 8) == (1, 1)      # every row may be read
    for nb in (1, 7, 64):
        for n_users in (100, 5000, 138494):
            r = cp.masked_flush_rows((1, 3), nb, 512, n_users, 8)[0]
            assert r in (1, 2, 4, 8) and (r == 1 or r * min(1.0, nb * 512 / n_users) <= 1.0)
            assert r == 8 or 2 * r * min(1.0, nb * 512 / n_users) > 1.0
