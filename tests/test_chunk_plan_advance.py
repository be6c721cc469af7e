"""The chunk-advance part of the chunk plan (trainer/chunk_plan.py): which chunks' graphs
are preceded by the advance launch, that no chunk does on the eager, streamed, replicated or
sharded paths or below the minimum length, and the rows per wave of the advance launch.
CPU only: pure integer logic, loaded from its file."""
import importlib.util
import os

from conftest import ROOT

PATH = os.path.join(ROOT, 'recbole_amd', 'trainer', 'chunk_plan.py')
_spec = importlib.util.spec_from_file_location('_chunk_plan_adv_under_test', PATH)
cp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cp)


def test_bench_window_chunks():
    # bench.py's default window: 64 warm-up steps, 256 timed, cut at both ends
    plan = cp.plan_chunks(20_000_000, 512, 64, (8, 16, 32), cuts=(64, 320, 384), ramps=(0, 64))
    adv = cp.advance_chunks(plan, 512, 'deferred', True, True, min_steps=32)
    assert len(adv) == len(plan)
    timed = [(c[1], a) for c, a in zip(plan, adv) if 64 <= c[0] < 320]
    assert timed == [(8, False), (16, False), (32, True), (64, True), (64, True), (64, True),
                     (8, False)]
    # whether a chunk flushes or starts with an entry catch-up plays no part: length only
    assert [a for c, a in zip(plan, cp.advance_chunks(plan, 512, 'deferred', True, True))
            if 64 <= c[0] < 320] == [True] * 7
    # the driver window (warm-up 5, 20 steps): chunks of 5, 8 and 12 are short
    plan = cp.plan_chunks(20_000_000, 512, 64, (8, 16, 32), cuts=(5, 25, 89), ramps=(0, 5))
    adv = cp.advance_chunks(plan, 512, 'deferred', True, True, min_steps=32)
    assert [c[1] for c in plan[:4]] == [5, 8, 12, 64] and adv[:4] == [False, False, False, True]
    # the ragged last batch is not a chunk of full batches
    assert plan[-1][2] != 512 and not adv[-1]
    assert not cp.advance_chunks(plan, 512, 'deferred', True, True, min_steps=1)[-1]


def test_no_advance_off_the_fused_graph_path():
    plan = cp.plan_chunks(96 * 300, 96, 64, (8, 16, 32))
    assert all(cp.advance_chunks(plan, 96, 'deferred', True, True))
    assert not any(cp.advance_chunks(plan, 96, 'deferred', True, True, enabled=False))
    assert not any(cp.advance_chunks(plan, 96, 'deferred', True, True, min_steps=65))     # short
    # K3 + K5, replicated and sharded steps (fused_step False)
    assert not any(cp.advance_chunks(plan, 96, 'deferred', False, True))
    # eager: no captured graphs
    assert not any(cp.advance_chunks(plan, 96, 'deferred', True, False))
    # the streamed schedule has no lag to advance
    assert not any(cp.advance_chunks(plan, 96, 'streamed', True, True))
    assert not any(cp.advance_chunks(plan, 96, 'streamed', False, True))
    assert cp.advance_chunks([], 96, 'deferred', True, True) == []


def test_advance_rows_bound():
    n_rows = (138494, 26745)
    assert cp.advance_rows(64, 512, 4, n_rows, 8) == (4, 1)      # users 0.237, items all
    assert cp.advance_rows(16, 512, 4, n_rows, 8) == (8, 1)      # users 0.059, items all
    assert cp.advance_rows(2, 512, 4, n_rows, 8) == (8, 4)       # items 0.191
    assert cp.advance_rows(8, 64, 4, (600, 200), 8) == (1, 1)
    assert cp.advance_rows(1, 64, 4, (600, 2000), 8) == (8, 4)   # 0.107 / 0.16
    # the user table's choice is the masked foreground flush's
    for nb in (1, 7, 64):
        for n_users in (100, 5000, 138494):
            r = cp.advance_rows(nb, 512, 4, (n_users, 1000), 8)
            assert r[0] == cp.masked_flush_rows((1, 1), nb, 512, n_users, 8)[0]
            assert r[0] in (1, 2, 4, 8) and r[1] in (1, 2, 4, 8)
