"""The chunk plan of the fused train step (trainer/chunk_plan.py) as pure functions,
pinned to the values the methods of FusedBPRTrainStep computed before they moved
there (obtained by calling them on a bare object with the attributes filled in).
CPU only: the module is loaded from its file, and imports nothing but the stdlib
and numpy."""
import ast
import importlib.util
import os
import sys

from conftest import ROOT

PATH = os.path.join(ROOT, 'recbole_amd', 'trainer', 'chunk_plan.py')
_spec = importlib.util.spec_from_file_location('_chunk_plan_under_test', PATH)
cp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cp)

F, T_ = False, True


def _flags(plan, Bg, n_rows=(138494, 26745), busy0=None, flush_every=64, flush_at=(),
           adam_mode='deferred', d=128, times=4, max_rows=8):
    return cp.chunk_flags(plan, Bg, flush_every, set(flush_at), times, adam_mode, d, n_rows,
                          n_rows if busy0 is None else busy0, max_rows)


def test_module_needs_no_torch():
    tree = ast.parse(open(PATH).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name.split('.')[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or '.').split('.')[0] if node.level == 0 else '.')
    assert mods <= set(sys.stdlib_module_names) | {'numpy'}, mods


def test_bench_shaped_plan():
    plan = cp.plan_chunks(20_000_000, 512, 64, (8, 16, 32), cuts=(5, 25, 89), ramps=(0, 5))
    assert len(plan) == 614
    assert plan[:6] == [(0, 5, 512), (5, 8, 512), (13, 12, 512), (25, 64, 512), (89, 64, 512),
                        (153, 64, 512)]
    assert plan[-2:] == [(39001, 61, 512), (39062, 1, 256)]
    flags = _flags(plan, 512, flush_at={25, 89})
    assert flags[:3] == [(F, F), (T_, F), (T_, (1, 1))]
    assert set(flags[3:]) == {(F, (1, 1))} and len(flags) == 614
    assert [cp.chunk_of(plan, b) for b in (0, 4, 5, 12, 13, 24, 25, 88, 89, 39062)] == \
        [0, 0, 1, 1, 2, 2, 3, 3, 4, 613]
    # every batch of the first chunks, against a linear scan
    for b in range(0, 400):
        k = cp.chunk_of(plan, b)
        assert plan[k][0] <= b < plan[k][0] + plan[k][1]


def test_ragged_plan():
    plan = cp.plan_chunks(1000, 96, 8, (8, 16, 32))
    assert plan == [(0, 8, 96), (8, 2, 96), (10, 1, 40)]
    assert _flags(plan, 96) == [(F, F), (T_, (1, 1)), (F, (1, 1))]
    assert _flags(plan, 96, busy0=(0, 0)) == [(F, F), (T_, (8, 4)), (F, (8, 4))]


def test_sparse_flush_rows():
    plan = cp.plan_chunks(96 * 300 + 5, 96, 64, (8, 16, 32))
    assert [c[1] for c in plan[:-1]] == [8, 16, 32, 64, 64, 64, 52] and plan[0][0] == 0
    assert all(a[0] + a[1] == b[0] for a, b in zip(plan[:-1], plan[1:]))
    assert plan[-1] == (300, 1, 5)
    assert _flags(plan, 96, n_rows=(100000, 100000), busy0=(10, 10)) == \
        [(F, F), (T_, F), (T_, (8, 2)), (F, (8, 1)), (F, (4, 1)), (F, (4, 1)), (F, (2, 1)),
         (F, (2, 1))]
    # the flush after the epoch's last enqueued batch (sync_params)
    assert cp.flush_rows(56, 96, 4, 'deferred', 128, (100000, 100000), (10, 10), 8) == (8, 2)
    assert cp.flush_rows(56, 96, 4, 'deferred', 32, (100000, 100000), (10, 10), 8) == (1, 1)


def test_streamed_plan():
    plan = cp.plan_chunks(96 * 300, 96, 64, (8, 16, 32))
    assert [c[1] for c in plan] == [8, 16, 32, 64, 64, 64, 52]
    assert all(c[2] == 96 for c in plan)
    assert _flags(plan, 96, adam_mode='streamed') == \
        [(F, F), (T_, F), (T_, (1, 1)), (F, (1, 1)), (F, (1, 1)), (F, (1, 1)), (F, (1, 1))]


def test_custom_ramp_plan():
    plan = cp.plan_chunks(96 * 40, 96, 4, (2,), cuts=(7,))
    assert plan == [(b0, nb, 96) for b0, nb in
                    [(0, 2), (2, 4), (6, 1), (7, 4), (11, 4), (15, 4), (19, 4), (23, 4), (27, 4),
                     (31, 4), (35, 4), (39, 1)]]
    assert _flags(plan, 96, flush_every=8, flush_at={7}) == \
        [(F, F), (T_, F), (T_, (1, 1)), (F, F), (T_, (1, 1)), (F, F), (T_, (1, 1)), (F, F),
         (T_, (1, 1)), (F, F), (T_, (1, 1)), (F, (1, 1))]
