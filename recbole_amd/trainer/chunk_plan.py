"""The chunk plan of the fused train step (trainer/fused.py) as pure integer
arithmetic: which global batches form a chunk, which chunks start with an entry
catch-up and end with a flush of the deferred Adam schedule, how many rows per
wave that flush runs, and which chunks split that flush (background flush) or are
preceded by the chunk advance. Nothing here touches a device (stdlib only)."""
from __future__ import annotations

import bisect
import math


def plan_chunks(n, Bg, C, ramp, cuts=(), ramps=(0,)):
    """(first global batch, batches, global batch size) per chunk for n positives in
    global batches of Bg: chunks of at most C full batches, starting at 0 and at
    every batch index in `cuts`, then the ragged last batch on its own. From each
    batch index in `ramps` (where the prep pipeline starts empty) up to the next
    cut, the chunk sizes ramp up (`ramp`, then C): the first steps wait for a short
    walk, not a C-batch one, and each next walk runs beside the previous chunk's
    steps."""
    full = n // Bg
    bounds = sorted({0, full} | {int(c) for c in cuts if 0 < int(c) < full})
    ramp_at = {int(r) for r in ramps}
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ri = 0 if lo in ramp_at else len(ramp)
        b0 = lo
        while b0 < hi:
            size = ramp[ri] if ri < len(ramp) else C
            ri += 1
            nb = min(size, C, hi - b0)
            out.append((b0, nb, Bg))
            b0 += nb
    if n % Bg:
        out.append((full, 1, n % Bg))
    return out


def flush_rows(b_end, Bg, times, adam_mode, d, n_rows, busy0, max_rows):
    """Rows per wave of the flush after global batch b_end - 1, per table (users,
    items): an upper bound on the rows that can lag = the rows outside the zero
    state at the epoch start (busy0) + every row the steps since then touched (Bg
    users, (1 + times) * Bg item slots per step) out of the table's n_rows; R = the
    largest power of two <= max_rows with R x that fraction <= 1 (one wave per row,
    R = 1, where most rows lag)."""
    if adam_mode != 'deferred' or d < 64:
        return (1, 1)
    out = []
    for per, rows, busy in zip((Bg, (1 + times) * Bg), n_rows, busy0):
        frac = min(1.0, (busy + b_end * per) / max(rows, 1))
        r = 1
        while r * 2 <= max_rows and r * 2 * frac <= 1.0:
            r *= 2
        out.append(r)
    return tuple(out)


def chunk_flags(plan, Bg, flush_every, flush_at, times, adam_mode, d, n_rows, busy0, max_rows):
    """(entry, flush) per chunk of `plan`: a chunk flushes every row at its end once
    flush_every or more steps have run since the last flush, or when the next chunk
    would take the count past 1.5 x flush_every (the ramp's steps flush before the
    first C-step chunk instead of after it), before a ragged batch / the end, and
    where it ends at a batch index in `flush_at`; a chunk after one that did not
    flush starts with an entry catch-up of the rows its first batch reads. `flush`
    is False or the flush's rows per wave per table (flush_rows: a tuple, part of the
    chunk graph's key)."""
    flags, since = [], 0
    for i, (b0, nb, _) in enumerate(plan):
        entry = since > 0
        since += nb
        nxt_full = i + 1 < len(plan) and plan[i + 1][2] == Bg
        nxt_nb = plan[i + 1][1] if i + 1 < len(plan) else 0
        flush = (since >= flush_every or since + nxt_nb > flush_every * 3 // 2
                 or not nxt_full or b0 + nb in flush_at)
        if flush:
            since = 0
        flags.append((entry, flush_rows(b0 + nb, Bg, times, adam_mode, d, n_rows, busy0,
                                        max_rows) if flush else False))
    return flags


def bg_flush_chunks(plan, flags, Bg, adam_mode, fused_step, use_graph, min_steps=1,
                    enabled=True):
    """Per chunk of `plan`: does its flush split into a background part (the user rows
    the chunk never reads, flushed early beside the chunk's steps) and a masked
    foreground part (fused.py)? Only for a chunk of full batches that ends with a flush
    on the one-GPU fused step (K35: `fused_step`) with the deferred schedule and captured
    chunk graphs; never on the streamed, replicated or sharded steps (their fused_step
    is False). The background part runs on a bounded grid, several times slower than
    the full flush it replaces, so it pays only where the chunk's own steps cover it:
    the chunk has at least min_steps steps, and the lag it flushes is no longer than the
    chunk (the chunk before it flushed: no entry catch-up). Whether such a chunk then
    runs as a whole graph is decided when it runs (bg_flush_now)."""
    on = bool(enabled and fused_step and use_graph and adam_mode == 'deferred')
    return [bool(on and flush and not entry and Bc == Bg and nb >= min_steps)
            for (_, nb, Bc), (entry, flush) in zip(plan, flags)]


def bg_flush_now(planned, c0, c1, nb, graph_ready, timed_kernels):
    """Does the run of batches [c0, c1) of an nb-batch chunk launch the background flush:
    the chunk was planned for it (bg_flush_chunks) and replays its captured graph as a
    whole. A chunk entered mid-way, cut short, timed per kernel or without a captured
    graph runs eagerly and keeps the full flush."""
    return bool(planned and c0 == 0 and c1 == nb and graph_ready and not timed_kernels)


def masked_flush_rows(flush, nb, Bg, n_users, max_rows):
    """Rows per wave of a chunk's masked foreground flush, from its full flush's `flush`
    (flush_rows): the user table takes only the rows the chunk's nb batches read, at
    most nb * Bg of its n_users rows, so R = the largest power of two <= max_rows with
    R x min(1, nb * Bg / n_users) <= 1; the item table is flushed whole, as before."""
    frac = min(1.0, nb * Bg / max(n_users, 1))
    r = 1
    while r * 2 <= max_rows and r * 2 * frac <= 1.0:
        r *= 2
    return (r,) + tuple(flush[1:])


def advance_chunks(plan, Bg, adam_mode, fused_step, use_graph, min_steps=1, enabled=True):
    """Per chunk of `plan`: is its captured graph preceded by the chunk advance (fused.py:
    every row the chunk reads is brought to the step of its first read in one flush launch,
    in place of the entry catch-up and of the look-ahead replays of those first reads)?
    Only for a chunk of full batches on the one-GPU fused step (K35: `fused_step`) with the
    deferred schedule and captured chunk graphs; never on the streamed, replicated or
    sharded steps (their fused_step is False), which keep the entry catch-up and the step
    kernel's own look-ahead. The advance is one more launch in front of the chunk's steps,
    so the chunk has at least min_steps steps. The advance goes with the captured graph
    only: a planned chunk that is entered mid-way, cut short or timed per kernel runs
    eagerly, with the entry catch-up and the step kernel's look-ahead."""
    on = bool(enabled and fused_step and use_graph and adam_mode == 'deferred')
    return [bool(on and Bc == Bg and nb >= min_steps) for _, nb, Bc in plan]


def advance_rows(nb, Bg, times, n_rows, max_rows):
    """Rows per wave of a chunk's advance launch, per table (users, items), chosen as
    masked_flush_rows chooses: the launch takes only the rows the chunk's nb batches read,
    at most nb * Bg users and nb * (1 + times) * Bg items of the tables' n_rows, so R = the
    largest power of two <= max_rows with R x that fraction <= 1."""
    out = []
    for per, rows in zip((Bg, (1 + times) * Bg), n_rows):
        frac = min(1.0, nb * per / max(rows, 1))
        r = 1
        while r * 2 <= max_rows and r * 2 * frac <= 1.0:
            r *= 2
        out.append(r)
    return tuple(out)


def chunk_of(plan, b):
    """Index of the chunk of `plan` holding global batch b (0 below the first)."""
    return max(bisect.bisect_right(plan, (b, math.inf)) - 1, 0)
