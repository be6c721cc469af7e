"""The fused pairwise train step with row-sharded tables (see ShardedBPRTrainStep)."""
from __future__ import annotations

import ctypes
import logging
import math
import os

import torch

from recbole_amd import ops
from recbole_amd._native import check, lib
from recbole_amd.trainer.fused import FusedBPRTrainStep, _Lists, _Slot


class _ShardLists(_Lists):
    """A table's grouping of the slots this rank owns (over owner-major keys), and
    what the sharded step derives from it: `keyed` / `sel` the selected slots' keys
    and places in the global batch, `own` the owned rows' lists with the
    contributions' places in the backward messages (the step's Adam lists), and for
    the ipc exchange `next_t` / `next_a`, the owner's push lists (mirec_shard_next)."""

    def __init__(self, C, per, dev, push):
        super().__init__(C, per, dev, True)
        i32 = dict(dtype=torch.int32, device=dev)
        self.keyed = torch.empty(C * per, dtype=torch.int64, device=dev)
        self.sel = torch.empty(C * per, **i32)
        self.own = _Lists(C, per, dev, True)
        self.next_t = torch.empty(C * per, **i32) if push else None
        self.next_a = torch.empty(C * per, **i32) if push else None


class _ShardSlot(_Slot):
    """A chunk's buffers for the sharded step: the base's keys, per table the
    _ShardLists, and the exchange plans."""

    def __init__(self, C, B, T, G, dev, push):
        Bg = G * B
        super().__init__(C, B, T, G, dev, True,
                         tab=[_ShardLists(C, per, dev, push) for per in (Bg, (1 + T) * Bg)])
        self.map2 = torch.empty(C * (2 + T) * Bg, dtype=torch.int32, device=dev)
        self.pos = torch.empty(C * (2 + T) * B, dtype=torch.int64, device=dev)
        # this chunk's plan status ([overflow, largest message, owned user / item slots]),
        # read by the host before the chunk's model side is launched (_enter_chunk)
        self.plan_status = torch.zeros(4, dtype=torch.int32, device=dev)
        self.plan_status_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.planned = torch.cuda.Event()
        self.fwd_rows = self.bwd_src = None     # the message plans, sized by cap (_alloc_exchange)


class ShardedBPRTrainStep(FusedBPRTrainStep):
    """The fused pairwise step with ROW-SHARDED tables over G ranks:
    rank r owns rows id % G == r of both tables (parameters, Adam m / v and the
    deferred step counts) as a [S, d] shard, S = ceil(n / G).

    Per optimizer step over a global batch of G*B positives (csrc/shard.hip):
      prep (replicated on every rank, prep stream): walk + K2 grouping of the global
        batch over owner-major keys, the exchange plans and this rank's slice of the
        grouping (mirec_shard_plan / mirec_shard_own);
      forward exchange: each owner gathers the rows every slice needs from its shards
        (mirec_shard_gather_f32) and one all-to-all (RCCL over xGMI; equal blocks of
        `cap` rows per rank pair) delivers them;
      K3 on this rank's slice of positives, reading rows from the receive buffer;
      backward exchange: the slice's per-slot gradient rows go back to the owners
        in the same message positions (second all-to-all);
      K5 (deferred) on the owned rows only, summing each row's contributions in the
        global grouping order — the result is bit-identical to one GPU running the
        global batch;
      per chunk: one all-gather of the per-positive losses for the loss history.
    The dominant optimizer work (touched rows + flush) is 1/G per rank. The model's
    full parameter tensors are written back from the shards at end_epoch() (one
    all-gather of p, m, v per epoch) for evaluation and checkpoints, and re-read
    into the shards at begin_epoch(). With dist=None it runs the same protocol on
    one rank (G = 1; the all-to-alls are copies)."""

    CAP_SLACK = 1.25
    # the per-step row exchanges: 'rccl' (two all-to-alls of equal blocks) or 'ipc' (the
    # owners' gather stores into the readers' IPC-mapped windows, K3 stores the gradient
    # rows into the owners' windows, flags on the GPU: csrc/comm.hip, trainer/comm.py)
    EXCHANGE = os.environ.get('MIREC_EXCHANGE', 'rccl')

    def __init__(self, model, optimizer, train_data, chunk=None, use_graph=True,
                 adam_mode='deferred', dist=None, cap=None, exchange=None):
        if adam_mode != 'deferred':
            raise ValueError('the row-sharded step runs the deferred Adam schedule')
        exchange = exchange or self.EXCHANGE
        if exchange not in ('rccl', 'ipc'):
            raise ValueError(f"exchange must be 'rccl' or 'ipc', got {exchange!r}")
        self._solo = dist is None            # one rank, no process group: no collectives
        self.exchange = 'rccl' if self._solo else exchange
        self.cap = cap                       # (None: _allocate sizes it)
        super().__init__(model, optimizer, train_data, chunk=chunk, use_graph=use_graph,
                         adam_mode=adam_mode, dist=dist, fused_step=False)

    def _allocate(self):
        """The shards instead of full-size step counts and gradient rows, the sharded
        slots and the exchange buffers."""
        G, B, T, d, dev, C = self.G, self.B, self.times, self.d, self.device, self.C
        Bg, KI = self.Bg, (1 + T) * self.Bg
        self.SU, self.SI = -(-self.nU // G), -(-self.nI // G)
        # rows per (slice, owner) message: the slice's (2+T)*B slots spread over G
        # owners (cyclic ownership); a chunk whose plan overflows is re-planned with a
        # larger cap before it runs (_enter_chunk), never run on a truncated plan
        self.cap = int(self.cap or min((2 + T) * B,
                                       math.ceil(self.CAP_SLACK * (2 + T) * B / G) + 64))
        self.shU = [torch.zeros(self.SU, d, device=dev) for _ in range(3)]   # p, m, v
        self.shI = [torch.zeros(self.SI, d, device=dev) for _ in range(3)]
        self.lastU = torch.zeros(self.SU, dtype=torch.int32, device=dev)
        self.lastI = torch.zeros(self.SI, dtype=torch.int32, device=dev)
        self.xbuf = torch.empty(1, dtype=torch.float32, device=dev)   # _entry's unread rows
        self.win = None
        if self.exchange == 'ipc':           # every rank's receive window, mapped everywhere
            from recbole_amd.trainer.comm import PeerWindows
            self.win = PeerWindows(self.group, (2 + T) * B, d, dev)
        self.loss_mine = torch.zeros(C * B, dtype=torch.float32, device=dev)
        self.status = torch.zeros(2, dtype=torch.int32, device=dev)    # epoch backstop
        self.cap_growths = 0
        self.slots = [_ShardSlot(C, B, T, G, dev, self.win is not None)
                      for _ in range(self.SLOTS)]
        # slots per (batch, table) a rank's owner-filtered grouping holds (its ~1/G share
        # of the global batch with slack; a batch over it is re-selected at the table's
        # full size before its chunk runs: _enter_chunk)
        self.cap_sel = {tag: min(per, math.ceil(self.CAP_SLACK * per / G) + 64)
                        for tag, per in (('u', Bg), ('i', KI))}
        self.sel_growths = 0
        self._alloc_exchange()
        self._n_max = (ctypes.c_int64 * 2)(min(Bg, self.SU), min(KI, self.SI))
        self._fill_tables()

    def _alloc_exchange(self):
        """Buffers sized by `cap`: the two all-to-all send / receive buffers (rccl; the
        ipc exchange receives in the windows, sized for the largest cap) and the per-slot
        message plans."""
        M, d, dev = self.G * self.cap, self.d, self.device
        if self.win is None:
            self.sendF = torch.empty(M, d, device=dev)
            self.recvF = self.sendF if self._solo else torch.empty(M, d, device=dev)
            self.sendB = torch.empty(M, d, device=dev)
            self.recvB = self.sendB if self._solo else torch.empty(M, d, device=dev)
        for sl in self.slots:
            sl.fwd_rows = torch.empty(self.C * M, dtype=torch.int64, device=dev)
            sl.bwd_src = torch.empty(self.C * M, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------ shards <-> full tensors
    def _owned_ids(self, n, S):
        ids = torch.arange(S, device=self.device, dtype=torch.int64) * self.G + self.rank
        return ids[ids < n]

    def _full_and_shards(self):
        """(full p, m, v), their shards, rows, rows per shard — per table."""
        stU, stI = self.opt.state[self.pU], self.opt.state[self.pI]
        return (((self.pU.data, stU['exp_avg'], stU['exp_avg_sq']), self.shU, self.nU, self.SU),
                ((self.pI.data, stI['exp_avg'], stI['exp_avg_sq']), self.shI, self.nI, self.SI))

    def _load_shards(self):
        """Owned rows of the model's full p and the optimizer's m, v -> the shards."""
        for full, sh, n, S in self._full_and_shards():
            ids = self._owned_ids(n, S)
            for dst, src in zip(sh, full):
                dst[:ids.numel()].copy_(src[ids])

    def _store_shards(self):
        """All shards -> the full p, m, v on every rank (one all-gather each)."""
        for full, sh, n, S in self._full_and_shards():
            for src, dst in zip(sh, full):
                g = self._all_gather(src)                       # [G*S, d], owner-major
                dst.copy_(g.view(self.G, S, self.d).transpose(0, 1).reshape(-1, self.d)[:n])

    def _all_gather(self, x):
        if self.group is None:
            return x
        from recbole_amd.trainer.dist import _gather_cat
        return _gather_cat(x, self.group)

    def _all_to_all(self, recv, send):
        if self.group is not None:                              # (one rank: recv is send)
            from recbole_amd.trainer.dist import all_to_all_blocks
            all_to_all_blocks(recv, send, self.group)

    # ------------------------------------------------------------ data side
    def _prepare(self, slot, chunk, on=None):     # on: a one-rank restart chunk's stream
        if slot.free_recorded:                    # (unused: the prep stream prepares it)
            self.prep_stream.wait_event(slot.free)
        with torch.cuda.stream(self.prep_stream):
            self._copy_keys_and_walk(slot, chunk)
            self._plan_chunk(slot, chunk, self.prep_stream.cuda_stream)
            slot.ready.record(self.prep_stream)
        slot.chunk = chunk

    def _plan_chunk(self, slot, chunk, st):
        """This rank's grouping of a walked chunk and its exchange plans (on the current
        stream, `st`): per table, the slots of the rows this rank owns (mirec_shard_select,
        ~1/G of the global batch), their K2 grouping over owner-major keys and look-ahead
        lists; the plans from the unsorted keys (mirec_shard_plan); the owned lists with the
        contributions' places in the backward messages (mirec_shard_own_sel). The plan
        status goes to pinned host memory."""
        _, nb, Bc = chunk
        T, G, r = self.times, self.G, self.rank
        KI = (1 + T) * Bc
        L = lib()
        p = lambda x: x.data_ptr()
        users = slot.user_keys[:nb * Bc]
        items = slot.item_keys[:nb * KI]
        tables = list(zip('ui', slot.tab, (Bc, KI), (self.SU, self.SI)))
        slot.plan_status.zero_()
        cs = {}
        for k, (ids, (tag, l, per, S)) in enumerate(zip((users, items), tables)):
            cs[tag] = c_ = min(self.cap_sel[tag], per)
            keyed = l.keyed[:nb * c_]
            check(L.mirec_shard_select(p(ids), nb, per, G, S, r, c_, p(keyed), p(l.sel),
                                       p(slot.plan_status) + 4 * (2 + k), st),
                  'mirec_shard_select')
            self.sort_ws = ops.segment_sort_batched(keyed, c_, G * S + 1, l.perm, l.uniq,
                                                    l.seg, l.nu, ws=self.sort_ws)
            ops.uniq_ahead_diff(l.uniq, l.nu, c_, nb, l.ahead, l.nah)
        check(L.mirec_shard_plan(p(users), p(items), nb, Bc, self.B, T, G, r, self.cap,
                                 p(slot.fwd_rows), p(slot.map2), p(slot.pos), p(slot.bwd_src),
                                 p(slot.plan_status), st), 'mirec_shard_plan')
        for (tag, l, per, S), off in zip(tables, (0, Bc)):
            o = l.own
            check(L.mirec_shard_own_sel(p(l.uniq), p(l.seg), p(l.nu), p(l.perm), cs[tag], nb,
                                        p(l.ahead), p(l.nah), p(slot.map2), Bc + KI, off, S, r,
                                        p(l.sel), per, p(o.uniq), p(o.seg), p(o.nu), p(o.perm),
                                        p(o.ahead), p(o.nah), st), 'mirec_shard_own_sel')
            if self.win is not None:
                check(L.mirec_shard_next(p(o.uniq), p(o.nu), p(o.ahead), p(o.nah), per, nb,
                                         p(l.next_t), p(l.next_a), st), 'mirec_shard_next')
        # epoch backstop: overflow flag (min: -4 < 0) and the largest message (max)
        torch.minimum(self.status[:1], slot.plan_status[:1], out=self.status[:1])
        torch.maximum(self.status[1:], slot.plan_status[1:2], out=self.status[1:])
        slot.plan_status_host.copy_(slot.plan_status, non_blocking=True)
        slot.planned.record(torch.cuda.current_stream(self.device))

    def _enter_chunk(self, k, stream):
        """Before chunk k's model side is enqueued: its plan must fit `cap`. Every rank
        counts every message, so all ranks see the same status and grow `cap` to the
        same value (no collective); the chunk and the prepared ones after it are
        re-planned. No step ever runs on an overflowed plan."""
        new = self._cur != k
        super()._enter_chunk(k, stream)
        if not new:
            return
        slot = self.slots[k % len(self.slots)]
        if not slot.planned.query():          # the plan status reaches pinned memory
            slot.planned.synchronize()
        over, most, sel_u, sel_i = (int(x) for x in slot.plan_status_host)
        _, _, Bc = self._plan[k]
        grow = {tag: n for tag, n, per in (('u', sel_u, Bc), ('i', sel_i, (1 + self.times) * Bc))
                if n > min(self.cap_sel[tag], per)}
        if grow:
            self._grow_sel(grow)
            over, most = (int(x) for x in slot.plan_status_host[:2])
        if over == -4:
            self._grow_cap(most)

    def _replan(self):
        """Re-plan the prepared chunks, from the one being entered, in order, from their
        walked keys; returns when they are done."""
        for q in range(self._cur, self._next_chunk):
            slot = self.slots[q % len(self.slots)]
            with torch.cuda.stream(self.prep_stream):
                self._plan_chunk(slot, self._plan[q], self.prep_stream.cuda_stream)
        torch.cuda.synchronize(self.device)

    def _grow_sel(self, grow):
        """A batch owns more slots of a table than its owner-filtered grouping holds:
        re-select + re-plan every prepared chunk with that table's full batch size (no
        overflow possible). The graphs stay (they read the owned lists, whose strides do
        not change)."""
        T, Bg = self.times, self.Bg
        logging.getLogger().warning(f'owner-filtered grouping: {grow} owned slots exceed '
                                    f'cap_sel={self.cap_sel}; re-selecting at full size')
        torch.cuda.synchronize(self.device)
        for tag in grow:
            self.cap_sel[tag] = Bg if tag == 'u' else (1 + T) * Bg
        self.sel_growths += 1
        self._replan()

    def _grow_cap(self, most):
        """Larger messages: reallocate the cap-sized buffers, re-plan every prepared
        chunk from its walked keys and recapture the chunk graphs."""
        T, B = self.times, self.B
        new_cap = min((2 + T) * B, max(most, math.ceil(self.CAP_SLACK * self.cap)))
        logging.getLogger().warning(f'row exchange: a (slice, owner) message of {most} rows '
                                    f'exceeds cap={self.cap}; re-planning with cap={new_cap}')
        torch.cuda.synchronize(self.device)
        self.cap = new_cap
        self.cap_growths += 1
        self._alloc_exchange()
        self._fill_tables()
        self.status.zero_()
        self._replan()
        if int(self.slots[self._cur % len(self.slots)].plan_status_host[0]) == -4:
            raise RuntimeError('row exchange plan still overflows after re-planning')
        self._drop_graphs()                                     # later chunks: checked on entry
        if self.use_graph:
            self._capture_variants()

    # ------------------------------------------------------------ model side
    def _fill_tables(self):
        for t, sh, last, S in zip(self._tables, (self.shU, self.shI), (self.lastU, self.lastI),
                                  (self.SU, self.SI)):
            t.p, t.m, t.v = (x.data_ptr() for x in sh)
            t.n_rows = S
            t.last = last.data_ptr()
            t.dense_grad = None
            t.rows = self.win.bwd if self.win is not None else self.recvB.data_ptr()

    def _adam_state(self):
        return [(self.shU[1], self.shU[2], self.lastU), (self.shI[1], self.shI[2], self.lastI)]

    def _entry_lists(self, slot):
        return [(l.own.uniq, l.own.nu) for l in slot.tab]

    def _n_local(self, Bc):
        return max(0, min(self.B, Bc - self.rank * self.B))

    def _step(self, slot, c, Bc, stream, step_off, ahead):
        T, B = self.times, self.B
        own = [l.own for l in slot.tab]
        n = self._n_local(Bc)
        pos = slot.pos.data_ptr() + 8 * c * (2 + T) * B     # this slice's rows in the messages
        bpr = (pos, pos + 8 * n, pos + 16 * n, n, T, 1e-10, self._grad_scale(Bc),
               self.loss_mine.data_ptr() + 4 * c * B)
        if self.win is not None:
            self._step_ipc(slot, c, bpr, stream)
        else:
            self._step_rccl(slot, c, bpr, stream)
        self._point_tables(self._tables, own, c, (Bc, (1 + T) * Bc), ahead)
        if self.win is not None:
            self._adam_ipc(slot, c, Bc, stream, step_off, ahead)
        else:
            self._adam(stream, step_off)
        self._note_uniq(own, c)

    def _step_ipc(self, slot, c, bpr, stream):
        """The forward half of a step through the peer windows (csrc/comm.hip). The chunk's
        first step pushes its rows with a gather launch (after the entry catch-up); later
        steps' rows were pushed by the step before's optimizer launch (_adam_ipc). K3's
        blocks wait for the owners' flags on the GPU (no separate wait launch), read the
        rows in the window and store each gradient row into its owner's window."""
        w = self.win.comm
        if c == 0:
            self._launch('gather', stream, 'mirec_comm_push_rows_f32', w, self.shU[0].data_ptr(),
                         self.shI[0].data_ptr(), slot.fwd_rows.data_ptr(), self.cap)
        # every rank launches it (n = 0 too): its last block raises the flags
        self._launch('bpr', stream, 'mirec_comm_bpr_f32', w, *bpr, self.cap)

    def _adam_ipc(self, slot, c, Bc, stream, step_off, ahead):
        """The owner's deferred Adam with the backward wait and, unless c is the chunk's
        last step, the next step's forward push folded in (mirec_comm_adam_deferred_f32):
        every row step c+1 reads is in this launch's touched or look-ahead list, and goes
        from registers to its readers' windows right after its update."""
        nxt = seg = dst = None
        if ahead:
            at = lambda x, off: x.data_ptr() + 4 * off
            tabs = list(zip(slot.tab, (Bc, (1 + self.times) * Bc)))
            nxt = (ctypes.c_void_p * 4)(*(at(x, c * per) for l, per in tabs
                                          for x in (l.next_t, l.next_a)))
            seg = (ctypes.c_void_p * 2)(*(at(l.own.seg, (c + 1) * (per + 1)) for l, per in tabs))
            dst = (ctypes.c_void_p * 2)(*(at(l.own.perm, (c + 1) * per) for l, per in tabs))
        self._launch('adam', stream, 'mirec_comm_adam_deferred_f32', self.win.comm, self._tables,
                     2, self._n_max, self.d, *self._sched(step_off), nxt, seg, dst, self.cap)

    def _step_rccl(self, slot, c, bpr, stream):
        """The forward half of a step through two all-to-alls: the owners gather the rows
        the slices read; K3 reads the received rows, and each slot's gradient row goes
        straight into its backward message position (the position its row came in): no
        separate backward gather (sendB's padding rows are never read by the owners)."""
        M = self.G * self.cap
        self._launch('gather', stream, 'mirec_shard_gather_f32', self.shU[0].data_ptr(),
                     self.shI[0].data_ptr(), self.d, slot.fwd_rows.data_ptr() + 8 * c * M, M,
                     self.sendF.data_ptr())
        self._record('exchange', stream, lambda: self._all_to_all(self.recvF, self.sendF))
        if bpr[3]:                                   # this rank's slice has positives
            self._launch('bpr', stream, 'mirec_bpr_fwd_bwd_at_ids_f32', self.recvF.data_ptr(), M,
                         self.d, *bpr, self.sendB.data_ptr())
        else:
            self._record('bpr', stream, lambda: None)
        self._record('exchange_bwd', stream, lambda: self._all_to_all(self.recvB, self.sendB))

    def _finish(self, c0, n_steps, Bc, stream):
        """Losses of this rank's slices of steps c0..c0+n_steps -> all ranks (one
        all-gather), laid out in global positive order, then chunk_finish."""
        B, G = self.B, self.G
        mine = self.loss_mine[c0 * B:(c0 + n_steps) * B]
        gathered = self._all_gather(mine).view(G, n_steps, B)
        self.loss_k.view(self.C, self.Bg)[c0:c0 + n_steps].view(n_steps, G, B).copy_(
            gathered.transpose(0, 1))
        super()._finish(c0, n_steps, Bc, stream)

    # ------------------------------------------------------------ epoch API
    def begin_epoch(self, cuts=(), hold_prep_from=None, flush_at=()):
        self.status.zero_()
        self._load_shards()
        return super().begin_epoch(cuts=cuts, hold_prep_from=hold_prep_from, flush_at=flush_at)

    def close(self):
        super().close()
        if self.win is not None:             # after a barrier: no rank still stores into it
            self.win.close()
            self.win = None

    def end_epoch(self, n_done=None):
        losses = super().end_epoch(n_done)
        if self.win is not None and self.win.status() != 0:
            raise RuntimeError('row exchange: a wait for a peer\'s flags timed out (a rank '
                               'stopped or fell out of step)')
        if int(self.status[0].item()) == -4:                 # backstop: _enter_chunk re-plans
            raise RuntimeError(f'row exchange overflow: a (slice, owner) message exceeded '
                               f'cap={self.cap} rows')
        self._store_shards()
        return losses
