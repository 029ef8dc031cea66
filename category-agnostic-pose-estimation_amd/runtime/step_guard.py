"""Device-side loss guard of the captured training step and its lagged host reader.

A captured step cannot ask the host whether the loss is finite.  `StepGuard` holds the device state of `cape_step_guard`
(csrc/optim.hip): a serial, the sticky flag `bad`, and a ring of rows -- one per training iteration -- with the criterion's
scalars, the gradient norm, the clip coefficient, the learning rate and an `ok` word.  `ArenaAdamW(guard=...)` launches the
guard inside its step and applies AdamW only while `bad` is clear; `GraphedTrainStep` launches it on micro-batches.

`LaggedRowReader` brings the rows to the host without stalling it: after every iteration the row just written is copied into a
pinned mirror (`non_blocking`) behind an event; `poll()` hands out the rows of EARLIER iterations only, waiting at most on the
event of the previous one, so the host always runs one iteration ahead of what it reads.  `drain()` waits for the rest."""
from collections import deque

import torch

from ..hip import lib
from ..hip import ops


class GuardRow:
    """One decoded ring row.  `grad_norm` is None on a micro-batch that took no optimizer step."""
    __slots__ = ("serial", "ok", "total", "grad_norm", "coef", "lr", "losses")

    def __init__(self, row):
        ints = row.view(torch.int32)
        self.serial, self.ok = int(ints[lib.GUARD_ROW_SERIAL]), int(ints[lib.GUARD_ROW_OK])
        vals = row.tolist()
        self.total, self.coef, self.lr = vals[lib.GUARD_ROW_TOTAL], vals[lib.GUARD_ROW_COEF], vals[lib.GUARD_ROW_LR]
        norm = vals[lib.GUARD_ROW_NORM]
        self.grad_norm = None if norm == lib.GUARD_NO_STEP else norm
        self.losses = vals[lib.GUARD_ROW_LOSSES:]

    def __repr__(self):
        return (f"GuardRow(serial={self.serial}, ok={self.ok}, total={self.total}, grad_norm={self.grad_norm}, coef={self.coef}, "
                f"lr={self.lr})")


class LaggedRowReader:
    """Host side of the ring.  `ring` is the (ring_len, row) tensor the guard writes (any device); `event_factory()` returns an
    object with `record()`, `query()` and `synchronize()` (torch.cuda.Event by default).  `first_serial` is the serial of the
    first row that will be pushed."""

    def __init__(self, ring, event_factory=None, first_serial=0):
        if ring.dim() != 2 or ring.shape[0] < 4:
            raise ValueError("the guard ring needs at least 4 rows: one being written, one in flight to the host, one being read")
        self.ring, self.ring_len = ring, ring.shape[0]
        self.mirror = torch.zeros(ring.shape, dtype=ring.dtype, pin_memory=ring.is_cuda)
        self.event_factory = event_factory if event_factory is not None else torch.cuda.Event
        self.next_serial = int(first_serial)        # serial of the next row to be pushed
        self.pending = deque()                      # (serial, slot, event), oldest first

    def push(self):
        """Call right after the launch that wrote a row (same stream): starts its copy to the host and records its event."""
        if len(self.pending) >= self.ring_len - 1:
            raise RuntimeError(f"{len(self.pending)} guard rows are waiting to be read: poll() must run once per iteration "
                               f"(ring of {self.ring_len})")
        slot = self.next_serial % self.ring_len
        self.mirror[slot].copy_(self.ring[slot], non_blocking=True)
        ev = self.event_factory()
        ev.record()
        self.pending.append((self.next_serial, slot, ev))
        self.next_serial += 1

    def _take(self):
        serial, slot, ev = self.pending.popleft()
        if not ev.query():
            raise RuntimeError(f"guard row {serial} read before its copy completed")
        row = GuardRow(self.mirror[slot].clone())
        if row.serial != serial:
            raise RuntimeError(f"guard ring out of step: expected the row of iteration {serial}, slot {slot} holds serial "
                               f"{row.serial} (a launch was skipped, or the ring was overrun)")
        return row

    def poll(self):
        """Rows of every iteration before the latest push, in order.  Waits at most on the previous iteration's event; the row
        of the iteration just enqueued is never handed out here."""
        out = []
        while len(self.pending) > 1:
            ev = self.pending[0][2]
            if not ev.query():
                ev.synchronize()
            out.append(self._take())
        return out

    def drain(self):
        """Every remaining row, in order (waits for them): the end of an epoch."""
        out = []
        while self.pending:
            self.pending[0][2].synchronize()
            out.append(self._take())
        return out


class StepGuard:
    """Device state of the loss guard.  A row has room for `max_losses` criterion values (2 per decoder layer); a criterion
    that returns fewer leaves the tail of the row zero."""

    def __init__(self, device, max_losses=2 * lib.DECODE_MAX_LAYERS, ring_len=8):
        device = torch.device(device)
        self.n_losses = int(max_losses)
        self.state = torch.zeros(2, dtype=torch.int32, device=device)          # [serial, bad]
        self.serial, self.bad = self.state[0:1], self.state[1:2]
        self.ring = torch.zeros(ring_len, lib.GUARD_ROW_LOSSES + self.n_losses, dtype=torch.float32, device=device)
        self.reader = LaggedRowReader(self.ring)
        self._total = self._losses = None

    def set_losses(self, total, losses):
        """The criterion's device scalars of the iteration whose row the next launch writes (`total` 1 element, `losses`
        at most max_losses elements).  Consumed by that launch."""
        if losses.numel() > self.n_losses or total.numel() != 1:
            raise ValueError(f"guard rows hold {self.n_losses} loss values, the criterion returned {losses.numel()}")
        self._total, self._losses = total, losses

    def launch(self, optimizer, is_step):
        """One `cape_step_guard` on the current stream.  With losses set it writes a row; without (an optimizer step that no
        forward pass precedes -- the tail flush) it only gates the step on the gradient norm."""
        total, losses, self._total, self._losses = self._total, self._losses, None, None
        ops.step_guard(total, losses, optimizer.sumsq if is_step else None, optimizer.max_norm, optimizer.lr_dev[0:1],
                       optimizer.step_count, self.serial, self.bad, self.ring if total is not None else None)

    def is_bad(self):
        """Host read of the sticky flag (synchronizes)."""
        return bool(int(self.bad.item()))

    def reset(self):
        """Clear the sticky flag (after the caller dealt with the bad batch, e.g. reloaded a checkpoint)."""
        self.bad.zero_()
