"""Host logic of the lagged guard-row reader (runtime/step_guard.py) against CPU tensors and stub events, and the new
entry points in the binding table (test_abi_cpu.py checks that the header declares the same set)."""
import pytest
import torch

import cape_amd  # noqa: F401
from cape_amd.hip import lib
from cape_amd.runtime.step_guard import LaggedRowReader

ROW = lib.GUARD_ROW_LOSSES + 4


class StubEvent:
    """An event that completes when the test says so (or when somebody waits for it)."""
    made = []

    def __init__(self):
        self.recorded, self.done, self.waited = False, False, False
        StubEvent.made.append(self)

    def record(self):
        self.recorded = True

    def query(self):
        return self.done

    def synchronize(self):
        assert self.recorded
        self.done = self.waited = True


def write_row(ring, serial, ok=1, total=0.0):
    """What cape_step_guard does on the device: row serial % len, serial and ok as int32 bits."""
    row = ring[serial % ring.shape[0]]
    row.view(torch.int32)[lib.GUARD_ROW_SERIAL] = serial
    row.view(torch.int32)[lib.GUARD_ROW_OK] = ok
    row[lib.GUARD_ROW_TOTAL] = total
    row[lib.GUARD_ROW_NORM] = lib.GUARD_NO_STEP if serial % 2 == 0 else 3.0
    row[lib.GUARD_ROW_COEF] = 1.0
    row[lib.GUARD_ROW_LR] = 1e-4
    row[lib.GUARD_ROW_LOSSES:] = torch.arange(4, dtype=torch.float32) + serial


@pytest.fixture
def reader():
    StubEvent.made = []
    ring = torch.zeros(4, ROW)
    return LaggedRowReader(ring, event_factory=StubEvent), ring


def test_new_entry_points_are_bound():
    for name in ("cape_step_guard", "cape_adamw_step_guarded"):
        assert name in lib.EXPORTS and hasattr(lib.raw(), name)


def test_rows_arrive_in_order_exactly_once_one_call_late(reader):
    rd, ring = reader
    got = []
    for it in range(11):                                    # wraps the ring of 4 more than twice
        write_row(ring, it, total=float(it))
        rd.push()
        rows = rd.poll()
        assert [r.serial for r in rows] == ([] if it == 0 else [it - 1])      # iteration i's row arrives at iteration i + 1
        got += rows
    got += rd.drain()                                       # the end of the epoch returns the rest
    assert [r.serial for r in got] == list(range(11))
    assert [r.total for r in got] == [float(i) for i in range(11)]
    assert got[3].losses == [3.0, 4.0, 5.0, 6.0] and got[3].grad_norm == 3.0 and got[2].grad_norm is None
    assert got[0].ok == 1 and got[0].lr == pytest.approx(1e-4)
    assert rd.poll() == [] and rd.drain() == []


def test_row_is_delivered_only_after_its_event_completed(reader):
    rd, ring = reader
    write_row(ring, 0)
    rd.push()
    assert rd.poll() == []                                  # the call just enqueued: never handed out, never waited for
    assert not StubEvent.made[0].waited and not StubEvent.made[0].done
    write_row(ring, 1)
    rd.push()
    rows = rd.poll()                                        # waits on the previous call's event, and on no other
    assert [r.serial for r in rows] == [0]
    assert StubEvent.made[0].waited and StubEvent.made[0].done
    assert not StubEvent.made[1].waited and not StubEvent.made[1].done
    StubEvent.made[1].done = True                           # completed early: still the latest call, still held back
    assert rd.poll() == []
    assert [r.serial for r in rd.drain()] == [1]


def test_mirror_holds_the_row_of_push_time(reader):
    """The copy to the host is taken at push: the device may overwrite the ring slot (serial + ring length) before the read."""
    rd, ring = reader
    write_row(ring, 0, total=5.0)
    rd.push()
    ring[0].zero_()
    assert rd.drain()[0].total == 5.0


def test_wrong_serial_raises(reader):
    rd, ring = reader
    write_row(ring, 0)
    rd.push()
    write_row(ring, 1)
    ring[1].view(torch.int32)[lib.GUARD_ROW_SERIAL] = 7     # a skipped launch / an overrun ring
    rd.push()
    assert [r.serial for r in rd.poll()] == [0]
    with pytest.raises(RuntimeError, match="out of step"):
        rd.drain()


def test_unread_rows_cannot_be_overrun(reader):
    rd, ring = reader
    for it in range(3):
        write_row(ring, it)
        rd.push()
    write_row(ring, 3)
    with pytest.raises(RuntimeError, match="poll"):
        rd.push()


def test_ring_needs_four_rows():
    with pytest.raises(ValueError):
        LaggedRowReader(torch.zeros(3, ROW), event_factory=StubEvent)
