"""The loudness meter of a stream on the device: FlowHighSR.loudness_meter / meter_push, and the meter a DeliveryStream opened with
meter=True owns (meter.py is the schedule and the definition, csrc/loudness.hip the kernels).

A LoudnessMeter takes the float32 blocks of one stream at `rate` and keeps, per channel row, the K-weighting's record
(fh_meter_state), the samples behind the last whole span (two buffers that take turns) and the row of the energy log, double,
indexed by absolute sub-block number.  A push is ONE fh_stream_kweight_energy_f32 launch for all rows of all meters of one rate
and one upload of its job table; nothing is read back: what was walked follows from the blocks' lengths (meter.Counters).  The log
holds the bits of fh_kweight_energy_f32 on the whole stream, so read() -- one fh_loudness_report_f32 launch over the log's complete
sub-blocks -- is FlowHighSR.measure_loudness_report(x[:, :measured])[0] bit for bit, and after flush() that of all of x.
The log grows by doubling with a device copy.
"""
import ctypes

import numpy as np
import torch

from . import hip
from . import meter as _meter
from .delivery import _coef
from .frontend import upload_tables

LOG_CAPACITY = 4096               # sub-blocks of a new meter's log (6.8 minutes at 100 ms): 32 KB per channel


class LoudnessMeter:
    """One meter of FlowHighSR.loudness_meter().  push(block): float32 [1, n] / [n] ([C, n] with n_channels=C) on the device, n
    may be 0; read() -> float32 [6] on the device (meter.FIELDS) over the `measured` samples (a host int); flush() processes the
    rest and closes the meter."""

    def __init__(self, owner, rate=48000, n_channels=None, log_capacity=LOG_CAPACITY):
        self.channels = _meter.check_channels(n_channels)
        self.counters = _meter.Counters(rate)                 # (ValueError for a rate without a sub-block of 16 samples)
        self.rate, self.rows, self.owner = int(rate), self.channels or 1, owner
        if isinstance(log_capacity, bool) or not isinstance(log_capacity, (int, np.integer)) or not 1 <= log_capacity <= _meter.MAX_SUB:
            raise ValueError(f"log_capacity must be an int 1 .. 2^20 sub-blocks, got {log_capacity!r}")
        self.device = owner.delivery.device
        self.capacity = int(log_capacity)
        self.state = self.log = self.kept = None              # made by the first push: opening a meter touches no device
        self.cur = 0

    @property
    def closed(self):
        return self.counters.ended

    @property
    def measured(self):
        return self.counters.measured

    def push(self, block):
        self.owner.meter_push([self], [block])

    def flush(self):
        self.owner.meter_push([self], [None], final=True)

    def read(self):
        with hip.device_guard(self.device):
            self._allocate()
            return self.owner.delivery._report(self.log, [self.measured] * self.rows, [self.rows], self.counters.hop)[0]

    def _allocate(self, need=0):
        """The device state, and a log of at least `need` sub-blocks: doubled, what it held copied over."""
        if self.state is None:
            assert hip.lib().fh_loudness_span_len() == _meter.SPAN
            self.state = torch.zeros(self.rows, ctypes.sizeof(hip.MeterState) // 8, dtype=torch.float64, device=self.device)
            self.kept = [torch.empty(self.rows, _meter.SPAN, dtype=torch.float32, device=self.device) for _ in range(2)]
        capacity = self.capacity
        while capacity < need:
            capacity = min(2 * capacity, _meter.MAX_SUB)
        if self.log is None or capacity != self.capacity:
            log = torch.zeros(self.rows, capacity, dtype=torch.float64, device=self.device)
            if self.log is not None:
                log[:, :self.capacity].copy_(self.log)
            self.log, self.capacity = log, capacity

    def jobs(self, fresh, final):
        """The fh_meter_jobs of this push, one per row (fresh: contiguous float32 [rows, n]); the counters move on and the kept
        buffers change places."""
        n = fresh.shape[1]
        step = self.counters.step(n, final)
        self._allocate(step["log_need"])
        out = []
        for r in range(self.rows):
            kept = self.kept[self.cur][r].data_ptr() if step["n_kept"] else 0
            keep = self.kept[self.cur ^ 1][r].data_ptr() if step["n_keep"] else 0
            out.append(hip.MeterJob(kept, fresh.data_ptr() + 4 * r * n if n else 0, keep, self.state[r].data_ptr(),
                                    self.log[r].data_ptr(), step["base"], step["n_kept"], n, self.capacity, int(final)))
        self.cur ^= 1                            # (with n_keep == 0 nothing is kept: either buffer will do)
        return out


def _block(b, m):
    from .delivery_stream import _block as stream_block
    return stream_block(b, m.device, m.channels)


def check(meters, lens, final):
    """Before anything moves: no meter twice, none closed, none past its log's bound (RuntimeError)."""
    if len({id(m) for m in meters}) != len(meters):
        raise ValueError("a meter is in the list twice")
    for m, n in zip(meters, lens):
        m.counters.log_need(n, final)


def plan(meters, blocks, final):
    """The launches of one push over checked blocks (contiguous float32 [rows, n] on the device): a list of
    (rate, the host table of fh_meter_jobs) -- one per rate -- for `launch`, the tables to go up with whatever else the caller
    uploads.  A meter with nothing new and nothing to end stays as it is."""
    by_rate = {}
    for m, b in zip(meters, blocks):
        if final or b.shape[1]:
            by_rate.setdefault(m.rate, []).extend(m.jobs(b, final))
    return [(rate, (hip.MeterJob * len(jobs))(*jobs)) for rate, jobs in by_rate.items()]


def launch(planned, ptrs):
    """ptrs: the device addresses of the planned tables."""
    from . import loudness as _loudness
    for (rate, table), ptr in zip(planned, ptrs):
        entry = "fh_stream_kweight_energy_f32"
        hip.check(getattr(hip.lib(), entry)(ptr, ctypes.addressof(table), len(table), _coef(rate), _loudness.geometry(rate)[0],
                                            hip.stream()), entry)


def push(delivery, meters, blocks, final=False):
    """One block per meter (None: nothing this time): ONE launch for all rows of all meters of one rate, one table upload.
    final: the meters end here.  A meter's result does not depend on its company."""
    meters, blocks = list(meters), list(blocks)
    if len(meters) != len(blocks):
        raise ValueError(f"one block per meter: {len(blocks)} blocks for {len(meters)} meters")
    for m in meters:
        if not isinstance(m, LoudnessMeter) or m.device != delivery.device:
            raise ValueError(f"meter_push takes the LoudnessMeters of this model on {delivery.device}, got {m!r}")
    with hip.device_guard(delivery.device):
        fresh = [_block(b, m) for m, b in zip(meters, blocks)]                # (every block is checked before any meter moves)
        check(meters, [b.shape[1] for b in fresh], final)
        planned = plan(meters, fresh, final)
        if planned:
            keep, ptrs = upload_tables([table for _, table in planned], delivery.device)
            launch(planned, ptrs)
        del fresh                                # (a block made contiguous lives until the launch that reads it is queued)
