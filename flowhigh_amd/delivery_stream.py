"""Streaming delivery on the device: FlowHighSR.stream(delivery=) / delivery_stream / delivery_push (stream_delivery.py is the
schedule and the definition, csrc/stream_delivery.hip the kernels).

A DeliveryStream takes the 48 kHz float32 blocks of one mono stream and returns them delivered -- resampled to output_rate, held
under true_peak by the look-ahead limiter, encoded to int16 with dither -- with the bits of Delivery.batch(whole stream, [1],
'input', ...).  Each stage keeps its counters (stream_delivery.Stage) and two device carry buffers that take turns; a push is
at most three launches for all of its streams that share a plan, each launch one job per stream, and one upload of that plan's
job tables.  Nothing is read back: what a push emits follows from the lengths of the blocks alone.  The blocks a push returns are
views of one buffer per plan.

A stream opened with n_channels=C (1 .. 8; the count is the stream's, fixed when it opens, never read from a block's shape) takes
[C, n] blocks and gives the bits of Delivery.batch(whole stream [C, T], [C], 'input', ...): its channels are C consecutive jobs
with one set of counters per stage and carry buffers of [C, capacity], the resampler runs them as rows, the limiter is
channel-linked (fh_stream_limit_linked_f32: one envelope, one gain) and the encoder gives channel c its own dither, planar [C, m]
or sample frames [m, C] (fh_stream_pcm_i16_rows_f32).  Streams of any channel counts that share a plan share its launches.
A stream without n_channels calls the three mono entries exactly as before.
pcm='s24' / 's24in32' (24 bits: uint8 with a last axis of 3 bytes, or int32): the encode stage is fh_stream_pcm_s24_rows_f32 for
every stream, a mono one as a group of one job; the plan key holds the format, so streams of different formats never share an
encode launch.
meter=True: the stream owns a LoudnessMeter (loudness_meter.py) at the delivered rate, fed the float32 samples the stream makes
final -- behind the resampler and the limiter, in front of the encoder -- by one more launch behind the plan's stages, its job
table in the plan's one upload; loudness() reads it.  The delivered blocks are those of the stream without the meter; a stream
with nothing but the meter returns its blocks as they came.
"""
import numpy as np
import torch

from . import delivery as _delivery
from . import hip
from . import loudness_meter as _lm
from . import stream_delivery as SD
from . import truepeak as _truepeak
from .frontend import upload_tables

KEYWORDS = ("output_rate", "pcm", "dither", "dither_seed", "true_peak", "limiter", "meter")
_REFUSED = dict(loudness="loudness is a statistic of the whole stream (meter=True reads it: DeliveryStream.loudness())",
                channels="a stream is mono unless it is opened with n_channels=C",
                interleaved="a stream is mono: there is nothing to interleave (a stream opened with n_channels=C takes it)")


def check_channels(n_channels):
    """n_channels= of stream() / delivery_stream(): None (one mono stream) or an int 1 .. 8."""
    if n_channels is None:
        return None
    if isinstance(n_channels, (bool, float)) or not isinstance(n_channels, (int, np.integer)) or not 1 <= n_channels <= SD.MAX_CHANNELS:
        raise ValueError(f"n_channels must be None or an int 1 .. {SD.MAX_CHANNELS} (the stream's channel count, fixed when it "
                         f"opens), got {n_channels!r}")
    return int(n_channels)


def resolve(delivery, session_pcm=None, n_channels=None):
    """delivery= of stream() / the keywords of delivery_stream(), checked (ValueError, before any GPU work) -> None when every
    value is a default, else dict(rate: None | R, true_peak: None | the ceiling in dBTP, pcm, key: None | the dither's (seed, stream)),
    with n_channels=C also channels: C and interleaved (a key of delivery that only such a stream takes), with meter=True also
    meter: True (a key that counts as non-default: a plan may hold nothing else)."""
    n_channels = check_channels(n_channels)
    if delivery is None:
        return None
    if not isinstance(delivery, dict):
        raise ValueError(f"delivery must be None or a dict of {', '.join(KEYWORDS)}, got {delivery!r}")
    for name in delivery:
        if name in _REFUSED and not (name == "interleaved" and n_channels is not None):
            raise ValueError(f"delivery= does not take {name}=: {_REFUSED[name]}")
        if name not in KEYWORDS and name != "interleaved":
            raise ValueError(f"delivery= has no key {name!r}: it takes {', '.join(KEYWORDS)}")
    kw = {k: delivery.get(k) for k in KEYWORDS if k not in ("dither_seed", "meter")}
    meter = delivery.get("meter", False)
    if meter not in (False, True):
        raise ValueError(f"meter must be a bool, got {meter!r}")
    if n_channels is not None:
        kw["interleaved"] = delivery.get("interleaved", False)
    if kw["true_peak"] is not None and kw["limiter"] is None:
        raise ValueError("true_peak= without limiter='lookahead' is one gain from the whole stream's peak: a stream takes "
                         "true_peak= with limiter='lookahead'")
    opt = _delivery.resolve_delivery(1, dither_seed=delivery.get("dither_seed", 0), level="input", **kw)
    if opt is None and not meter:
        return None
    if session_pcm is not None:
        raise ValueError("delivery= and the session's pcm= are two encoders for one stream: give pcm in delivery=")
    if opt is None:
        return SD.make_plan(channels=n_channels, meter=True)
    return SD.make_plan(opt["rate"], opt.get("true_peak"), opt["pcm"], None if opt["keys"] is None else opt["keys"][0],
                        n_channels, opt["interleaved"], bool(meter))


class _StageState:
    """One stage of one stream on the device: the schedule's counters and two carry buffers of `capacity` samples per row."""

    def __init__(self, counters, capacity, rows=1):
        self.counters, self.capacity, self.rows = counters, int(capacity), int(rows)
        self.buffers, self.cur = None, 0

    def jobs(self, fresh, n_fresh, dst, ended, device):
        """The fh_stream_jobs of this push, one per row (fresh, dst: the rows' addresses); the counters move on and the carry
        buffers change places."""
        step = self.counters.step(n_fresh, ended)
        if self.buffers is None and self.capacity:
            self.buffers = [torch.empty(self.rows * self.capacity, dtype=torch.float32, device=device) for _ in range(2)]
        c = self.counters
        assert step["n_carry"] <= self.capacity and step["n_keep"] <= self.capacity, (step, self.capacity)
        assert step["base"] + step["n_carry"] + n_fresh == c.arrived and step["first"] + step["n_out"] == c.emitted
        assert step["n_out"] == 0 or step["base"] <= c._lowest(step["first"])
        out = []
        for r in range(self.rows):
            carry = self.buffers[self.cur].data_ptr() + 4 * r * self.capacity if step["n_carry"] else 0
            keep = self.buffers[self.cur ^ 1].data_ptr() + 4 * r * self.capacity if step["n_keep"] else 0
            out.append(hip.StreamJob(carry, fresh[r] if n_fresh else 0, dst[r] if step["n_out"] else 0, keep, step["base"],
                                     step["first"], step["n_carry"], n_fresh, step["n_out"], step["n_keep"], int(ended), 0))
        self.cur ^= 1                            # (with n_keep == 0 the next carry is empty: either buffer will do)
        return out, step["n_out"]


class DeliveryStream:
    """One stream of FlowHighSR.delivery_stream().  push(block48) -> the delivered samples that block made final, float32
    (int16 with pcm) [1, n] on the device, n may be 0; flush() -> the rest, and the stream is closed.  Opened with n_channels=C:
    blocks [C, n] in, [C, m] out, int16 [m, C] with interleaved."""

    def __init__(self, plan, owner=None):
        if plan is None:
            raise ValueError("every delivery keyword is at its default: there is nothing to deliver")
        self.plan, self.owner, self.closed = plan, owner, False
        self.channels, self.interleaved = plan.get("channels"), bool(plan.get("interleaved"))
        self.rows = rows = self.channels or 1
        # streams of one key share launches (streams with n_channels: whatever their counts, the group table carries them)
        self.key = (plan["rate"], plan["true_peak"], plan["pcm"], plan["key"] is not None)
        if self.channels is not None:
            self.key += ("linked", self.interleaved)
        self.meter = None
        if plan.get("meter"):                    # (metered streams form plans of their own: their push has one launch more)
            self.meter = _lm.LoudnessMeter(owner, plan["rate"] or 48000, self.channels)
            self.key += ("meter",)
        self.stages = {}
        if plan["rate"] is not None:
            flt = SD.ResampleFilter(plan["rate"])
            self.stages["resample"] = _StageState(SD.ResampleStage(flt), flt.carry_bound, rows)
        if plan["true_peak"] is not None:
            H = _truepeak.half_window(plan["rate"] or 48000)
            self.stages["limit"] = _StageState(SD.LimitStage(H), 2 * (2 * H + _truepeak.HALF), rows)
        if plan["pcm"] is not None:
            self.stages["encode"] = _StageState(SD.EncodeStage(), 0, rows)

    def push(self, block48):
        return self.owner.delivery_push([self], [block48])[0]

    def flush(self):
        return self.owner.delivery_push([self], [None], final=True)[0]

    def loudness(self):
        """The meter's reading (LoudnessMeter.read) of a stream opened with meter=True: float32 [6] on the device."""
        if self.meter is None:
            raise RuntimeError("the stream has no meter: open it with meter=True")
        return self.meter.read()


def _block(b, device, channels=None):
    """A pushed block as contiguous float32 [rows, n] on the device (None: nothing).  channels None: one mono stream, [n] or [1, n]."""
    rows = channels or 1
    if b is None:
        return torch.empty(rows, 0, dtype=torch.float32, device=device)
    ok = isinstance(b, torch.Tensor) and b.dtype == torch.float32 and b.device == device
    if channels is None:
        if not ok or b.ndim not in (1, 2) or (b.ndim == 2 and b.shape[0] != 1):
            raise ValueError(f"a block is a float32 [1, n] tensor on {device} at 48 kHz, got {getattr(b, 'dtype', type(b))} "
                             f"{tuple(getattr(b, 'shape', ()))} on {getattr(b, 'device', 'the host')}")
        return b.reshape(1, -1).contiguous()
    if not ok or b.ndim != 2 or b.shape[0] != channels:
        raise ValueError(f"a block of this stream is a float32 [{channels}, n] tensor on {device} at 48 kHz (n_channels={channels}), "
                         f"got {getattr(b, 'dtype', type(b))} {tuple(getattr(b, 'shape', ()))} on {getattr(b, 'device', 'the host')}")
    return b.contiguous()


def push(delivery, streams, blocks, final=False):
    """One 48 kHz block per stream (None: nothing this time) -> one delivered block per stream, [1, n] ([C, n], or [n, C]
    interleaved, from a stream of C channels).  delivery: the model's
    Delivery (its device, its tap cache and limiter windows).  final: the streams end here; they are closed afterwards.
    Every stage is ONE launch for all the streams that share a plan; a stream's result does not depend on its company."""
    with hip.device_guard(delivery.device):
        return _push(delivery, streams, blocks, final)


def _push(delivery, streams, blocks, final):
    streams, blocks = list(streams), list(blocks)
    if len(streams) != len(blocks):
        raise ValueError(f"one block per stream: {len(blocks)} blocks for {len(streams)} streams")
    if len({id(s) for s in streams}) != len(streams):
        raise ValueError("a stream is in the list twice")
    for s in streams:
        if s.closed:
            raise RuntimeError("the stream is closed: flush() ends a stream")
    dev = delivery.device
    cur = [_block(b, dev, s.channels) for s, b in zip(streams, blocks)]             # (every block is checked before any stream moves)
    fresh = list(cur)          # (a block made contiguous is a copy of this push's own: it lives until the launches that read it are queued)
    metered = [i for i, s in enumerate(streams) if s.meter is not None]
    if metered:                # (what reaches a meter follows from the lengths: its log's bound is checked before any stream moves)
        reach = []
        for i in metered:
            n = cur[i].shape[1]
            for name in ("resample", "limit"):
                if name in streams[i].stages and (final or n):
                    n = streams[i].stages[name].counters.peek(n, final)
            reach.append(n)
        _lm.check([streams[i].meter for i in metered], reach, final)
    if final:
        for s in streams:
            s.closed = True
    groups = {}
    for i, s in enumerate(streams):
        groups.setdefault(s.key, []).append(i)
    for key, idx in groups.items():
        s0 = streams[idx[0]]                     # (what the key names is the same for all of them; the key itself is not taken apart)
        rate, ceiling_db, dithered = s0.plan["rate"], s0.plan["true_peak"], s0.plan["key"] is not None
        linked, frames = s0.channels is not None, s0.interleaved
        pcm = s0.plan["pcm"]
        wide = pcm in ("s24", "s24in32")
        # What every stage emits follows from the blocks' lengths, so the jobs of all stages are made first and go up as ONE
        # buffer; a stage's outputs are one buffer too, a stream's part of it ([rows, n_out], contiguous) the next stage's fresh block.
        n_in = {i: cur[i].shape[1] for i in idx}
        src = {i: [cur[i].data_ptr() + 4 * r * n_in[i] for r in range(streams[i].rows)] for i in idx}
        stages, tables_, floats = [], [], None
        for name in ("resample", "limit", "encode"):
            if name == "encode" and s0.meter is not None:                # the meter takes the floats in front of the encoder
                floats = [cur[i] for i in idx]
            if name not in s0.stages:
                continue
            # (a stream with nothing new and nothing to end stays as it is: its job would write and move nothing)
            live = [i for i in idx if final or n_in[i]]
            if not live:
                continue
            rooms = [streams[i].stages[name].counters.peek(n_in[i], final) for i in live]
            sizes = [r * streams[i].rows for i, r in zip(live, rooms)]
            offs = [int(o) for o in np.cumsum([0] + [-(-n // 8) * 8 for n in sizes[:-1]])]          # (16-byte aligned parts)
            # (esz: bytes per sample; per: the buffer's elements per sample -- 3 uint8 for 's24', else 1)
            if name == "encode":
                buf = _delivery.pcm_buffer(pcm, offs[-1] + sizes[-1], dev)
                esz, shape = _delivery.PCM_FORMATS[pcm][1], (lambda *s: _delivery.pcm_shape(pcm, *s))
            else:
                buf, esz, shape = torch.empty(offs[-1] + sizes[-1], dtype=torch.float32, device=dev), 4, (lambda *s: s)
            jobs, per = [], esz // buf.element_size()
            for i, off, room in zip(live, offs, rooms):
                rows = streams[i].rows
                base = buf.data_ptr() + off * esz
                part = buf[off * per:(off + room * rows) * per]
                if name == "encode" and frames:          # sample frames [n_out, C]: the first job's dst is the frame buffer
                    dst, part = [base] * rows, part.view(shape(room, rows))
                else:
                    dst, part = [base + r * room * esz for r in range(rows)], part.view(shape(rows, room))
                js, n_out = streams[i].stages[name].jobs(src[i], n_in[i], dst, final, dev)
                assert n_out == room
                jobs += js
                cur[i], src[i], n_in[i] = part, dst, room
            # (the resampler runs a row per job as it is; the 24-bit encoder has no mono entry: a mono stream is a group of one job)
            grouped = (linked and name != "resample") or (name == "encode" and wide)
            stages.append((name, live, max(rooms), len(jobs), len(tables_), grouped, buf))      # (buf: alive until its launches are queued)
            tables_.append((hip.StreamJob * len(jobs))(*jobs))
            if grouped:
                tables_.append(np.cumsum([0] + [streams[i].rows for i in live]).astype(np.int32))
        planned = _lm.plan([streams[i].meter for i in idx], floats, final) if floats is not None else []
        if not stages and not planned:
            continue
        tables_ += [table for _, table in planned]                          # (the meter's jobs go up with the plan's)
        at_keys = len(tables_)
        if dithered and stages and stages[-1][0] == "encode":
            tables_.append(np.array([streams[i].plan["key"] for i in stages[-1][1]], dtype=np.uint64).view(np.int64))
        keep, ptrs = upload_tables(tables_, dev)
        L = hip.lib()
        for name, live, max_out, n_jobs, at, grouped, _ in stages:      # one launch per stage: the mono entry, or the one that takes groups
            tables = (ptrs[at], n_jobs) + ((ptrs[at + 1], len(live)) if grouped else ())
            if name == "resample":
                taps, n_taps, pre, up, down = delivery.resampler._filter(rate, 48000)
                entry, args = "fh_stream_resample_f32", (taps, up, down, n_taps, pre)
            elif name == "limit":
                H = streams[live[0]].stages[name].counters.H
                c32 = float(np.float32(_truepeak.ceiling(ceiling_db)))
                entry, args = f"fh_stream_limit{'_linked' if linked else ''}_f32", (delivery._tp_taps(), delivery._window(H), H, c32)
            elif max_out:                                # (the mono entry takes no `interleaved`: one channel has one layout)
                entry, tail = _delivery.pcm_entry(pcm, "stream rows" if grouped else "stream mono")
                args = (ptrs[at_keys] if dithered else 0,) + ((int(frames), *tail) if grouped else ())
            else:
                continue
            hip.check(getattr(L, entry)(*tables, max_out, *args, hip.stream()), entry)
        _lm.launch(planned, ptrs[at_keys - len(planned):at_keys])           # (behind the stage that made its floats)
        del floats
    del fresh
    out = []
    for s, c in zip(streams, cur):                       # (what stood still at some stage emits an empty block of the result's type)
        fmt = s.plan["pcm"]
        if c.numel():
            out.append(c)
        elif fmt is None:
            out.append(torch.empty((s.rows, 0), dtype=torch.float32, device=dev))
        else:
            out.append(torch.empty(_delivery.pcm_shape(fmt, *((0, s.rows) if s.interleaved else (s.rows, 0))),
                                   dtype=_delivery.PCM_FORMATS[fmt][0], device=dev))
    return out
