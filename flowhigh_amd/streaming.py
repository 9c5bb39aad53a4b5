"""Streaming sessions on the device: FlowHighSR.stream / stream_push / generate_long (stream.py is the definition of what they compute).

A session cuts its stream into the windows of its StreamPlan.  Window i runs exactly as generate(window_i, sr, level='input')
runs, with its prior drawn by fh_prior_normal_at_f32 from the session's key at the window's absolute first frame; consecutive
windows are joined over their overlap by fh_xfade_seg_f32.  Every runnable window of every session of a push that shares a plan
and a number of time steps is a row of ONE batch (rows of a batch have the bits of a clip alone) and a job of ONE seam launch.
Pending input samples live on the host, the previous window's last O48 output samples on the device, in a buffer of the session's own.
A session opened with delivery= hands what it emits to a DeliveryStream of its own (delivery_stream.py): all such sessions of a push
go through one launch sequence there.
A session opened with n_channels=C takes [C, n] blocks: window i is generate(window_i [C, n], sr, channels='first', level='input'),
one clip of C rows that share the session's prior; a seam is one fh_xfade_seg_f32 job per row, the tail [C, O48], the emitted
blocks [C, m].  Sessions of different channel counts share a batch like any others of one plan.
"""
import numpy as np
import torch

from . import hip
from .delivery import PCM_FORMATS, pcm_entry, pcm_shape
from .frontend import upload_tables
from .stream import StreamPlan

# keywords of generate() that a session does not take, and why
_CARRIED = "delivery=dict(...) carries it across pushes"
_NOT_BUILT = dict(channels="a session is one mono stream unless it is opened with n_channels=C, which takes [C, n] blocks",
                  dither=f"dither needs a sample-index offset across blocks (csrc/pcm.hip): {_CARRIED}",
                  output_rate=f"resampling a stream needs resampler state across blocks: {_CARRIED}",
                  loudness="loudness is a statistic of a whole clip (delivery=dict(meter=True) reads the stream's)",
                  true_peak=f"the true peak is a statistic of a whole clip: {_CARRIED} with limiter='lookahead'")


def check_not_built(**kw):
    for name, value in kw.items():
        if value is not None:
            raise ValueError(f"{name}= is not built for streaming sessions: {_NOT_BUILT[name]}")


class StreamSession:
    """One stream of a FlowHighSR.stream() call.  push(block) -> the newly final samples, flush() -> the rest."""

    def __init__(self, model, plan, timestep, key, pcm, delivery=None, channels=None):
        self.model, self.plan, self.timestep, self.key, self.pcm = model, plan, int(timestep), key, pcm
        self.channels = channels                # None: one mono stream | C: blocks are [C, n], fixed when the session opens
        self.rows = channels or 1
        self.delivery = delivery                # None | the session's DeliveryStream: what it emits goes through it
        self.closed = False
        self.integer = None                     # the sample format, fixed by the first block: integer dtype (/ 32768) or float
        self.dtype = None
        self.pending = None                     # input samples from window `done`'s first one on (host; [C, n] with channels)
        self.arrived = 0                        # input samples pushed so far
        self.done = 0                           # windows run so far
        self.tail = None                        # the last window's final O48 output samples, [rows, O48] (device, the session's own)

    # ---- host side ---------------------------------------------------------------------------------------------------
    def _take(self, block):
        """A pushed block as 1-D samples ([C, n] with channels) in the session's format, appended to the pending input.
        A refused block leaves the session as it was."""
        if isinstance(block, torch.Tensor):
            block = block.detach().cpu().numpy()
        a = np.asarray(block)
        if self.channels is not None:
            if a.ndim != 2 or a.shape[0] != self.channels:
                raise ValueError(f"a block of this session is [{self.channels}, n] (n_channels={self.channels}), got shape {a.shape}")
        else:
            if a.ndim == 2 and a.shape[0] == 1:
                a = a[0]
            if a.ndim != 1:
                raise ValueError(f"a block is 1-D or [1, n] (one mono stream), got shape {a.shape}")
        if a.size == 0:
            return
        integer = np.issubdtype(a.dtype, np.integer)
        if not integer and not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f"a block holds integer or float samples, got dtype {a.dtype}")
        if self.integer is None:
            self.integer = bool(integer)
            self.dtype = np.float64 if integer else a.dtype
            self.pending = np.empty(a.shape[:-1] + (0,), dtype=self.dtype)
        elif integer != self.integer:
            raise ValueError(f"the session's sample format is fixed by its first block ({'integer' if self.integer else 'float'}): "
                             f"got a block of dtype {a.dtype}")
        # (an integer block is int16 full scale whatever its largest sample: no block is guessed from its own peak)
        a = a / 32768.0 if integer else a.astype(self.dtype, copy=False)
        self.pending = np.concatenate([self.pending, a], -1)
        self.arrived += a.shape[-1]

    def _cut(self, final):
        """The windows that can run now as (index, [rows, n] samples, last of the stream); the pending input moves on.
        final: the stream ends here -- what is left past the last full window is the last window, if it is more than the overlap
        it shares with that window (or the stream's only window); -> (windows, whether the kept tail is the stream's end)."""
        p = self.plan
        out = []
        if self.pending is None:
            return out, False
        rows = (lambda a: a[None]) if self.channels is None else (lambda a: a)
        while self.pending.shape[-1] >= p.W:
            out.append([self.done + len(out), rows(self.pending[..., :p.W]), False])
            self.pending = self.pending[..., p.H:]
        if not final:
            return out, False
        k, left = self.done + len(out), self.pending
        self.pending = None
        if left.shape[-1] > (p.O if k else 0):
            out.append([k, rows(left), True])
        elif out:
            out[-1][2] = True                   # the stream ends with this window's last sample
        return out, bool(k) and not out

    def push(self, block):
        """float32 (int16 with pcm=) [1, n] on the device ([C, n] with n_channels=C): the samples this block made final (with
        delivery=: at the delivered rate, those its delivery made final; int16 [n, C] with its interleaved=); n may be 0."""
        return self.model.stream_push([self], [block])[0]

    def flush(self):
        """Runs the last, partial window and returns what is left; the session is closed afterwards."""
        return self.model._stream_run([self], final=True)[0]


def open_session(model, sr, window_ms, overlap_ms, guard_ms, timestep, seed, stream, pcm, not_built, delivery=None, n_channels=None):
    from .delivery_stream import DeliveryStream, resolve
    from .prior import normalize_key
    check_not_built(**not_built)
    if model.prior != 'device':
        raise ValueError("a streaming session shares one keyed prior between its windows: construct the model with prior='device' "
                         "(a prior='reference' model draws from a generator, window by window)")
    if pcm is not None and pcm not in PCM_FORMATS:
        raise ValueError(f"pcm must be None or one of {tuple(PCM_FORMATS)}, got {pcm!r}")
    if isinstance(timestep, bool) or int(timestep) != timestep or timestep < 1:
        raise ValueError(f"timestep must be a positive integer, got {timestep!r}")
    plan = StreamPlan(sr, window_ms, overlap_ms, guard_ms)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))
    elif isinstance(seed, (bool, float)) or not isinstance(seed, (int, np.integer)):
        raise TypeError(f"seed must be an int, got {seed!r}")
    opt = resolve(delivery, pcm, n_channels)                 # (n_channels is checked there, behind every older check)
    return StreamSession(model, plan, timestep, normalize_key(seed, stream), pcm, None if opt is None else DeliveryStream(opt, model),
                         None if n_channels is None else int(n_channels))


def _ramp(model, plan):
    """(w_in, w_out) of the plan on the device, kept per (O48, G48)."""
    cache = model.__dict__.setdefault("_stream_ramps", {})
    k = (plan.O48, plan.G48)
    if k not in cache:
        cache[k] = tuple(model._upload(torch.from_numpy(w)) for w in plan.ramp())
    return cache[k]


def _encode(model, block, pcm="int16"):
    """float32 [C, n] -> int16 [C, n], planar: pcm.py's encoding without dither, which is stateless (fh_pcm_i16_f32);
    pcm='s24in32': int32 [C, n], 's24': uint8 [C, n, 3] (fh_pcm_s24_f32)."""
    out = torch.empty(pcm_shape(pcm, *block.shape), dtype=PCM_FORMATS[pcm][0], device=block.device)
    if block.shape[1]:
        entry, tail = pcm_entry(pcm, "batched")
        hip.check(getattr(hip.lib(), entry)(block.data_ptr(), out.data_ptr(), 0, 1, block.shape[0], block.shape[1], 0, *tail,
                                            hip.stream()), entry)
    return out


def check_sessions(model, sessions):
    if len({id(s) for s in sessions}) != len(sessions):
        raise ValueError("a session is in the list twice")
    for s in sessions:
        if s.model is not model:
            raise ValueError("a session of another model")
        if s.closed:
            raise RuntimeError("the session is closed: flush() ends a stream")


def run(model, sessions, final):
    """Every runnable window of `sessions` (final: and their last ones; the sessions then close) -> one output block per session."""
    sessions = list(sessions)
    check_sessions(model, sessions)
    work = {}                 # (plan key, time steps, samples of a window) -> [(session index, window index, [rows, n], last)]
    ends_in_tail = []
    for si, s in enumerate(sessions):
        windows, tail_ends = s._cut(final)
        ends_in_tail.append(tail_ends)
        for wi, x, last in windows:
            work.setdefault((s.plan.key, s.timestep, x.shape[1]), []).append((si, wi, x, last))
    if final:
        for s in sessions:
            s.closed = True                      # (whatever the last run raises: a flush ends the stream)
    parts = [[] for _ in sessions]
    # full windows first: a last, shorter window reads the tail its predecessor leaves
    for key in sorted(work, key=lambda k: k[2] != sessions[work[k][0][0]].plan.W):
        items = work[key]
        p = sessions[items[0][0]].plan
        # (a window of C channels is one clip of C rows that share the prior: sessions of any channel counts in one batch)
        y = model._generate_rows([x for _, _, x, _ in items], p.sr, key[1], None, [sessions[si].key for si, _, _, _ in items], None,
                                 "input", False, first_frames=[p.first_frame(wi) for _, wi, _, _ in items])
        o, esz = p.O48, y.element_size()
        jobs, row_of, r = [], {}, 0
        for si, wi, x, _ in items:
            if wi:                               # the older window: rows of this batch, or the tail the session kept
                prev = row_of.get((si, wi - 1))
                for c in range(x.shape[0]):      # a seam per row
                    tail = sessions[si].tail[c].data_ptr() if prev is None else y[prev + c].data_ptr() + (p.W48 - o) * esz
                    jobs.append(hip.XfadeJob(y[r + c].data_ptr(), tail))
            row_of[(si, wi)] = r
            r += x.shape[0]
        if jobs:
            w_in, w_out = _ramp(model, p)
            keep, (jp,) = upload_tables([(hip.XfadeJob * len(jobs))(*jobs)], model.device)
            hip.check(hip.lib().fh_xfade_seg_f32(jp, len(jobs), w_in.data_ptr(), w_out.data_ptr(), o, hip.stream()), "fh_xfade_seg_f32")
        # (y belongs to the post-processor's workspace: what is emitted and the kept tail are copied out before the next batch)
        for si, wi, x, last in items:
            s, rows = sessions[si], slice(row_of[(si, wi)], row_of[(si, wi)] + x.shape[0])
            parts[si].append(y[rows] if last else y[rows, :p.H48])
            s.tail = None if last else y[rows, p.W48 - o:].clone()
            s.done = wi + 1
        for si in {si for si, _, _, _ in items}:
            parts[si] = [torch.cat(parts[si], 1)]
    out = []
    for si, s in enumerate(sessions):
        if final:
            if ends_in_tail[si]:
                parts[si].append(s.tail)         # the stream ended with the last window's right overlap: it is final as it is
            s.tail = None
        block = torch.cat(parts[si], 1) if parts[si] else torch.empty(s.rows, 0, dtype=torch.float32, device=model.device)
        out.append(_encode(model, block, s.pcm) if s.pcm is not None else block)
    # every delivering session's block of this push through one launch sequence (delivery_stream.py)
    carried = [si for si, s in enumerate(sessions) if s.delivery is not None]
    if carried:
        from .delivery_stream import push
        for si, y in zip(carried, push(model.delivery, [sessions[si].delivery for si in carried], [out[si] for si in carried], final)):
            out[si] = y
    return out
