"""Streaming sessions, stated on the host in numpy: the DEFINITION of how a stream is cut into windows, when a window may run, what
has been emitted after it, and how consecutive windows are joined -- what FlowHighSR.stream / stream_push / generate_long do and
what csrc/stream.hip (fh_xfade_seg_f32) is tested against, bit for bit.

A plan has three lengths, all multiples of the rate's grain (grain_ms: the smallest multiple of 10 ms that is a whole number of
input samples), so that the hop H = W - O is a whole number of input samples AND of 480-sample mel frames at 48 kHz:
  window W    every window but the last has W input samples; window i covers input samples [i H, min(i H + W, T))
  overlap O   consecutive windows share O input samples = O48 output samples
  guard G     the first and last G48 output samples of an overlap take one window only (the other's edge region -- resampler
              tail, the STFT's reflect pad -- stays out of the mix altogether)
Window i starts at absolute mel frame i * H48 / 480: its prior is rows [that, + frames) of the SESSION's stream (prior.py:
prior_normal_host(first_frame=)), so the frames two windows share get the same noise and the windows differ through their
context alone.  That is what makes a sum-to-one cross-fade the right tool: with independent draws the generated bands of the
two windows are incoherent in the overlap and the cross-fade dips by up to 3 dB at every seam.

The ramp over an overlap, F = O48 - 2 G48:
  w_in[u]  = 0 for u < G48, 1 for u >= O48 - G48, else 0.5 - 0.5 cos(pi (u - G48 + 0.5) / F)      float64
  w_out[u] = 1 - w_in[u]                                                                            float64
both rounded to float32 once.  The seam, in float32:
  out[u] = fmaf(w_in[u], cur[u], fl(w_out[u] * prev[u]))
where a term whose weight is exactly 0 is skipped, not multiplied: in a guard the result is the other window's bits, and a NaN
behind a zero weight does not pass.

A session opened with n_channels=C cuts [C, n] blocks into [C, n] windows on the same schedule; every row is joined with the one
ramp (stitch(..., channels=C)).

numpy only: nothing here touches torch or the GPU.
"""
import math

import numpy as np

F32 = np.float32
HOP = 480                       # samples of a mel frame at 48 kHz (tables.HOP)
MIN_OVERLAP_MS = 20             # 960 samples at 48 kHz: a final window, longer than the overlap, clears the front end's 785


def resample_out_len(n_in, up, down):
    """tables.resample_out_len, restated (this module imports numpy only): ceil(n_in * up / down)."""
    return -(-int(n_in) * int(up) // int(down))


def grain_ms(sr):
    """The smallest multiple of 10 ms that is a whole number of input samples at `sr` (10 ms at 8 / 12 / 16 / 24 / 32 / 44.1 / 48 kHz,
    20 ms at 22 050 Hz, 40 ms at 11 025 Hz)."""
    sr = int(sr)
    if sr <= 0:
        raise ValueError(f"sr must be a positive integer rate, got {sr}")
    return 10 * (100 // math.gcd(sr, 100))


class StreamPlan:
    """How a stream at `sr` is windowed.  Lengths in input samples: W, O, H; in 48 kHz output samples: W48, O48, H48, G48."""

    def __init__(self, sr, window_ms=1000, overlap_ms=200, guard_ms=50):
        self.sr = sr = int(sr)
        g = grain_ms(sr)
        for name, ms in (("window_ms", window_ms), ("overlap_ms", overlap_ms), ("guard_ms", guard_ms)):
            if isinstance(ms, bool) or not isinstance(ms, (int, np.integer)) or ms < 0 or ms % g:
                raise ValueError(f"{name}={ms!r} is not a non-negative multiple of the {g} ms grain of {sr} Hz (the smallest "
                                 "multiple of 10 ms that is a whole number of input samples)")
        self.window_ms, self.overlap_ms, self.guard_ms = int(window_ms), int(overlap_ms), int(guard_ms)
        if self.overlap_ms < MIN_OVERLAP_MS:
            raise ValueError(f"overlap_ms={overlap_ms} is under {MIN_OVERLAP_MS} ms (a final window, which is longer than the "
                             "overlap, must clear the mel front end's minimum length)")
        if 2 * self.overlap_ms > self.window_ms:
            raise ValueError(f"2 * overlap_ms={overlap_ms} exceeds window_ms={window_ms}: a window's two overlaps must not meet")
        if 2 * self.guard_ms >= self.overlap_ms:
            raise ValueError(f"2 * guard_ms={guard_ms} leaves nothing of overlap_ms={overlap_ms} to fade over")
        self.W, self.O = self.window_ms * sr // 1000, self.overlap_ms * sr // 1000
        self.H = self.W - self.O
        self.W48, self.O48, self.G48 = self.window_ms * 48, self.overlap_ms * 48, self.guard_ms * 48
        self.H48 = self.W48 - self.O48
        assert self.W * 1000 == self.window_ms * sr and self.O * 1000 == self.overlap_ms * sr and self.H48 % HOP == 0
        self.hop_frames = self.H48 // HOP
        self.window_frames = self.W48 // HOP
        self._ramp = None

    @property
    def key(self):
        """What two sessions must share to run in one batch (beside the time steps)."""
        return self.sr, self.window_ms, self.overlap_ms, self.guard_ms

    def __repr__(self):
        return f"StreamPlan(sr={self.sr}, window_ms={self.window_ms}, overlap_ms={self.overlap_ms}, guard_ms={self.guard_ms})"

    # ---- windows of a stream of T input samples ------------------------------------------------------------------------
    def n_windows(self, T):
        T = int(T)
        if T < 1:
            raise ValueError("an empty stream has no windows")
        return 1 if T <= self.W else 1 + -(-(T - self.W) // self.H)

    def span(self, i, T):
        """[start, stop) of window i in input samples."""
        return i * self.H, min(i * self.H + self.W, int(T))

    def spans(self, T):
        return [self.span(i, T) for i in range(self.n_windows(T))]

    def first_frame(self, i):
        """The absolute mel frame window i starts at."""
        return i * self.hop_frames

    def runnable(self, arrived):
        """The windows that may run once `arrived` input samples are there (before a flush): i H + W <= arrived."""
        return 0 if arrived < self.W else 1 + (int(arrived) - self.W) // self.H

    def out_len(self, T):
        return resample_out_len(int(T), 48000, self.sr)

    def emitted(self, i, T):
        """Output samples a stream of T input samples has emitted after window i: (i + 1) H48, everything after the last."""
        n = self.n_windows(T)
        if not 0 <= i < n:
            raise ValueError(f"window {i} of {n}")
        if i < n - 1:
            return (i + 1) * self.H48
        start, stop = self.span(i, T)
        total = i * self.H48 + resample_out_len(stop - start, 48000, self.sr)
        assert total == self.out_len(T)                        # (i H is a whole number of grains: the ceilings agree)
        return total

    def final_regions(self, T):
        """[(start, stop)] in output samples: what window i's run makes final.  They tile [0, T48)."""
        return [(self.emitted(i - 1, T) if i else 0, self.emitted(i, T)) for i in range(self.n_windows(T))]

    # ---- the seam ------------------------------------------------------------------------------------------------------
    def ramp(self):
        """(w_in, w_out): float32 [O48] each."""
        if self._ramp is None:
            self._ramp = ramp_tables(self.O48, self.G48)
        return self._ramp


def ramp_tables(o48, g48):
    """(w_in, w_out), float32 [o48] each, of an overlap of o48 output samples with a guard of g48 at either end (the formulas
    of the module's head: float64, rounded to float32 once)."""
    o, g = int(o48), int(g48)
    if g < 0 or 2 * g >= o:
        raise ValueError(f"a guard of {g} samples at either end leaves nothing of {o} to fade over")
    F = o - 2 * g
    u = np.arange(o, dtype=np.float64)
    w_in = 0.5 - 0.5 * np.cos(np.pi * (u - g + 0.5) / F)
    w_in[:g] = 0.0
    w_in[o - g:] = 1.0
    w_out = 1.0 - w_in
    return w_in.astype(F32), w_out.astype(F32)


def _fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded: the product is exact in float64; its sum with c is rounded to odd there
    (two-sum for the error), which a final rounding to float32 cannot tell from the exact sum (53 >= 24 + 2 bits)."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        s = c.astype(np.float64)
        t = p + s
        bb = t - p
        err = (p - (t - bb)) + (s - bb)
        inexact = np.isfinite(err) & (err != 0) & np.isfinite(t)
        even = (t.view(np.int64) & 1) == 0
        t = np.where(inexact & even, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
        return t.astype(F32)


def seam(prev, cur, w_in, w_out):
    """float32 [O48]: the last O48 samples of the older window (prev) and the first O48 of the newer one (cur) joined."""
    prev, cur = np.asarray(prev, dtype=F32), np.asarray(cur, dtype=F32)
    w_in, w_out = np.asarray(w_in, dtype=F32), np.asarray(w_out, dtype=F32)
    if not prev.shape == cur.shape == w_in.shape == w_out.shape or prev.ndim != 1:
        raise ValueError(f"seam: shapes {prev.shape} {cur.shape} {w_in.shape} {w_out.shape} must be one 1-D shape")
    zi, zo = w_in == 0, w_out == 0
    with np.errstate(over="ignore", invalid="ignore"):
        s = (w_out * prev).astype(F32)
        own = (w_in * cur).astype(F32)
        out = _fma32(w_in, cur, s)
    out = np.where(zi, s, out)                                  # a zero weight: that term is skipped, whatever it holds
    out = np.where(zo, own, out)
    return np.where(zi & zo, F32(0), out).astype(F32)


def stitch(windows, plan, channels=None):
    """The stream's output, float32 [T48], from its windows' outputs (window i: 1-D, W48 samples, the last one what is left).
    channels=C (a session opened with n_channels=C): the windows are [C, n] and the output [C, T48]; every row is stitched on
    its own with the one ramp."""
    if channels is not None:
        windows = [np.asarray(w, dtype=F32) for w in windows]
        if not windows or any(w.ndim != 2 or w.shape[0] != channels for w in windows):
            raise ValueError(f"a stream of {channels} channels has at least one window and every window is [{channels}, n]")
        return np.stack([stitch([w[c] for w in windows], plan) for c in range(channels)])
    windows = [np.asarray(w, dtype=F32).reshape(-1) for w in windows]
    if not windows:
        raise ValueError("a stream has at least one window")
    for i, w in enumerate(windows):
        last = i == len(windows) - 1
        if (w.size != plan.W48 and not last) or (last and not (plan.O48 < w.size <= plan.W48 or (i == 0 and 0 < w.size <= plan.W48))):
            raise ValueError(f"window {i} of {len(windows)} has {w.size} samples (W48 {plan.W48}, O48 {plan.O48})")
    w_in, w_out = plan.ramp()
    o, h = plan.O48, plan.H48
    total = (len(windows) - 1) * h + windows[-1].size
    out = np.empty(total, dtype=F32)
    for i, w in enumerate(windows):
        w = w.copy()
        if i:
            w[:o] = seam(windows[i - 1][-o:], w[:o], w_in, w_out)
        out[i * h: i * h + w.size] = w                          # (the right overlap is written again by the next window's seam)
    return out
