"""The loudness meter (EBU R128: integrated, momentary, short-term, loudness range), stated on the host in numpy float64: the
DEFINITION that fh_loudness_report_f32 and fh_stream_kweight_energy_f32 (csrc/loudness.hip) are tested against, and the
SCHEDULE of a metered stream that loudness_meter.py runs.

A clip is [C, T] at `rate`; e [C, n_sub] are its sub-block energies (loudness.sub_energies; hop, block = loudness.geometry):
  channel sum   s[i] = sum_c e[c, i], channels added in ascending order
  momentary     zm = loudness.block_energies(e, T, rate): the 400 ms blocks at 100 ms hop of the integrated measure, the project's
                departure included (a clip shorter than one block is one block of its whole length);
                M[j] = -0.691 + 10 log10(zm[j]), -inf for zm[j] = 0
  short-term    K = T // hop complete sub-blocks, ns = K - 29 windows of 3 s when K >= 30, else none;
                zs[j] = (s[j] + s[j + 1] + ... + s[j + 29]) / (30 hop), one addition at a time in ascending order;
                S[j] = -0.691 + 10 log10(zs[j])
  range         EBU Tech 3342 over zs: absolute gate zs > loudness.ZA, relative gate zs > 0.01 mean(absolute-gated zs) (-20 LU),
                both strict; v = the n survivors sorted ascending, lo = v[(10 (n - 1) + 50) // 100], hi = v[(95 (n - 1) + 50) // 100]
                (the nearest-rank rule of the Tech 3342 example code, in integers); LRA = 10 log10(hi / lo) LU, 0.0 when n = 0
  report        (I, M_max, S_max, LRA, M_last, S_last), I = loudness.integrated; a maximum or last value of an empty series is -inf

A stream is metered in whole spans of SPAN = 4096 samples, counted from its sample 0 (the kernel's span: the K-weighting
recursion hands its state over at span boundaries, and only with the boundaries where the one-shot kernel has them are the
energies its bits), the rest when it ends.  With P samples processed a reading covers measured(P, hop) = (P // hop) * hop of
them, the complete sub-blocks; after the end it covers all T samples.  Counters holds this arithmetic for the device classes;
StreamMeter is the numpy meter.

numpy only: nothing here touches torch or the GPU.
"""
import math

import numpy as np

from . import loudness as _loudness

ST_SUB = 30                      # sub-blocks of a short-term window (3 s)
LRA_REL_GATE = 0.01              # -20 LU
LRA_LOW, LRA_HIGH = 10, 95       # the percentiles of the range
SPAN = 4096                      # fh_loudness_span_len()
MAX_SUB = 1 << 20                # sub-blocks of a stream's log, and of a clip fh_loudness_report_f32 takes (29 hours at 100 ms)
MAX_CHANNELS = 8
FIELDS = ("integrated", "momentary_max", "short_term_max", "range", "momentary", "short_term")


def channel_sum(e):
    """e [C, n_sub] -> s [n_sub], the channels added in ascending order."""
    e = np.asarray(e, dtype=np.float64)
    s = e[0].copy()
    for c in range(1, e.shape[0]):
        s = s + e[c]
    return s


def lufs(z):
    """Energies -> -0.691 + 10 log10(z), -inf at 0."""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def momentary(e, T, rate):
    """-> zm [nb]: the energies of the 400 ms blocks."""
    return _loudness.block_energies(e, T, rate)


def n_short_term(T, hop):
    K = int(T) // int(hop)
    return K - (ST_SUB - 1) if K >= ST_SUB else 0


def short_term(e, T, rate):
    """-> zs [ns]: the energies of the 3 s windows over the complete sub-blocks."""
    hop, _ = _loudness.geometry(rate)
    ns = n_short_term(T, hop)
    if ns == 0:
        return np.zeros(0)
    s = channel_sum(e)
    z = s[0:ns].copy()
    for i in range(1, ST_SUB):               # (29 shifted additions: numpy's pairwise .sum() is another order)
        z = z + s[i:i + ns]
    return z / (ST_SUB * hop)


def percentile_ranks(n):
    """The indices of the 10th and the 95th percentile among n sorted survivors."""
    n = int(n)
    return (LRA_LOW * (n - 1) + 50) // 100, (LRA_HIGH * (n - 1) + 50) // 100


def range_gate(zs):
    """-> the mask of the windows that pass both gates of the range.  Both are strict `>`; NaN passes none."""
    zs = np.asarray(zs, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        absolute = zs > _loudness.ZA
        if not absolute.any():
            return absolute
        return absolute & (zs > LRA_REL_GATE * zs[absolute].mean())


def loudness_range(zs):
    """LRA in LU of the short-term energies zs."""
    zs = np.asarray(zs, dtype=np.float64)
    v = np.sort(zs[range_gate(zs)])
    if v.size == 0:
        return 0.0
    lo, hi = percentile_ranks(v.size)
    return 10.0 * math.log10(v[hi] / v[lo])


def report_from_energies(e, T, rate):
    """e [C, n_sub] of a clip of T samples -> (I, M_max, S_max, LRA, M_last, S_last)."""
    e = np.asarray(e, dtype=np.float64)
    if int(T) == 0:
        return (-math.inf, -math.inf, -math.inf, 0.0, -math.inf, -math.inf)
    zm = momentary(e, T, rate)
    zs = short_term(e, T, rate)
    M, S = lufs(zm), lufs(zs)
    return (_loudness.gate(zm)[0], float(M.max()) if M.size else -math.inf, float(S.max()) if S.size else -math.inf,
            loudness_range(zs), float(M[-1]) if M.size else -math.inf, float(S[-1]) if S.size else -math.inf)


def report(x, rate):
    """One clip x [C, T] (or [T]) -> (I, M_max, S_max, LRA, M_last, S_last)."""
    x = _loudness._clip(x)
    T = x.shape[1]
    if T == 0:
        return report_from_energies(np.zeros((x.shape[0], 0)), 0, rate)
    return report_from_energies(_loudness.sub_energies(_loudness.k_weight(x, rate), rate), T, rate)


def measured(P, hop):
    """The samples a reading covers while the stream is open and P samples are processed: the complete sub-blocks."""
    return (int(P) // int(hop)) * int(hop)


def check_channels(n_channels):
    """n_channels= of a meter: None (one mono stream) or an int 1 .. 8."""
    if n_channels is None:
        return None
    if isinstance(n_channels, (bool, float)) or not isinstance(n_channels, (int, np.integer)) or not 1 <= n_channels <= MAX_CHANNELS:
        raise ValueError(f"n_channels must be None or an int 1 .. {MAX_CHANNELS} (the meter's channel count, fixed when it opens), "
                         f"got {n_channels!r}")
    return int(n_channels)


class Counters:
    """The counters of one metered stream: what a push walks, what it keeps and what a reading covers follow from the blocks'
    lengths alone."""

    def __init__(self, rate):
        self.hop, _ = _loudness.geometry(rate)
        self.arrived = 0                     # samples pushed
        self.processed = 0                   # samples walked: a multiple of SPAN until the end
        self.ended = False

    @property
    def kept(self):
        return self.arrived - self.processed

    @property
    def measured(self):
        return self.processed if self.ended else measured(self.processed, self.hop)

    def log_need(self, n_fresh, ended=False):
        """The entries of the energy log behind step(n_fresh, ended): the sub-blocks begun among the samples walked by then.
        RuntimeError past MAX_SUB (and for a closed meter): the counters stay as they are."""
        if self.ended:
            raise RuntimeError("the meter is closed: flush() ends a meter")
        A = self.arrived + int(n_fresh)
        P = A if ended else A // SPAN * SPAN
        need = -(-P // self.hop)
        if need > MAX_SUB:
            raise RuntimeError(f"a meter holds at most 2^20 sub-blocks ({MAX_SUB * self.hop} samples at this rate): this push "
                               f"would begin sub-block {need}")
        return need

    def step(self, n_fresh, ended=False):
        """-> dict(base, n_kept, n_fresh, n_keep, ended, log_need) of this push; the counters then stand behind it."""
        n_fresh = int(n_fresh)
        if n_fresh < 0:
            raise ValueError(f"n_fresh {n_fresh}")
        need = self.log_need(n_fresh, ended)
        A = self.arrived + n_fresh
        P = A if ended else A // SPAN * SPAN
        job = dict(base=self.processed, n_kept=self.kept, n_fresh=n_fresh, n_keep=A - P, ended=bool(ended), log_need=need)
        assert job["base"] % SPAN == 0 and 0 <= job["n_kept"] < SPAN and 0 <= job["n_keep"] < SPAN
        self.arrived, self.processed, self.ended = A, P, bool(ended)
        return job


def _block(b, channels):
    """A pushed block as float32 [rows, n] (None: nothing).  channels None: one mono stream, [n] or [1, n]."""
    rows = channels or 1
    if b is None:
        return np.zeros((rows, 0), np.float32)
    b = np.asarray(b)
    if channels is None and b.ndim == 1:
        b = b[None]
    if b.dtype != np.float32 or b.ndim != 2 or b.shape[0] != rows:
        raise ValueError(f"a block of this meter is float32 [{rows}, n]" + ("" if channels else " or [n]") +
                         f", got {b.dtype} {b.shape}")
    return b


class StreamMeter:
    """The numpy meter: push(block) takes float32 [n] / [1, n] ([C, n] with n_channels=C), read() -> the report over
    x[:, :measured], flush() processes the rest and closes the meter: read() is then the report of all of x."""

    def __init__(self, rate=48000, n_channels=None):
        self.channels = check_channels(n_channels)
        self.rate = int(rate)
        self.counters = Counters(rate)
        self.x = np.zeros((self.channels or 1, 0), np.float32)

    @property
    def measured(self):
        return self.counters.measured

    def push(self, block, final=False):
        b = _block(block, self.channels)         # (checked before anything moves)
        self.counters.step(b.shape[1], final)
        self.x = np.concatenate([self.x, b], 1)

    def flush(self):
        self.push(None, final=True)

    def read(self):
        return report(self.x[:, :self.measured], self.rate)
