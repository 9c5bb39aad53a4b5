"""True peak (ITU-R BS.1770-4 Annex 2) and the look-ahead limiter of generate*(true_peak=, limiter=), stated on the host in numpy
float64: the DEFINITION that csrc/truepeak.hip (fh_true_peak_*, fh_tp_envelope_*, fh_limit_*, fh_delivery_gain_f32) is tested against.

A clip is x [C, T] float32 at `rate`:
  oversampling   factor 4 at every rate, by the project's own tables.resample_poly_plan(4, 1) = scipy.signal.resample_poly(x, 4, 1):
                 81 taps firwin(81, 1/4, ('kaiser', 5.0)) * 4, zeros outside the clip, output 4 n aligned to input n.  float64
                 arithmetic on those FLOAT32 taps: x4[4 n + p] = sum_i h[p + 4 i] x[n + 10 - i] (21 taps at p = 0, 20 otherwise)
  envelope       m[n] = fl32(max over channels c and phases p of max(|x[c, n]|, |x4[c, 4 n + p]|)): one envelope for all channels
                 (the limiter is channel-linked: the stereo image stays).  The |x[c, n]| term is needed: phase 0 of this filter is
                 not the identity
  true peak      TP = max_n m[n]; dbtp = fl32(20 log10(TP)), -inf for silence
  static rule    (limiter=None) one gain per clip, g = fl32(min(g_L, c / TP)), c = 10^(true_peak / 20); g_L = 1 without loudness=,
                 else loudness.gain(L, target, peak), the capped gain of loudness= alone; g = g_L when TP is 0
  limiter        (limiter='lookahead') zero delay, symmetric, no recursion; H = (rate + 100) // 200 samples (5 ms), c32 = fl32(c):
                   r[n] = c32 / m[n] in float32 where m[n] > c32, else 1; r = 1 outside [0, T)
                   q[n] = min(r[n - H .. n + H]) on [-H, T + H)   (the extension past the ends is required: a peak at the first or
                                                                   last sample is then held over the whole of its window)
                   g[n] = fl32(sum_{|k| <= H} w[k] q[n + k]), w = np.hanning(2 H + 3)[1:-1] normalised in float64, the sum in float64
                   y[c, n] = clamp(fl32(x[c, n] g[n]), -c32, c32)
                 every q[n + k] is at most r[n], so g[n] <= r[n], also after the rounding to float32; the clamp moves a value by one
                 ulp at the most and makes "no delivered sample exceeds the ceiling" exact
  with loudness= and the limiter: the loudness gain is UNCAPPED, fl32(10^((target - fl32(L)) / 20)), applied first; the limiter
                 runs on the result.  Limiting removes energy: the delivered loudness ends slightly under the target, nothing iterates.

Departures from the Recommendation (DESIGN.md "True peak and limiter"): Annex 2 uses a 48-tap filter and allows factor 2 from 96 kHz
on; this is 81 taps and factor 4 at every rate.  On tones at 0.02, 0.125, 0.25 and 0.45 fs it reads within +0.016 / -0.038 dB.

Non-finite input is outside the contract (the model does not produce it): what a NaN or an infinity in x gives is not defined.

numpy and scipy: nothing here touches torch or the GPU.
"""
import math

import numpy as np

from . import loudness as _loudness
from . import tables

FACTOR = 4
HALF = 10                                       # input samples either side of n that x4[4 n + p] reads
N_TAPS = 20 * FACTOR + 1
MIN_DBTP, MAX_DBTP = -20.0, 0.0                 # the ceilings true_peak= takes
MAX_H = 512                                     # the limiter kernel's window: 2 H + 1 <= 1025
MAX_RATE = 200 * MAX_H                          # 102 400 Hz
_LIMITERS = (None, "lookahead")


def taps():
    """The 81 float32 taps h (the plan's taps without its one leading pad)."""
    plan, n_pre_remove, up, down = tables.resample_poly_plan(FACTOR, 1)
    h = plan.numpy()
    assert h.shape == (N_TAPS + 1,) and h[0] == 0 and n_pre_remove == 4 * HALF + 1 and (up, down) == (FACTOR, 1)
    return h[1:]


def _clip(x):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2:
        raise ValueError(f"a clip is [C, T], got shape {x.shape}")
    return x


def oversample(x):
    """x [..., T] -> float64 [..., 4 T]: resample_poly(x, 4, 1) in float64 on the float32 taps."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    h = taps().astype(np.float64)
    flat = x.reshape(-1, T)
    out = np.zeros((flat.shape[0], FACTOR * T))
    for r in range(flat.shape[0]):
        up = np.zeros(FACTOR * T)
        up[::FACTOR] = flat[r]
        if T:
            out[r] = np.convolve(up, h)[FACTOR * HALF:FACTOR * HALF + FACTOR * T]
    return out.reshape(x.shape[:-1] + (FACTOR * T,))


def envelope(x):
    """x [C, T] float32 -> m [T] float32: the joint oversampled envelope of the clip."""
    x = _clip(x).astype(np.float32)
    C, T = x.shape
    if C == 0 or T == 0:
        return np.zeros(T, dtype=np.float32)
    x4 = np.abs(oversample(x)).reshape(C, T, FACTOR).max(-1)
    return np.maximum(np.abs(x.astype(np.float64)), x4).max(0).astype(np.float32)


def true_peak(x):
    """TP of one clip x [C, T] as a float32 (0 for silence or an empty clip)."""
    m = envelope(x)
    return np.float32(m.max()) if m.size else np.float32(0.0)


def dbtp(tp):
    """fl32(20 log10(TP)); -inf for TP = 0."""
    tp = float(tp)
    return np.float32(20.0 * math.log10(tp)) if tp > 0 else np.float32(-math.inf)


def ceiling(true_peak_db):
    """c = 10^(true_peak / 20) as a Python float (float64)."""
    return 10.0 ** (float(true_peak_db) / 20.0)


def half_window(rate):
    """H = (rate + 100) // 200 samples: 5 ms either side."""
    if isinstance(rate, (bool, str, bytes)) or int(rate) != rate or int(rate) <= 0:
        raise ValueError(f"rate must be a positive integer, got {rate!r}")
    H = (int(rate) + 100) // 200
    if H < 1:
        raise ValueError(f"rate {rate}: a look-ahead of {H} samples; limiter='lookahead' needs a rate of at least 100 Hz")
    if H > MAX_H:
        raise ValueError(f"rate {rate}: a look-ahead of {H} samples is more than the limiter's {MAX_H}; limiter='lookahead' takes "
                         f"rates up to {MAX_RATE + 99} Hz")
    return H


def window(H):
    """w [2 H + 1] float64: np.hanning(2 H + 3) without its two zeros, normalised to sum 1."""
    w = np.hanning(2 * int(H) + 3)[1:-1].astype(np.float64)
    return w / w.sum()


def static_gain(tp, true_peak_db, g_l=1.0):
    """g = fl32(min(g_L, c / TP)); g_L when TP is 0."""
    tp, g_l = float(np.float32(tp)), np.float32(g_l)
    if not tp > 0:
        return g_l
    return np.float32(min(float(g_l), ceiling(true_peak_db) / tp))


def uncapped_gain(L, target):
    """fl32(10^((target - fl32(L)) / 20)); 1 when L is not finite or there is no target."""
    if target is None:
        return np.float32(1.0)
    L = float(np.float32(L))
    if not math.isfinite(L) or not math.isfinite(float(target)):
        return np.float32(1.0)
    return np.float32(10.0 ** ((float(target) - L) / 20.0))


def reduction(m, true_peak_db):
    """m [T] float32 -> r [T] float32: c32 / m where m > c32, else 1."""
    m = np.asarray(m, dtype=np.float32)
    c32 = np.float32(ceiling(true_peak_db))
    r = np.ones_like(m)
    over = m > c32
    r[over] = c32 / m[over]
    return r


def limiter_gain(m, H, true_peak_db):
    """m [T] float32 -> (g [T] float32, r [T] float32) of the look-ahead limiter with half window H."""
    from scipy.ndimage import minimum_filter1d
    H = int(H)
    r = reduction(m, true_peak_db)
    T = r.shape[0]
    if T == 0:
        return r.copy(), r
    rp = np.ones(T + 4 * H, dtype=np.float32)
    rp[2 * H:2 * H + T] = r
    q = minimum_filter1d(rp, size=2 * H + 1, mode="constant", cval=1.0)[H:H + T + 2 * H]      # q on [-H, T + H)
    g = np.convolve(q.astype(np.float64), window(H)[::-1], mode="valid")
    assert g.shape == (T,)
    return g.astype(np.float32), r


def limit(x, rate, true_peak_db, m=None):
    """x [C, T] float32 -> (y [C, T] float32, g [T] float32, m [T] float32): limiter='lookahead' on one clip; m: its envelope,
    measured here when None."""
    x = _clip(x).astype(np.float32)
    H = half_window(rate)
    m = envelope(x) if m is None else np.asarray(m, dtype=np.float32)
    g, _ = limiter_gain(m, H, true_peak_db)
    c32 = np.float32(ceiling(true_peak_db))
    y = np.clip((x * g[None, :]).astype(np.float32), -c32, c32)
    return y, g, m


def deliver(x, rate, true_peak_db, limiter=None, loudness=None):
    """What generate*(true_peak=, limiter=, loudness=) does to the clip x [C, T] float32 that the call without them delivers at
    `rate` -> y [C, T] float32."""
    x = _clip(x).astype(np.float32)
    resolve_true_peak(true_peak_db, limiter)
    L = _loudness.integrated(x, rate) if loudness is not None else None
    if limiter is None:
        g_l = np.float32(1.0)
        if loudness is not None:
            g_l = _loudness.gain(L, loudness, float(np.abs(x).max()) if x.size else 0.0)
        return (x * static_gain(true_peak(x), true_peak_db, g_l)).astype(np.float32)
    x = (x * uncapped_gain(L, loudness)).astype(np.float32) if loudness is not None else x
    return limit(x, rate, true_peak_db)[0]


def resolve_true_peak(true_peak, limiter=None, rate=None):
    """true_peak=, limiter= -> (None | the ceiling in dBTP as a float, None | 'lookahead').  rate: the delivered rate, checked
    against the limiter's window when given."""
    if limiter not in _LIMITERS:
        raise ValueError(f"limiter must be one of {_LIMITERS}, got {limiter!r}")
    if true_peak is None:
        if limiter is not None:
            raise ValueError("limiter= goes with true_peak=: the limiter holds the result under that ceiling")
        return None, None
    if isinstance(true_peak, (bool, str, bytes)) or not isinstance(true_peak, (int, float, np.integer, np.floating)):
        raise ValueError(f"true_peak must be None or a ceiling in dBTP ({MIN_DBTP:g} .. {MAX_DBTP:g}), got {true_peak!r}")
    tp = float(true_peak)
    if not math.isfinite(tp) or not MIN_DBTP <= tp <= MAX_DBTP:
        raise ValueError(f"true_peak must be None or a ceiling in dBTP ({MIN_DBTP:g} .. {MAX_DBTP:g}), got {true_peak!r}")
    if limiter is not None and rate is not None:
        half_window(rate)
    return tp, limiter
