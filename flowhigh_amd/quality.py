"""The spectral quality report (log-spectral distance by band, and SNR), stated on the host in numpy float64: the DEFINITION that
fh_quality_frames_f32, fh_quality_frames_seg_f32 and fh_quality_report_f32 (csrc/quality.hip, FlowHighSR.measure_quality) are
tested against.

A clip is an estimate e and a reference r, both float32 [C, T] with T >= 1:
  STFT        the geometry of the post-processing STFT: n_fft 2048, hop 480, tables.hann_window() with its float32 values taken
              as float64, 1024 zeros either side (fh_frame_f32 with pad_mode = 1): F = 1 + T // 480 frames, bins k = 0 .. 1024,
              P[t, k] = |X[t, k]|^2
  difference  L = log10(max(P, FLOOR)), FLOOR = 1e-8; d = L_ref - L_est: digital silence on both sides gives exactly 0
  bands       kc = cutoff_bin(cutoff_hz, rate) = clamp(floor(cutoff_hz * 2048 / rate + 0.5), 0, 1025): full = [0, 1025),
              low = [0, kc), high = [kc, 1025).  An empty band is NaN; without a cutoff (kc = None) low and high are NaN.  `rate`
              is used for this conversion only: the STFT does not depend on it.
  per frame   l[t] = sqrt(mean over the band's bins of d[t, k]^2)
  per clip    lsd, lsd_low, lsd_high = the mean of l[t] over all C * F frames;
              snr_db = 10 log10(sum r^2 / sum (r - e)^2) over all samples of all channels, the differences formed per sample in
              float64; the IEEE results stand: +inf for identical rows, -inf for a silent reference beside another estimate,
              NaN for 0 / 0.

Super-resolution is judged by LSD against a full-band reference, below and above the input's cutoff: the low band should come
through untouched, the high band is what the model made.  For a clip generated from sr_in the cutoff is sr_in / 2.

numpy only: nothing here touches the GPU.
"""
import math

import numpy as np

from . import tables

N_FFT = 2048
HOP = 480
PAD = N_FFT // 2
N_BINS = N_FFT // 2 + 1
FLOOR = 1e-8
FIELDS = ("lsd", "lsd_low", "lsd_high", "snr_db")


def n_frames(T):
    return 1 + int(T) // HOP


def cutoff_bin(cutoff_hz, rate=48000):
    """cutoff_hz (None: no cutoff) -> kc, the first bin of the high band, or None."""
    if cutoff_hz is None:
        return None
    c = float(cutoff_hz)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"cutoff_hz must be finite and positive, got {cutoff_hz!r}")
    if isinstance(rate, (bool, str, bytes)) or not (math.isfinite(rate) and rate > 0):
        raise ValueError(f"rate must be positive, got {rate!r}")
    return int(min(max(math.floor(c * N_FFT / float(rate) + 0.5), 0), N_BINS))


def powers(x):
    """One row x [T] (float32) -> P [F, 1025] float64."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 1 or x.size < 1:
        raise ValueError(f"a row is float32 [T >= 1], got {x.dtype} {x.shape}")
    w = tables.hann_window().numpy().astype(np.float64)
    F = n_frames(x.size)
    padded = np.zeros(HOP * (F - 1) + N_FFT, dtype=np.float64)
    padded[PAD:PAD + x.size] = x                # (T < 480 F: every sample lies inside the last frame)
    idx = HOP * np.arange(F)[:, None] + np.arange(N_FFT)[None, :]
    X = np.fft.rfft(padded[idx] * w[None, :], axis=1)
    return X.real ** 2 + X.imag ** 2


def log_power_difference(e, r):
    """Rows e, r [T] -> d [F, 1025] = log10(max(P_r, FLOOR)) - log10(max(P_e, FLOOR))."""
    return np.log10(np.maximum(powers(r), FLOOR)) - np.log10(np.maximum(powers(e), FLOOR))


def frame_lsd(d, kc=None):
    """d [F, 1025] -> l [F, 3]: full, low, high (NaN for an empty band, and for low and high when kc is None)."""
    d2 = np.asarray(d, dtype=np.float64) ** 2
    out = np.full((d2.shape[0], 3), np.nan)
    out[:, 0] = np.sqrt(d2.mean(axis=1))
    if kc is not None:
        if not 0 <= kc <= N_BINS:
            raise ValueError(f"kc {kc} outside 0 .. {N_BINS}")
        if kc > 0:
            out[:, 1] = np.sqrt(d2[:, :kc].mean(axis=1))
        if kc < N_BINS:
            out[:, 2] = np.sqrt(d2[:, kc:].mean(axis=1))
    return out


def snr_db(e, r):
    """e, r [C, T] -> 10 log10(sum r^2 / sum (r - e)^2) over all samples."""
    e, r = np.asarray(e, dtype=np.float64), np.asarray(r, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(np.float64((r * r).sum()) / np.float64(((r - e) ** 2).sum())))


def report(est, ref, cutoff_hz=None, rate=48000, kc=None):
    """One clip: est, ref float32 [C, T] (or [T]) -> (lsd, lsd_low, lsd_high, snr_db) as Python floats.  kc: the cutoff bin
    itself, in place of cutoff_hz."""
    est, ref = np.asarray(est), np.asarray(ref)
    if est.ndim == 1:
        est, ref = est[None], ref[None]
    if est.shape != ref.shape or est.ndim != 2 or est.dtype != np.float32 or ref.dtype != np.float32 or min(est.shape) < 1:
        raise ValueError(f"est and ref are float32 [C, T] of one shape, got {est.dtype} {est.shape} and {ref.dtype} {ref.shape}")
    if kc is None:
        kc = cutoff_bin(cutoff_hz, rate)
    elif cutoff_hz is not None:
        raise ValueError("give cutoff_hz or kc, not both")
    l = np.concatenate([frame_lsd(log_power_difference(e, r), kc) for e, r in zip(est, ref)])
    return (float(l[:, 0].mean()), float(l[:, 1].mean()), float(l[:, 2].mean()), snr_db(est, ref))
