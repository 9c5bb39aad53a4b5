"""The input pairs of test_quality_cpu.py and test_hip_quality.py, numpy only.  Every maker returns (est, ref) float32 [C, T].

Frame t of the quality report's STFT covers the samples [480 t - 1024, 480 t + 1024).  A pair with stretches of exact zeros keeps
every frame either free of content or holding at least 336 samples of it, away from the window's ends, so that no bin power lies
between 0 and the floor's neighbourhood: content ends at c with c + 1024 = 400 (mod 480) and resumes at b = 624 (mod 480)."""
import numpy as np

from flowhigh_amd import quality

T_CASES = (1, 479, 480, 481, 2047, 2048, 4807)
KC_CASES = (-1, 0, 1, 341, 1024, 1025)
ZERO_FROM, ZERO_TO = 336, 480 * 7 + 624


def noise(C, T, amp=0.1, seed=0):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (C, T)) * amp).astype(np.float32)


def noise_pair(C, T, seed=0):
    """Two independent noises of amplitude 0.1."""
    return noise(C, T, 0.1, 2 * seed + 1), noise(C, T, 0.1, 2 * seed)


def scaled_pair(C, T, g=2.0, seed=0):
    """est = g ref, exact for a power of two."""
    r = noise(C, T, 0.1, seed)
    return (np.float32(g) * r).astype(np.float32), r


def band_pair(C, T, kc, gain, amp, seed=0):
    """ref = noise of amplitude amp; est = its part below bin kc of 1024 (a brick wall over the whole row's spectrum) + gain times
    the rest."""
    r = noise(C, T, amp, seed).astype(np.float64)
    R = np.fft.rfft(r, axis=1)
    R[:, int(np.ceil(kc / 1024.0 * (R.shape[1] - 1))):] = 0.0
    low = np.fft.irfft(R, n=T, axis=1) if T > 1 else r
    return (low + gain * (r - low)).astype(np.float32), r.astype(np.float32)


def brick_wall_pair(C, T, kc=341, seed=0):
    """The low band kept, the high band scaled by 0.01 (amplitude 4: the scaled bins stay 100 times above the floor)."""
    return band_pair(C, T, kc, 0.01, 4.0, seed)


def hundred_db_pair(C, T, kc=341, seed=0):
    """The estimate's high band 100 dB under the reference's (amplitude 2000 for the same reason)."""
    return band_pair(C, T, kc, 1e-5, 2000.0, seed)


def zero_stretch_pair(C, T, seed=0):
    """Two independent noises (amplitude 1: the frames that hold the content's last 336 samples stay clear of the floor) with
    exact zeros on both sides over [336, 3984): whole frames of digital silence from T = 2047 on."""
    e, r = noise(C, T, 1.0, 2 * seed + 101), noise(C, T, 1.0, 2 * seed + 100)
    e[:, ZERO_FROM:ZERO_TO] = 0.0
    r[:, ZERO_FROM:ZERO_TO] = 0.0
    return e, r


MAKERS = {"noise": noise_pair, "scaled": scaled_pair, "brick wall": brick_wall_pair, "100 dB": hundred_db_pair,
          "zero stretch": zero_stretch_pair}


def clear_of_the_floor(x):
    """From the definition alone: every bin power of every row of x is exactly 0 or at least 1e-6, 100 times the floor."""
    for row in x:
        P = quality.powers(row)
        if not ((P == 0.0) | (P >= 100.0 * quality.FLOOR)).all():
            return False
    return True


def define(est, ref, kc):
    """The definition's four figures of one clip; kc -1: no cutoff."""
    return quality.report(est, ref, kc=None if kc < 0 else kc)
