"""Integrated loudness (ITU-R BS.1770-4) and the gain of generate*(loudness=L), stated on the host in numpy float64: the
DEFINITION that csrc/loudness.hip (fh_kweight_energy_f32, fh_kweight_energy_seg_f32, fh_loudness_gate_f32) is tested against.

A clip is [C, T] at `rate`:
  K-weighting      two biquads in cascade (a high shelf, then a high-pass), re-designed for the rate from the analogue prototypes
                   (k_weighting); at 48 kHz they are the Recommendation's table to 9e-16.
  sub-blocks       hop = (rate + 5) // 10 samples (100 ms); e[c, i] = sum of y[c, n]^2 over n in [i hop, min((i + 1) hop, T))
  blocks           block = 4 hop (400 ms, 75 % overlap), nb = (T - block) // hop + 1;
                   z[j] = sum_c (e[c, j] + e[c, j + 1] + e[c, j + 2] + e[c, j + 3]) / block
  gating           absolute: z[j] > ZA = 10^((-70 + 0.691) / 10); relative: z[j] > 0.1 mean(z over the absolute-gate passers)
  loudness         L = -0.691 + 10 log10(mean(z over the blocks that pass both)); -inf when no block passes
  gain             g = fl32(min(10^((target - fl32(L)) / 20), 0.99 / peak)), peak = max |y| over the clip's channels;
                   g = 1 when L is not finite or the peak is 0.  L goes in as the float32 that is reported (measure_loudness).

Departures from the Recommendation, all stated in DESIGN.md "Loudness":
  * a clip shorter than one block is ONE block of its whole length, z[0] = sum_c sum_i e[c, i] / T (serving traffic has 0.3 s clips;
    the Recommendation leaves them unmeasured);
  * every channel weight is 1.0: exact for mono and stereo, 1.5 dB low per surround channel of a 5.1 layout;
  * the gain is capped so that the peak stays at or below 0.99, the project's convention, so with loudness= alone a clip whose
    target needs more than the cap allows comes out quieter than the target (measure_loudness reads what was delivered); with
    true_peak= and limiter='lookahead' the gain is not capped and the limiter of truepeak.py takes what is over.

numpy (and scipy.signal.lfilter for the recursion): nothing here touches torch or the GPU.
"""
import math

import numpy as np

SHELF = dict(f0=1681.974450955533, gain_db=3.999843853973347, q=0.7071752369554196, vb_exp=0.4996667741545416)
HIGHPASS = dict(f0=38.13547087602444, q=0.5003270373238773)
ZA = 10.0 ** ((-70.0 + 0.691) / 10.0)          # the absolute gate, -70 LUFS, as a block energy
REL_GATE = 0.1                                 # -10 LU
PEAK_CAP = 0.99
MIN_LUFS, MAX_LUFS = -70.0, 0.0                # the targets loudness= takes
MIN_HOP = 16                                   # the kernels' chunk: a chunk straddles at most one sub-block boundary


def k_weighting(rate):
    """-> ((b, a) of the shelf, (b, a) of the high-pass): float64 arrays of 3 coefficients each, a[0] = 1."""
    rate = float(rate)
    if not rate > 0:
        raise ValueError(f"rate must be positive, got {rate!r}")
    K = math.tan(math.pi * SHELF["f0"] / rate)
    Vh = 10.0 ** (SHELF["gain_db"] / 20.0)
    Vb = Vh ** SHELF["vb_exp"]
    Q = SHELF["q"]
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    K = math.tan(math.pi * HIGHPASS["f0"] / rate)
    Q = HIGHPASS["q"]
    a0 = 1.0 + K / Q + K * K
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, highpass


def coefficients(rate):
    """The 10 doubles the kernels take: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2."""
    (b1, a1), (b2, a2) = k_weighting(rate)
    return [float(v) for v in (*b1, a1[1], a1[2], *b2, a2[1], a2[2])]


def geometry(rate):
    """-> (hop, block) in samples."""
    if isinstance(rate, (bool, str, bytes)) or int(rate) != rate or int(rate) <= 0:
        raise ValueError(f"rate must be a positive integer, got {rate!r}")
    hop = (int(rate) + 5) // 10
    if hop < MIN_HOP:
        raise ValueError(f"rate {rate}: a sub-block of {hop} samples is shorter than {MIN_HOP}; loudness needs a rate of at least "
                         f"{10 * MIN_HOP - 5}")
    return hop, 4 * hop


def k_weight(x, rate):
    """float64 K-weighted copy of x [..., T] (float64 direct-form II transposed recursion from rest)."""
    from scipy.signal import lfilter
    (b1, a1), (b2, a2) = k_weighting(rate)
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] == 0:
        return x.copy()
    return lfilter(b2, a2, lfilter(b1, a1, x, axis=-1), axis=-1)


def state_space(rate):
    """The cascade as s' = A s + B x, y = C s + D x over the 4 transposed-form states (shelf s1 s2, high-pass t1 t2):
    -> (A [4, 4], B [4], C [4], D)."""
    (b, a), (d, c) = k_weighting(rate)
    # shelf: y1 = b0 x + s1; s1' = b1 x - a1 y1 + s2; s2' = b2 x - a2 y1.  high-pass on y1: y = d0 y1 + t1; t1' = d1 y1 - c1 y + t2; ...
    A = np.zeros((4, 4))
    B = np.zeros(4)
    y1_s, y1_x = np.array([1.0, 0, 0, 0]), b[0]                    # y1 = y1_s . s + y1_x x
    y_s, y_x = d[0] * y1_s + np.array([0, 0, 1.0, 0]), d[0] * y1_x
    A[0] = -a[1] * y1_s + np.array([0, 1.0, 0, 0])
    B[0] = b[1] - a[1] * y1_x
    A[1] = -a[2] * y1_s
    B[1] = b[2] - a[2] * y1_x
    A[2] = d[1] * y1_s - c[1] * y_s + np.array([0, 0, 0, 1.0])
    B[2] = d[1] * y1_x - c[1] * y_x
    A[3] = d[2] * y1_s - c[2] * y_s
    B[3] = d[2] * y1_x - c[2] * y_x
    return A, B, y_s, y_x


def k_weight_chunked(x, rate, chunk):
    """k_weight of one row x [T] the way the kernels run it: every chunk of `chunk` samples from zero state, the chunks' end
    states handed over with A^chunk, every chunk again from its true start state.  float64; equals k_weight to rounding."""
    A, B, C, D = state_space(rate)
    x = np.asarray(x, dtype=np.float64)
    T, L = x.shape[0], int(chunk)
    n = -(-T // L)
    xp = np.zeros(n * L)
    xp[:T] = x
    xp = xp.reshape(n, L)

    def run(start):                       # all chunks at once from their start states [n, 4] -> (outputs [n, L], end states)
        s, y = start.copy(), np.empty((n, L))
        for k in range(L):
            y[:, k] = s @ C + D * xp[:, k]
            s = s @ A.T + np.outer(xp[:, k], B)
        return y, s
    _, z = run(np.zeros((n, 4)))
    AL = np.linalg.matrix_power(A, L)
    start = np.zeros((n, 4))
    for j in range(1, n):                 # (the kernels scan this in log steps with A^(L 2^i))
        start[j] = AL @ start[j - 1] + z[j - 1]
    y, _ = run(start)
    return y.reshape(-1)[:T]


def sub_energies(y, rate):
    """K-weighted y [..., T] -> e [..., ceil(T / hop)] float64: the energies of the 100 ms sub-blocks, the last one as long as it is."""
    hop, _ = geometry(rate)
    y = np.asarray(y, dtype=np.float64)
    T = y.shape[-1]
    n_sub = -(-T // hop)
    sq = np.zeros(y.shape[:-1] + (n_sub * hop,))
    sq[..., :T] = y * y
    return sq.reshape(y.shape[:-1] + (n_sub, hop)).sum(-1)


def block_energies(e, T, rate):
    """e [C, n_sub] of a clip of T samples -> z [nb] float64."""
    hop, block = geometry(rate)
    e = np.asarray(e, dtype=np.float64)
    if e.ndim != 2 or e.shape[1] != -(-int(T) // hop):
        raise ValueError(f"sub-energies {e.shape} do not belong to a clip of {T} samples at hop {hop}")
    if T < block:
        return np.array([e.sum() / T]) if T > 0 else np.zeros(0)
    nb = (int(T) - block) // hop + 1
    s = e.sum(0)
    return (s[0:nb] + s[1:nb + 1] + s[2:nb + 2] + s[3:nb + 3]) / block


def gate(z):
    """Block energies -> (L in LUFS, the mask of the blocks that pass both gates).  Both gates are strict `>`; NaN passes none."""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        absolute = z > ZA
        if not absolute.any():
            return -math.inf, absolute
        both = absolute & (z > REL_GATE * z[absolute].mean())
    if not both.any():
        return -math.inf, both
    return -0.691 + 10.0 * math.log10(z[both].mean()), both


def gain(L, target, peak):
    """The float32 gain that takes a clip of loudness L (LUFS) and peak `peak` to `target` LUFS, the peak kept at or below 0.99.
    L is rounded to float32 first: it is the value measure_loudness reports, and the gain is a function of that."""
    L, peak = float(np.float32(L)), float(peak)
    if not math.isfinite(L) or not peak > 0 or not math.isfinite(peak) or not math.isfinite(float(target)):
        return np.float32(1.0)
    return np.float32(min(10.0 ** ((float(target) - L) / 20.0), PEAK_CAP / peak))


def _clip(x):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2:
        raise ValueError(f"a clip is [C, T], got shape {x.shape}")
    return x


def integrated(x, rate):
    """Integrated loudness in LUFS of one clip x [C, T] (or [T])."""
    x = _clip(x)
    if x.shape[1] == 0:
        return -math.inf
    return gate(block_energies(sub_energies(k_weight(x, rate), rate), x.shape[1], rate))[0]


def normalise(x, rate, target):
    """x [C, T] float32 -> (fl32(x * g), g, L): the clip at `target` LUFS as generate*(loudness=target) delivers it."""
    x = _clip(x).astype(np.float32)
    L = integrated(x, rate)
    with np.errstate(invalid="ignore"):
        peak = float(np.abs(x).max()) if x.size else 0.0
    g = gain(L, target, peak)
    return (x * g).astype(np.float32), g, L


def resolve_loudness(loudness):
    """loudness= -> None or the target as a float: finite, -70 <= L <= 0."""
    if loudness is None:
        return None
    if isinstance(loudness, (bool, str, bytes)) or not isinstance(loudness, (int, float, np.integer, np.floating)):
        raise ValueError(f"loudness must be None or a target in LUFS ({MIN_LUFS:g} .. {MAX_LUFS:g}), got {loudness!r}")
    L = float(loudness)
    if not math.isfinite(L) or not MIN_LUFS <= L <= MAX_LUFS:
        raise ValueError(f"loudness must be None or a target in LUFS ({MIN_LUFS:g} .. {MAX_LUFS:g}), got {loudness!r}")
    return L
