"""The device prior's stream, restated on the host in numpy: the DEFINITION that csrc/prior.hip (fh_prior_normal_f32) is tested
against, and the way to rebuild a clip's noise on a CPU from its key (to hand it to the oracle or to the reference as `noise=`).

Element (f, m) of a clip of [n_frames, n_mels]: flat index e = f * n_mels + m, quad q = e >> 2, lane e & 3.
  (r0, r1, r2, r3) = Philox4x32-10(counter = (q & 0xffffffff, q >> 32, stream & 0xffffffff, stream >> 32),
                                   key     = (seed & 0xffffffff, seed >> 32))
  u1 = ((r >> 8) + 1) * 2^-24 in (0, 1],  u2 = (r' >> 8) * 2^-24 in [0, 1)
  lanes 0, 1 = sqrt(-2 ln u1) * (cos, sin)(2 pi u2) from (r0, r1); lanes 2, 3 the same from (r2, r3).
A value depends on (seed, stream, f, m, n_mels) only.  The stream is this project's own: it is neither torch's CPU stream
(flowhighsr.reference_prior_draw restates that one) nor torch's GPU stream.

numpy only: nothing here touches torch or the GPU.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57            # multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85            # Weyl increments of the key
_MASK32, _MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123) vectorised over counters.
    counter: [..., 4] 32-bit words, key: (k0, k1) 32-bit words -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(_MASK32)
    if c.shape[-1] != 4:
        raise ValueError(f"counter must end in 4 words, got shape {c.shape}")
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = int(key[0]) & _MASK32, int(key[1]) & _MASK32
    m32, s32 = np.uint64(_MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0                   # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + PHILOX_W0) & _MASK32, (k1 + PHILOX_W1) & _MASK32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def normalize_key(seed, stream=0):
    """(seed, stream) as two unsigned 64-bit python ints (a negative int64 counts as its two's complement, as on the device)."""
    return int(seed) & _MASK64, int(stream) & _MASK64


def prior_normal_host(seed, stream, n_frames, n_mels=256, dtype=np.float64, first_frame=0):
    """[n_frames, n_mels] prior noise of the key (seed, stream): the formulas above, evaluated in float64 and cast to `dtype`.
    first_frame=f: rows f .. f + n_frames of the key's stream (the quad counter starts at f * n_mels / 4, in 64 bits): what
    fh_prior_normal_at_f32 draws for a window of a streaming session that starts at absolute frame f (stream.py)."""
    seed, stream = normalize_key(seed, stream)
    n_frames, n_mels = int(n_frames), int(n_mels)
    if n_mels % 4 or n_mels <= 0 or n_frames < 0:
        raise ValueError(f"n_mels {n_mels} must be a positive multiple of 4 and n_frames {n_frames} >= 0")
    first_frame = int(first_frame)
    if first_frame < 0 or (first_frame + n_frames) * (n_mels // 4) > _MASK64:
        raise ValueError(f"first_frame {first_frame} must be >= 0 and leave the quad counter within 64 bits")
    q = np.arange(n_frames * n_mels // 4, dtype=np.uint64) + np.uint64(first_frame * (n_mels // 4))
    ctr = np.empty((q.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = q & np.uint64(_MASK32), q >> np.uint64(32)
    ctr[:, 2], ctr[:, 3] = stream & _MASK32, stream >> 32
    r = philox4x32_10(ctr, (seed & _MASK32, seed >> 32))
    ra, rb = r[:, 0::2], r[:, 1::2]                                           # (r0, r2), (r1, r3)
    u1 = ((ra >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (rb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)                 # [quads, pair, (cos, sin)] = lanes 0 .. 3
    return z.reshape(n_frames, n_mels).astype(dtype)


def expand_seed(seed, n_clips):
    """The per-call `seed=` keyword -> one (seed, stream) key per clip.  An int s: clip i gets (s, i).  A sequence with one item
    per clip: an int s_i stands for (s_i, 0), a (seed, stream) pair for itself."""
    if isinstance(seed, (bool, float)) or seed is None:
        raise TypeError(f"seed must be an int or a sequence of ints / (seed, stream) pairs, got {seed!r}")
    if isinstance(seed, (int, np.integer)):
        return [normalize_key(seed, i) for i in range(n_clips)]
    items = list(seed)
    if len(items) != n_clips:
        raise ValueError(f"seed= has {len(items)} items for {n_clips} clips (one int or (seed, stream) pair per clip)")
    keys = []
    for it in items:
        if isinstance(it, (int, np.integer)) and not isinstance(it, bool):
            keys.append(normalize_key(it, 0))
        else:
            pair = tuple(it)
            if len(pair) != 2:
                raise ValueError(f"seed= item {it!r} is neither an int nor a (seed, stream) pair")
            keys.append(normalize_key(pair[0], pair[1]))
    return keys
