"""The int16 encoding of delivery (generate*(pcm='int16', dither='tpdf')), stated on the host in numpy: the DEFINITION that
csrc/pcm.hip (fh_pcm_i16_f32, fh_pcm_i16_seg_f32) is tested against, bit for bit.

A sample x (float32):
  v = fl32(x * 32768)                  the product is exact (a power of two)
  v = fl32(v + d)                      when dithering
  q = rint(v), ties to even, clamped to [-32768, 32767]; NaN encodes as 0, +-inf saturates.
The dither d of channel c, sample t of a clip with the key (seed, stream):
  (r0, r1, r2, r3) = Philox4x32-10(counter = (q & m32, q >> 32, stream & m32, stream >> 32), q = t >> 1,
                                   key     = ((seed & m32) ^ 0x50434D31, ((seed >> 32) ^ c) & m32))          (prior.philox4x32_10)
  even t: (ra, rb) = (r0, r1); odd t: (r2, r3)
  d = (ra >> 8) * 2^-24 - (rb >> 8) * 2^-24
the difference of two uniforms on [0, 1): triangular on (-1, 1) LSB with variance 1/6, a multiple of 2^-24 and so exact in
float32.  It depends on (seed, stream, c, t) only -- not on the batch, the layout, the number of channels or the clip's length --
and the key's tag keeps its Philox blocks apart from the prior's under the same (seed, stream).


The 24-bit encodings (pcm='s24': packed signed 24-bit little-endian, 3 bytes a sample; pcm='s24in32': the same integer in an
int32; fh_pcm_s24_f32, fh_pcm_s24_seg_f32, fh_stream_pcm_s24_rows_f32).  A sample x (float32):
  v = float64(x) * 2^23                exact
  v = v + float64(d)                   when dithering: ONE float64 add, round to nearest even
  q = rint(v), ties to even, clamped to [-8388608, 8388607]; NaN encodes as 0, +-inf saturates.
d is the dither above, unchanged: the 24-bit dither of a sample is its 16-bit one, one LSB being 256 times smaller.  The add is
in float64 because x * 2^23 fills the float32 significand: fl32(x * 2^23 + d) rounds on a grid of 0.5 and throws the dither away
(constant float32(0.7), key (7, 0), 2^20 samples: a DC bias of +0.187 LSB against -0.0004; DESIGN.md "Delivery").

numpy only: nothing here touches torch or the GPU.
"""
import numpy as np

from .prior import _MASK32, normalize_key, philox4x32_10

KEY_TAG = 0x50434D31            # 'PCM1'
FULL_SCALE = 32768.0
FULL_SCALE24 = 8388608.0
# the values of pcm=.  The 24-bit names are the sample-format names of ffmpeg and ALSA: the result is a byte layout, not a dtype.
FORMATS = ("int16", "s24", "s24in32")


def encoder(pcm):
    """pcm -> the format's (quantize, encode): functions of (x, d) and of (x, key, interleaved)."""
    if pcm == "int16":
        return quantize, encode
    if pcm not in FORMATS:
        raise ValueError(f"pcm must be one of {FORMATS}, got {pcm!r}")
    packed = pcm == "s24"
    return ((lambda x, d=None: pack24(quantize24(x, d))) if packed else quantize24,
            lambda x, key=None, interleaved=False: encode24(x, key, interleaved, packed))


def dither_uniforms(seed, stream, channel, n, first=0):
    """(ra >> 8, rb >> 8) of samples first .. first + n - 1 of one channel: two uint32 arrays [n] of 24-bit integers.
    first: the absolute index of the first sample (a block of a stream, stream_delivery.py); the counter has 64 bits."""
    seed, stream = normalize_key(seed, stream)
    n, first = int(n), int(first)
    if n < 0 or not 0 <= int(channel) < 2 ** 32:
        raise ValueError(f"n {n} must be >= 0 and channel {channel} a 32-bit index")
    if first < 0 or first + n > 2 ** 64:
        raise ValueError(f"first {first} must be >= 0 and leave the sample index within 64 bits")
    q = np.arange(first >> 1, (first + n + 1) >> 1, dtype=np.uint64)         # the blocks that hold the samples
    odd = first & 1
    ctr = np.empty((q.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = q & np.uint64(_MASK32), q >> np.uint64(32)
    ctr[:, 2], ctr[:, 3] = stream & _MASK32, stream >> 32
    r = philox4x32_10(ctr, ((seed & _MASK32) ^ KEY_TAG, ((seed >> 32) ^ int(channel)) & _MASK32))
    ra = r[:, 0::2].reshape(-1)[odd:odd + n] >> np.uint32(8)          # (r0, r2) of every block = samples 2q, 2q + 1
    rb = r[:, 1::2].reshape(-1)[odd:odd + n] >> np.uint32(8)
    return ra, rb


def tpdf_dither(seed, stream, channel, n, first=0):
    """float32 [n]: the dither of samples first .. first + n - 1 of channel `channel` under the key (seed, stream), in LSB."""
    ra, rb = dither_uniforms(seed, stream, channel, n, first)
    d = (ra.astype(np.int64) - rb.astype(np.int64)).astype(np.float64) * 2.0 ** -24
    out = d.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), d)          # exact by construction
    return out


def quantize(x, d=None):
    """float32 samples (any shape) -> int16, d: the dither in LSB (same shape) or None."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(x, dtype=np.float32) * np.float32(FULL_SCALE)
        if d is not None:
            v = (v + np.asarray(d, dtype=np.float32)).astype(np.float32)
        q = np.rint(v)
        q = np.where(np.isnan(v), np.float32(0), np.clip(q, np.float32(-32768), np.float32(32767)))
    return q.astype(np.int16)


def encode(x, key=None, interleaved=False):
    """One clip, planar float32 [C, T] (or [T]: one channel) -> int16 [C, T], or [T, C] with interleaved.
    key: None (no dither) or the clip's (seed, stream)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2:
        raise ValueError(f"a clip is [C, T], got shape {x.shape}")
    d = None
    if key is not None:
        d = np.stack([tpdf_dither(key[0], key[1], c, x.shape[1]) for c in range(x.shape[0])])
    q = quantize(x, d)
    return np.ascontiguousarray(q.T) if interleaved else q


def quantize24(x, d=None):
    """float32 samples (any shape) -> the 24-bit integer in an int32, d: the dither in LSB (same shape) or None."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.asarray(x, dtype=np.float32).astype(np.float64) * FULL_SCALE24
        if d is not None:
            v = v + np.asarray(d, dtype=np.float32).astype(np.float64)
        q = np.where(np.isnan(v), 0.0, np.clip(np.rint(v), -8388608.0, 8388607.0))
    return q.astype(np.int32)


def pack24(q):
    """int32 [...] -> uint8 [..., 3]: the low three bytes of every sample, least significant first (pcm_s24le)."""
    u = np.asarray(q, dtype=np.int32).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], -1).astype(np.uint8)


def unpack24(b):
    """uint8 [..., 3] -> int32 [...]: pack24's inverse, sign-extended."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int32)
    u = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return (u ^ 0x800000) - 0x800000


def encode24(x, key=None, interleaved=False, packed=True):
    """One clip, planar float32 [C, T] (or [T]: one channel) -> packed: uint8 [C, T, 3], or [T, C, 3] with interleaved
    ('s24'); not packed: int32 [C, T] / [T, C] ('s24in32').  key: None (no dither) or the clip's (seed, stream)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2:
        raise ValueError(f"a clip is [C, T], got shape {x.shape}")
    d = None
    if key is not None:
        d = np.stack([tpdf_dither(key[0], key[1], c, x.shape[1]) for c in range(x.shape[0])])
    q = quantize24(x, d)
    q = np.ascontiguousarray(q.T) if interleaved else q
    return pack24(q) if packed else q
