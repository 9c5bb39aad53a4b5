"""Streaming delivery (FlowHighSR.stream(delivery=), FlowHighSR.delivery_stream), stated on the host in numpy: the SCHEDULE that
delivery_stream.py runs and the DEFINITION that csrc/stream_delivery.hip is tested against, bit for bit.

A stream of 48 kHz samples arrives in blocks; every block goes through up to three stages, each of which keeps what it needs of
the past in a carry and gives the bits of the one-shot delivery of the whole stream (delivery.Delivery.batch at level='input'):

  resampler   (taps, pre, up, down) = tables.resample_poly_plan(R, 48000); out[i] = sum_j x[j] h[(i + pre) down - j up], the
              float32 fma loop of resample_poly_kernel from j_hi(i) = (i + pre) down // up downwards.  With E inputs final:
                n_final(E) = max(0, (E up - 1) // down - pre + 1)     outputs whose highest input is there (j_hi(i) <= E - 1)
                             resample_out_len(E, R, 48000) at the stream's end (the kernel clamps j_hi to the last input)
                j_lo(i)    = max(0, ceil(((i + pre) down - n_taps + 1) / up))      the lowest input output i reads
              the carry is the inputs from j_lo(first unemitted output) on: at most ceil(n_taps / up) + 1 samples.
  limiter     at the delivered rate, H = truepeak.half_window(rate), D = 2 H + truepeak.HALF: y[n] reads x[n - D .. n + D].  With F
              samples final, max(0, F - D) outputs are final while the stream is open and F at its end; the carry is the samples
              from max(0, first unemitted - D) on: at most 2 D.  The edge rules of truepeak.py (zeros outside for the
              oversampling, r = 1 outside, q extended by H) hold at the stream's first and last sample and nowhere else.
  encoder     sample t of the stream takes pcm.py's dither of channel 0 at the absolute index t: no carry, one counter.  The
              format is the plan's pcm: 'int16', or 24 bits as 's24' (3 bytes a sample: blocks [C, n, 3] / [n, C, 3]) or
              's24in32' (int32): pcm.quantize24 / pcm.pack24.

A stream of C channels (1 <= C <= 8, fixed when it opens) is C rows [C, T] that move together: ONE set of counters per stage, the
resampler per row, the limiter channel-linked as truepeak.limit is on a [C, T] clip (m is the maximum over the rows of what a
row alone gives, one gain for every row), the encoder with channel c's dither at the absolute index, planar [C, n] or sample
frames [n, C] (interleaved).  A [T] stream is the one row it always was.

A stage's step is (base, first, n_out, n_keep): its source is carry + fresh block, `base` the absolute index of the carry's first
sample; it writes the outputs [first, first + n_out) and keeps the last n_keep source samples as the next carry.  `chunked` walks
these steps in numpy and equals the whole-stream definitions (`whole`: the fma loop below, truepeak.limit, pcm.encode).

numpy only: nothing here touches torch or the GPU.
"""
import numpy as np

from . import pcm as _pcm
from . import tables
from . import truepeak as _truepeak

F32 = np.float32


# ---- resampler -------------------------------------------------------------------------------------------------------------
class ResampleFilter:
    """tables.resample_poly_plan(rate, 48000) as numpy: taps float32 [n_taps] (pre-padding included), pre, up, down."""

    def __init__(self, rate):
        plan = tables.resample_poly_plan(int(rate), 48000)
        if plan is None:
            raise ValueError("48 kHz is delivered as it is: there is no filter")
        taps, self.pre, self.up, self.down = plan
        self.taps = taps.numpy()
        self.n_taps = int(self.taps.size)
        self.rate = int(rate)

    def n_final(self, E, ended=False):
        """Outputs that are final with E inputs (ended: E is the whole stream)."""
        E = int(E)
        if ended:
            return tables.resample_out_len(E, self.rate, 48000)
        return max(0, (E * self.up - 1) // self.down - self.pre + 1)

    def j_hi(self, i):
        return (int(i) + self.pre) * self.down // self.up

    def j_lo(self, i):
        return max(0, -((self.n_taps - 1 - (int(i) + self.pre) * self.down) // self.up))

    @property
    def carry_bound(self):
        return -(-self.n_taps // self.up) + 1


class Stage:
    """The counters of one stage of one stream.  step(n_fresh, ended) -> the job of this push and moves the counters on."""

    def __init__(self, first=0):
        self.base = int(first)       # absolute index of the carry's first sample
        self.n_carry = 0
        self.emitted = int(first)    # outputs written so far = the absolute index of the next one
        self.ended = False

    @property
    def arrived(self):
        return self.base + self.n_carry

    def _final(self, E, ended):       # outputs final with E inputs
        raise NotImplementedError

    def _lowest(self, i):             # the lowest input that output i reads
        raise NotImplementedError

    def peek(self, n_fresh, ended=False):
        """n_out of step(n_fresh, ended), the counters left as they are: what a push will emit, known before any launch."""
        return max(self.emitted, self._final(self.arrived + int(n_fresh), ended)) - self.emitted

    def step(self, n_fresh, ended=False):
        """-> dict(base, n_carry, n_fresh, first, n_out, n_keep, ended) of this push; the stage then stands behind it."""
        n_fresh = int(n_fresh)
        if self.ended or n_fresh < 0:
            raise ValueError("the stage has ended" if self.ended else f"n_fresh {n_fresh}")
        E = self.arrived + n_fresh
        n_fin = self.emitted + self.peek(n_fresh, ended)
        job = dict(base=self.base, n_carry=self.n_carry, n_fresh=n_fresh, first=self.emitted, n_out=n_fin - self.emitted,
                   ended=bool(ended))
        new_base = E if ended else min(E, max(self.base, self._lowest(n_fin)))
        job["n_keep"] = E - new_base
        # what the kernels rely on: every output's inputs lie in the two spans, and the next carry is a tail of them
        assert job["n_out"] == 0 or self.base <= self._lowest(self.emitted), (self.base, self.emitted)
        assert 0 <= job["n_keep"] <= self.n_carry + n_fresh and job["n_out"] >= 0
        self.base, self.n_carry, self.emitted, self.ended = new_base, E - new_base, n_fin, bool(ended)
        return job


class ResampleStage(Stage):
    def __init__(self, flt):
        super().__init__()
        self.flt = flt

    def _final(self, E, ended):
        return self.flt.n_final(E, ended)

    def _lowest(self, i):
        return self.flt.j_lo(i)


class LimitStage(Stage):
    def __init__(self, H):
        super().__init__()
        self.H = int(H)
        self.D = 2 * self.H + _truepeak.HALF

    def _final(self, F, ended):
        return F if ended else max(0, F - self.D)

    def _lowest(self, n):
        return max(0, n - self.D)


class EncodeStage(Stage):
    """No carry: output t is input t.  first: the absolute index of the stream's first sample (the dither's counter)."""

    def _final(self, E, ended):
        return E

    def _lowest(self, t):
        return t


def _fma32(a, b, c):
    """fl32(a b + c) through float64: the product of two float32 is exact there, the sum is rounded twice.  The restatement pins
    which samples an output reads and in which order; the device's single rounding is compared with the device's."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def resample_span(flt, src, base, E, first, n_out, reads=None):
    """Outputs [first, first + n_out) from src = the inputs [base, base + len(src)), E = base + len(src) inputs there: the
    kernel's loop (j descending from min(j_hi, E - 1), break at k >= n_taps), vectorised over the outputs (and over the rows
    of src [C, n], each row a stream of its own under the one schedule).
    reads: a dict that gets the lowest and highest input index read (min, max)."""
    src = np.asarray(src, dtype=F32)
    assert base + src.shape[-1] == E
    i = first + np.arange(int(n_out), dtype=np.int64)
    pos = (i + flt.pre) * flt.down
    j = np.minimum(pos // flt.up, E - 1)
    acc = np.zeros(src.shape[:-1] + (i.size,), dtype=F32)
    live = np.ones(i.size, dtype=bool)
    while True:
        k = pos - j * flt.up
        live &= (j >= 0) & (k < flt.n_taps)
        if not live.any():
            break
        jj, kk = j[live], k[live]
        assert jj.min() >= base and jj.max() < E, "an output reads outside the two spans"
        if reads is not None:
            reads["min"], reads["max"] = min(reads.get("min", E), int(jj.min())), max(reads.get("max", -1), int(jj.max()))
        acc[..., live] = _fma32(src[..., jj - base], flt.taps[kk], acc[..., live])
        j = j - 1
    return acc


def resample_whole(x48, rate):
    """The whole stream at `rate`: float32 [resample_out_len(T48, rate, 48000)]."""
    x48 = np.asarray(x48, dtype=F32).reshape(-1)
    flt = ResampleFilter(rate)
    return resample_span(flt, x48, 0, x48.size, 0, flt.n_final(x48.size, True)) if x48.size else np.zeros(0, F32)


# ---- limiter ---------------------------------------------------------------------------------------------------------------
def envelope_span(src, base, E, lo, hi, ended):
    """m[lo .. hi) of a stream from src = its samples [base, E), one row or rows [C, n]: truepeak.envelope's values (the
    maximum over the rows of a row's own), every sum in float64 in ascending tap order whatever the span; zeros before sample 0,
    and past E (read only when the stream ends there)."""
    src = np.asarray(src, dtype=F32)
    HALF, FACTOR = _truepeak.HALF, _truepeak.FACTOR
    h = _truepeak.taps().astype(np.float64)
    n = hi - lo
    assert lo >= 0 and (ended or hi + HALF <= E) and (lo - HALF >= base or base == 0)
    pad = np.zeros(src.shape[:-1] + (n + 2 * HALF,), dtype=np.float64)   # x[lo - HALF .. hi + HALF)
    a, b = max(lo - HALF, base, 0), min(hi + HALF, E)
    pad[..., a - (lo - HALF):b - (lo - HALF)] = src[..., a - base:b - base]
    best = np.abs(pad[..., HALF:HALF + n])
    for p in range(FACTOR):
        acc = np.zeros(best.shape)
        for i in range(2 * HALF + 1):
            if p + FACTOR * i < h.size:
                acc += h[p + FACTOR * i] * pad[..., 2 * HALF - i:2 * HALF - i + n]          # x[n + 10 - i]
        best = np.maximum(best, np.abs(acc))
    best = best.astype(F32)
    return best.max(0) if src.ndim == 2 else best


def limit_span(src, base, E, first, n_out, ended, H, true_peak_db):
    """The limiter's outputs [first, first + n_out) from src = the samples [base, E), one row or rows [C, n] under one gain."""
    src = np.asarray(src, dtype=F32)
    if n_out == 0:
        return np.zeros(src.shape[:-1] + (0,), F32)
    a, b = first, first + n_out
    lo, hi = max(0, a - 2 * H), (min(b + 2 * H, E) if ended else b + 2 * H)
    assert ended or hi + _truepeak.HALF <= E
    m = envelope_span(src, base, E, lo, hi, ended)
    # limiter_gain's own ends (r = 1 outside, q extended by H) fall on the stream's ends or outside what [a, b) reads
    g = _truepeak.limiter_gain(m, H, true_peak_db)[0][a - lo:b - lo]
    c32 = F32(_truepeak.ceiling(true_peak_db))
    return np.clip((src[..., a - base:b - base] * g).astype(F32), -c32, c32)


# ---- the chain -------------------------------------------------------------------------------------------------------------
MAX_CHANNELS = 8


def make_plan(rate=None, true_peak=None, pcm=None, key=None, channels=None, interleaved=False, meter=False):
    """The stages of a delivery, as delivery_stream.resolve gives them: rate None | R, true_peak None | the ceiling in dBTP
    (limiter='lookahead'), pcm None | 'int16' | 's24' | 's24in32', key None | the dither's (seed, stream); channels None (one mono stream: the plan
    it always was) | C rows that move together, 1 .. 8; interleaved: the encoder's output as sample frames [n, C]; meter: the stream
    owns a loudness meter (meter.py) fed the float32 samples it makes final, in front of the encoder: no stage, and the plan's
    key "meter" only when it is set."""
    if pcm is not None and pcm not in _pcm.FORMATS:
        raise ValueError(f"pcm must be None or one of {_pcm.FORMATS}, got {pcm!r}")
    plan = dict(rate=rate, true_peak=true_peak, pcm=pcm, key=key)
    if meter not in (False, True):
        raise ValueError(f"meter must be a bool, got {meter!r}")
    if meter:
        plan["meter"] = True
    if channels is None:
        if interleaved:
            raise ValueError("interleaved goes with channels: a mono stream has nothing to interleave")
        return plan
    if isinstance(channels, (bool, float)) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels must be None or an int 1 .. {MAX_CHANNELS}, got {channels!r}")
    if interleaved and pcm is None:
        raise ValueError("interleaved is the int16 encoder's layout: it goes with pcm")
    plan.update(channels=int(channels), interleaved=bool(interleaved))
    return plan


def _rows(x48, plan):
    """x48 [T] or [C, T] -> (float32 [C, T], whether it came as [T]), checked against the plan's channels."""
    x = np.asarray(x48, dtype=F32)
    flat = x.ndim == 1
    x = x[None] if flat else x
    if x.ndim != 2 or not 1 <= x.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"a stream is [T] or [C, T] with 1 <= C <= {MAX_CHANNELS}, got shape {np.shape(x48)}")
    C = plan.get("channels")
    if C is not None and x.shape[0] != C:
        raise ValueError(f"the plan's channels {C!r} and a stream of shape {np.shape(x48)}")
    return x, flat


def chunked(x48, cuts, plan, stats=None, first=0):
    """x48 float32 [T48] or [C, T48] pushed in the blocks x48[..., c_{k-1}:c_k] for c in cuts (ascending, the last one T48), then
    flushed -> the concatenated delivery: [n] for [T48], else [C, n], or [n, C] from an interleaved plan.  first: the encoder's
    first absolute index.
    stats: a dict that gets the largest carries ('resample_carry', 'limit_carry'), the resampler's read range per push
    ('reads': [(E, min, max)]) and the blocks' lengths ('lens')."""
    x48, flat = _rows(x48, plan)
    C, T = x48.shape
    cuts = [int(c) for c in cuts]
    assert cuts == sorted(cuts) and (not cuts or cuts[-1] == T)
    rate, tp, key = plan["rate"], plan["true_peak"], plan["key"]
    flt = ResampleFilter(rate) if rate is not None else None
    H = _truepeak.half_window(rate or 48000) if tp is not None else None
    rs, ls, es = (ResampleStage(flt) if flt else None), (LimitStage(H) if tp is not None else None), EncodeStage(first)
    carry_r, carry_l = np.zeros((C, 0), F32), np.zeros((C, 0), F32)
    stats = {} if stats is None else stats
    stats.update(resample_carry=0, limit_carry=0, reads=[], lens=[])
    out, prev = [], 0
    for c, ended in [(c, False) for c in cuts] + [(T, True)]:
        block, prev = x48[:, prev:c], c
        if rs is not None:
            job = rs.step(block.shape[1], ended)                  # (one set of counters for all the rows)
            src = np.concatenate([carry_r, block], 1)
            reads = {}
            block = resample_span(flt, src, job["base"], job["base"] + src.shape[1], job["first"], job["n_out"], reads)
            if reads:
                stats["reads"].append((job["base"] + src.shape[1], reads["min"], reads["max"]))
            carry_r = src[:, src.shape[1] - job["n_keep"]:]
            stats["resample_carry"] = max(stats["resample_carry"], carry_r.shape[1])
        if ls is not None:
            job = ls.step(block.shape[1], ended)
            src = np.concatenate([carry_l, block], 1)
            block = limit_span(src, job["base"], job["base"] + src.shape[1], job["first"], job["n_out"], ended, H, tp)
            carry_l = src[:, src.shape[1] - job["n_keep"]:]
            stats["limit_carry"] = max(stats["limit_carry"], carry_l.shape[1])
        if plan["pcm"] is not None:
            job = es.step(block.shape[1], ended)
            d = None
            if key is not None:
                d = np.stack([_pcm.tpdf_dither(key[0], key[1], ch, block.shape[1], first=job["first"]) for ch in range(C)])
            block = _pcm.encoder(plan["pcm"])[0](block, d)                  # ('s24': [C, n, 3])
        stats["lens"].append(block.shape[1])
        out.append(block)
    y = np.concatenate(out, 1)
    if flat:
        return y[0]
    return np.ascontiguousarray(np.swapaxes(y, 0, 1)) if plan.get("interleaved") else y


def whole(x48, plan):
    """The one-shot delivery of the whole stream at level='input': what `chunked` has to give."""
    x48, flat = _rows(x48, plan)
    y = x48
    if plan["rate"] is not None:
        y = np.stack([resample_whole(row, plan["rate"]) for row in y])
    if plan["true_peak"] is not None:
        y = _truepeak.limit(y, plan["rate"] or 48000, plan["true_peak"])[0] if y.shape[1] else y
    if plan["pcm"] is not None:
        y = _pcm.encoder(plan["pcm"])[1](y, plan["key"], bool(plan.get("interleaved")) and not flat)
    return y[0] if flat else y
