"""CPU: true peak and the look-ahead limiter as flowhigh_amd/truepeak.py defines them -- the oversampling against scipy, the meter
on tones, the limiter's guarantees on random clips and at its edges -- the keywords' resolution and errors, the entries of
csrc/truepeak.hip in header / EXPORTS / _SIGS and their argument checks, and the batching server with a stub model.

Bars.  Oversampling: 2^-24 * 2.2415 * peak against scipy.signal.resample_poly on float64 -- the two differ only in the rounding of
the taps to float32 (relative 2^-24 each), and 2.2415 is the largest per-phase sum |h|.  Tones: +-0.05 dB (measured +0.016 / -0.038).
Limiter: g <= r everywhere and max |y| <= c32 exactly (both follow from the definition); the re-measured true peak of the result at
most 1.001 c (the look-ahead holds the gain at or under c / m over every oversampled sample's 21 input samples only on the Hann
window's average: the prototype measured 1.00005, the bar is 20 times that excess; a broken look-ahead overshoots by whole dB)."""
import ctypes
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.signal
import torch

from flowhigh_amd import delivery, hip, loudness, truepeak
from flowhigh_amd.flowhighsr import FlowHighSR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"fh_tp_tile_len": 0, "fh_true_peak_f32": 6, "fh_true_peak_seg_f32": 8, "fh_tp_envelope_f32": 7, "fh_tp_envelope_seg_f32": 6,
           "fh_limit_f32": 11, "fh_limit_seg_f32": 9, "fh_delivery_gain_f32": 12}
SUM_ABS_H = 2.2415
f32 = np.float32


# ---- the meter ------------------------------------------------------------------------------------------------------------------
def test_the_taps_are_scipy_s_and_their_phase_sums():
    h = truepeak.taps()
    want = scipy.signal.firwin(81, 0.25, window=("kaiser", 5.0)) * 4
    assert h.dtype == np.float32 and h.shape == (81,) and np.abs(h - want).max() <= 2.0 ** -24 * np.abs(want).max()
    sums = [float(np.abs(h[p::4].astype(np.float64)).sum()) for p in range(4)]
    assert [len(h[p::4]) for p in range(4)] == [21, 20, 20, 20]
    assert max(sums) <= SUM_ABS_H and max(sums) > SUM_ABS_H - 1e-3, sums
    assert h[40] != 1.0 or np.abs(h[0::4]).sum() != 1.0            # phase 0 is not the identity: the envelope keeps |x[n]| itself


def test_oversampling_is_scipy_s_resample_poly():
    rng = np.random.default_rng(3)
    worst = 0.0
    for T in (1, 2, 9, 10, 11, 21, 100, 1027):
        x = (rng.standard_normal((2, T)) * 0.3).astype(np.float32)
        got = truepeak.oversample(x)
        want = scipy.signal.resample_poly(x.astype(np.float64), 4, 1, axis=-1)
        assert got.shape == want.shape == (2, 4 * T) and got.dtype == np.float64
        bar = 2.0 ** -24 * SUM_ABS_H * float(np.abs(x).max())
        worst = max(worst, float(np.abs(got - want).max()) / bar)
        assert np.abs(got - want).max() <= bar, T
    print(f"truepeak: oversampling against scipy: worst error / bar {worst:.3f}")
    # the sum as the kernels take it: x4[4 n + p] = sum_i h[p + 4 i] x[n + 10 - i]
    x = (rng.standard_normal(50) * 0.3).astype(np.float64)
    h = truepeak.taps().astype(np.float64)
    xp = np.concatenate([np.zeros(10), x, np.zeros(10)])
    for n, p in ((0, 0), (0, 3), (7, 1), (49, 2), (49, 0)):
        s = sum(h[p + 4 * i] * xp[n + 10 - i + 10] for i in range(21 if p == 0 else 20))
        assert abs(s - truepeak.oversample(x)[4 * n + p]) <= 1e-15


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_tones_read_within_a_twentieth_of_a_db(rate):
    """Tones sin(2 pi f t) of true peak 1 at 0.02, 0.125, 0.25 and 0.45 of the rate, read away from the clip's ends, and the tone at
    a quarter of the rate with its phase at 45 degrees, whose samples sit at 0.707 of the crest: +-0.05 dB.
    What is printed and not asserted: the worst reading over a sweep of 16 phases.  A factor-4 meter under-reads a crest that falls
    between its points by up to cos(pi f / (4 fs)) (-0.17 dB at fs / 4; measured -0.126 at 1 rad), and this filter is 0.66 dB down
    at 0.45 fs, where the reading rests on the samples themselves (measured -0.102 at 45 degrees): both belong to the factor and
    the filter the definition states, not to its arithmetic."""
    T = 2000
    t = np.arange(T) / rate
    lo, hi, sweep = 0.0, 0.0, 0.0
    for f in (0.02, 0.125, 0.25, 0.45):
        for phase in [0.0] + ([math.pi / 4] if f == 0.25 else []):
            x = np.sin(2 * np.pi * (f * rate) * t + phase).astype(np.float32)
            m = truepeak.envelope(x)[100:-100]
            db = float(truepeak.dbtp(m.max()))
            lo, hi = min(lo, db), max(hi, db)
            assert abs(db) <= 0.05, (rate, f, phase, db)
        for k in range(16):
            x = np.sin(2 * np.pi * (f * rate) * t + k * math.pi / 16).astype(np.float32)
            sweep = min(sweep, float(truepeak.dbtp(truepeak.envelope(x)[100:-100].max())))
    print(f"truepeak: tones at {rate} Hz read within {hi:+.3f} / {lo:+.3f} dB; worst over 16 phases {sweep:+.3f} dB")
    n = np.arange(T)
    # the issue's example: fs / 4 at 45 degrees has its samples at 0.707 of the crest
    x = np.sin(2 * np.pi * 0.25 * n + math.pi / 4).astype(np.float32)
    assert abs(float(np.abs(x).max()) - 0.7071) < 1e-3 and abs(float(truepeak.envelope(x)[100:-100].max()) - 1.0017) < 2e-4
    assert truepeak.dbtp(0.0) == -math.inf and truepeak.true_peak(np.zeros((2, 40), dtype=np.float32)) == 0
    assert truepeak.dbtp(1.0) == 0 and truepeak.dbtp(0.5).dtype == np.float32


def test_the_envelope_is_joint_over_the_channels_and_holds_the_samples():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((3, 300)) * 0.2).astype(np.float32)
    m = truepeak.envelope(x)
    each = np.stack([truepeak.envelope(x[c]) for c in range(3)])
    assert m.dtype == np.float32 and np.array_equal(m, each.max(0)) and (m >= np.abs(x).max(0)).all()
    assert truepeak.true_peak(x) == m.max() and truepeak.envelope(x[0]).shape == (300,)


# ---- the limiter ----------------------------------------------------------------------------------------------------------------
def random_case(seed):
    rng = np.random.default_rng(seed)
    C, T = int(rng.integers(1, 4)), int(rng.integers(1, 3001))
    rate = [8000, 16000, 44100, 48000][seed % 4]
    ceiling = -float(rng.uniform(0.0, 6.0))
    x = (rng.standard_normal((C, T)) * 0.3).astype(np.float32)
    x[rng.integers(0, C), rng.integers(0, T)] = 5.0
    return x, rate, ceiling


def test_the_limiter_on_40_random_clips():
    worst = 0.0
    for seed in range(40):
        x, rate, ceiling = random_case(seed)
        y, g, m = truepeak.limit(x, rate, ceiling)
        r = truepeak.reduction(m, ceiling)
        c32 = f32(truepeak.ceiling(ceiling))
        assert y.dtype == g.dtype == np.float32 and y.shape == x.shape and g.shape == (x.shape[1],)
        assert (g <= r).all() and (g > 0).all(), seed
        assert float(np.abs(y).max()) <= float(c32), seed
        again = float(truepeak.true_peak(y)) / truepeak.ceiling(ceiling)
        worst = max(worst, again)
        assert again <= 1.001, (seed, again)
    print(f"truepeak: limiter on 40 random clips: worst re-measured true peak / ceiling {worst:.6f} ({20 * math.log10(worst):+.4f} dB)")


@pytest.mark.parametrize("rate", [8000, 48000])
def test_the_limiter_at_its_edges(rate):
    H = truepeak.half_window(rate)
    rng = np.random.default_rng(rate)
    for T in (1, 2, H, 2 * H + 1, 4 * H + 7):
        for at in sorted({0, T - 1}):
            x = (rng.standard_normal((2, T)) * 0.05).astype(np.float32)
            x[1, at] = 3.0
            y, g, m = truepeak.limit(x, rate, -1.0)
            r = truepeak.reduction(m, -1.0)
            c32 = f32(truepeak.ceiling(-1.0))
            assert (g <= r).all() and float(np.abs(y).max()) <= float(c32), (T, at)
            assert float(truepeak.true_peak(y)) <= 1.001 * truepeak.ceiling(-1.0), (T, at)
            assert abs(float(y[1, at])) >= 0.99 * float(c32) * min(1.0, 3.0 / float(m[at])), (T, at)      # held at the ceiling, not crushed
    # a clip already under the ceiling comes back bit for bit
    x = (rng.standard_normal((2, 3 * H)) * 0.05).astype(np.float32)
    y, g, m = truepeak.limit(x, rate, -1.0)
    assert float(m.max()) < truepeak.ceiling(-1.0) and (g == 1).all() and np.array_equal(y, x)
    # far from a peak the gain is 1, and the window's weights are what the definition says
    x = np.zeros((1, 6 * H + 1), dtype=np.float32)
    x[0, 3 * H] = 2.0
    _, g, m = truepeak.limit(x, rate, 0.0)
    assert g[3 * H] == g.min() and (g[:3 * H - 2 * H - 10] == 1).all() and (g[3 * H + 2 * H + 11:] == 1).all()
    w = truepeak.window(H)
    assert w.shape == (2 * H + 1,) and abs(w.sum() - 1) < 1e-15 and np.array_equal(w, w[::-1]) and w.min() > 0


def test_half_windows_and_their_limits():
    assert [truepeak.half_window(r) for r in (48000, 44100, 8000, 16000, 96000, 102400, 100)] == [240, 221, 40, 80, 480, 512, 1]
    with pytest.raises(ValueError, match="512"):
        truepeak.half_window(102500)
    with pytest.raises(ValueError, match="512"):
        truepeak.half_window(192000)
    for bad in (99, 0, -8000, 44100.5, "48000", True):
        with pytest.raises(ValueError):
            truepeak.half_window(bad)


def test_the_static_rule_and_the_delivery_as_a_whole():
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((2, 30000)) * 0.1).astype(np.float32)
    x *= f32(0.99) / np.abs(x).max()
    tp = truepeak.true_peak(x)
    g = truepeak.static_gain(tp, -1.0)
    assert g.dtype == np.float32 and g == f32(min(1.0, truepeak.ceiling(-1.0) / float(tp))) and g < 1
    y = truepeak.deliver(x, 48000, -1.0)
    assert np.array_equal(y, (x * g).astype(np.float32)) and float(truepeak.dbtp(truepeak.true_peak(y))) <= -1.0 + 1e-4
    assert truepeak.static_gain(0.0, -1.0) == 1 and truepeak.static_gain(0.0, -1.0, 0.25) == f32(0.25)
    assert truepeak.static_gain(0.05, -1.0) == 1                     # it only attenuates
    # with loudness=: the capped gain of loudness= alone, then the ceiling
    L = loudness.integrated(x, 48000)
    g_l = loudness.gain(L, -30.0, float(np.abs(x).max()))
    assert np.array_equal(truepeak.deliver(x, 48000, -1.0, loudness=-30.0), (x * f32(min(float(g_l), truepeak.ceiling(-1.0) / float(tp)))).astype(np.float32))
    # with the limiter the loudness gain is not capped: a target the cap keeps 6 dB away is reached within the limiter's toll
    target = float(L) + 6.0
    capped = loudness.integrated(loudness.normalise(x, 48000, target)[0], 48000)
    y = truepeak.deliver(x, 48000, -1.0, limiter="lookahead", loudness=target)
    got = loudness.integrated(y, 48000)
    assert truepeak.uncapped_gain(L, target) == f32(10.0 ** ((target - float(f32(L))) / 20.0))
    assert capped < target - 5.0 and abs(got - target) < abs(capped - target) and got <= target + 1e-6
    assert float(np.abs(y).max()) <= float(f32(truepeak.ceiling(-1.0))) and float(truepeak.true_peak(y)) <= 1.001 * truepeak.ceiling(-1.0)
    assert truepeak.uncapped_gain(-math.inf, -16.0) == 1 and truepeak.uncapped_gain(-20.0, None) == 1


# ---- the keywords ---------------------------------------------------------------------------------------------------------------
def test_resolve_true_peak_and_its_errors():
    r = truepeak.resolve_true_peak
    assert r(None, None) == (None, None) and r(-1, None) == (-1.0, None) and r(np.float32(-2.5), "lookahead") == (-2.5, "lookahead")
    assert r(0, None) == (0.0, None) and r(-20.0, "lookahead", 48000) == (-20.0, "lookahead") and isinstance(r(-1, None)[0], float)
    for bad in (0.5, -20.5, math.nan, math.inf, "-1", True, [-1.0]):
        with pytest.raises(ValueError, match="true_peak must be"):
            r(bad, None)
    with pytest.raises(ValueError, match="limiter must be"):
        r(-1.0, "brickwall")
    with pytest.raises(ValueError, match="goes with true_peak"):
        r(None, "lookahead")
    with pytest.raises(ValueError, match="512"):
        r(-1.0, "lookahead", 192000)
    assert r(-1.0, None, 192000) == (-1.0, None)                     # the static rule has no window


def test_resolve_delivery_takes_the_keywords_and_leaves_the_other_results_as_they_were():
    rd = delivery.resolve_delivery
    assert rd(3) is None and rd(3, true_peak=None, limiter=None) is None
    assert rd(2, 44100) == dict(rate=44100, pcm=None, keys=None, interleaved=False)
    assert rd(2, loudness=-16) == dict(rate=None, pcm=None, keys=None, interleaved=False, loudness=-16.0)
    assert rd(2, None, "int16", "tpdf", 7, True) == dict(rate=None, pcm="int16", keys=[(7, 0), (7, 1)], interleaved=True)
    assert rd(2, true_peak=-1) == dict(rate=None, pcm=None, keys=None, interleaved=False, true_peak=-1.0, limiter=None)
    assert rd(2, 44100, "int16", loudness=-16, true_peak=-1, limiter="lookahead") == dict(
        rate=44100, pcm="int16", keys=None, interleaved=False, loudness=-16.0, true_peak=-1.0, limiter="lookahead")
    assert rd(1, true_peak=-1.0, level="input")["true_peak"] == -1.0          # the rule only attenuates
    with pytest.raises(ValueError, match="goes with true_peak"):
        rd(1, limiter="lookahead")
    with pytest.raises(ValueError, match="true_peak must be"):
        rd(1, true_peak=3)
    with pytest.raises(ValueError, match="512"):
        rd(1, 192000, true_peak=-1, limiter="lookahead")
    assert rd(1, 96000, true_peak=-1, limiter="lookahead")["rate"] == 96000
    with pytest.raises(ValueError, match="two rules for one gain"):
        rd(1, loudness=-16.0, true_peak=-1.0, level="input")


def test_the_public_entries_have_the_keywords_and_refuse_before_any_gpu_work():
    from flowhigh_amd.serve import BatchingServer
    for fn in (FlowHighSR.generate, FlowHighSR.generate_batch, FlowHighSR.generate_many, BatchingServer.submit, BatchingServer.generate):
        for name in ("true_peak", "limiter"):
            p = inspect.signature(fn).parameters[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, (fn, name)
    for fn in (FlowHighSR.generate_from_device, FlowHighSR.capture, FlowHighSR.sample, FlowHighSR.sample_many):
        assert not {"true_peak", "limiter"} & set(inspect.signature(fn).parameters), fn
    assert list(inspect.signature(FlowHighSR.measure_true_peak).parameters) == ["self", "rows", "chans", "rate"]
    assert inspect.signature(FlowHighSR.measure_true_peak).parameters["rate"].default == 48000
    m = FlowHighSR.__new__(FlowHighSR)                               # no device, no library: anything past the checks would raise
    m.flowhigh = type("F", (), {"device": torch.device("cpu")})()
    m.prior = "reference"
    x = np.linspace(-0.5, 0.5, 50, dtype=np.float32)
    for kw, say in ((dict(true_peak=1.0), "true_peak must be"), (dict(true_peak=-21), "true_peak must be"),
                    (dict(true_peak=math.nan), "true_peak must be"), (dict(limiter="lookahead"), "goes with true_peak"),
                    (dict(true_peak=-1.0, limiter="soft"), "limiter must be"),
                    (dict(true_peak=-1.0, limiter="lookahead", output_rate=192000), "512"),
                    (dict(true_peak=-1.0, dither="tpdf"), "goes with pcm")):
        with pytest.raises(ValueError, match=say):
            m.generate(x, 12000, **kw)
        with pytest.raises(ValueError, match=say):
            m.generate_batch([x, x], 12000, **kw)
        with pytest.raises(ValueError, match=say):
            m.generate_many([x, x[:40]], 12000, **kw)
    with pytest.raises(ValueError, match="return_stages"):
        m.generate_batch([x], 12000, true_peak=-1.0, return_stages=True)


# ---- the library ----------------------------------------------------------------------------------------------------------------
def test_header_exports_and_abi_are_consistent():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    for name, n_params in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/flowhigh_hip.h"
        params = [p.strip() for p in m.group(1).split(",") if p.strip() != "void"]
        assert name in hip.EXPORTS and len(hip._SIGS[name]) == len(params) == n_params, name
        for p, ctype in zip(params, hip._SIGS[name]):
            want = hip._P if "*" in p else (hip._D if p.startswith("double") else (hip._F if p.startswith("float") else hip._I))
            assert ctype is want, (name, p)
    build = __import__("flowhigh_amd.build", fromlist=["SOURCES"])
    assert "truepeak.hip" in build.SOURCES
    text = (ROOT / "flowhigh_amd" / "csrc" / "truepeak.hip").read_text()            # (its constants are truepeak_common.h's, stated once)
    assert '#include "truepeak_common.h"' in text and "MAX_H =" not in text and "HALO =" not in text
    text = (ROOT / "flowhigh_amd" / "csrc" / "truepeak_common.h").read_text()
    assert f"MAX_H = {truepeak.MAX_H};" in text and f"HALO = {truepeak.HALF};" in text


def test_the_entries_check_their_arguments():
    """The checks run on the host before anything is launched: the device pointers are fake addresses, never read."""
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    A, B, E, K, W = 256, 512, 1024, 2048, 4096
    assert L.fh_tp_tile_len() == 1024
    bad = [("fh_true_peak_f32", a) for a in ((0, K, E, 1, 8), (A, 0, E, 1, 8), (A, K, 0, 1, 8), (A, K, E, 0, 8), (A, K, E, 65536, 8),
                                             (A, K, E, 1, 0), (A, K, E, 1, 2 ** 30 + 1), (A + 2, K, E, 1, 8), (A, K, E + 1, 1, 8))]
    bad += [("fh_true_peak_seg_f32", a) for a in ((0, B, 1, 1, 8, K, E), (A, 0, 1, 1, 8, K, E), (A, B, 0, 1, 8, K, E), (A, B, 2, 1, 8, K, E),
                                                 (A, B, 1, 65536, 8, K, E), (A, B, 1, 1, 0, K, E), (A, B, 1, 1, 8, 0, E), (A, B, 1, 1, 8, K, 0))]
    bad += [("fh_tp_envelope_f32", a) for a in ((0, K, E, 1, 1, 8), (A, 0, E, 1, 1, 8), (A, K, 0, 1, 1, 8), (A, K, E, 0, 1, 8),
                                               (A, K, E, 1, 0, 8), (A, K, E, 1, 9, 8), (A, K, E, 1, 1, 0), (A, K, E, 1, 1, -5))]
    bad += [("fh_tp_envelope_seg_f32", a) for a in ((0, 1, 8, K, E), (A, 0, 8, K, E), (A, 65536, 8, K, E), (A, 1, 0, K, E), (A, 1, 8, 0, E),
                                                   (A, 1, 8, K, 0))]
    good = (A, A, E, W, 0, 1, 2, 8, 240, 0.9)
    for i, v in ((0, 0), (1, 0), (2, 0), (3, 0), (5, 0), (5, 65536), (6, 0), (6, 9), (7, 0), (7, 2 ** 30 + 1), (8, 0), (8, 513), (9, 0.0),
                 (9, 1.5), (9, math.nan), (3, W + 4), (2, E + 2)):
        args = list(good)
        args[i] = v
        bad.append(("fh_limit_f32", tuple(args)))
    good = (A, 1, 8, E, W, 0, 240, 0.9)
    for i, v in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (6, 0), (6, 513), (7, 0.0), (7, 1.0001)):
        args = list(good)
        args[i] = v
        bad.append(("fh_limit_seg_f32", tuple(args)))
    good = (A, -16.0, B, E, K, 2, 1, 0.9, 0, W, 0)
    for i, v in ((4, 0), (5, 0), (6, 0), (6, 3), (5, 65536), (1, 1.0), (1, -71.0), (0, 0), (2, 0), (7, 0.0), (7, 1.5), (9, 0)):
        args = list(good)
        args[i] = v
        bad.append(("fh_delivery_gain_f32", tuple(args)))
    for name, args in bad:
        assert getattr(L, name)(*args, 0) == -1, (name, args)
        assert name.encode() in L.fh_last_error(), (name, args)


# ---- the serving front ----------------------------------------------------------------------------------------------------------
class _Stub:
    """A model whose generate_many has no true_peak keyword unless it is handed one: records what it was called with."""

    def __init__(self):
        self.calls = []

    def generate_many(self, clips, sr, target, steps, noise=None, max_batch=64, **kw):
        self.calls.append(dict(n=len(clips), **kw))
        return [torch.from_numpy(np.repeat(np.asarray(c, dtype=np.float32).reshape(1, -1), 4, axis=1)) for c in clips]


def test_batching_server_groups_by_the_keywords_and_hands_them_on_only_when_given():
    from flowhigh_amd.serve import BatchingServer
    m = _Stub()
    mono = np.linspace(-1, 1, 100, dtype=np.float32)
    srv = BatchingServer(m, max_batch=8, max_wait_ms=30000)
    try:
        futs = [srv.submit(mono, 12000, true_peak=-1.0), srv.submit(mono[:60], 12000, true_peak=-1.0, limiter="lookahead"),
                srv.submit(mono, 12000), srv.submit(mono[:70], 12000, true_peak=-1), srv.submit(mono, 12000, true_peak=None),
                srv.submit(mono, 12000, true_peak=-2.0), srv.submit(mono, 12000, loudness=-16.0, true_peak=-1.0, limiter="lookahead"),
                srv.submit(mono[:50], 12000, true_peak=-1.0, limiter="lookahead")]
        got = [f.result(timeout=30) for f in futs]
        assert all(g.dtype == np.float32 for g in got)
        calls = sorted(((c["n"], c.get("loudness"), c.get("true_peak"), c.get("limiter")) for c in m.calls), key=str)
        assert calls == sorted([(2, None, -1.0, None), (2, None, -1.0, "lookahead"), (2, None, None, None), (1, None, -2.0, None),
                                (1, -16.0, -1.0, "lookahead")], key=str)
        assert all((k in c) == (c.get(k) is not None) for c in m.calls for k in ("true_peak", "limiter", "loudness"))      # never passed as None
        for kw in (dict(true_peak=1.0), dict(true_peak="x"), dict(limiter="lookahead"), dict(true_peak=-1.0, limiter="x")):
            with pytest.raises(ValueError):
                srv.submit(mono, 12000, **kw)
    finally:
        srv.close()
    one = BatchingServer(m, max_batch=2, max_wait_ms=5)
    try:
        n = len(m.calls)
        sr, y = one.generate((12000, mono), 48000, 1, true_peak=-1.0, limiter="lookahead")
        assert sr == 48000 and y.shape == (400,) and m.calls[n] == dict(n=1, true_peak=-1.0, limiter="lookahead")
        one.generate((12000, mono), 48000, 1)
        assert m.calls[n + 1] == dict(n=1)
    finally:
        one.close()
