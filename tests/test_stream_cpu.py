"""CPU: the definition of streaming sessions (flowhigh_amd/stream.py) -- the grain and the plan's conditions, the windows of a
stream and what has been emitted after each, the ramp, the seam and stitch -- the host prior's first_frame=, and the two new
entries' declarations.  No GPU, no library."""
import re
from pathlib import Path

import numpy as np
import pytest

from flowhigh_amd import hip, tables
from flowhigh_amd import stream as S
from flowhigh_amd.prior import philox4x32_10, prior_normal_host

F32 = np.float32
RATES = {8000: 10, 12000: 10, 16000: 10, 24000: 10, 32000: 10, 44100: 10, 48000: 10, 22050: 20, 11025: 40}
# (sr, window, overlap, guard): the GPU tests' plan, the defaults, no guard, and a rate whose grain is 40 ms
PLANS = [(12000, 200, 60, 10), (12000, 1000, 200, 50), (12000, 200, 60, 0), (11025, 1000, 200, 40)]


def test_grain_at_the_nine_rates():
    for sr, g in RATES.items():
        assert S.grain_ms(sr) == g, sr
        assert (g * sr) % 1000 == 0 and all((k * sr) % 1000 for k in range(10, g, 10))          # the smallest such multiple of 10 ms
    with pytest.raises(ValueError):
        S.grain_ms(0)


@pytest.mark.parametrize("sr,kw,word", [
    (12000, dict(window_ms=1005), "10 ms grain"),                # not a multiple of the grain, each of the three lengths
    (12000, dict(overlap_ms=205), "10 ms grain"),
    (12000, dict(guard_ms=5), "10 ms grain"),
    (22050, dict(window_ms=1010), "20 ms grain"),                # 10 ms is no whole number of samples at 22 050 Hz
    (11025, dict(overlap_ms=220), "40 ms grain"),
    (11025, dict(guard_ms=50), "40 ms grain"),
    (12000, dict(window_ms=1000.0), "grain"),                    # lengths are integers
    (12000, dict(guard_ms=-10), "grain"),
    (12000, dict(overlap_ms=10, guard_ms=0), "under 20 ms"),     # overlap >= 20 ms
    (12000, dict(window_ms=300, overlap_ms=160), "exceeds window_ms"),      # 2 * overlap <= window
    (12000, dict(overlap_ms=100, guard_ms=50), "nothing"),       # 2 * guard < overlap
    (12000, dict(overlap_ms=20, guard_ms=10), "nothing"),
])
def test_plan_conditions(sr, kw, word):
    with pytest.raises(ValueError, match=word):
        S.StreamPlan(sr, **kw)


def test_plan_lengths():
    p = S.StreamPlan(12000)                                          # the defaults
    assert (p.window_ms, p.overlap_ms, p.guard_ms) == (1000, 200, 50)
    assert (p.W, p.O, p.H, p.W48, p.O48, p.H48, p.G48) == (12000, 2400, 9600, 48000, 9600, 38400, 2400)
    assert p.hop_frames == 80 and p.window_frames == 100 and [p.first_frame(i) for i in range(3)] == [0, 80, 160]
    q = S.StreamPlan(11025, 1000, 200, 40)
    assert (q.W, q.O, q.H, q.H48) == (11025, 2205, 8820, 38400) and q.H48 % 480 == 0
    S.StreamPlan(12000, 400, 200, 0)                                 # 2 * overlap == window is allowed
    S.StreamPlan(12000, 40, 20, 0)                                   # the smallest overlap
    assert p.key != q.key and p.key == S.StreamPlan(12000).key


@pytest.mark.parametrize("sr,window,overlap,guard", [(12000, 200, 60, 10), (11025, 200, 80, 0), (12000, 1000, 200, 50)])
def test_windows_spans_and_the_emission_schedule(sr, window, overlap, guard):
    p = S.StreamPlan(sr, window, overlap, guard)
    W, O, H = p.W, p.O, p.H
    want_n = {1: 1, O + 1: 1, W - 1: 1, W: 1, W + 1: 2, W + H: 2, W + H + 1: 3}
    for T, n in want_n.items():
        assert p.n_windows(T) == n, T
        spans = p.spans(T)
        assert len(spans) == n and spans[0][0] == 0 and spans[-1][1] == T
        for i, (a, b) in enumerate(spans):
            assert a == i * H and b == min(i * H + W, T)
            assert b - a == W or i == n - 1
            if i:
                assert b - a > O                                      # the last window is longer than the overlap
        # a window may run once its last sample is there: before a flush, the full ones
        assert p.runnable(T) == sum(1 for a, b in spans if b - a == W)
        # after window i: (i + 1) H48 samples; after the last one: all of them
        T48 = tables.resample_out_len(T, 48000, sr)
        assert p.out_len(T) == T48
        for i in range(n - 1):
            assert p.emitted(i, T) == (i + 1) * p.H48
        assert p.emitted(n - 1, T) == T48
        # the windows' final regions tile [0, T48): no gap, no double count
        regions = p.final_regions(T)
        assert regions[0][0] == 0 and regions[-1][1] == T48
        assert all(r0[1] == r1[0] for r0, r1 in zip(regions, regions[1:])) and all(b > a for a, b in regions)
        # and window i's region lies inside what window i computed
        for i, (a, b) in enumerate(regions):
            assert i * p.H48 <= a and b <= i * p.H48 + tables.resample_out_len(spans[i][1] - spans[i][0], 48000, sr)
    with pytest.raises(ValueError):
        p.n_windows(0)
    assert p.runnable(W - 1) == 0 and p.runnable(W + H - 1) == 1 and p.runnable(W + 2 * H) == 3


@pytest.mark.parametrize("sr,window,overlap,guard", PLANS)
def test_ramp(sr, window, overlap, guard):
    p = S.StreamPlan(sr, window, overlap, guard)
    w_in, w_out = p.ramp()
    o, g = p.O48, p.G48
    assert w_in.dtype == F32 and w_out.dtype == F32 and w_in.shape == w_out.shape == (o,)
    # exact 0 and 1 in the guards, and nowhere else
    assert (w_in[:g] == 0).all() and (w_out[:g] == 1).all() and (w_in[o - g:] == 1).all() and (w_out[o - g:] == 0).all()
    assert (w_in[g:] > 0).all() and (w_out[:o - g] > 0).all()
    assert (np.diff(w_in.astype(np.float64)) >= 0).all() and (np.diff(w_out.astype(np.float64)) <= 0).all()
    assert np.abs(w_in.astype(np.float64) + w_out.astype(np.float64) - 1.0).max() <= 2.0 ** -24
    assert np.array_equal(w_in.view(np.uint32), w_out[::-1].view(np.uint32))            # w_in[u] == w_out[O48 - 1 - u], bit for bit
    # the formula, in float64
    u = np.arange(g, o - g)
    want = 0.5 - 0.5 * np.cos(np.pi * (u - g + 0.5) / (o - 2 * g))
    assert np.array_equal(w_in[g:o - g], want.astype(F32))
    assert np.array_equal(w_out[g:o - g], (1.0 - want).astype(F32))


def test_seam_is_one_fma_with_zero_weights_skipped():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    n = 4096
    prev, cur = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    w_in = rng.random(n).astype(F32)
    w_out = (1.0 - w_in.astype(np.float64)).astype(F32)
    prev[:64] *= F32(1e-20)                                          # terms of very different magnitudes
    cur[64:128] *= F32(1e20)
    w_in[200:210], w_out[200:210] = 0, 1
    w_in[300:310], w_out[300:310] = 1, 0
    got = S.seam(prev, cur, w_in, w_out)
    for i in list(range(0, 140)) + list(range(195, 215)) + list(range(295, 315)) + list(range(n - 50, n)):
        s = F32(w_out[i] * prev[i])
        exact = Fraction(float(w_in[i])) * Fraction(float(cur[i])) + Fraction(float(s))
        # the correctly rounded float32 of the exact sum: no float32 is strictly closer
        v = got[i]
        lo, hi = np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))
        err = abs(Fraction(float(v)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
    assert np.array_equal(got[200:210], prev[200:210]) and np.array_equal(got[300:310], cur[300:310])
    with pytest.raises(ValueError):
        S.seam(prev, cur[:-1], w_in, w_out)


@pytest.mark.parametrize("sr,window,overlap,guard", [(12000, 200, 60, 10), (12000, 200, 60, 0), (12000, 200, 100, 20)])
def test_stitch_returns_a_signal_its_windows_were_cut_from(sr, window, overlap, guard):
    p = S.StreamPlan(sr, window, overlap, guard)
    rng = np.random.default_rng(11)
    for n_windows, last in ((1, 777), (2, p.O48 + 1), (3, p.W48), (4, p.W48 - 3)):
        T48 = (n_windows - 1) * p.H48 + last
        x = rng.standard_normal(T48).astype(F32)
        windows = [x[i * p.H48:i * p.H48 + p.W48] for i in range(n_windows)]
        assert windows[-1].size == last
        y = S.stitch(windows, p)
        assert y.dtype == F32 and y.shape == (T48,)
        # w_in + w_out is 1 within 2^-24 and every operation rounds once: within 1 ulp per sample; outside the fades, the bits
        assert (np.abs(y.astype(np.float64) - x) <= np.spacing(np.abs(x))).all()
        fade = np.zeros(T48, dtype=bool)
        for i in range(1, n_windows):
            fade[i * p.H48 + p.G48:i * p.H48 + p.O48 - p.G48] = True
        assert np.array_equal(y[~fade], x[~fade])
    with pytest.raises(ValueError):
        S.stitch([x[:p.W48 - 1], x[:p.W48]], p)                      # only the last window may be short
    with pytest.raises(ValueError):
        S.stitch([x[:p.W48], x[:p.O48]], p)                          # and it is longer than the overlap
    with pytest.raises(ValueError):
        S.stitch([], p)


def test_stitch_guards_take_one_window_only():
    p = S.StreamPlan(12000, 200, 60, 10)
    rng = np.random.default_rng(12)
    a, b, c = (rng.standard_normal(p.W48).astype(F32) for _ in range(3))
    c = c[:p.O48 + 100]
    o, g, h = p.O48, p.G48, p.H48
    clean = S.stitch([a, b, c], p)
    # the guard regions are the other window's bits exactly
    assert np.array_equal(clean[h:h + g], a[-o:][:g]) and np.array_equal(clean[h + o - g:h + o], b[o - g:o])
    assert np.array_equal(clean[2 * h:2 * h + g], b[-o:][:g]) and np.array_equal(clean[2 * h + o - g:2 * h + o], c[o - g:o])
    # inside the fade both windows count
    mid = slice(h + g, h + o - g)
    assert not np.array_equal(clean[mid], a[-o:][g:o - g]) and not np.array_equal(clean[mid], b[g:o - g])
    # a NaN (an inf) behind a zero weight does not appear: the head guard of the newer window, the tail guard of the older one
    a2, b2, c2 = a.copy(), b.copy(), c.copy()
    b2[:g], c2[:g] = np.nan, np.inf
    a2[p.W48 - g:], b2[p.W48 - g:] = np.nan, -np.inf
    dirty = S.stitch([a2, b2, c2], p)
    assert np.isfinite(dirty).all() and np.array_equal(dirty, clean)
    # one step into the fade it does
    b3 = b.copy()
    b3[g] = np.nan
    assert np.isnan(S.stitch([a, b3, c], p)).sum() == 1


def test_host_prior_first_frame():
    seed, stream = 12345 + (678 << 32), 3
    for d in (8, 256):
        long = prior_normal_host(seed, stream, 40, d)
        for f in (0, 1, 5, 33):
            assert np.array_equal(prior_normal_host(seed, stream, 40 - f, d, first_frame=f), long[f:])
        assert np.array_equal(prior_normal_host(seed, stream, 40, d, first_frame=0), long)           # the default: every value as it was
    assert prior_normal_host(seed, stream, 0, 8, first_frame=7).shape == (0, 8)
    with pytest.raises(ValueError):
        prior_normal_host(seed, stream, 4, 8, first_frame=-1)


def test_host_prior_first_frame_past_32_bits_of_quads():
    """first_frame = 2^26 + 3 at 256 mels: the first quad is (2^26 + 3) * 64 = 2^32 + 192, so the counter's high word is 1."""
    seed, stream, f0, d, n = 7, 5 + (9 << 32), 2 ** 26 + 3, 256, 2
    got = prior_normal_host(seed, stream, n, d, first_frame=f0)
    q = f0 * (d // 4) + np.arange(n * d // 4, dtype=np.uint64)
    assert int(q[0]) == 2 ** 32 + 192 and int(q[0]) >> 32 == 1
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, stream & 0xFFFFFFFF), np.full_like(q, stream >> 32)], -1)
    assert (ctr[:, 1] == 1).all()
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((r[:, 0::2] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (r[:, 1::2] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    want = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1).reshape(n, d)
    assert np.array_equal(got, want)
    # with the high word dropped the values are others: the 64-bit counter is what is tested
    assert not np.array_equal(got, prior_normal_host(seed, stream, n, d, first_frame=3))


def test_entries_are_bound_and_declared():
    assert hip.ABI_VERSION == 6
    header = (Path(__file__).resolve().parents[1] / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header)
    assert "fh_prior_normal_at_f32" in hip.EXPORTS and "fh_xfade_seg_f32" in hip.EXPORTS
    assert hip._SIGS["fh_prior_normal_at_f32"] == [hip._P, hip._P, hip._P, hip._P, hip._I, hip._I, hip._I, hip._P]
    assert hip._SIGS["fh_xfade_seg_f32"] == [hip._P, hip._I, hip._P, hip._P, hip._I, hip._P]
    assert ("int fh_prior_normal_at_f32(float* out, const uint64_t* keys, const int64_t* first_frames, const int32_t* seg, int n_seg, "
            "int n, int d,") in header
    assert "int fh_xfade_seg_f32(const fh_xfade_job* jobs, int n_jobs, const float* w_in, const float* w_out, int o48, void* stream);" in header
    assert re.search(r"typedef struct \{\s*float\* head;\s*const float\* tail;\s*\} fh_xfade_job;", header)
    import ctypes
    assert ctypes.sizeof(hip.XfadeJob) == 16
    from flowhigh_amd import build
    assert "stream.hip" in build.SOURCES and "prior.hip" in build.SOURCES


def test_session_keywords_are_checked_before_any_launch():
    """The checks of stream() need no device: a stub with the model's `prior` goes through FlowHighSR.stream itself."""
    from flowhigh_amd import FlowHighSR
    from flowhigh_amd.streaming import StreamSession

    class Stub:
        prior = "device"
    s = FlowHighSR.stream(Stub(), 12000, window_ms=200, overlap_ms=60, guard_ms=10, seed=5, stream=2)
    assert isinstance(s, StreamSession) and s.key == (5, 2) and s.plan.key == (12000, 200, 60, 10) and s.timestep == 1
    for kw in (dict(channels="first"), dict(dither="tpdf"), dict(output_rate=44100), dict(loudness=-16.0), dict(true_peak=-1.0)):
        with pytest.raises(ValueError, match="not built for streaming"):
            FlowHighSR.stream(Stub(), 12000, **kw)
    with pytest.raises(ValueError, match="grain"):
        FlowHighSR.stream(Stub(), 22050, window_ms=1010)
    with pytest.raises(ValueError, match="pcm"):
        FlowHighSR.stream(Stub(), 12000, pcm="int8")
    Stub.prior = "reference"
    with pytest.raises(ValueError, match="prior='device'"):
        FlowHighSR.stream(Stub(), 12000, seed=1)


def test_session_cuts_its_stream_as_the_plan_says():
    """The host side of a session: blocks of any size add up to the plan's windows, the format is fixed by the first block."""
    from flowhigh_amd.streaming import StreamSession
    p = S.StreamPlan(12000, 200, 60, 10)
    for T in (1, p.O + 1, p.W - 1, p.W, p.W + 1, p.W + p.H, p.W + p.H + 1):
        x = np.arange(T, dtype=np.float32) / T
        for block in (1, 137, 2400, T):
            s = StreamSession(None, p, 1, (0, 0), None)
            got = []
            for a in range(0, T, block):
                s._take(x[a:a + block])
                cut, _ = s._cut(False)
                got += cut
                s.done += len(cut)
                assert s.done == p.runnable(min(a + block, T))
            cut, tail_ends = s._cut(True)
            got += cut
            assert [(wi, w.shape[1]) for wi, w, _ in got] == [(i, b - a) for i, (a, b) in enumerate(p.spans(T))]
            assert all(np.array_equal(w[0], x[a:b]) for (_, w, _), (a, b) in zip(got, p.spans(T)))
            assert [last for _, _, last in got] == [False] * (len(got) - 1) + [True] or tail_ends
            assert tail_ends == (T in (p.W, p.W + p.H))          # the stream ended with a full window's last sample
    s = StreamSession(None, p, 1, (0, 0), None)
    s._take(np.array([1, -1, 0], dtype=np.int16))                   # |x| <= 1 and still int16 full scale
    assert s.pending.dtype == np.float64 and np.array_equal(s.pending, np.array([1, -1, 0]) / 32768.0)
    with pytest.raises(ValueError, match="fixed by its first block"):
        s._take(np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError):
        s._take(np.zeros((2, 3), dtype=np.int16))
