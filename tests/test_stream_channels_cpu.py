"""CPU: streams of channels -- stream_delivery.py's chunked restatement on [C, T] against the whole-stream definitions bit for bit
(the resampler per row, truepeak.limit on [C, T], pcm.encode with channel c's dither, planar and interleaved), that the limiter
is channel-linked, the checks of n_channels= / interleaved= through a stub (the older refusals first), the host side of a
session on [C, n] blocks, stream.stitch on rows, and the two new entries' declarations.  No GPU, no library."""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

from flowhigh_amd import hip, pcm, truepeak
from flowhigh_amd import stream as S
from flowhigh_amd import stream_delivery as SD

F32 = np.float32
T48 = 5000
CUTS = {"one": [T48], "odd": [1, 7, 300, 301, 1500, 2222, 4999, 5000], "every37": list(range(37, T48, 37)) + [T48]}
KEY = (9, 0)
_STATE = {}


def linked_clip(C, cuts, n=T48, seed=1):
    """[C, n]: channel 0 is 0.3 noise with one sample of 1.5 at the first and the last index and on each side of a cut; the
    other channels are 0.3 noise."""
    x = (0.3 * np.random.default_rng(seed).uniform(-1.0, 1.0, (C, n))).astype(F32)
    c = cuts[len(cuts) // 2] if len(cuts) > 1 else n // 2
    for i in (0, n - 1, c - 1, c):
        x[0, i] = 1.5
    return x


def spikes(cuts, n=T48):
    c = cuts[len(cuts) // 2] if len(cuts) > 1 else n // 2
    return [0, n - 1, c - 1, c]


def whole(C, cuts, rate, tp, enc, frames):
    """SD.whole, once per case (the cut sets that share their spikes share it too)."""
    plan = SD.make_plan(rate, tp, "int16" if enc else None, KEY if enc == "dither" else None, C, frames)
    k = (C, tuple(spikes(CUTS[cuts])), rate, tp, enc, frames)
    if k not in _STATE:
        _STATE[k] = SD.whole(linked_clip(C, CUTS[cuts]), plan)
    return plan, _STATE[k]


# rates x limiter x (float | dithered int16, planar and interleaved); the undithered encoder once, at the full chain
CASES = [(rate, tp, enc, frames) for rate, tp, enc in itertools.product([None, 44100, 8000], [None, -6.0], [None, "dither"])
         for frames in ((False, True) if enc else (False,))] + [(44100, -6.0, "plain", False), (44100, -6.0, "plain", True)]


@pytest.mark.parametrize("cuts", sorted(CUTS))
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_chunked_is_the_whole_stream(C, cuts):
    x = linked_clip(C, CUTS[cuts])
    cases = CASES
    for rate, tp, enc, frames in cases:
        plan, want = whole(C, cuts, rate, tp, enc, frames)
        got = SD.chunked(x, CUTS[cuts], plan)
        n = want.shape[0] if frames else want.shape[1]
        assert got.dtype == want.dtype == (np.int16 if enc else F32) and got.shape == want.shape == ((n, C) if frames else (C, n))
        assert np.array_equal(got.view(np.uint16 if enc else np.uint32), want.view(np.uint16 if enc else np.uint32)), (rate, tp, enc, frames)
        assert got.flags["C_CONTIGUOUS"]


def test_whole_is_the_definitions_on_a_clip():
    x = linked_clip(3, CUTS["odd"])
    y = np.stack([SD.resample_whole(r, 8000) for r in x])
    lim = truepeak.limit(y, 8000, -6.0)[0]
    assert np.array_equal(SD.whole(x, SD.make_plan(8000, -6.0, channels=3)), lim)
    for frames in (False, True):
        want = pcm.encode(lim, KEY, frames)
        assert np.array_equal(SD.whole(x, SD.make_plan(8000, -6.0, "int16", KEY, 3, frames)), want)
    assert not np.array_equal(pcm.encode(lim, KEY)[1], pcm.quantize(lim[1], pcm.tpdf_dither(KEY[0], KEY[1], 0, lim.shape[1])))   # c's own dither


@pytest.mark.parametrize("plan", [SD.make_plan(44100, -6.0, "int16", KEY), SD.make_plan(true_peak=-6.0), SD.make_plan(8000)])
def test_one_row_has_the_bits_of_the_flat_stream(plan):
    x = linked_clip(1, CUTS["odd"])
    flat = SD.chunked(x[0], CUTS["odd"], plan)
    for p in (plan, dict(plan, channels=1, interleaved=False)):
        got = SD.chunked(x, CUTS["odd"], p)
        assert flat.ndim == 1 and got.shape == (1, flat.size) and got.dtype == flat.dtype and np.array_equal(got[0], flat)
        assert np.array_equal(SD.whole(x, p)[0], SD.whole(x[0], plan))


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_the_limiter_is_channel_linked(cuts):
    """A quiet channel moves where channel 0 peaks, by channel 0's gain; limited alone it comes back as it went in."""
    x = linked_clip(3, CUTS[cuts])
    TP = -1.0                                   # 0.89: over the quiet rows' true peak (asserted), far under the spikes
    plan = SD.make_plan(true_peak=TP, channels=3)
    y = SD.chunked(x, CUTS[cuts], plan)
    _, g, m = truepeak.limit(x[:1], 48000, TP)
    c32 = F32(truepeak.ceiling(TP))
    assert m.max() > 1.4 and g.min() < 0.7 and truepeak.envelope(x[1:]).max() < c32
    for c in (1, 2):
        # (the quiet rows stay under the ceiling, so wherever m is over it m is channel 0's: the one gain is channel 0's)
        assert np.array_equal(y[c], np.clip((x[c] * g).astype(F32), -c32, c32))
        for i in spikes(CUTS[cuts]):
            near = slice(max(0, i - 100), i + 100)
            assert not np.array_equal(y[c, near], x[c, near])
        alone = SD.chunked(x[c], CUTS[cuts], SD.make_plan(true_peak=TP))
        assert np.array_equal(alone.view(np.uint32), x[c].view(np.uint32))
    assert np.abs(y).max() <= c32


def test_envelope_and_limit_spans_take_rows():
    x = linked_clip(2, CUTS["one"], 700)
    m = SD.envelope_span(x, 0, 700, 0, 700, True)
    rows = [SD.envelope_span(r, 0, 700, 0, 700, True) for r in x]
    assert m.dtype == F32 and np.array_equal(m, np.maximum(rows[0], rows[1])) and np.array_equal(m, truepeak.envelope(x))
    y = SD.limit_span(x, 0, 700, 0, 700, True, 240, -6.0)
    assert y.shape == (2, 700) and np.array_equal(y, truepeak.limit(x, 48000, -6.0)[0])
    assert SD.limit_span(x, 0, 700, 0, 0, False, 240, -6.0).shape == (2, 0)
    assert SD.limit_span(x[0], 0, 700, 0, 0, False, 240, -6.0).shape == (0,)


# ---- plans and keywords --------------------------------------------------------------------------------------------------------
def test_make_plan_defaults_are_the_mono_plan():
    assert SD.make_plan(44100, -3.0, "int16", (9, 0)) == dict(rate=44100, true_peak=-3.0, pcm="int16", key=(9, 0))
    assert SD.make_plan() == SD.make_plan(channels=None, interleaved=False) == dict(rate=None, true_peak=None, pcm=None, key=None)
    assert SD.make_plan(pcm="int16", channels=2, interleaved=True) == dict(rate=None, true_peak=None, pcm="int16", key=None, channels=2,
                                                                           interleaved=True)
    for bad in (True, 2.0, 0, 9, "2"):
        with pytest.raises(ValueError, match="channels"):
            SD.make_plan(channels=bad)
    with pytest.raises(ValueError, match="interleaved"):
        SD.make_plan(pcm="int16", interleaved=True)
    with pytest.raises(ValueError, match="pcm"):
        SD.make_plan(channels=2, interleaved=True)
    with pytest.raises(ValueError):
        SD.chunked(np.zeros((3, 10), F32), [10], SD.make_plan(8000, channels=2))
    with pytest.raises(ValueError):
        SD.chunked(np.zeros((9, 10), F32), [10], SD.make_plan(8000))


class Stub:
    prior = "device"


def open_stub(**kw):
    from flowhigh_amd import FlowHighSR
    return FlowHighSR.stream(Stub(), 12000, **{**dict(window_ms=200, overlap_ms=60, guard_ms=10, seed=5), **kw})


FULL = dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=9, true_peak=-3.0, limiter="lookahead")


def test_n_channels_opens_streams_of_channels():
    from flowhigh_amd import FlowHighSR
    from flowhigh_amd.delivery_stream import DeliveryStream
    s = open_stub(n_channels=2, delivery=dict(FULL, interleaved=True))
    assert s.channels == 2 and s.rows == 2 and isinstance(s.delivery, DeliveryStream) and s.delivery.channels == 2 and s.delivery.interleaved
    assert s.delivery.plan == SD.make_plan(44100, -3.0, "int16", (9, 0), 2, True)
    assert [st.rows for st in s.delivery.stages.values()] == [2, 2, 2] and list(s.delivery.stages) == ["resample", "limit", "encode"]
    mono = open_stub(delivery=FULL)
    assert mono.channels is None and mono.rows == 1 and mono.delivery.channels is None and mono.delivery.plan == SD.make_plan(44100, -3.0, "int16", (9, 0))
    assert len(mono.delivery.key) == 4                                                        # the mono plan's key as it was
    # streams of one plan share launches whatever their channel counts; planar and interleaved, mono and n_channels=1 do not
    keys = [FlowHighSR.delivery_stream(Stub(), n_channels=c, **FULL).key for c in (1, 2, 3)]
    assert keys[0] == keys[1] == keys[2] != mono.delivery.key
    assert FlowHighSR.delivery_stream(Stub(), n_channels=2, interleaved=True, **FULL).key != keys[1]
    assert open_stub(n_channels=3).delivery is None and open_stub(n_channels=3, pcm="int16").pcm == "int16"
    assert open_stub(n_channels=np.int64(8)).channels == 8
    d = FlowHighSR.delivery_stream(Stub(), n_channels=3, pcm="int16")
    assert d.channels == 3 and not d.interleaved and list(d.stages) == ["encode"]


@pytest.mark.parametrize("bad", [True, False, 2.0, 0, 9, -1, "2"])
def test_n_channels_refusals(bad):
    from flowhigh_amd import FlowHighSR
    with pytest.raises(ValueError, match="n_channels"):
        open_stub(n_channels=bad)
    with pytest.raises(ValueError, match="n_channels"):
        open_stub(n_channels=bad, delivery=FULL)
    with pytest.raises(ValueError, match="n_channels"):
        FlowHighSR.delivery_stream(Stub(), n_channels=bad, **FULL)


def test_new_and_old_refusals_beside_n_channels():
    from flowhigh_amd import FlowHighSR

    class LongStub(Stub):
        stream = FlowHighSR.stream
    # interleaved: with n_channels and pcm only
    with pytest.raises(ValueError, match="mono"):
        open_stub(delivery=dict(FULL, interleaved=True))
    with pytest.raises(ValueError, match="mono"):
        FlowHighSR.delivery_stream(Stub(), interleaved=True, **FULL)
    with pytest.raises(ValueError, match="goes with pcm"):
        open_stub(n_channels=2, delivery=dict(output_rate=44100, interleaved=True))
    with pytest.raises(ValueError, match="goes with pcm"):
        FlowHighSR.delivery_stream(Stub(), n_channels=2, output_rate=44100, interleaved=True)
    with pytest.raises(ValueError, match="interleaved must be a bool"):
        open_stub(n_channels=2, delivery=dict(FULL, interleaved=1.5))
    # channels= stays refused inside delivery= with the message it had, n_channels or not
    for kw in ({}, dict(n_channels=2)):
        with pytest.raises(ValueError, match="mono"):
            open_stub(delivery=dict(FULL, channels="first"), **kw)
        with pytest.raises(ValueError, match="statistic of the whole stream"):
            open_stub(delivery=dict(FULL, loudness=-16.0), **kw)
        with pytest.raises(ValueError, match="limiter='lookahead'"):
            open_stub(delivery=dict(true_peak=-1.0), **kw)
        with pytest.raises(ValueError, match="two encoders"):
            open_stub(delivery=dict(pcm="int16"), pcm="int16", **kw)
        with pytest.raises(ValueError, match="no key 'rate'"):
            open_stub(delivery=dict(rate=44100), **kw)
    # the older checks come first: beside a bad n_channels they still are what is raised
    for kw in (dict(channels="first"), dict(dither="tpdf"), dict(output_rate=44100), dict(loudness=-16.0), dict(true_peak=-1.0)):
        for n in (2, 9):
            with pytest.raises(ValueError, match="not built for streaming"):
                open_stub(n_channels=n, delivery=FULL, **kw)
            with pytest.raises(ValueError, match="not built for streaming"):
                FlowHighSR.generate_long(LongStub(), np.zeros((2, 10), F32), 12000, n_channels=n, delivery=FULL, **kw)
    with pytest.raises(ValueError, match="grain"):
        open_stub(n_channels=9, overlap_ms=65)
    with pytest.raises(ValueError, match="pcm must be"):
        open_stub(n_channels=9, pcm="int8")
    Stub.prior = "reference"
    try:
        with pytest.raises(ValueError, match="prior='device'"):
            open_stub(n_channels=9)
    finally:
        Stub.prior = "device"


# ---- the host side of a session ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3])
def test_a_session_cuts_rows_as_the_plan_says(C):
    from flowhigh_amd.streaming import StreamSession
    p = S.StreamPlan(12000, 200, 60, 10)
    for T in (1, p.O + 1, p.W, p.W + 1, p.W + p.H, p.W + p.H + 1):
        x = (np.arange(C * T, dtype=F32) / (C * T)).reshape(C, T)
        for block in (137, 2400, T):
            s = StreamSession(None, p, 1, (0, 0), None, None, C)
            got = []
            for a in range(0, T, block):
                s._take(x[:, a:a + block])
                cut, _ = s._cut(False)
                got += cut
                s.done += len(cut)
                assert s.done == p.runnable(min(a + block, T)) and s.arrived == min(a + block, T)
            cut, tail_ends = s._cut(True)
            got += cut
            assert [(wi, w.shape) for wi, w, _ in got] == [(i, (C, b - a)) for i, (a, b) in enumerate(p.spans(T))]
            assert all(np.array_equal(w, x[:, a:b]) for (_, w, _), (a, b) in zip(got, p.spans(T)))
            assert tail_ends == (T in (p.W, p.W + p.H))


def test_a_block_of_another_row_count_leaves_the_session_as_it_was():
    import torch
    from flowhigh_amd.streaming import StreamSession
    p = S.StreamPlan(12000, 200, 60, 10)
    s = StreamSession(None, p, 1, (0, 0), None, None, 2)
    s._take(np.ones((2, 5), dtype=np.int16))
    s._take(torch.ones(2, 3, dtype=torch.int16))
    assert s.pending.shape == (2, 8) and s.pending.dtype == np.float64 and s.arrived == 8 and np.all(s.pending == 1 / 32768.0)
    for bad in (np.zeros((3, 4), np.int16), np.zeros(4, np.int16), np.zeros((1, 4), np.int16), np.zeros((2, 2, 2), np.int16),
                np.zeros((4, 2), np.int16)):
        with pytest.raises(ValueError, match=r"\[2, n\]"):
            s._take(bad)
        assert s.pending.shape == (2, 8) and s.arrived == 8
    with pytest.raises(ValueError, match="fixed by its first block"):
        s._take(np.zeros((2, 3), dtype=F32))
    one = StreamSession(None, p, 1, (0, 0), None, None, 1)           # n_channels=1: [1, n], not [n]
    with pytest.raises(ValueError, match=r"\[1, n\]"):
        one._take(np.zeros(4, F32))
    one._take(np.zeros((1, 4), F32))
    assert one.pending.shape == (1, 4)
    # a [2, 2] block is two channels of two samples: the count is the session's
    s2 = StreamSession(None, p, 1, (0, 0), None, None, 2)
    s2._take(np.array([[1, 2], [3, 4]], dtype=F32))
    assert np.array_equal(s2.pending, [[1, 2], [3, 4]])


def test_stitch_takes_rows():
    p = S.StreamPlan(12000, 200, 60, 10)
    rng = np.random.default_rng(3)
    wins = [rng.standard_normal((3, n)).astype(F32) for n in (p.W48, p.W48, p.O48 + 100)]
    y = S.stitch(wins, p, channels=3)
    assert y.shape == (3, 2 * p.H48 + p.O48 + 100) and y.dtype == F32
    for c in range(3):
        assert np.array_equal(y[c].view(np.uint32), S.stitch([w[c] for w in wins], p).view(np.uint32))
    one = S.stitch([w[:1] for w in wins], p, channels=1)
    assert one.shape == (1, y.shape[1]) and np.array_equal(one[0], y[0])
    with pytest.raises(ValueError):
        S.stitch(wins, p, channels=2)
    with pytest.raises(ValueError):
        S.stitch([], p, channels=2)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_entries_are_bound_and_declared():
    assert hip.ABI_VERSION == 6
    header = (Path(__file__).resolve().parents[1] / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header)
    P, I, F = hip._P, hip._I, hip._F
    sigs = {"fh_stream_limit_linked_f32": [P, I, P, I, I, P, P, I, F, P], "fh_stream_pcm_i16_rows_f32": [P, I, P, I, I, P, I, P]}
    for name, sig in sigs.items():
        assert name in hip.EXPORTS and hip._SIGS[name] == sig
    flat = " ".join(header.split())
    assert ("int fh_stream_limit_linked_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out, "
            "const float* taps4, const double* w, int H, float ceiling, void* stream);") in flat
    assert ("int fh_stream_pcm_i16_rows_f32(const fh_stream_job* jobs, int n_jobs, const int32_t* groups, int n_groups, int max_out, "
            "const uint64_t* keys, int interleaved, void* stream);") in flat
    # the older three as they were, and the job's 72 bytes
    assert hip._SIGS["fh_stream_limit_f32"] == [P, I, I, P, P, I, F, P] and hip._SIGS["fh_stream_pcm_i16_f32"] == [P, I, I, P, P]
    import ctypes
    assert ctypes.sizeof(hip.StreamJob) == 72 and len(hip.StreamJob._fields_) == 12
