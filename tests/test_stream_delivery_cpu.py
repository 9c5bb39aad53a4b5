"""CPU: streaming delivery -- the schedule of flowhigh_amd/stream_delivery.py (what is final after E inputs, what an output reads,
what a stage carries) and its chunked restatement against the whole-stream definitions bit for bit, the checks of
stream(delivery=) through a stub, and the new entries' declarations.  No GPU, no library."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from flowhigh_amd import hip, pcm, tables, truepeak
from flowhigh_amd import stream_delivery as SD

F32 = np.float32
T48 = 5000
CUTS = {"one": [T48], "odd": [1, 7, 300, 301, 1500, 2222, 4999, 5000], "every37": list(range(37, T48, 37)) + [T48]}
RATES = [44100, 16000, 96000, 22050, 8000]
KEY = (9, 0)
_STATE = {}


def noise(n=T48, seed=1):
    return (0.9 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)).astype(F32)


def resampled(rate):
    if rate not in _STATE:
        _STATE[rate] = SD.resample_whole(noise(), rate)
    return _STATE[rate]


@pytest.mark.parametrize("rate", RATES)
def test_resampler_schedule(rate):
    flt = SD.ResampleFilter(rate)
    taps, pre, up, down = tables.resample_poly_plan(rate, 48000)
    assert (flt.n_taps, flt.pre, flt.up, flt.down) == (taps.numel(), pre, up, down)
    finals = [flt.n_final(E) for E in range(T48 + 1)]
    assert finals[0] == 0 and all(b >= a for a, b in zip(finals, finals[1:]))                # monotone
    assert finals[-1] <= flt.n_final(T48, ended=True) == tables.resample_out_len(T48, rate, 48000)
    for E in (1, 2, 63, 300, 301, 4999, 5000):
        n = finals[E]
        assert n == 0 or flt.j_hi(n - 1) <= E - 1                                             # the last final output's inputs are there
        assert flt.j_hi(n) >= E or n < 0                                                      # and the next one's are not
    for i in (0, 1, 17, 1000, 4592):                                                          # j_lo: the first j with a tap under it
        pos, j = (i + pre) * down, flt.j_lo(i)
        assert pos - j * up < flt.n_taps and (j == 0 or pos - (j - 1) * up >= flt.n_taps)
    assert flt.carry_bound == -(-flt.n_taps // up) + 1


@pytest.mark.parametrize("cuts", sorted(CUTS))
@pytest.mark.parametrize("rate", RATES)
def test_chunked_resampler_is_the_whole_stream(rate, cuts):
    x, stats = noise(), {}
    plan = SD.make_plan(rate=rate)
    got = SD.chunked(x, CUTS[cuts], plan, stats=stats)
    want = resampled(rate)
    assert want.size == tables.resample_out_len(T48, rate, 48000) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(SD.whole(x, plan), want)
    flt = SD.ResampleFilter(rate)
    assert stats["resample_carry"] <= flt.carry_bound, (stats["resample_carry"], flt.carry_bound)
    assert all(hi < E and lo >= 0 for E, lo, hi in stats["reads"]) and stats["reads"]        # no read at or past E
    # what every push emits is the schedule's: n_final of what has arrived, the rest at the flush
    done = np.cumsum(stats["lens"])
    assert [int(d) for d in done[:-1]] == [flt.n_final(c) for c in CUTS[cuts]] and done[-1] == want.size


def planted(x, cuts):
    """One sample of 1.5 at the stream's first and last index and on each side of a cut."""
    x = x.copy()
    c = cuts[len(cuts) // 2] if len(cuts) > 1 else x.size // 2
    for i in (0, x.size - 1, c - 1, c):
        x[i] = 1.5
    return x


@pytest.mark.parametrize("cuts", sorted(CUTS))
@pytest.mark.parametrize("rate,H", [(8000, 40), (48000, 240)])
def test_chunked_limiter_is_truepeak_limit(rate, H, cuts):
    assert truepeak.half_window(rate) == H
    # the limiter's own stage: its input is the stream at `rate` whatever made it, so the cuts are cuts of that stream
    x = planted(noise(seed=rate), CUTS[cuts])
    ls, blocks, carry, carries, prev = SD.LimitStage(H), [], np.zeros(0, F32), 0, 0
    for c, ended in [(c, False) for c in CUTS[cuts]] + [(T48, True)]:
        job = ls.step(c - prev, ended)
        src = np.concatenate([carry, x[prev:c]])
        assert job["base"] + src.size == c and job["n_carry"] == carry.size
        assert job["first"] + job["n_out"] == (c if ended else max(0, c - ls.D))              # F - D while open, F at the end
        blocks.append(SD.limit_span(src, job["base"], c, job["first"], job["n_out"], ended, H, -6.0))
        carry, prev = src[src.size - job["n_keep"]:], c
        carries = max(carries, carry.size)
    want, g, m = truepeak.limit(x, rate, -6.0)
    assert g.min() < 0.9 and m.max() > 1.4                                                    # the limiter works
    got = np.concatenate(blocks)
    assert got.shape == want[0].shape and np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
    assert carries <= 2 * ls.D and ls.D == 2 * H + truepeak.HALF


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_chunked_chain_is_the_whole_stream(cuts):
    """8000 Hz -> limiter at -6 dBTP (H = 40) -> dithered int16, against resample_whole + truepeak.limit + pcm.encode."""
    x = planted(noise(seed=3), CUTS[cuts])
    plan = SD.make_plan(rate=8000, true_peak=-6.0, pcm="int16", key=KEY)
    stats = {}
    got = SD.chunked(x, CUTS[cuts], plan, stats)
    y = truepeak.limit(SD.resample_whole(x, 8000), 8000, -6.0)[0]
    want = pcm.encode(y, KEY)[0]
    assert got.dtype == np.int16 and np.array_equal(got, want) and np.array_equal(SD.whole(x, plan), want)
    assert stats["limit_carry"] <= 2 * (2 * 40 + 10) and sum(stats["lens"]) == tables.resample_out_len(T48, 8000, 48000)


def test_dither_takes_the_absolute_index():
    seed, stream = 12345 + (678 << 32), 3
    long = pcm.tpdf_dither(seed, stream, 1, 101)
    assert np.array_equal(pcm.tpdf_dither(seed, stream, 1, 101, first=0), long)               # the default: today's values
    for first in (1, 2, 7, 50, 100, 101):
        assert np.array_equal(pcm.tpdf_dither(seed, stream, 1, 101 - first, first=first), long[first:])
    ra, rb = pcm.dither_uniforms(seed, stream, 0, 5, first=3)
    ra0, rb0 = pcm.dither_uniforms(seed, stream, 0, 8)
    assert np.array_equal(ra, ra0[3:]) and np.array_equal(rb, rb0[3:])
    # the counter has 64 bits: at 2^33 + 5 the block index is 2^32 + 2, and the values are not those of index 5
    big = pcm.tpdf_dither(seed, stream, 0, 16, first=2 ** 33 + 5)
    assert big.shape == (16,) and not np.array_equal(big, pcm.tpdf_dither(seed, stream, 0, 16, first=5))
    with pytest.raises(ValueError):
        pcm.tpdf_dither(seed, stream, 0, 4, first=-1)
    # the encoder's blocks of a stream
    x = noise(300, 5)
    plan = SD.make_plan(pcm="int16", key=KEY)
    assert np.array_equal(SD.chunked(x, [1, 7, 150, 300], plan), pcm.encode(x, KEY)[0])
    d = pcm.tpdf_dither(KEY[0], KEY[1], 0, 300, first=2 ** 33 + 5)
    assert np.array_equal(SD.chunked(x, [1, 7, 150, 300], plan, first=2 ** 33 + 5), pcm.quantize(x, d))


# ---- keywords ----------------------------------------------------------------------------------------------------------------
class Stub:
    prior = "device"


def open_stub(**kw):
    from flowhigh_amd import FlowHighSR
    return FlowHighSR.stream(Stub(), 12000, **{**dict(window_ms=200, overlap_ms=60, guard_ms=10, seed=5), **kw})


FULL = dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=9, true_peak=-3.0, limiter="lookahead")


def test_delivery_keyword_opens_a_delivering_session():
    from flowhigh_amd.delivery_stream import DeliveryStream
    s = open_stub(delivery=FULL)
    assert isinstance(s.delivery, DeliveryStream) and list(s.delivery.stages) == ["resample", "limit", "encode"]
    assert s.delivery.plan == SD.make_plan(rate=44100, true_peak=-3.0, pcm="int16", key=(9, 0)) and s.pcm is None
    assert s.delivery.stages["limit"].counters.H == truepeak.half_window(44100)
    assert open_stub(delivery=dict(output_rate=48000)).delivery is None                       # 48 kHz is the default
    assert list(open_stub(delivery=dict(pcm="int16")).delivery.stages) == ["encode"]
    # every value a default: a plain session, also beside the session's own pcm=
    for d in (None, {}, dict(output_rate=None, pcm=None, dither=None, dither_seed=0, true_peak=None, limiter=None)):
        s = open_stub(delivery=d, pcm="int16")
        assert s.delivery is None and s.pcm == "int16"


@pytest.mark.parametrize("delivery,kw,word", [
    (dict(rate=44100), {}, "no key 'rate'"),
    (dict(loudness=-16.0), {}, "statistic of the whole stream"),
    (dict(interleaved=True), {}, "mono"),
    (dict(channels="first"), {}, "mono"),
    (dict(true_peak=-1.0), {}, "limiter='lookahead'"),
    (dict(limiter="lookahead"), {}, "goes with true_peak"),
    (dict(true_peak=-1.0, limiter="soft"), {}, "limiter must be"),
    (dict(true_peak=1.0, limiter="lookahead"), {}, "true_peak must be"),
    (dict(dither="tpdf"), {}, "dither= goes with pcm="),
    (dict(pcm="int8"), {}, "pcm must be"),
    (dict(pcm="int16", dither="tpdf", dither_seed=1.5), {}, "dither_seed"),
    (dict(output_rate=44101), {}, "at most 640"),
    (dict(output_rate=-8000), {}, "positive integer"),
    (dict(output_rate=192000, true_peak=-1.0, limiter="lookahead"), {}, "look-ahead of 960"),
    (dict(pcm="int16"), dict(pcm="int16"), "two encoders"),
    ("int16", {}, "must be None or a dict"),
])
def test_delivery_keyword_refusals(delivery, kw, word):
    with pytest.raises(ValueError, match=word):
        open_stub(delivery=delivery, **kw)


def test_old_keywords_and_order_of_checks():
    from flowhigh_amd import FlowHighSR

    class LongStub(Stub):                                                                     # (generate_long opens its session itself)
        stream = FlowHighSR.stream
    for kw in (dict(channels="first"), dict(dither="tpdf"), dict(output_rate=44100), dict(loudness=-16.0), dict(true_peak=-1.0)):
        with pytest.raises(ValueError, match="not built for streaming"):
            open_stub(delivery=FULL, **kw)                                                    # the old checks come first
        with pytest.raises(ValueError, match="not built for streaming"):
            FlowHighSR.generate_long(LongStub(), np.zeros(10, F32), 12000, delivery=FULL, **kw)
    with pytest.raises(ValueError, match="grain"):
        open_stub(delivery=dict(rate=1), overlap_ms=65)                                       # the plan's before delivery's
    with pytest.raises(ValueError, match="pcm must be"):
        open_stub(delivery=dict(rate=1), pcm="int8")


def test_standalone_stream_keywords():
    from flowhigh_amd import FlowHighSR
    from flowhigh_amd.delivery_stream import DeliveryStream
    s = FlowHighSR.delivery_stream(Stub(), **FULL)
    assert isinstance(s, DeliveryStream) and s.plan["key"] == (9, 0) and not s.closed
    with pytest.raises(ValueError, match="nothing to deliver"):
        FlowHighSR.delivery_stream(Stub())
    with pytest.raises(ValueError, match="no key"):
        FlowHighSR.delivery_stream(Stub(), rate=8000)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_bound_and_declared():
    assert hip.ABI_VERSION == 6
    header = (Path(__file__).resolve().parents[1] / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header)
    sigs = {"fh_sizeof_stream_job": [],
            "fh_stream_resample_f32": [hip._P, hip._I, hip._I, hip._P, hip._I, hip._I, hip._I, hip._I, hip._P],
            "fh_stream_limit_f32": [hip._P, hip._I, hip._I, hip._P, hip._P, hip._I, hip._F, hip._P],
            "fh_stream_pcm_i16_f32": [hip._P, hip._I, hip._I, hip._P, hip._P]}
    for name, sig in sigs.items():
        assert name in hip.EXPORTS and hip._SIGS[name] == sig
        assert re.search(r"\bint " + name + r"\(", header), name
    flat = " ".join(header.split())
    assert ("int fh_stream_resample_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const float* taps, int up, int down, "
            "int n_taps, int pre, void* stream);") in flat
    assert ("int fh_stream_limit_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const float* taps4, const double* w, int H, "
            "float ceiling, void* stream);") in flat
    assert "int fh_stream_pcm_i16_f32(const fh_stream_job* jobs, int n_jobs, int max_out, const uint64_t* keys, void* stream);" in flat
    # the struct, field by field, on both sides: 4 pointers, 2 int64, 6 int32
    body = re.search(r"typedef struct \{([^}]*)\} fh_stream_job;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in hip.StreamJob._fields_]
    assert ctypes.sizeof(hip.StreamJob) == 4 * 8 + 2 * 8 + 6 * 4 == 72
    assert hip.StreamJob.base.offset == 32 and hip.StreamJob.first.offset == 40 and hip.StreamJob.n_carry.offset == 48
    from flowhigh_amd import build
    assert "stream_delivery.hip" in build.SOURCES
    assert "pcm_common.h" in build.HEADERS and "truepeak_common.h" in build.HEADERS
    # one statement of the limiter's constants and helpers for clips and streams, and it is the definition's
    csrc = Path(__file__).resolve().parents[1] / "flowhigh_amd" / "csrc"
    common = (csrc / "truepeak_common.h").read_text()
    assert f"MAX_H = {truepeak.MAX_H};" in common and f"HALO = {truepeak.HALF};" in common
    for src in ("truepeak.hip", "stream_delivery.hip"):
        text = (csrc / src).read_text()
        assert '#include "truepeak_common.h"' in text and "tp_phase(const float*" not in text, src
