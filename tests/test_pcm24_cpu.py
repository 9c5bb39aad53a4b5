"""CPU: the 24-bit encodings pcm='s24' / 's24in32' as flowhigh_amd/pcm.py defines them (quantize24 against an independent
restatement in Python integers and fractions, pack24, the float64 add pinned by its statistics, the dither's identity across
blocks), the keywords' resolution and refusals, the numpy stream restatement against the one-shot encoding, and the three new
entries in the header and the bindings.  No GPU, no library."""
import ctypes
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from flowhigh_amd import delivery, hip, pcm
from flowhigh_amd import stream_delivery as SD

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
ENTRIES = {"fh_pcm_s24_f32": 9, "fh_pcm_s24_seg_f32": 8, "fh_stream_pcm_s24_rows_f32": 9}
KEY = (7, 0)
LSB = 2.0 ** -23
EDGES = np.array([1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 2.0 ** -24, -2.0 ** -24, 0.5 * LSB, -0.5 * LSB, 1.5 * LSB, -1.5 * LSB,
                  2.5 * LSB, -2.5 * LSB, 0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, -1.5], dtype=F32)
_STATE = {}


def samples():
    """2000 random samples (some small enough that the dither decides everything) and the edge values; their dither."""
    if "x" not in _STATE:
        rng = np.random.default_rng(24)
        x = np.concatenate([rng.uniform(-1.1, 1.1, 1500), rng.uniform(-4, 4, 500) * LSB]).astype(F32)
        _STATE["x"] = np.concatenate([x, EDGES])
        _STATE["d"] = pcm.tpdf_dither(3, 1, 0, _STATE["x"].size)
    return _STATE["x"], _STATE["d"]


def rint_even(v):
    """A Fraction rounded to the nearest integer, ties to even."""
    f = math.floor(v)
    r = v - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2):
        return f + 1
    return f


def restated(x, d):
    """quantize24 of one sample in exact arithmetic: x 2^23 is exact; the one float64 add is the float64 nearest the exact sum."""
    x = float(x)
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return 8388607 if x > 0 else -8388608
    v = Fraction(x) * 2 ** 23
    if d is not None:
        v = Fraction(float(v) + float(d))          # (v is a float64 exactly; Python's float add IS one float64 add, to nearest even)
    return max(-8388608, min(8388607, rint_even(v)))


@pytest.mark.parametrize("dithered", [False, True])
def test_quantize24_against_integers_and_fractions(dithered):
    x, d = samples()
    d = d if dithered else None
    q = pcm.quantize24(x, d)
    assert q.dtype == np.int32 and q.shape == x.shape
    want = [restated(a, None if d is None else d[i]) for i, a in enumerate(x)]
    assert q.tolist() == want
    if not dithered:
        # the edges by hand: the clamp is asymmetric, ties go to even, NaN gives 0
        assert pcm.quantize24(EDGES).tolist() == [8388607, -8388608, 8388607, -8388608, 0, 0, 0, 0, 2, -2, 2, -2, 0, 0, 0,
                                                  8388607, -8388608, 8388607, -8388608]
        assert pcm.quantize24(F32(1 - 2.0 ** -23)).tolist() == 8388607 and pcm.quantize24(F32(3 * LSB)).tolist() == 3


def test_pack24_and_encode24_layouts():
    q = np.array([0, 1, -1, 0x123456, -0x123456, 8388607, -8388608, 256, -256], dtype=np.int32)
    b = pcm.pack24(q)
    assert b.dtype == np.uint8 and b.shape == (9, 3)
    assert b[3].tolist() == [0x56, 0x34, 0x12] and b[2].tolist() == [255, 255, 255] and b[6].tolist() == [0, 0, 0x80]
    assert b.tobytes() == b"".join(int(v).to_bytes(3, "little", signed=True) for v in q)
    assert np.array_equal(pcm.unpack24(b), q)
    rng = np.random.default_rng(5)
    for C in (1, 2, 3):
        x = rng.uniform(-1, 1, (C, 37)).astype(F32)
        for inter in (False, True):
            for key in (None, KEY):
                wide = pcm.encode24(x, key, inter, packed=False)
                packed = pcm.encode24(x, key, inter, packed=True)
                assert wide.dtype == np.int32 and wide.shape == ((37, C) if inter else (C, 37))
                assert packed.dtype == np.uint8 and packed.shape == wide.shape + (3,)
                assert np.array_equal(packed, pcm.pack24(wide)) and np.array_equal(pcm.unpack24(packed), wide)
        d = np.stack([pcm.tpdf_dither(KEY[0], KEY[1], c, 37) for c in range(C)])
        assert np.array_equal(pcm.encode24(x, KEY, True, packed=False), pcm.quantize24(x, d).T)
    assert np.array_equal(pcm.encode24(x[0]), pcm.encode24(x[:1]))                            # [T] is one channel
    # the int16 functions are what they were
    assert pcm.quantize(F32(0.5)).dtype == np.int16 and pcm.encode(x).dtype == np.int16


def test_the_add_is_float64():
    """Constant float32(0.7), key (7, 0), 2^20 samples: the error's mean is 0 within 0.005 LSB (measured 0.0004, its standard error
    0.0005; a float32 add gives a DC bias of 0.187) and, on a uniform input of amplitude 0.9, its variance 0.25 within 0.01
    (1/6 of the dither + 1/12 of the rounding; a float32 add gives 0.283)."""
    n = 2 ** 20
    d = pcm.tpdf_dither(7, 0, 0, n)
    x = np.full(n, 0.7, dtype=F32)
    e = pcm.quantize24(x, d).astype(np.float64) - x.astype(np.float64) * 2.0 ** 23
    print(f"pcm24: constant 0.7: mean error {e.mean():+.5f} LSB, variance {e.var():.4f}")
    assert abs(e.mean()) <= 0.005
    assert abs(e.var() - 0.25) <= 0.01
    u = (0.9 * np.random.default_rng(1).uniform(-1, 1, n)).astype(F32)
    e = pcm.quantize24(u, d).astype(np.float64) - u.astype(np.float64) * 2.0 ** 23
    print(f"pcm24: uniform 0.9: mean error {e.mean():+.5f} LSB, variance {e.var():.4f}")
    assert abs(e.var() - 0.25) <= 0.01 and abs(e.mean()) <= 0.005
    # and the float32 form this replaces is the biased one: the definition cannot quietly go back to it
    with np.errstate(all="ignore"):
        q32 = np.rint((x * F32(2.0 ** 23) + d).astype(F32))
    assert abs((q32 - x.astype(np.float64) * 2.0 ** 23).mean()) > 0.1


@pytest.mark.parametrize("k", [0, 1, 8, 333, 2 ** 32 + 6, 2 ** 32 + 7])
def test_dither_identity_across_blocks(k):
    n = 64
    x = (0.9 * np.random.default_rng(2).uniform(-1, 1, n)).astype(F32)
    if k < 1000:
        whole_x = np.concatenate([np.zeros(k, F32), x])
        whole = pcm.quantize24(whole_x, pcm.tpdf_dither(5, 3, 2, k + n))
        assert np.array_equal(pcm.quantize24(x, pcm.tpdf_dither(5, 3, 2, n, first=k)), whole[k:])
    else:                                                                                     # a window of the whole around k
        lo = k - 9
        whole = pcm.quantize24(np.concatenate([np.zeros(9, F32), x]), pcm.tpdf_dither(5, 3, 2, 9 + n, first=lo))
        assert np.array_equal(pcm.quantize24(x, pcm.tpdf_dither(5, 3, 2, n, first=k)), whole[9:])
        assert not np.array_equal(pcm.tpdf_dither(5, 3, 2, n, first=k), pcm.tpdf_dither(5, 3, 2, n, first=k - 2 ** 32))
    # the 24-bit dither of a sample is its 16-bit one
    assert np.array_equal(pcm.tpdf_dither(5, 3, 2, n, first=k), pcm.tpdf_dither(5, 3, 2, n + 1, first=k)[:n])


# ---- keywords ----------------------------------------------------------------------------------------------------------------
class Stub:
    prior = "device"


def open_stub(**kw):
    from flowhigh_amd import FlowHighSR
    return FlowHighSR.stream(Stub(), 12000, **{**dict(window_ms=200, overlap_ms=60, guard_ms=10, seed=5), **kw})


@pytest.mark.parametrize("name", ["s24", "s24in32"])
def test_names_are_accepted_everywhere(name):
    opt = delivery.resolve_delivery(2, pcm=name, dither="tpdf", dither_seed=4, interleaved=True)
    assert opt["pcm"] == name and len(opt["keys"]) == 2 and opt["interleaved"] is True
    assert SD.make_plan(44100, -3.0, name, (9, 0)) == dict(rate=44100, true_peak=-3.0, pcm=name, key=(9, 0))
    assert SD.make_plan(pcm=name, channels=2, interleaved=True)["pcm"] == name
    assert open_stub(pcm=name).pcm == name                                                     # the session's own encoder
    s = open_stub(delivery=dict(pcm=name, dither="tpdf", dither_seed=9), n_channels=2)
    assert s.delivery.plan["pcm"] == name and s.pcm is None
    from flowhigh_amd.delivery_stream import DeliveryStream
    a, b = DeliveryStream(SD.make_plan(pcm=name)), DeliveryStream(SD.make_plan(pcm="int16"))
    assert a.key != b.key                                                                      # formats never share an encode launch
    assert DeliveryStream(SD.make_plan(pcm="s24")).key != DeliveryStream(SD.make_plan(pcm="s24in32")).key
    dtype, size, stem = delivery.PCM_FORMATS[name]
    assert (size, stem) == ((3, "s24") if name == "s24" else (4, "s24"))
    assert delivery.pcm_shape(name, 2, 5) == ((2, 5, 3) if name == "s24" else (2, 5))


@pytest.mark.parametrize("bad", ["int24", "float16", "int8"])
def test_other_names_are_still_refused(bad):
    with pytest.raises(ValueError, match="^pcm must be"):
        delivery.resolve_delivery(1, pcm=bad)
    with pytest.raises(ValueError, match="^pcm must be"):
        SD.make_plan(pcm=bad)
    with pytest.raises(ValueError, match="^pcm must be"):
        open_stub(pcm=bad)
    with pytest.raises(ValueError, match="^pcm must be"):
        open_stub(delivery=dict(pcm=bad))


def test_dither_still_goes_with_pcm():
    with pytest.raises(ValueError, match="dither= goes with pcm="):
        delivery.resolve_delivery(1, dither="tpdf")
    with pytest.raises(ValueError, match="interleaved=True goes with pcm="):
        delivery.resolve_delivery(1, interleaved=True)
    with pytest.raises(ValueError, match="two encoders"):
        open_stub(delivery=dict(pcm="s24"), pcm="s24")
    assert delivery.resolve_delivery(1) is None


# ---- the stream restatement ----------------------------------------------------------------------------------------------------
CUTS = [0, 1, 8, 16, 25, 25, 32, 33, 300, 1000]          # block sizes 0, 1, 7, 8, 9, 0, 7, 1, 267, 700


@pytest.mark.parametrize("name", ["s24", "s24in32"])
@pytest.mark.parametrize("C", [1, 3])
def test_stream_restatement_equals_one_shot(name, C):
    assert {b - a for a, b in zip([0] + CUTS, CUTS)} >= {0, 1, 7, 8, 9}
    x = (0.9 * np.random.default_rng(C).uniform(-1, 1, (C, 1000))).astype(F32)
    x[:, :EDGES.size] = EDGES
    packed = name == "s24"
    plan = SD.make_plan(pcm=name, key=KEY, channels=C, interleaved=True)
    got = SD.chunked(x, CUTS, plan)
    want = pcm.encode24(x, KEY, True, packed)
    assert got.dtype == want.dtype and got.shape == want.shape == ((1000, C, 3) if packed else (1000, C))
    assert np.array_equal(got, want) and np.array_equal(SD.whole(x, plan), want)
    planar = SD.chunked(x, CUTS, SD.make_plan(pcm=name, key=KEY, channels=C))
    assert np.array_equal(planar, pcm.encode24(x, KEY, False, packed))
    if C == 1:                                                                                # the mono stream it always was: [T] in
        mono = SD.chunked(x[0], CUTS, SD.make_plan(pcm=name, key=KEY))
        assert np.array_equal(mono, pcm.encode24(x, KEY, False, packed)[0])
        assert np.array_equal(SD.whole(x[0], SD.make_plan(pcm=name, key=KEY)), mono)
    # behind the resampler and the limiter, at a first index past 2^32
    first = 2 ** 32 + 3
    d = np.stack([pcm.tpdf_dither(KEY[0], KEY[1], c, 1000, first=first) for c in range(C)])
    q = pcm.quantize24(x, d)
    assert np.array_equal(SD.chunked(x, CUTS, SD.make_plan(pcm=name, key=KEY, channels=C), first=first), pcm.pack24(q) if packed else q)


def test_stream_restatement_behind_the_other_stages():
    x = (0.9 * np.random.default_rng(8).uniform(-1, 1, (2, 3000))).astype(F32)
    plan = SD.make_plan(8000, -6.0, "s24", KEY, 2, True)
    got = SD.chunked(x, [1, 7, 300, 301, 1500, 2222, 3000], plan)
    assert got.dtype == np.uint8 and got.shape[1:] == (2, 3) and np.array_equal(got, SD.whole(x, plan))


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_header_and_bindings():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    for name, n_params in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/flowhigh_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert name in hip.EXPORTS and len(hip._SIGS[name]) == len(params) == n_params, name
        for p, ctype in zip(params, hip._SIGS[name]):
            assert ctype is (hip._P if "*" in p else hip._I), (name, p)
        assert params[-2] == "int container" and params[-3] == "int interleaved", name
    assert ctypes.sizeof(hip.PcmClip) == 32 and re.search(r"int16_t\* dst;", header)          # the struct did not change
    csrc = ROOT / "flowhigh_amd" / "csrc"
    common = (csrc / "pcm_common.h").read_text()
    # the samples, the stores and the four encoder bodies are stated once, in the header; the kernels of both files only call them
    for text in ("encode(", "encode24(", "__dmul_rn", "__dadd_rn", "store_run24(", "void encode_row(", "void encode_frames(",
                 "void encode_scattered(", "void encode_flat("):
        assert common.count(text) >= 1, text
    for src in ("pcm.hip", "stream_delivery.hip"):
        text = (csrc / src).read_text()
        for word in ("__dmul_rn", "rintf(", "encode24(", "encode(", "store_run", "philox4x32", "dither_"):
            assert word not in text, (src, word)
        assert '#include "pcm_common.h"' in text and "encode_row(" in text and "encode_interleaved(" in text, src
