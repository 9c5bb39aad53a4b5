"""CPU: the host side of delivery (output_rate=, pcm=, dither=, dither_seed=, interleaved=): the int16 encoding and its dither as
flowhigh_amd/pcm.py defines them, the keywords' resolution and errors, the delivered length against scipy, the polyphase plans
in the down direction against float64, the entries of csrc/pcm.hip in header / EXPORTS / _SIGS, and the batching server with
stub models."""
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.signal
import torch

import ref_frontend
from flowhigh_amd import delivery, hip, pcm, prior, tables
from flowhigh_amd.flowhighsr import FlowHighSR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"fh_pcm_i16_f32": 8, "fh_pcm_i16_seg_f32": 7, "fh_sizeof_pcm_clip": 0}
KEYS = [(0, 0), (1234567890123, 7), (2 ** 64 - 1, 2 ** 40 + 3)]
LSB = np.float32(2.0 ** -15)
DOWN_RATES = [44100, 32000, 24000, 22050, 16000, 11025, 8000, 96000]
U = 2.0 ** -24


# ---- pcm.py: the encoding ------------------------------------------------------------------------------------------------------
def test_quantize_rounds_ties_to_even_and_saturates():
    f = np.float32
    assert pcm.quantize(f([0.5, 1.5, 2.5, -0.5, -1.5]) * LSB).tolist() == [0, 2, 2, 0, -2]
    assert pcm.quantize(f([1.0, -1.0])).tolist() == [32767, -32768]
    assert pcm.quantize(f([1.5, -1.5, np.inf, -np.inf, np.nan])).tolist() == [32767, -32768, 32767, -32768, 0]
    assert pcm.quantize(f([32767 * LSB, 32766.5 * LSB, 32767.5 * LSB, -32767.5 * LSB])).tolist() == [32767, 32766, 32767, -32768]
    assert pcm.quantize(f([1e-40, -1e-40, 0.0, -0.0])).tolist() == [0, 0, 0, 0]                     # denormals
    assert pcm.quantize(f([[0.25], [-0.25]])).dtype == np.int16 and pcm.quantize(f([[0.25], [-0.25]])).tolist() == [[8192], [-8192]]
    # the dither is added after the scaling, in float32
    assert pcm.quantize(f([0.3 * LSB]), f([0.3])).tolist() == [1] and pcm.quantize(f([0.3 * LSB]), f([0.1])).tolist() == [0]


@pytest.mark.parametrize("key", KEYS)
def test_dither_is_exact_triangular_and_white(key):
    n = 65536
    d = pcm.tpdf_dither(key[0], key[1], 0, n)
    assert d.dtype == np.float32 and d.shape == (n,)
    k = d.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.rint(k)) and np.abs(d).max() < 1.0                    # a multiple of 2^-24 inside (-1, 1)
    mean, var = float(d.astype(np.float64).mean()), float(d.astype(np.float64).var())
    lag1 = float(np.corrcoef(d[:-1], d[1:])[0, 1])
    print(f"delivery: dither key {key}: mean {mean:+.4f} var {var:.4f} lag-1 {lag1:+.4f}")
    assert abs(mean) <= 0.01 and abs(var - 1 / 6) <= 0.005
    x = np.full(n, 0.3, dtype=np.float32) * LSB                                        # 0.3 LSB: lost without dither
    with_d = float(pcm.quantize(x, d).astype(np.float64).mean())
    print(f"delivery: 0.3 LSB constant encodes to a mean of {with_d:.4f} with dither")
    assert abs(with_d - 0.3) <= 0.01 and not pcm.quantize(x).any()


def test_dither_depends_on_key_channel_and_sample_only():
    n, m = 1001, 4096
    for key in KEYS:
        long = pcm.tpdf_dither(key[0], key[1], 3, m)
        assert np.array_equal(pcm.tpdf_dither(key[0], key[1], 3, n), long[:n])            # prefix property, odd n
        assert np.array_equal(pcm.tpdf_dither(key[0], key[1], 3, 1), long[:1])
    base = pcm.tpdf_dither(5, 9, 0, m)
    for other in (pcm.tpdf_dither(5, 9, 1, m), pcm.tpdf_dither(5, 10, 0, m), pcm.tpdf_dither(6, 9, 0, m),
                  pcm.tpdf_dither(5 + 2 ** 32, 9, 0, m), pcm.tpdf_dither(5, 9 + 2 ** 32, 0, m)):
        assert float(np.mean(other == base)) < 0.01
    assert pcm.tpdf_dither(5, 9, 0, 0).shape == (0,)
    # ... and its blocks are not the prior's under the same (seed, stream)
    q = np.arange(m // 2, dtype=np.uint64)
    ctr = np.stack([q, np.zeros_like(q), np.full_like(q, 9), np.zeros_like(q)], -1)
    r = prior.philox4x32_10(ctr, (5, 0))
    ra, rb = pcm.dither_uniforms(5, 9, 0, m)
    assert float(np.mean(ra == (r[:, 0::2].reshape(-1) >> np.uint32(8)))) < 0.01
    assert float(np.mean(rb == (r[:, 1::2].reshape(-1) >> np.uint32(8)))) < 0.01
    # the definition, spelled out for one sample: t = 5 is the odd sample of block 2
    r = prior.philox4x32_10(np.array([[2, 0, 9, 0]], dtype=np.uint64), (5 ^ 0x50434D31, 0 ^ 3))[0]
    want = np.float32((int(r[2]) >> 8) * 2.0 ** -24 - (int(r[3]) >> 8) * 2.0 ** -24)
    assert pcm.tpdf_dither(5, 9, 3, 6)[5] == want


def test_encode_layouts():
    x = (np.arange(14, dtype=np.float32).reshape(2, 7) - 6) / np.float32(16)
    planar = pcm.encode(x)
    assert planar.shape == (2, 7) and planar.dtype == np.int16 and np.array_equal(planar, pcm.quantize(x))
    assert np.array_equal(pcm.encode(x, interleaved=True), planar.T) and pcm.encode(x, interleaved=True).flags["C_CONTIGUOUS"]
    assert pcm.encode(x[0]).shape == (1, 7) and pcm.encode(x[0], interleaved=True).shape == (7, 1)
    d = pcm.encode(x * LSB, key=(3, 1))
    assert np.array_equal(d[1], pcm.quantize(x[1] * LSB, pcm.tpdf_dither(3, 1, 1, 7)))     # channel 1 draws with c = 1
    assert np.array_equal(pcm.encode(x[1] * LSB, key=(3, 1))[0], pcm.quantize(x[1] * LSB, pcm.tpdf_dither(3, 1, 0, 7)))
    with pytest.raises(ValueError):
        pcm.encode(np.zeros((1, 2, 3)))


# ---- keyword resolution --------------------------------------------------------------------------------------------------------
def test_resolve_delivery_defaults_are_none_and_errors_name_the_rule():
    rd = delivery.resolve_delivery
    assert rd(3) is None and rd(3, 48000) is None and rd(1, None, None, None, 5, False) is None
    assert rd(2, 44100) == dict(rate=44100, pcm=None, keys=None, interleaved=False)
    assert rd(2, 48000, "int16") == dict(rate=None, pcm="int16", keys=None, interleaved=False)
    assert rd(2, None, "int16", "tpdf", 7, True) == dict(rate=None, pcm="int16", keys=[(7, 0), (7, 1)], interleaved=True)
    assert rd(2, None, "int16", "tpdf", [4, (5, 6)])["keys"] == [(4, 0), (5, 6)]
    for rate in (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 88200, 96000):
        assert delivery.resolve_output_rate(rate) == rate
    for bad in (44101, 48001, 7, 192001):
        with pytest.raises(ValueError, match="640"):
            delivery.resolve_output_rate(bad)
    for bad in (0, -44100, 44100.5, "44100", True, float("nan")):
        with pytest.raises(ValueError, match="positive integer"):
            delivery.resolve_output_rate(bad)
    for kw, say in ((dict(pcm="int24"), "pcm must be"), (dict(pcm="int16", dither="rpdf"), "dither must be"),
                    (dict(dither="tpdf"), "goes with pcm"), (dict(interleaved=True), "goes with pcm"),
                    (dict(output_rate=44100, dither="tpdf"), "goes with pcm"), (dict(pcm="int16", interleaved="yes"), "bool"),
                    (dict(pcm="int16", dither="tpdf", dither_seed=[1]), "2 clips"),
                    (dict(pcm="int16", dither="tpdf", dither_seed=1.5), "dither_seed")):
        with pytest.raises(ValueError, match=say):
            rd(2, **kw)


@pytest.mark.parametrize("rate", [8000, 11025, 16000, 22050, 32000, 44100, 96000])
def test_delivered_length_is_scipy_s(rate):
    for t48 in (15840, 15841, 33600):
        assert delivery.delivered_len(t48, rate) == len(scipy.signal.resample_poly(np.zeros(t48), rate, 48000)), (rate, t48)
    assert delivery.delivered_len(15840) == delivery.delivered_len(15840, 48000) == 15840


def test_the_public_entries_have_the_keywords_and_refuse_before_any_gpu_work():
    from flowhigh_amd.serve import BatchingServer
    want = dict(output_rate=None, pcm=None, dither=None, dither_seed=0, interleaved=False)
    for fn in (FlowHighSR.generate, FlowHighSR.generate_batch, FlowHighSR.generate_many):
        p = inspect.signature(fn).parameters
        for name, default in want.items():
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (fn, name)
    p = inspect.signature(BatchingServer.submit).parameters
    for name in ("output_rate", "pcm", "dither", "dither_seed"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == want[name]
    p = inspect.signature(BatchingServer.generate).parameters
    assert p["pcm"].kind is p["dither"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (FlowHighSR.generate_from_device, FlowHighSR.capture, FlowHighSR.sample, FlowHighSR.sample_many):
        assert not set(want) & set(inspect.signature(fn).parameters), fn
    m = FlowHighSR.__new__(FlowHighSR)                               # no device, no library: anything past the checks would raise
    m.flowhigh = type("F", (), {"device": torch.device("cpu")})()
    m.prior = "reference"
    x = np.linspace(-0.5, 0.5, 50, dtype=np.float32)
    for kw, say in ((dict(output_rate=44101), "640"), (dict(pcm="float16"), "pcm must be"), (dict(dither="tpdf"), "goes with pcm"),
                    (dict(interleaved=True), "goes with pcm"), (dict(pcm="int16", dither="noise"), "dither must be")):
        with pytest.raises(ValueError, match=say):
            m.generate(x, 12000, **kw)
        with pytest.raises(ValueError, match=say):
            m.generate_batch([x, x], 12000, **kw)
        with pytest.raises(ValueError, match=say):
            m.generate_many([x, x[:40]], 12000, **kw)
    with pytest.raises(ValueError, match="3 clips"):
        m.generate_many([x, x, x], 12000, pcm="int16", dither="tpdf", dither_seed=[1, 2])
    with pytest.raises(ValueError, match="return_stages"):
        m.generate_batch([x], 12000, output_rate=44100, return_stages=True)


# ---- the polyphase plans in the down direction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", DOWN_RATES)
def test_resample_poly_plan_restates_scipy_for_output_rates(rate):
    """scipy.signal.resample_poly(x float32, R, 48000) against the plan's sum in float64 (tests/ref_frontend.resample): within
    (ceil(n_taps / up) + 1) u A, A = sum |x h| -- the bar of the existing resampler test (a chain of at most ceil(n_taps / up)
    fused terms and one to spare), here with the plan's own chain length."""
    taps, pre, up, down = tables.resample_poly_plan(rate, 48000)
    g = math.gcd(rate, 48000)
    assert (up, down) == (rate // g, 48000 // g) and max(up, down) <= 640
    terms = math.ceil(taps.numel() / up) + 1
    worst = 0.0
    for n_in in (1, 2, 19, 601, 4801):
        x = torch.randn(1, n_in, generator=torch.Generator().manual_seed(rate + n_in)) * 0.3
        n_out = tables.resample_out_len(n_in, rate, 48000)
        got = scipy.signal.resample_poly(x[0].numpy(), rate, 48000)
        assert got.dtype == np.float32 and got.shape == (n_out,)
        ref, A = ref_frontend.resample(x, taps, up, down, pre, n_out)
        bar = terms * U * A[0].numpy()
        err = np.abs(got.astype(np.float64) - ref[0].numpy())
        assert float(ref.abs().max()) > 0.0
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), (rate, n_in, float((err - bar).max()))
    print(f"delivery: plan {rate} -> {up}/{down}, {taps.numel()} taps: scipy reaches {worst:.2f} of the bar")


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_header_exports_and_abi_are_consistent():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    for name, n_params in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/flowhigh_hip.h"
        params = [p.strip() for p in m.group(1).split(",") if p.strip() != "void"]
        assert name in hip.EXPORTS and len(hip._SIGS[name]) == len(params) == n_params, name
        for p, ctype in zip(params, hip._SIGS[name]):
            assert ctype is (hip._P if "*" in p else hip._I), (name, p)
    build = __import__("flowhigh_amd.build", fromlist=["SOURCES"])
    assert "pcm.hip" in build.SOURCES and "philox.h" in build.HEADERS
    # fh_pcm_clip as hip.PcmClip lays it out
    m = re.search(r"typedef struct \{([^}]*)\} fh_pcm_clip;", header)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert fields == [f[0] for f in hip.PcmClip._fields_] and __import__("ctypes").sizeof(hip.PcmClip) == 32
    # Philox lives in one header that both users include
    csrc = ROOT / "flowhigh_amd" / "csrc"
    for src in ("prior.hip", "pcm.hip"):
        text = (csrc / src).read_text()
        assert '#include "philox.h"' in text and "PHILOX_M0 =" not in text, src
    assert "PHILOX_M0 = 0xD2511F53u" in (csrc / "philox.h").read_text()


# ---- the serving front ---------------------------------------------------------------------------------------------------------
class _OldStub:
    """A model whose generate_many predates the delivery keywords."""

    def generate_many(self, clips, sr, target, steps, noise=None, max_batch=64):
        return [torch.from_numpy(np.repeat(np.asarray(c, dtype=np.float32).reshape(1, -1), 4, axis=1)) for c in clips]


class _Stub:
    """A model with the keywords: records them, returns what they ask for in shape and dtype."""

    def __init__(self):
        self.calls = []

    def generate_many(self, clips, sr, target, steps, noise=None, max_batch=64, channels=None, level="peak", output_rate=None,
                      pcm=None, dither=None, dither_seed=0, interleaved=False):
        from flowhigh_amd.flowhighsr import resolve_channels
        planar = [resolve_channels(c, channels) for c in clips]
        self.calls.append(dict(n=len(clips), output_rate=output_rate, pcm=pcm, dither=dither, dither_seed=dither_seed,
                               interleaved=interleaved, channels=channels))
        outs = []
        for p in planar:
            t = delivery.delivered_len(4 * p.shape[1], output_rate)
            y = torch.arange(p.shape[0] * t, dtype=torch.float32).view(p.shape[0], t)
            if pcm:
                y = y.to(torch.int16)
                if interleaved:
                    y = y.t().contiguous()
            outs.append(y)
        return outs


def test_batching_server_hands_the_delivery_keywords_on_and_groups_by_them():
    from flowhigh_amd.serve import BatchingServer
    m = _Stub()
    mono = np.linspace(-1, 1, 100, dtype=np.float32)
    up = (np.arange(240).reshape(120, 2) % 11 - 5).astype(np.int16)
    srv = BatchingServer(m, max_batch=8, max_wait_ms=20)
    try:
        sr, y = srv.generate((12000, mono), 44100, 1)
        assert sr == 44100 and y.dtype == np.float32 and y.shape == (delivery.delivered_len(400, 44100),)
        assert m.calls[-1]["output_rate"] == 44100 and m.calls[-1]["pcm"] is None
        sr, y = srv.generate((12000, mono), 44100, 1, pcm="int16", dither="tpdf")
        assert sr == 44100 and y.dtype == np.int16 and y.shape == (368,)
        assert m.calls[-1]["pcm"] == "int16" and m.calls[-1]["dither"] == "tpdf" and m.calls[-1]["dither_seed"] == [0]
        sr, y = srv.generate((12000, up), 48000, 1, pcm="int16")                          # [T, C] from the device: no host transpose
        assert sr == 48000 and y.dtype == np.int16 and y.shape == (480, 2) and m.calls[-1]["interleaved"] is True
        assert np.array_equal(y, np.arange(960).reshape(2, 480).T) and m.calls[-1]["output_rate"] is None
        sr, y = srv.generate((12000, up), 48000, 1)                                       # the float path: as it was
        assert y.dtype == np.float32 and y.shape == (480, 2) and m.calls[-1]["pcm"] is None
        n = len(m.calls)
        sr, y = srv.generate((12000, mono), 48000, 1)                                     # every default: no keyword is passed
        assert y.shape == (400,) and m.calls[n] == dict(n=1, output_rate=None, pcm=None, dither=None, dither_seed=0,
                                                        interleaved=False, channels=None)
        y = srv.submit(mono, 12000, pcm="int16", dither="tpdf", dither_seed=(3, 4)).result(timeout=30)
        assert y.dtype == np.int16 and y.shape == (400,) and m.calls[-1]["dither_seed"] == [(3, 4)]
        y = srv.submit(up, 12000, channels="last", pcm="int16").result(timeout=30)
        assert y.shape == (480, 2)
        y = srv.submit(up.T, 12000, channels="first", pcm="int16", output_rate=16000).result(timeout=30)
        assert y.shape == (2, 160) and m.calls[-1]["interleaved"] is False
        # one window, three deliveries: three calls
        group = BatchingServer(m, max_batch=4, max_wait_ms=30000)
        n = len(m.calls)
        futs = [group.submit(mono, 12000, output_rate=44100), group.submit(mono[:60], 12000, output_rate=44100, dither_seed=9),
                group.submit(mono, 12000, pcm="int16"), group.submit(mono, 12000)]
        got = [f.result(timeout=30) for f in futs]
        group.close()
        assert sorted(((c["n"], c["output_rate"], c["pcm"]) for c in m.calls[n:]), key=str) == [(1, None, "int16"), (1, None, None), (2, 44100, None)]
        assert [g.dtype for g in got] == [np.float32, np.float32, np.int16, np.float32]
        for kw in (dict(output_rate=44101), dict(pcm="int8"), dict(dither="tpdf"), dict(pcm="int16", dither="x"),
                   dict(pcm="int16", dither="tpdf", dither_seed=(1, 2, 3)), dict(output_rate=-1)):
            with pytest.raises(ValueError):
                srv.submit(mono, 12000, **kw)
    finally:
        srv.close()
    old = BatchingServer(_OldStub(), max_batch=2, max_wait_ms=5)
    try:
        with pytest.raises(NotImplementedError, match="fixed at 48 kHz"):
            old.generate((12000, mono), 44100, 1)
        sr, y = old.generate((12000, mono), 48000, 1)
        assert sr == 48000 and y.shape == (400,)
    finally:
        old.close()
