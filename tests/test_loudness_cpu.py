"""CPU: the definition of loudness (flowhigh_amd/loudness.py: ITU-R BS.1770-4 in numpy float64) against the Recommendation's
table and anchor and the EBU Tech 3341 tone sequences, its gates and gain on planted numbers, the chunked evaluation of the
recurrence the kernels use, the loudness= keyword's resolution and errors, the entries of csrc/loudness.hip in header / EXPORTS /
_SIGS with their argument checks, and the batching server with a stub model."""
import ctypes
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.signal
import torch

from flowhigh_amd import delivery, hip, loudness
from flowhigh_amd.flowhighsr import FlowHighSR

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"fh_loudness_span_len": 0, "fh_kweight_energy_f32": 7, "fh_kweight_energy_seg_f32": 9, "fh_loudness_gate_f32": 12}


def tone(db, seconds, rate=48000, f=1000.0, start=0):
    n = np.arange(start, start + int(round(seconds * rate)))
    return 10.0 ** (db / 20.0) * np.sin(2 * np.pi * f * n / rate)


# ---- the filter -----------------------------------------------------------------------------------------------------------------
def test_k_weighting_at_48k_is_the_recommendation_s_table():
    (b, a), (d, c) = loudness.k_weighting(48000)
    assert np.abs(b - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() <= 1e-12
    assert np.abs(a - [1.0, -1.69065929318241, 0.73248077421585]).max() <= 1e-12
    assert np.array_equal(d, [1.0, -2.0, 1.0])
    assert np.abs(c - [1.0, -1.99004745483398, 0.99007225036621]).max() <= 1e-12
    assert loudness.coefficients(48000) == [*b, a[1], a[2], *d, c[1], c[2]]
    # re-designed for another rate (bilinear, pre-warped at f0): the shelf is 0 dB at DC and +4 dB at Nyquist, the high-pass has
    # its double zero at DC, at every rate
    for rate in (8000, 11025, 44100, 96000):
        (b2, a2), (d2, c2) = loudness.k_weighting(rate)
        assert a2[0] == c2[0] == 1.0 and not np.allclose(b2, b) and np.array_equal(d2, [1.0, -2.0, 1.0])
        assert abs(b2.sum() / a2.sum() - 1.0) <= 1e-9
        assert abs(20 * math.log10((b2[0] - b2[1] + b2[2]) / (a2[0] - a2[1] + a2[2])) - loudness.SHELF["gain_db"]) <= 1e-9
        assert np.abs(np.roots(a2)).max() < 1.0 and np.abs(np.roots(c2)).max() < 1.0
    assert loudness.geometry(48000) == (4800, 19200) and loudness.geometry(44100) == (4410, 17640)
    assert loudness.geometry(22050) == (2205, 8820) and loudness.geometry(11025) == (1103, 4412) and loudness.geometry(8000) == (800, 3200)
    for bad in (0, -1, 44100.5, "48000", True, 154):
        with pytest.raises(ValueError):
            loudness.geometry(bad)


def test_the_chunked_recurrence_is_lfilter():
    """Zero-state chunks plus the A^L hand-over, in float64, against scipy.signal.lfilter: 1e-9 (two float64 orderings of this
    filter differ by about 1e-12); the state-space form against the two biquads' transposed form."""
    for rate, T, chunk in ((48000, 9001, 16), (44100, 5000, 16), (8000, 4097, 7), (11025, 333, 64)):
        x = (torch.randn(T, generator=torch.Generator().manual_seed(rate)) * 0.3).numpy()
        (b1, a1), (b2, a2) = loudness.k_weighting(rate)
        ref = scipy.signal.lfilter(b2, a2, scipy.signal.lfilter(b1, a1, x.astype(np.float64)))
        assert np.array_equal(loudness.k_weight(x, rate), ref)
        got = loudness.k_weight_chunked(x, rate, chunk)
        err = float(np.abs(got - ref).max())
        print(f"loudness: chunked recurrence rate {rate} chunk {chunk}: max-abs {err:.2e}")
        assert got.shape == ref.shape and err <= 1e-9
    # a low-frequency-heavy row, where a float32 recursion is off by 5e-4 of a sub-block's energy
    x = 0.5 * np.sin(2 * np.pi * 20.0 * np.arange(24000) / 48000)
    e_ref = loudness.sub_energies(loudness.k_weight(x, 48000), 48000)
    e_got = loudness.sub_energies(loudness.k_weight_chunked(x, 48000, 16), 48000)
    assert float((np.abs(e_got - e_ref) / e_ref).max()) <= 1e-9


def test_sub_and_block_energies_follow_the_geometry():
    rate, hop, block = 8000, 800, 3200
    y = np.arange(1, 2 * hop + 4, dtype=np.float64)[None] / 1000
    e = loudness.sub_energies(y, rate)
    assert e.shape == (1, 3)
    assert np.allclose(e[0], [(y[0, :hop] ** 2).sum(), (y[0, hop:2 * hop] ** 2).sum(), (y[0, 2 * hop:] ** 2).sum()], rtol=1e-14, atol=0)
    assert loudness.sub_energies(np.ones(hop), rate).tolist() == [hop] and loudness.sub_energies(np.ones(hop + 1), rate).tolist() == [hop, 1]
    # a clip shorter than one block is one block of its whole length
    z = loudness.block_energies(e, 2 * hop + 3, rate)
    assert z.shape == (1,) and z[0] == e.sum() / (2 * hop + 3)
    # blocks at 75 % overlap over all channels, weights 1
    e = np.arange(12, dtype=np.float64).reshape(2, 6) + 1
    z = loudness.block_energies(e, 6 * hop, rate)
    assert z.tolist() == [(1 + 2 + 3 + 4 + 7 + 8 + 9 + 10) / block, (2 + 3 + 4 + 5 + 8 + 9 + 10 + 11) / block, (3 + 4 + 5 + 6 + 9 + 10 + 11 + 12) / block]
    assert loudness.block_energies(e, 6 * hop - 1, rate).shape == (2,) and loudness.block_energies(e[:, :4], block, rate).shape == (1,)
    with pytest.raises(ValueError):
        loudness.block_energies(e, 7 * hop, rate)


# ---- the meter ------------------------------------------------------------------------------------------------------------------
def test_a_997_hz_sine_at_full_scale_reads_minus_3_01():
    L = loudness.integrated(tone(0.0, 3.0, f=997.0), 48000)
    print(f"loudness: 997 Hz 0 dBFS mono: {L:.4f} LUFS")
    assert abs(L + 3.01) <= 0.01


def _sequence(parts):
    rows, start = [], 0
    for db, seconds in parts:
        rows.append(tone(db, seconds, start=start))
        start += len(rows[-1])
    x = np.concatenate(rows)
    return np.stack([x, x])


@pytest.mark.parametrize("parts,want", [
    ([(-23.0, 20.0)], -23.0),
    ([(-33.0, 20.0)], -33.0),
    ([(-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0)], -23.0),
    ([(-72.0, 10.0), (-36.0, 10.0), (-23.0, 60.0), (-36.0, 10.0), (-72.0, 10.0)], -23.0),
    ([(-26.0, 20.0), (-20.0, 20.1), (-26.0, 20.0)], -23.0),
])
def test_the_ebu_tech_3341_tone_sequences(parts, want):
    """Stereo 1 kHz sequences of EBU Tech 3341 (cases 1 to 5), within the Tech Doc's own meter tolerance of 0.1 LU."""
    L = loudness.integrated(_sequence(parts), 48000)
    print(f"loudness: Tech 3341 {parts}: {L:.3f} LUFS")
    assert abs(L - want) <= 0.1


def test_both_gates_are_strict_and_silence_reads_minus_infinity():
    ZA = loudness.ZA
    assert ZA == 10.0 ** ((-70.0 + 0.691) / 10.0) and float.hex(ZA) == "0x1.f791ec6e1d5b7p-24"      # (the kernel holds these bits)
    up = np.nextafter(ZA, 1.0)
    L, mask = loudness.gate([ZA, 0.0, ZA])
    assert L == -math.inf and not mask.any()                      # a block exactly at ZA is out
    L, mask = loudness.gate([ZA, up, 0.0])
    assert mask.tolist() == [False, True, False] and abs(L + 70.0) < 1e-9
    # the relative gate: 0.1 of the mean of the absolute-gate passers, strictly above
    L, mask = loudness.gate([1.0, 1.0, 0.25, 0.0])               # mean 0.75 -> threshold 0.075
    assert mask.tolist() == [True, True, True, False] and L == -0.691 + 10 * math.log10(0.75)
    z = np.array([8.0, 1.0, 1.0, 0.0])                            # passers' mean 10 / 3; a block AT 0.1 of it is out
    z[1] = 0.1 * z[[0, 1, 2]].mean()
    for _ in range(60):                                           # (the fixed point of z1 = 0.1 mean(8, z1, 1))
        z[1] = 0.1 * z[[0, 1, 2]].mean()
    thr = 0.1 * z[:3].mean()
    assert z[1] == thr
    L, mask = loudness.gate(z)
    assert mask.tolist() == [True, False, True, False] and L == -0.691 + 10 * math.log10(4.5)
    assert loudness.gate(np.zeros(5))[0] == -math.inf and loudness.gate(np.zeros(0))[0] == -math.inf
    assert loudness.gate([np.nan, np.nan])[0] == -math.inf
    # all-silent and NaN input: -inf and gain 1
    assert loudness.integrated(np.zeros((2, 30000)), 48000) == -math.inf
    y, g, L = loudness.normalise(np.zeros((2, 30000), dtype=np.float32), 48000, -23.0)
    assert g == 1.0 and L == -math.inf and not y.any()
    x = np.full((1, 30000), np.nan, dtype=np.float32)
    y, g, L = loudness.normalise(x, 48000, -23.0)
    assert g == 1.0 and L == -math.inf
    assert loudness.integrated(np.zeros((1, 0)), 48000) == -math.inf


def test_the_gain_rule_and_its_cap_on_worked_numbers():
    f = np.float32
    assert loudness.gain(-23.0, -23.0, 0.5) == f(1.0)
    assert loudness.gain(-43.0, -23.0, 0.05) == f(10.0)                          # +20 dB, cap at 19.8 not reached
    assert loudness.gain(-43.0, -23.0, 0.099) == f(10.0) and loudness.gain(-43.0, -23.0, 0.1) == f(0.99 / 0.1)      # 9.9: the cap
    assert loudness.gain(-3.0, -23.0, 0.99) == f(0.1)                            # attenuation is never capped
    assert loudness.gain(-29.0, -23.0, 0.25) == f(10.0 ** 0.3)
    assert loudness.gain(-23.0, 0.0, 0.5) == f(1.98)
    assert loudness.gain(-math.inf, -23.0, 0.5) == f(1.0) and loudness.gain(math.nan, -23.0, 0.5) == f(1.0)
    assert loudness.gain(-30.0, -23.0, 0.0) == f(1.0) and loudness.gain(-30.0, -23.0, math.nan) == f(1.0)
    assert loudness.gain(-30.0, math.nan, 0.5) == f(1.0)                          # no target: measure only
    assert loudness.gain(-30.0, -23.0, 0.1).dtype == np.float32
    # the gain is a function of the float32 loudness that is reported
    L = -21.476840186475837
    assert loudness.gain(L, -23.0, 0.1) == loudness.gain(float(f(L)), -23.0, 0.1) == f(10.0 ** ((-23.0 - float(f(L))) / 20.0))
    # normalise: a -20 dBFS tone to -23 LUFS; then to 0 LUFS, where the cap binds
    x = tone(-20.0, 2.0)[None].astype(np.float32)
    y, g, L = loudness.normalise(x, 48000, -23.0)
    assert y.dtype == np.float32 and np.array_equal(y, (x * g).astype(np.float32))
    assert abs(loudness.integrated(y, 48000) + 23.0) <= 1e-4
    y, g, L = loudness.normalise(x, 48000, 0.0)
    assert g == f(0.99 / float(np.abs(x).max())) and abs(float(np.abs(y).max()) - 0.99) <= 2.0 ** -23


# ---- the keyword ----------------------------------------------------------------------------------------------------------------
def test_resolve_delivery_takes_loudness_and_leaves_the_other_results_as_they_were():
    rd = delivery.resolve_delivery
    assert rd(3) is None and rd(3, loudness=None) is None
    assert rd(2, 44100) == dict(rate=44100, pcm=None, keys=None, interleaved=False)                # no "loudness" key without the keyword
    assert rd(2, loudness=-16) == dict(rate=None, pcm=None, keys=None, interleaved=False, loudness=-16.0)
    assert rd(2, 44100, "int16", loudness=np.float32(-23.0))["loudness"] == -23.0
    assert rd(1, loudness=0)["loudness"] == 0.0 and rd(1, loudness=-70.0)["loudness"] == -70.0
    assert isinstance(rd(1, loudness=-16)["loudness"], float)
    for bad in (1, 0.001, -70.5, math.nan, math.inf, -math.inf, "-16", True, [-16.0], (-16.0,)):
        with pytest.raises(ValueError, match="loudness must be"):
            rd(1, loudness=bad)
    with pytest.raises(ValueError, match="two rules for one gain"):
        rd(1, loudness=-16.0, level="input")
    assert rd(1, loudness=-16.0, level="peak")["loudness"] == -16.0
    assert loudness.resolve_loudness(None) is None


def test_the_public_entries_have_the_keyword_and_refuse_before_any_gpu_work():
    from flowhigh_amd.serve import BatchingServer
    for fn in (FlowHighSR.generate, FlowHighSR.generate_batch, FlowHighSR.generate_many, BatchingServer.submit):
        p = inspect.signature(fn).parameters["loudness"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    for fn in (FlowHighSR.generate_from_device, FlowHighSR.capture, FlowHighSR.sample, FlowHighSR.sample_many):
        assert "loudness" not in inspect.signature(fn).parameters, fn
    assert list(inspect.signature(FlowHighSR.measure_loudness).parameters) == ["self", "rows", "chans", "rate"]
    assert inspect.signature(FlowHighSR.measure_loudness).parameters["rate"].default == 48000
    m = FlowHighSR.__new__(FlowHighSR)                               # no device, no library: anything past the checks would raise
    m.flowhigh = type("F", (), {"device": torch.device("cpu")})()
    m.prior = "reference"
    x = np.linspace(-0.5, 0.5, 50, dtype=np.float32)
    for kw, say in ((dict(loudness=1.0), "loudness must be"), (dict(loudness=-71), "loudness must be"),
                    (dict(loudness=math.nan), "loudness must be"), (dict(loudness="loud"), "loudness must be"),
                    (dict(loudness=-16.0, level="input"), "two rules for one gain"),
                    (dict(loudness=-16.0, level="lufs"), "level must be"), (dict(level="lufs"), "level must be"),
                    (dict(loudness=-16.0, dither="tpdf"), "goes with pcm"), (dict(loudness=-16.0, output_rate=44101), "640")):
        with pytest.raises(ValueError, match=say):
            m.generate(x, 12000, **kw)
        with pytest.raises(ValueError, match=say):
            m.generate_batch([x, x], 12000, **kw)
        with pytest.raises(ValueError, match=say):
            m.generate_many([x, x[:40]], 12000, **kw)
    with pytest.raises(ValueError, match="return_stages"):
        m.generate_batch([x], 12000, loudness=-16.0, return_stages=True)


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
            want = hip._P if "*" in p else (hip._D if p.startswith("double") else hip._I)
            assert ctype is want, (name, p)
    build = __import__("flowhigh_amd.build", fromlist=["SOURCES"])
    assert "loudness.hip" in build.SOURCES
    text = (ROOT / "flowhigh_amd" / "csrc" / "loudness.hip").read_text()
    assert float.hex(loudness.ZA) in text                            # the absolute gate, bit for bit


def test_the_entries_check_their_arguments():
    """The checks run on the host before anything is launched: the device pointers are fake addresses, never read."""
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    coef = (ctypes.c_double * 10)(*loudness.coefficients(48000))
    A, B, E, K = 256, 512, 1024, ctypes.addressof(coef)
    assert L.fh_loudness_span_len() == 4096
    bad = [("fh_kweight_energy_f32", a) for a in ((0, K, E, 1, 8, 4800), (A, 0, E, 1, 8, 4800), (A, K, 0, 1, 8, 4800),
                                                  (A, K, E, 0, 8, 4800), (A, K, E, 65536, 8, 4800), (A, K, E, 1, 0, 4800),
                                                  (A, K, E, 1, 8, 15), (A + 2, K, E, 1, 8, 4800), (A, K, E + 4, 1, 8, 4800))]
    bad += [("fh_kweight_energy_seg_f32", a) for a in ((0, B, 1, 1, 8, K, E, 4800), (A, 0, 1, 1, 8, K, E, 4800),
                                                      (A, B, 0, 1, 8, K, E, 4800), (A, B, 2, 1, 8, K, E, 4800),
                                                      (A, B, 1, 65536, 8, K, E, 4800), (A, B, 1, 1, 0, K, E, 4800),
                                                      (A, B, 1, 1, 8, 0, E, 4800), (A, B, 1, 1, 8, K, 0, 4800),
                                                      (A, B, 1, 1, 8, K, E, 15))]
    for name, args in bad:
        assert getattr(L, name)(*args, 0) == -1, (name, args)
        assert name.encode() in L.fh_last_error(), (name, args)
    nan_coef = (ctypes.c_double * 10)(*([math.nan] + loudness.coefficients(48000)[1:]))
    assert L.fh_kweight_energy_f32(A, ctypes.addressof(nan_coef), E, 1, 8, 4800, 0) == -1 and b"not finite" in L.fh_last_error()
    good = (E, 3, A, B, 1, 1, 4800, -23.0, A, B, A, 0)
    for i, v in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 2), (6, 15), (7, 1.0), (7, -71.0), (7, math.inf), (8, 0), (9, 0), (10, 0)):
        args = list(good)
        args[i] = v
        assert L.fh_loudness_gate_f32(*args) == -1, args
        assert b"fh_loudness_gate_f32" in L.fh_last_error(), args


# ---- the serving front ----------------------------------------------------------------------------------------------------------
class _Stub:
    """A model whose generate_many has no loudness keyword unless it is handed one: records what it was called with."""

    def __init__(self):
        self.calls = []

    def generate_many(self, clips, sr, target, steps, noise=None, max_batch=64, **kw):
        self.calls.append(dict(n=len(clips), **kw))
        return [torch.from_numpy(np.repeat(np.asarray(c, dtype=np.float32).reshape(1, -1), 4, axis=1)) for c in clips]


def test_batching_server_groups_by_loudness_and_hands_it_on_only_when_given():
    from flowhigh_amd.serve import BatchingServer
    m = _Stub()
    mono = np.linspace(-1, 1, 100, dtype=np.float32)
    srv = BatchingServer(m, max_batch=8, max_wait_ms=30000)
    try:
        futs = [srv.submit(mono, 12000, loudness=-16.0), srv.submit(mono[:60], 12000, loudness=-23.0), srv.submit(mono, 12000),
                srv.submit(mono[:70], 12000, loudness=-16), srv.submit(mono, 12000, loudness=None),
                srv.submit(mono, 12000, loudness=-16.0, output_rate=44100), srv.submit(mono, 12000, output_rate=44100),
                srv.submit(mono, 12000, loudness=-23.0)]
        got = [f.result(timeout=30) for f in futs]
        assert all(g.dtype == np.float32 for g in got)
        calls = sorted(((c["n"], c.get("loudness"), c.get("output_rate")) for c in m.calls), key=str)
        assert calls == sorted([(2, -16.0, None), (2, -23.0, None), (2, None, None), (1, -16.0, 44100), (1, None, 44100)], key=str)
        assert all(("loudness" in c) == (c.get("loudness") is not None) for c in m.calls)          # never passed as None
        for kw in (dict(loudness=1.0), dict(loudness="x"), dict(loudness=math.nan), dict(loudness=-16.0, level="input")):
            with pytest.raises(ValueError):
                srv.submit(mono, 12000, **kw)
    finally:
        srv.close()
