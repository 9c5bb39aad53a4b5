"""CPU: flowhigh_amd/quality.py, the numpy float64 definition of the spectral quality report (LSD by band, SNR), on cases whose
figures follow from the definition by hand; the header and hip.EXPORTS carry the new entries at ABI 6; and every input pair
of test_hip_quality.py keeps its bin powers clear of the floor."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import quality_inputs as qi
from flowhigh_amd import quality

ROOT = Path(__file__).resolve().parents[1]
NEW = ("fh_quality_frames_f32", "fh_quality_frames_seg_f32", "fh_quality_report_f32", "fh_sizeof_quality_clip")


def test_geometry_and_fields():
    assert quality.FIELDS == ("lsd", "lsd_low", "lsd_high", "snr_db")
    assert [quality.n_frames(T) for T in (1, 479, 480, 481, 4807)] == [1, 1, 2, 2, 11]
    assert quality.powers(qi.noise(1, 4807)[0]).shape == (11, 1025)
    # a single sample sits at the window's centre, where the periodic Hann window is 1: every bin has its square
    x = np.array([0.25], dtype=np.float32)
    assert np.allclose(quality.powers(x), 0.0625, rtol=1e-14, atol=0.0)


def test_cutoff_bin():
    assert quality.cutoff_bin(None) is None
    assert quality.cutoff_bin(8000, 48000) == 341            # floor(341.33 + 0.5)
    assert quality.cutoff_bin(4000, 48000) == 171            # floor(170.67 + 0.5)
    assert quality.cutoff_bin(24000, 48000) == 1024
    assert quality.cutoff_bin(1e9, 48000) == 1025            # clamped
    assert quality.cutoff_bin(1.0, 48000) == 0
    assert quality.cutoff_bin(12000, 48000) == quality.cutoff_bin(4000, 16000) == 512        # rate is for this conversion only
    for bad in (0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            quality.cutoff_bin(bad)


@pytest.mark.parametrize("T", qi.T_CASES)
def test_identical_rows(T):
    r = qi.noise(2, T)
    assert quality.report(r, r.copy(), kc=341) == (0.0, 0.0, 0.0, math.inf)


@pytest.mark.parametrize("g", [0.5, 2.0, -0.25, 8.0])
def test_a_power_of_two_gain(g):
    for T in (1, 481, 4807):
        e, r = qi.scaled_pair(1, T, g)
        lsd, low, high, snr = quality.report(e, r, kc=341)
        want = 2.0 * abs(math.log10(abs(g)))
        assert max(abs(lsd - want), abs(low - want), abs(high - want)) < 1e-13
        assert abs(snr - -20.0 * math.log10(abs(1.0 - g))) < 1e-12


def test_a_brick_wall_pair():
    """The low band is kept and the high band scaled by 0.01, 40 dB in power: d is 0 below the cutoff and 4 above it, but for
    the window's leakage across the wall -- the main lobe's few bins either side, and the frames at the row's ends, whose zero
    pad is an edge of its own.  Measured: 0.014 and 3.956 at 24000 samples; the bars are 0.05 and 0.1."""
    e, r = qi.brick_wall_pair(1, 24000)
    lsd, low, high, snr = quality.report(e, r, kc=341)
    assert 0.0 < low < 0.05
    assert abs(high - 4.0) < 0.1
    assert low < lsd < high


def test_bands_at_the_ends():
    e, r = qi.noise_pair(1, 2048)
    d2 = quality.log_power_difference(e[0], r[0]) ** 2
    full = float(np.sqrt(d2.mean(axis=1)).mean())
    for kc in (0, 1, 1024, 1025):
        lsd, low, high, _ = quality.report(e, r, kc=kc)
        assert lsd == full
        if kc == 0:
            assert math.isnan(low) and high == full
        elif kc == 1025:
            assert math.isnan(high) and low == full
        else:
            assert abs(low - float(np.sqrt(d2[:, :kc].mean(axis=1)).mean())) < 1e-15
            assert abs(high - float(np.sqrt(d2[:, kc:].mean(axis=1)).mean())) < 1e-15
    lsd, low, high, _ = quality.report(e, r)                 # no cutoff
    assert lsd == full and math.isnan(low) and math.isnan(high)
    assert quality.report(e, r, cutoff_hz=8000, rate=48000) == quality.report(e, r, kc=341)
    with pytest.raises(ValueError):
        quality.report(e, r, kc=1026)


def test_silence():
    z = np.zeros((1, 1000), dtype=np.float32)
    r = qi.noise(1, 1000)
    lsd, low, high, snr = quality.report(z, z, kc=341)
    assert (lsd, low, high) == (0.0, 0.0, 0.0) and math.isnan(snr)            # 0 / 0
    assert quality.report(r, z, kc=341)[3] == -math.inf                          # a silent reference
    # a silent estimate: every bin of it at the floor, snr 0 dB
    lsd, _, _, snr = quality.report(z, r, kc=341)
    P = quality.powers(r[0])
    assert abs(lsd - float(np.sqrt(((np.log10(P) + 8.0) ** 2).mean(axis=1)).mean())) < 1e-13 and snr == 0.0


def test_two_channels_are_the_mean_over_rows_and_the_pooled_snr():
    e, r = qi.noise_pair(2, 4807)
    e[1] *= np.float32(0.125)
    both = quality.report(e, r, kc=341)
    one = [quality.report(e[c], r[c], kc=341) for c in range(2)]
    for k in range(3):                                       # (equal frame counts: the mean over all frames is the mean of the rows')
        assert abs(both[k] - 0.5 * (one[0][k] + one[1][k])) < 1e-14
    sig = (r.astype(np.float64) ** 2).sum()
    err = ((r.astype(np.float64) - e.astype(np.float64)) ** 2).sum()
    assert abs(both[3] - 10.0 * math.log10(sig / err)) < 1e-12
    assert abs(both[3] - 0.5 * (one[0][3] + one[1][3])) > 0.1                    # pooled, not the mean of the rows' figures


def test_refuses_what_is_not_a_pair():
    r = qi.noise(1, 100)
    for e in (r.astype(np.float64), qi.noise(1, 99), qi.noise(2, 100), np.zeros((1, 0), np.float32)):
        with pytest.raises(ValueError):
            quality.report(e, r)


def test_header_declares_the_entries_at_abi_6():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header)
    for name in NEW:
        assert re.search(rf"\bint {name}\(", header), name
    assert "} fh_quality_clip;" in header


def test_exports_hold_the_entries():
    import ctypes

    from flowhigh_amd import hip
    assert hip.ABI_VERSION == 6
    for name in NEW:
        assert name in hip.EXPORTS and name in hip._SIGS, name
    assert len(hip._SIGS["fh_quality_frames_f32"]) == 9 and len(hip._SIGS["fh_quality_frames_seg_f32"]) == 10
    assert len(hip._SIGS["fh_quality_report_f32"]) == 8
    assert ctypes.sizeof(hip.QualityClip) == 48


def test_argument_errors_are_reported():
    from flowhigh_amd import build, hip
    build.build(verbose=False)
    L = hip.lib()
    assert L.fh_sizeof_quality_clip() == 48
    ok = 256                                                 # (a fake aligned non-null pointer is enough for the argument checks)
    assert L.fh_quality_frames_f32(ok, ok, ok, ok, ok, 1, 0, 341, 0) == -1 and b"len 0" in L.fh_last_error()
    assert L.fh_quality_frames_f32(ok, 0, ok, ok, ok, 1, 10, 341, 0) == -1 and b"null pointer" in L.fh_last_error()
    assert L.fh_quality_frames_f32(ok, ok, ok, 0, ok, 1, 10, 341, 0) == -1 and b"null pointer" in L.fh_last_error()
    for kc in (-2, 1026):
        assert L.fh_quality_frames_f32(ok, ok, ok, ok, ok, 1, 10, kc, 0) == -1 and b"kc" in L.fh_last_error()
    import ctypes
    for clip, what in ((hip.QualityClip(ok, ok, 10, 10, 1, 0, 341, 0), b"len 0"), (hip.QualityClip(ok, 0, 10, 10, 1, 10, 341, 0), b"null"),
                       (hip.QualityClip(ok, ok, 10, 10, 1, 10, 1026, 0), b"kc 1026"), (hip.QualityClip(ok, ok, 10, 10, 1, 10, -2, 0), b"kc -2"),
                       (hip.QualityClip(ok, ok, 10, 10, 1, 11, 0, 0), b"max_len 10")):
        table = (hip.QualityClip * 1)(clip)
        assert L.fh_quality_frames_seg_f32(ok, ctypes.addressof(table), ok, 1, 1, 10, ok, ok, ok, 0) == -1
        assert what in L.fh_last_error(), L.fh_last_error()
    assert L.fh_quality_frames_seg_f32(ok, 0, ok, 1, 1, 10, ok, ok, ok, 0) == -1 and b"null pointer" in L.fh_last_error()
    assert L.fh_quality_report_f32(ok, 1, ok, ok, 1, 1, 0, 0) == -1 and b"null pointer" in L.fh_last_error()
    assert L.fh_quality_report_f32(ok, 0, ok, ok, 1, 1, ok, 0) == -1 and b"f_pitch" in L.fh_last_error()


@pytest.mark.parametrize("name", list(qi.MAKERS))
def test_gpu_inputs_are_clear_of_the_floor(name):
    """What test_hip_quality.py asserts again before it runs a kernel: no bin power of its inputs between 0 and 1e-6."""
    for T in qi.T_CASES:
        e, r = qi.MAKERS[name](8, T)
        assert qi.clear_of_the_floor(e) and qi.clear_of_the_floor(r), (name, T)
