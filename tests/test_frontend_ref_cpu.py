"""CPU: the float64 references of the front / back end kernels (tests/ref_frontend.py) against torch.stft, torch.istft, scipy and
the oracle, so that the references do not hang on the code they judge; and the argument checks of the two batched entries, which
run on the host before anything is launched."""
import math

import numpy as np
import pytest
import scipy.signal
import torch

import ref_frontend as rf
from flowhigh_amd import hip, tables
from oracle import ref_cpu

N_FFT, HOP = 2048, 480


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def test_p_layout_helpers_follow_the_rule_and_round_trip():
    re, im = rnd(3, 1025, seed=1), rnd(3, 1025, seed=2)
    p = rf.p_pack(re, im, fill=float("nan"))
    assert p.shape == (3, 2112) and int(torch.isnan(p).sum()) == 3 * 62
    for f in (0, 1, 31, 32, 33, 1023, 1024):                            # 32 Re then 32 Im of bins 32 b .. 32 b + 31
        assert torch.equal(p[:, (f // 32) * 64 + f % 32], re[:, f]) and torch.equal(p[:, (f // 32) * 64 + 32 + f % 32], im[:, f])
    r2, i2, pad = rf.p_unpack(p)
    assert torch.equal(r2, re) and torch.equal(i2, im) and pad.shape == (3, 62) and torch.isnan(pad).all()
    cre, cim = tables._p_index()                                        # (the project's own table says the same)
    assert np.array_equal(cre, rf.p_columns()[0][:1025].numpy()) and np.array_equal(cim, rf.p_columns()[1][:1025].numpy())


@pytest.mark.parametrize("mode, pad, T, rows", [(0, 784, 785, 1), (0, 784, 1264, 2), (0, 784, 2401, 5),
                                                (1, 1024, 1, 1), (1, 1024, 480, 2), (1, 1024, 2401, 6)])
def test_frame_and_rfft_are_torch_stft(mode, pad, T, rows):
    """frame + rfft = torch.stft(float64, center=False) of the padded signal, with the fp32 hann upcast; the zero-pad mode also
    against the oracle's stft_center (its window is the float64 hann).  Bound: 1e-12 * sum |x|."""
    x = rnd(2, T, seed=10 + T).double()
    bound = 1e-12 * float(x.abs().sum(-1).max())
    for w in (tables.hann_window().double(), torch.hann_window(N_FFT, dtype=torch.float64)):
        got = rf.rfft(rf.frame(x, w, rows, N_FFT, HOP, pad, mode).reshape(-1, N_FFT)).view(2, rows, 1025)
        xp = torch.nn.functional.pad(x[:, None], (pad, pad), mode="reflect" if mode == 0 else "constant")[:, 0]
        ref = torch.stft(xp, N_FFT, hop_length=HOP, win_length=N_FFT, window=w, center=False, onesided=True, return_complex=True)
        assert ref.shape[-1] >= rows
        assert (got - ref[:, :, :rows].transpose(1, 2)).abs().max().item() <= bound
    if mode == 1:
        ref = ref_cpu.stft_center(x)
        assert ref.shape[-1] == rows and (got - ref.transpose(1, 2)).abs().max().item() <= bound


def test_rfft_of_unit_impulses_is_the_closed_form():
    n0 = [0, 1, 2, 1023, 1024, 1025, 2047]
    x = torch.zeros(len(n0), N_FFT)
    x[torch.arange(len(n0)), n0] = 1.0
    k = torch.arange(1025, dtype=torch.float64)
    ang = -2.0 * math.pi * ((k[None, :] * torch.tensor(n0, dtype=torch.float64)[:, None]) % N_FFT) / N_FFT
    assert (rf.rfft(x) - torch.complex(torch.cos(ang), torch.sin(ang))).abs().max().item() <= 1e-14


def test_irfft_ignores_the_imaginary_parts_of_dc_and_nyquist():
    spec = torch.complex(rnd(2, 1025, seed=20).double(), rnd(2, 1025, seed=21).double())
    clean = spec.clone()
    clean[:, 0], clean[:, -1] = spec[:, 0].real + 0j, spec[:, -1].real + 0j
    assert torch.equal(rf.irfft(spec), rf.irfft(clean))
    assert (rf.rfft(rf.irfft(spec)) - clean).abs().max().item() <= 1e-12


@pytest.mark.parametrize("T, rows", [(2401, 6), (961, 3), (480, 2)])
def test_istft_ola_is_torch_istft(T, rows):
    """Frames of random numbers, spec = rfft(frames), torch.istft(center=True, length=T) in float64: measured <= 1.4e-15, bar 1e-12.
    (A length past the overlap-add's end is kept out of here: torch.istft refuses it, the window envelope there is 5.5e-12.)"""
    frames, w = rnd(rows, N_FFT, seed=30 + rows), tables.hann_window()
    ref = torch.istft(rf.rfft(frames).t()[None], N_FFT, hop_length=HOP, win_length=N_FFT, window=w.double(), center=True, length=T)[0]
    y, A = rf.istft_ola(frames, w, T, N_FFT, HOP)
    assert y.shape == (T,) and (y - ref).abs().max().item() <= 1e-12
    assert (A >= y.abs() * (1 - 1e-12)).all()


def test_istft_ola_is_zero_past_the_overlap_adds_end():
    frames, w = rnd(3, N_FFT, seed=40), tables.hann_window()
    y, A = rf.istft_ola(frames, w, 2100, N_FFT, HOP)
    assert float(y[1984:].abs().max()) == 0.0 and float(A[1984:].abs().max()) == 0.0
    w64 = w.double()
    assert abs(float(y[1983]) - float(frames[2, 2047])  / float(w64[2047])) <= 1e-9 * abs(float(y[1983]))   # one tap of the last frame
    short, _ = rf.istft_ola(frames, w, 1500, N_FFT, HOP)
    assert torch.equal(short, y[:1500])


@pytest.mark.parametrize("sr", [8000, 12000, 16000, 22050, 24000, 44100])
def test_resample_is_scipy_resample_poly(sr):
    """Two clips: one shorter than the filter's reach, one of 601 samples.

    With scipy's own float64 design as taps the formula and its alignment are scipy's to float64 rounding: 1e-12.
    With the plan's fp32 taps the allowance is r * 2^-24 * A + 1e-12, r the fp32 roundings a tap has had.  The plan rounds scipy's
    design to fp32 and THEN multiplies by fp32(up) in fp32 (tables.resample_poly_plan), so r = 1 only where that product is exact,
    up a power of two (12000: 4, 24000: 2), and r = 2 at the other rates; each tap is checked against the design at r * 2^-24 too.
    (Taken as r = 1 everywhere, 22050 measured 1.05 of the allowance at n_in = 19, 8000 0.83.)"""
    taps, pre, up, down = tables.resample_poly_plan(48000, sr)
    half = 10 * max(up, down)
    design = scipy.signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    taps64 = torch.from_numpy(np.concatenate([np.zeros(taps.numel() - design.size), design]))
    r = 1 if up & (up - 1) == 0 else 2
    assert ((taps.double() - taps64).abs() <= r * rf.U * taps64.abs()).all()
    for n_in in (19, 601):
        x = rnd(2, n_in, seed=50 + n_in, scale=0.3)
        n_out = tables.resample_out_len(n_in, 48000, sr)
        ref = torch.from_numpy(np.stack([scipy.signal.resample_poly(v.double().numpy(), up, down) for v in x]))
        exact, _ = rf.resample(x, taps64, up, down, pre, n_out)
        got, A = rf.resample(x, taps, up, down, pre, n_out)
        assert got.shape == ref.shape == (2, n_out)
        assert (exact - ref).abs().max().item() <= 1e-12
        ratio = ((got - ref).abs() / (r * rf.U * A + 1e-12)).max().item()
        print(f"resample {sr} n_in {n_in}: max error / allowance {ratio:.3f} (r = {r})")
        assert ratio <= 1.0


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_cutoff_index_is_the_oracles(seed):
    """A random positive complex spectrum [1, 1025, F], white (seeds 0, 1) and with a roll-off that puts the cutoff mid-band."""
    F_ = 7
    spec = torch.complex(rnd(1, 1025, F_, seed=60 + seed), rnd(1, 1025, F_, seed=70 + seed))
    if seed >= 2:
        spec = spec * torch.exp(-torch.arange(1025.) / (40.0 * seed))[None, :, None]
    energy = spec.squeeze().abs().sum(-1)
    for thr in (0.99, 0.9995, 0.5):
        want = ref_cpu.cutoff_index(spec, thr)
        assert rf.cutoff_index(energy, thr) == want
        assert 0 < want < 1025
    assert rf.cutoff_index(torch.zeros(1025), 0.99) == 0
    assert rf.cutoff_index(torch.ones(64), 0.5) == 30                    # cum[31] = 32 equals the limit: `<` leaves it out


def test_cumsum_of_fp32_rounds_every_prefix_of_a_double_sum():
    """What the cutoff kernel restates: torch.cumsum of fp32 on the CPU accumulates in double and rounds each prefix to fp32."""
    e = torch.arange(1, 1026, dtype=torch.float32) * 40 + 1
    assert float(e.sum()) > 2 ** 24
    assert torch.equal(torch.cumsum(e, 0), torch.cumsum(e.double(), 0).float())


def test_small_references():
    mel = rnd(5, 40, seed=80)
    assert torch.equal(rf.mel_energy(mel), mel.double().exp().sum(0))
    x, y = rnd(7, seed=81), rnd(7, seed=82)
    assert (rf.axpby(x, 0.5, y, -2.0) - (0.5 * x.double() - 2.0 * y.double())).abs().max().item() == 0.0
    assert torch.equal(rf.peak_scale(x, 0.5, 0.99), x * 2 * torch.tensor(0.99, dtype=torch.float32))
    spec = torch.complex(rnd(1, 1025, seed=83).double(), rnd(1, 1025, seed=84).double())
    assert (rf.magnitude(spec) ** 2 - spec.abs() ** 2 - 1e-9).abs().max().item() <= 1e-15 * float(spec.abs().max()) ** 2 + 1e-16


def test_batched_frame_and_istft_entries_check_their_arguments():
    """fh_frame_f32 and fh_istft_ola_f32 reject what their segment forms reject.  The checks run on the host before anything is
    launched, so they are called here without a GPU: the device pointers are fake aligned addresses, never dereferenced."""
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    X, W, Fr, Pk = 1024, 2048, 4096, 8192

    def bad(fn, *args):
        assert getattr(L, fn)(*args, 0) == -1
        msg = L.fh_last_error()
        assert msg and fn.encode() in msg, msg

    #                     batch len rows nfft  hop  pad  pad_mode
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, N_FFT, HOP, 784, 2)
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, N_FFT, HOP, 784, -1)
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, 0, HOP, 784, 0)
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, -N_FFT, HOP, 784, 0)
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, N_FFT, 0, 784, 0)
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, N_FFT, -HOP, 784, 0)
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, N_FFT, HOP, -1, 0)
    bad("fh_frame_f32", X, W, Fr, 1, 2401, 5, N_FFT, HOP, -1, 1)
    bad("fh_frame_f32", X, W, Fr, 1, 784, 1, N_FFT, HOP, 784, 0)       # (as before: the reflect pad needs pad < len)
    #                             batch rows len nfft hop
    bad("fh_istft_ola_f32", Fr, W, X, Pk, 1, 6, 2401, 0, HOP)
    bad("fh_istft_ola_f32", Fr, W, X, Pk, 1, 6, 2401, -N_FFT, HOP)
    bad("fh_istft_ola_f32", Fr, W, X, Pk, 1, 6, 2401, N_FFT, 0)
    bad("fh_istft_ola_f32", Fr, W, X, Pk, 1, 6, 2401, N_FFT, -HOP)
