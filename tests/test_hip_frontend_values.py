"""GPU: the kernels either side of the model (csrc/frontend.hip, csrc/fft.hip) one at a time against plain float64 references
of the same operation (tests/ref_frontend.py, anchored on the CPU by tests/test_frontend_ref_cpu.py), at the sizes where each
changes path.  The batched entry, three batched calls and the segment entry are instantiations of one kernel body, so the sibling
comparisons of the form tests cannot see a wrong value that all three share; these can.

Every tolerance is derived from the arithmetic the kernel promises (u = 2^-24, half an fp32 ulp), not from a run of it, and every
test prints its largest error / bound before it asserts.  Every output is NaN- or sentinel-filled with a guard behind it, and the
guard is asserted untouched."""
import functools
import math

import pytest
import torch

import ref_frontend as rf
from flowhigh_amd import hip, tables

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_FFT, HOP = 2048, 480
U = rf.U
GUARD = 64
NAN = float("nan")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def on_device(args):
    """Tensor arguments on the device (a host tensor is uploaded and stays alive until the caller has synchronised)."""
    return [a.to(DEV) if torch.is_tensor(a) else a for a in args]


def call(name, *args):
    held = on_device(args)
    hip.check(getattr(hip.lib(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in held], hip.stream()), name)
    torch.cuda.synchronize()


def rejected(name, *args):
    """The call returns -1 and leaves a message that names the entry."""
    held = on_device(args)
    assert getattr(hip.lib(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in held], hip.stream()) == -1
    msg = hip.lib().fh_last_error()
    torch.cuda.synchronize()
    assert msg and name.encode() in msg, msg


def within(what, got, ref, bound):
    """|got - ref| <= bound elementwise; prints the largest error / bound first."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()
    print(f"\n[ratio] {what}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"


@functools.lru_cache(maxsize=None)
def hann():
    return tables.hann_window().to(DEV)


@functools.lru_cache(maxsize=None)
def twiddles():
    return tables.fft_twiddles().to(DEV)


# ---- the FFT's inputs and their float64 spectra, computed once ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fft_input(kind):
    """fp32 rows [R, 2048] and their float64 spectrum.
    band:    x = fp32(sum_{k=1..255} cos(2 pi k n / 2048 + phi_k) / 16), seeded phi: peak |X| = 64, the bins above 255 hold only
             the rounding of x to fp32 (below 1e-4), which an fp32 FFT buries under its own 1e-7 of the peak
    impulse: unit impulses at n0 = 0, 1, 2, 1023, 1024, 1025, 2047: X[k] = e^{-2 pi i k n0 / 2048}; n0 = 1 reads every twiddle,
             the others pin the bit reversal
    noise3 / noise1: white noise, 3 rows and 1 row"""
    if kind == "band":
        n, k = torch.arange(N_FFT, dtype=torch.float64), torch.arange(1, 256, dtype=torch.float64)
        rows = []
        for seed in (1, 2, 3):
            phi = torch.rand(255, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 * math.pi
            rows.append(torch.cos(2 * math.pi * k[None, :] * n[:, None] / N_FFT + phi[None, :]).sum(1) / 16)
        x = torch.stack(rows).float()
    elif kind == "impulse":
        n0 = [0, 1, 2, 1023, 1024, 1025, 2047]
        x = torch.zeros(len(n0), N_FFT)
        x[torch.arange(len(n0)), n0] = 1.0
    else:
        x = rnd({"noise3": 3, "noise1": 1}[kind], N_FFT, seed=11)
    return x, rf.rfft(x)


def run_rfft(x, mode):
    R, width = x.shape[0], (rf.P_WIDTH if mode == 0 else rf.MAG_WIDTH)
    out = nan(R + 1, width)
    call("fh_rfft2048_f32", x, twiddles(), out, R, mode)
    assert torch.isnan(out[R]).all()
    return out[:R].cpu()


@pytest.mark.parametrize("kind", ["band", "impulse", "noise3", "noise1"])
def test_rfft_is_the_correctly_rounded_float64_spectrum(kind):
    """fh_rfft2048_f32, mode 0: every component within u |ref component| + 1e-12 sum |x_row| -- half an fp32 ulp of the exact value
    plus the float64 FFT's own error (a radix-2 float64 FFT and torch's differ by 5e-17 sum |x|).  This is what fft.hip's float64
    butterflies are for: on the band-limited rows torch's fp32 FFT breaks the bound in 88 % of the real components, the float64
    FFT rounded to fp32 in none.  Padding columns are exactly 0."""
    x, ref = fft_input(kind)
    re, im, pad = rf.p_unpack(run_rfft(x, 0))
    if kind == "band":
        assert 60.0 < float(ref.abs().max()) < 68.0 and float(ref.abs()[:, 300:].median()) < 1e-4
    slack = 1e-12 * x.double().abs().sum(-1, keepdim=True)
    within(f"rfft mode 0 {kind} re", re, ref.real, U * ref.real.abs() + slack)
    within(f"rfft mode 0 {kind} im", im, ref.imag, U * ref.imag.abs() + slack)
    assert float(pad.abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["band", "noise3", "noise1"])
def test_rfft_magnitudes(kind):
    """fh_rfft2048_f32, mode 1: |got - m| <= 4 u m + 1e-12 sum |x_row|, m = sqrt(re^2 + im^2 + float32(1e-9)) of the float64
    spectrum: the rounding of re and im to fp32 (<= u of m^2 each way, 2 u together), three fp32 roundings under the root (3 u), the
    root halves the 5 u and adds its own u.  Columns 1025 .. 1055 are exactly 0."""
    x, ref = fft_input(kind)
    mag = run_rfft(x, 1)
    m = rf.magnitude(ref)
    within(f"rfft mode 1 {kind}", mag[:, :1025], m, 4 * U * m + 1e-12 * x.double().abs().sum(-1, keepdim=True))
    assert float(mag[:, 1025:].abs().max()) == 0.0


def run_irfft(spec_p):
    R = spec_p.shape[0]
    out = nan(R + 1, N_FFT)
    call("fh_irfft2048_f32", spec_p, twiddles(), out, R)
    assert torch.isnan(out[R]).all()
    return out[:R].cpu()


def irfft_bound(ref, spec):
    return U * ref.abs() + 1e-12 * spec.abs().sum(-1, keepdim=True) / N_FFT * 2


def test_irfft_single_bins():
    """fh_irfft2048_f32 on single bins k0 = 0, 1, 31, 32, 33, 1023, 1024 (the 32-bin block edges of the P-layout, DC, Nyquist) with
    Re = 1, and separately with Im = 1: |got - ref| <= u |ref| + 1e-12 * sum_k |X_k| / 2048 * 2.  The imaginary parts of DC and
    Nyquist are ignored, so those two rows are all zeros.  The padding columns hold NaN."""
    bins = [0, 1, 31, 32, 33, 1023, 1024]
    re, im = torch.zeros(14, 1025), torch.zeros(14, 1025)
    for r, k0 in enumerate(bins):
        re[r, k0] = 1.0
        im[7 + r, k0] = 1.0
    spec = torch.complex(re.double(), im.double())
    got, ref = run_irfft(rf.p_pack(re, im, fill=NAN)), rf.irfft(spec)
    assert float(ref[1].abs().max()) > 9e-4 and float(ref[7 + 1].abs().max()) > 9e-4        # 2 / 2048
    assert float(got[7].abs().max()) == 0.0 and float(got[13].abs().max()) == 0.0
    within("irfft single bins", got, ref, irfft_bound(ref, spec))


def test_irfft_random_spectrum_with_junk_in_what_it_ignores():
    re, im = rnd(3, 1025, seed=21), rnd(3, 1025, seed=22)
    spec = torch.complex(re.double(), im.double())                      # (the reference zeroes the two ignored parts itself)
    spec[:, 0], spec[:, -1] = spec[:, 0].real + 0j, spec[:, -1].real + 0j
    im[:, 0], im[:, -1] = 3.0, -2.0
    got, ref = run_irfft(rf.p_pack(re, im, fill=NAN)), rf.irfft(spec)
    within("irfft random", got, ref, irfft_bound(ref, spec))


# ---- framing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, pad, T, rows", [(0, 784, 785, 1), (0, 784, 1264, 2), (0, 784, 2401, 5),
                                                (1, 1024, 1, 1), (1, 1024, 479, 1), (1, 1024, 480, 2), (1, 1024, 2401, 6)])
def test_frame_has_the_bits_of_pad_unfold_times_window(mode, pad, T, rows):
    """fh_frame_f32 against F.pad + unfold + fp32 product, bitwise, batch 1 and batch 2 with different data.  Reflect 784 at the
    smallest legal length 785 (one row, every tap reflected at one end or the other), two rows, and 2401; zero 1024 at one
    sample, either side of the second row, and 2401."""
    for B in (1, 2):
        x = rnd(B, T, seed=30 + T + B, scale=0.4)
        ref = rf.frame(x, tables.hann_window(), rows, N_FFT, HOP, pad, mode)
        assert ref.shape == (B, rows, N_FFT) and ref.dtype == torch.float32
        out = nan(B * rows + 1, N_FFT)
        call("fh_frame_f32", x, hann(), out, B, T, rows, N_FFT, HOP, pad, mode)
        assert torch.isnan(out[B * rows]).all()
        got = out[:B * rows].cpu().view(B, rows, N_FFT)
        assert torch.isfinite(got).all() and torch.equal(got, ref), f"B {B}: {(got - ref).abs().max().item():.3e}"
        if B == 2:
            assert not torch.equal(got[0], got[1])


def test_frame_checks_its_arguments():
    """What fh_frame_seg_f32 rejects: pad_mode outside {0, 1}, nfft <= 0, hop <= 0, pad < 0.  Nothing is launched."""
    x, out = rnd(1, 2401, seed=31).to(DEV), nan(6, N_FFT)
    for nfft, hop, pad, pm in [(N_FFT, HOP, 1024, 2), (N_FFT, HOP, 784, -1), (0, HOP, 784, 0), (-N_FFT, HOP, 1024, 1),
                               (N_FFT, 0, 784, 0), (N_FFT, -HOP, 1024, 1), (N_FFT, HOP, -1, 0), (N_FFT, HOP, -1, 1)]:
        rejected("fh_frame_f32", x, hann(), out, 1, 2401, 5, nfft, hop, pad, pm)
    assert torch.isnan(out).all()


# ---- spectral energy and the cutoff search --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, B", [(1, 1), (31, 1), (32, 1), (33, 1), (64, 1), (65, 1), (129, 1), (33, 2)])
def test_spec_energy(rows, B):
    """fh_spec_energy_f32: rows of one frame lane, the second chain's first use (33), the loop's second pass (65) and tails on each.
    |got - ref| <= 3 u ref: each sqrtf(re re + im im) is within 2 u (two roundings under a correctly rounded root, which halves them,
    and the root's own), the sum is in double, and there is one final rounding.  The spectrum's padding columns hold NaN: all 1025
    energies must be finite; the slot behind the last clip stays NaN."""
    re, im = rnd(B * rows, 1025, seed=40 + rows), rnd(B * rows, 1025, seed=41 + rows)
    spec = rf.p_pack(re, im, fill=NAN)
    energy = nan(B + 1, 1025)
    call("fh_spec_energy_f32", spec, energy, B, rows)
    ref = torch.stack([rf.spec_energy(spec[b * rows:(b + 1) * rows]) for b in range(B)])
    assert torch.isnan(energy[B]).all()
    within(f"spec_energy rows {rows} B {B}", energy[:B], ref, 3 * U * ref)


@functools.lru_cache(maxsize=None)
def band_energy():
    """fp32 energies of the band-limited rows' float64 spectrum: the cutoff lies near bin 256"""
    _, ref = fft_input("band")
    return ref.abs().sum(0).float()


def cutoff_cases(nbins):
    """Energies [clips, nbins] whose answers differ."""
    z = torch.zeros(nbins)
    first, last = z.clone(), z.clone()
    first[0], last[-1] = 3.0, 5.0
    # an integer ramp whose prefixes pass 2^24 (every entry below 2^24, so exact in fp32): the fp32 rounding of each prefix decides
    step = math.ceil(2 ** 26 / (nbins * (nbins + 1)))
    ramp = torch.clamp(step * torch.arange(1, nbins + 1, dtype=torch.float64) + 1, max=2 ** 24 - 1).float()
    assert float(ramp.double().sum()) > 2 ** 24
    cases = [z, first, last, torch.ones(nbins), ramp, band_energy()[:nbins].clone()]
    f = torch.arange(nbins, dtype=torch.float32)
    for seed in range(20):                                               # random positive values with a roll-off of their own
        g = torch.Generator().manual_seed(100 + seed)
        cases.append(torch.rand(nbins, generator=g) * torch.exp(-f / (nbins * (0.02 + 0.05 * seed))) + 1e-6)
    return torch.stack(cases)


@pytest.mark.parametrize("thr", [0.99, 0.9995, 0.5])
@pytest.mark.parametrize("nbins", [1025, 256, 65, 64, 40, 2])
def test_cutoff_index_is_the_references_loop(nbins, thr):
    """fh_cutoff_index_f32, 26 clips in one launch, exactly the loop over torch.cumsum of the fp32 energies (0.99 / 1025 and
    0.9995 / 256 are the project's own launches): all zero (-> 0), only bin 0 (-> 0), only the last bin (-> nbins - 2), flat ones
    (thr 0.5 on an even count: a prefix EQUALS the limit and `<` decides), an integer ramp past 2^24, a band-limited spectrum's
    energies, twenty random draws."""
    e = cutoff_cases(nbins)
    n = e.shape[0]
    cr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    call("fh_cutoff_index_f32", e, cr, n, nbins, thr)
    want = [rf.cutoff_index(e[i], thr) for i in range(n)]
    assert want[:3] == [0, 0, nbins - 2]
    if thr == 0.5 and nbins % 2 == 0 and nbins > 2:
        assert want[3] == nbins // 2 - 2
    if nbins == 1025 and thr >= 0.99:
        assert 200 < want[5] < 300
    if nbins >= 40:
        assert len(set(want)) >= 6
    assert cr[:n].tolist() == want
    assert int(cr[n]) == -7


def test_cutoff_index_checks_nbins():
    e, cr = torch.ones(4, 1026, device=DEV), torch.full((4,), -7, dtype=torch.int32, device=DEV)
    for nbins in (1, 1026):
        rejected("fh_cutoff_index_f32", e, cr, 4, nbins, 0.99)
    assert cr.tolist() == [-7] * 4


# ---- inverse STFT's overlap-add -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, rows", [(480, 2), (961, 3), (2401, 6), (1, 1), (255, 1), (257, 2), (2100, 3)])
def test_istft_ola(T, rows):
    """fh_istft_ola_f32, batch 2 with different peaks: |got - ref| <= 12 u A, A = sum |w f| / sum w^2 -- at most 5 fused terms in
    each of numerator and denominator (5 u each, relative to sum |w f| and to sum w^2) and a correctly rounded division; emulated in
    fp32 the error reaches 0.28 of it.  (2100, 3) reaches past the overlap-add's end at 480 * 2 + 1024 = 1984: zeros from there,
    and sample 1983, where the window envelope is 5.5e-12, is within the bound like every other.  peak_bits are the bits of max |y|
    of the kernel's own output."""
    B = 2
    frames = rnd(B, rows, N_FFT, seed=50 + T)
    frames[1] *= 3.0
    y = nan(B * T + GUARD)
    peak = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    peak[B] = -7
    call("fh_istft_ola_f32", frames, hann(), y, peak, B, rows, T, N_FFT, HOP)
    assert torch.isnan(y[B * T:]).all() and int(peak[B]) == -7
    got = y[:B * T].cpu().view(B, T)
    refs = [rf.istft_ola(frames[b], tables.hann_window(), T, N_FFT, HOP) for b in range(B)]
    ref, A = torch.stack([r[0] for r in refs]), torch.stack([r[1] for r in refs])
    within(f"istft_ola T {T} rows {rows}", got, ref, 12 * U * A)
    assert torch.equal(peak[:B].cpu().view(torch.float32), got.abs().max(-1).values)
    assert float(got[0].abs().max()) > 0.0 and float(got[1].abs().max()) != float(got[0].abs().max())
    if T == 2100:
        assert float(got[:, 1984:].abs().max()) == 0.0
        assert (ref[:, 1983].abs() > 0).all() and ((got[:, 1983].double() - ref[:, 1983]).abs() <= 12 * U * A[:, 1983]).all()


def test_istft_ola_checks_its_arguments():
    """nfft <= 0 and hop <= 0 (an integer division by zero inside the kernel) are rejected as fh_istft_ola_seg_f32 rejects them."""
    frames, y, peak = rnd(6, N_FFT, seed=51).to(DEV), nan(2401), torch.zeros(1, dtype=torch.int32, device=DEV)
    for nfft, hop in [(0, HOP), (-N_FFT, HOP), (N_FFT, 0), (N_FFT, -HOP)]:
        rejected("fh_istft_ola_f32", frames, hann(), y, peak, 1, 6, 2401, nfft, hop)
    assert torch.isnan(y).all() and int(peak[0]) == 0


# ---- polyphase resampler ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", [1, 2, 19, 601])
@pytest.mark.parametrize("sr", [12000, 8000, 22050, 44100])
def test_resample_poly(sr, n_in):
    """fh_resample_poly_f32, unnormalised output, batch 2, plans 4/1, 6/1, 320/147 and 160/147: |got - ref| <= 23 u A with
    A = sum |x h| -- one chain of at most ceil(n_taps / up) <= 22 fused terms, each adding at most u of the running sum of |x h|,
    and one to spare.  n_in = 1, 2, 19 are shorter than the filter's reach, so both ends of the loop clip."""
    taps, pre, up, down = tables.resample_poly_plan(48000, sr)
    assert (up, down) == {12000: (4, 1), 8000: (6, 1), 22050: (320, 147), 44100: (160, 147)}[sr]
    assert math.ceil(taps.numel() / up) <= 22
    B, n_out = 2, tables.resample_out_len(n_in, 48000, sr)
    x = rnd(B, n_in, seed=60 + n_in, scale=0.3)
    y = nan(B * n_out + GUARD)
    call("fh_resample_poly_f32", x, taps, y, B, n_in, n_out, up, down, taps.numel(), pre)
    assert torch.isnan(y[B * n_out:]).all()
    ref, A = rf.resample(x, taps, up, down, pre, n_out)
    assert float(ref.abs().max()) > 0.0
    within(f"resample {sr} n_in {n_in}", y[:B * n_out].view(B, n_out), ref, 23 * U * A)


# ---- the small ones -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("d", [40, 256, 300])
def test_mel_energy(d, n):
    """fh_mel_energy_f32, batch 2; d = 300 reaches a second block.  |got - ref| <= 4 u ref: expf within an ulp (2 u), the sum in
    double, one final rounding, one to spare."""
    B = 2
    mel = rnd(B * n, d, seed=70 + d + n, scale=3.0) - 4.0
    energy = nan(B + 1, d)
    call("fh_mel_energy_f32", mel, energy, B, n, d)
    ref = torch.stack([rf.mel_energy(mel[b * n:(b + 1) * n]) for b in range(B)])
    assert torch.isnan(energy[B]).all()
    within(f"mel_energy d {d} n {n}", energy[:B], ref, 4 * U * ref)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_axpby(n):
    """fh_axpby_f32 either side of the 256-thread block: |got - ref| <= 2 u (|x a| + |y b|) (a product and a sum, or one of them fused)."""
    a, b = 1.37, -0.61
    x, y = rnd(n, seed=80 + n), rnd(n, seed=81 + n)
    out = nan(n + GUARD)
    call("fh_axpby_f32", x, a, y, b, out, n)
    assert torch.isnan(out[n:]).all()
    a32, b32 = float(torch.tensor(a, dtype=torch.float32)), float(torch.tensor(b, dtype=torch.float32))
    within(f"axpby n {n}", out[:n], rf.axpby(x, a, y, b), 2 * U * ((x.double() * a32).abs() + (y.double() * b32).abs()))


@pytest.mark.parametrize("T", [1, 255, 257])
def test_peak_scale(T):
    """fh_peak_scale_f32 with the peak given, three clips: the bits of fp32 (y / peak) * 0.99, both steps correctly rounded.  The third
    clip's peak is 0: no silent clip, the reference divides by zero there too (inf, and NaN for 0 / 0)."""
    B, peaks = 3, [0.7312, 2.5, 0.0]
    y = rnd(B, T, seed=90 + T)
    y[2, ::2] = 0.0
    buf = torch.cat([y.view(-1), torch.full((GUARD,), 123.0)]).to(DEV)
    bits = torch.tensor(peaks, dtype=torch.float32).view(torch.int32).to(DEV)
    call("fh_peak_scale_f32", buf, bits, B, T, 0.99)
    assert bool((buf[B * T:] == 123.0).all())
    got = buf[:B * T].cpu().view(B, T)
    ref = torch.stack([rf.peak_scale(y[b], peaks[b], 0.99) for b in range(B)])
    assert torch.isfinite(got[:2]).all() and torch.equal(got[:2], ref[:2])
    assert torch.equal(torch.isnan(got[2]), torch.isnan(ref[2])) and torch.isnan(got[2, 0])
    assert torch.equal(torch.nan_to_num(got[2], nan=7.0), torch.nan_to_num(ref[2], nan=7.0))
