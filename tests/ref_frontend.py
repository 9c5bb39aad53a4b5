"""Plain float64 references of the front / back end steps (csrc/frontend.hip, csrc/fft.hip), one per operation: what the value
tests of those kernels compare against.

Written from the formulas in the kernels' comments, with no project kernel and no flowhigh_amd.frontend class behind them.  Every
function takes the kernel's own fp32 inputs (the fp32 hann, the fp32 taps included) and works on their float64 upcasts, so what is
left between a kernel and its reference is the kernel's own rounding; the two that return fp32 (frame, peak_scale) restate
operations whose fp32 result is correctly rounded, and are compared bitwise.  tests/test_frontend_ref_cpu.py anchors them to
torch.stft / torch.istft / scipy / the oracle without a GPU."""
import torch
import torch.nn.functional as F

N_FFT = 2048
N_BINS = 1025
P_BLOCKS = 33                 # 33 * 32 = 1056 >= 1025 bins
P_WIDTH = P_BLOCKS * 64       # 2112 floats per row
MAG_WIDTH = P_BLOCKS * 32     # 1056
U = 2.0 ** -24                # half an fp32 ulp, relative


# ---- P-layout: 33 blocks of 64 floats = 32 Re then 32 Im of bins 32 b .. 32 b + 31 --------------------------------------------
def p_columns():
    """(column of Re, column of Im) of the bins 0 .. 1055; bins >= 1025 are block 32's padding."""
    k = torch.arange(P_BLOCKS * 32)
    re = (k // 32) * 64 + k % 32
    return re, re + 32


def p_pack(re, im, fill=0.0):
    """re, im [R, 1025] -> [R, 2112] of their dtype; the 62 padding columns hold `fill`."""
    out = torch.full((re.shape[0], P_WIDTH), fill, dtype=re.dtype)
    cre, cim = p_columns()
    out[:, cre[:N_BINS]] = re
    out[:, cim[:N_BINS]] = im
    return out


def p_unpack(spec):
    """[R, 2112] -> re [R, 1025], im [R, 1025], padding [R, 62]."""
    cre, cim = p_columns()
    return spec[:, cre[:N_BINS]], spec[:, cim[:N_BINS]], torch.cat([spec[:, cre[N_BINS:]], spec[:, cim[N_BINS:]]], dim=1)


# ---- framing and the DFT ------------------------------------------------------------------------------------------------------
def frame(x, window, rows, nfft, hop, pad, mode):
    """frames[b, t, k] = pad(x[b])[hop t + k] * window[k], t < rows; mode 0: reflect (no edge repeat), 1: zero.  x [B, len].
    In the dtype of x and window: for fp32 the product of two fp32 numbers, which a kernel either has bit for bit or has not."""
    xp = F.pad(x[:, None], (pad, pad), mode="reflect" if mode == 0 else "constant")[:, 0]
    return xp.unfold(-1, nfft, hop)[:, :rows] * window


def rfft(frames):
    """[R, 2048] -> complex128 [R, 1025]"""
    return torch.fft.rfft(frames.double(), dim=-1)


def irfft(spec):
    """complex [R, 1025] -> float64 [R, 2048]; the imaginary parts of DC and Nyquist are ignored (C2R)."""
    s = spec.to(torch.complex128).clone()
    s[:, 0] = s[:, 0].real.to(torch.complex128)
    s[:, -1] = s[:, -1].real.to(torch.complex128)
    return torch.fft.irfft(s, n=N_FFT, dim=-1)


def magnitude(spec):
    """m = sqrt(re^2 + im^2 + float32(1e-9)) of a complex128 spectrum (the mel front end's magnitudes)"""
    return torch.sqrt(spec.real ** 2 + spec.imag ** 2 + float(torch.tensor(1e-9, dtype=torch.float32)))


# ---- spectral energy and the cutoff search --------------------------------------------------------------------------------------
def spec_energy(spec_p):
    """sum_t sqrt(re^2 + im^2) over the rows of one clip's P-layout spectrum [rows, 2112] -> float64 [1025]"""
    re, im, _ = p_unpack(spec_p.double())
    return torch.sqrt(re * re + im * im).sum(0)


def cutoff_index(energy, thr):
    """The largest j in [1, n - 1] with cum[j] < cum[n - 1] * thr, else 0: the reference's loop from the top bin down over
    torch.cumsum of the fp32 energies on the CPU (every prefix an fp32 number), the threshold product an fp32 multiply."""
    cum = torch.cumsum(energy.detach().cpu().float(), dim=0)
    limit = float(cum[-1] * torch.tensor(thr, dtype=torch.float32))
    cum = cum.tolist()
    n = len(cum)
    for i in range(1, n):
        if cum[n - i] < limit:
            return n - i
    return 0


# ---- inverse STFT's overlap-add -------------------------------------------------------------------------------------------------
def istft_ola(frames, window, length, nfft, hop):
    """One clip's frames [rows, nfft] -> (y, A), float64 [length]: y = sum_t w f / sum_t w^2 over the whole frames, cut at nfft / 2,
    and zero from hop (rows - 1) + nfft / 2 on; A = sum_t |w f| / sum_t w^2, what an error bound of the quotient scales with."""
    f, w = frames.double(), window.double()
    rows = f.shape[0]
    total = hop * (rows - 1) + nfft
    num, mag, den = torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    for t in range(rows):
        num[hop * t:hop * t + nfft] += w * f[t]
        mag[hop * t:hop * t + nfft] += (w * f[t]).abs()
        den[hop * t:hop * t + nfft] += w * w
    n = min(length, total - nfft // 2)
    y, A = torch.zeros(length, dtype=torch.float64), torch.zeros(length, dtype=torch.float64)
    y[:n] = num[nfft // 2:nfft // 2 + n] / den[nfft // 2:nfft // 2 + n]
    A[:n] = mag[nfft // 2:nfft // 2 + n] / den[nfft // 2:nfft // 2 + n]
    return y, A


# ---- polyphase resampler ----------------------------------------------------------------------------------------------------
def resample(x, taps, up, down, pre, n_out):
    """out[b, i] = sum_j x[b, j] h[(i + pre) down - j up], h zero outside the taps, as the matrix it is.  x [B, n_in] ->
    (out, A), float64 [B, n_out]; A = sum_j |x h|."""
    x, h = x.double(), taps.double()
    i, j = torch.arange(n_out)[:, None], torch.arange(x.shape[1])[None, :]
    k = (i + pre) * down - j * up
    H = torch.where((k >= 0) & (k < h.numel()), h[k.clamp(0, h.numel() - 1)], torch.zeros((), dtype=torch.float64))
    return x @ H.t(), x.abs() @ H.abs().t()


# ---- the small ones -----------------------------------------------------------------------------------------------------------
def mel_energy(mel):
    """one clip's log-mel [n, d] -> float64 [d]: sum_n exp(mel)"""
    return torch.exp(mel.double()).sum(0)


def axpby(x, a, y, b):
    """x a + y b in float64, a and b as the fp32 numbers the kernel is given"""
    a32, b32 = torch.tensor(a, dtype=torch.float32).double(), torch.tensor(b, dtype=torch.float32).double()
    return x.double() * a32 + y.double() * b32


def peak_scale(y, peak, target):
    """fp32 (y / peak) * target, peak and target fp32: two correctly rounded operations, compared bitwise"""
    return (y.float() / torch.tensor(peak, dtype=torch.float32)) * torch.tensor(target, dtype=torch.float32)
