"""Log-mel front end, STFT-domain post-processing and the resampling pre-step on the HIP kernels.

  LogMel          MelVoco.encode                   /root/reference/src/flowhigh/models/melvoco.py:56-86
  PostProcessor   PostProcessing.post_processing   /root/reference/src/flowhigh/postprocessing.py:5-41
  Resampler       scipy.signal.resample_poly + peak normalise   flowhighsr.py:68-69

STFT / iSTFT are 2048-point FFTs in LDS (csrc/fft.hip; FH_FFT=0 selects the older DFT-by-GEMM on the
matrix cores, 8.4 MFLOP per frame) with the magnitude, the mel projection's log and the window /
overlap-add fused around them; the reference's python cutoff loop (one host sync per bin on GPU) is a
device scan.
"""
import os

import numpy as np
import torch

from . import hip, tables
from .tables import HOP, MAG_WIDTH, N_FFT, N_MELS, P_WIDTH


_USE_FFT = os.environ.get("FH_FFT", "1") != "0"


class _Const:
    _cache = {}

    @classmethod
    def get(cls, device):
        device = hip.norm_device(device)
        key = (device.type, device.index)
        if key not in cls._cache:
            c = dict(hann=tables.hann_window().to(device), w_mel=tables.mel_gemm_weight().to(device))
            if _USE_FFT:
                c["tw"] = tables.fft_twiddles().to(device)
            else:               # FH_FFT=0: STFT / iSTFT as DFT-by-GEMM (35 MB of bases, not uploaded otherwise)
                c["w_fwd"] = tables.dft_forward_weight().to(device)
                c["w_inv"] = tables.dft_inverse_weight().to(device)
            cls._cache[key] = c
        return cls._cache[key]


# ---- ragged calls: clips of different lengths through the segment-form entries (csrc/frontend_seg.hip) -------------------
def clip_rates(sr, n_clips):
    """The input rate of every clip of a list as ints: `sr` is one rate for all of them, or a sequence of one positive
    integer rate per clip (anything else is a ValueError)."""
    def rate(v):
        if isinstance(v, (bool, str, bytes)) or v != v or v in (float("inf"), float("-inf")) or int(v) != v or int(v) <= 0:
            raise ValueError(f"an input rate must be a positive integer, got {v!r}")
        return int(v)
    try:
        if np.ndim(sr) == 0:
            return [rate(sr)] * int(n_clips)
        rates = list(sr)
        if len(rates) != n_clips:
            raise ValueError(f"one input rate per clip: {len(rates)} rates for {n_clips} clips")
        return [rate(v) for v in rates]
    except TypeError as e:
        raise ValueError(f"an input rate must be a positive integer, got {sr!r}") from e


def rate_tables(rates, sr_out=48000):
    """Host side of the per-clip filters of fh_resample_poly_rates_seg_f32 for clips at `rates` (one per clip) ->
      bank      float32 numpy array: the taps of every distinct rate's tables.resample_poly_plan back to back
      rows      hip.Rate array, one row per distinct rate in order of first appearance (a rate equal to sr_out: n_taps = 0,
                up = down = 1: the copy)
      rate_of   int32 numpy array, the row of every clip."""
    rates = clip_rates(rates, len(rates))
    distinct = list(dict.fromkeys(rates))
    taps, rows, pos = [], [], 0
    for r in distinct:
        plan = tables.resample_poly_plan(sr_out, r)
        if plan is None:
            rows.append(hip.Rate(pos, 0, 1, 1, 0))
            continue
        h, pre, up, down = plan
        rows.append(hip.Rate(pos, h.numel(), up, down, pre))
        taps.append(h.numpy())
        pos += h.numel()
    if pos >= 2 ** 31:
        raise ValueError("tap bank too large")
    bank = np.concatenate(taps).astype(np.float32, copy=False) if taps else np.zeros(0, np.float32)
    return bank, (hip.Rate * len(rows))(*rows), np.array([distinct.index(r) for r in rates], dtype=np.int32)


def ragged_clip_tables(lengths_in, sr_in, sr_out=48000, pred_lens=None, check_mel=True):
    """Host side of the clip tables of a ragged call, for clips of `lengths_in` samples at sr_in (lists, one item per clip):
      len_in / in_off     samples and first sample of every clip in the packed low-rate input
      len_out / out_off   T_i = tables.resample_out_len and first sample in the packed 48 kHz buffers (cond, output)
      mel_rows / mel_row0 N_i = T_i // 480 frames of the mel front end and the clip's first row among the packed frames
      pred_len            Tp_i, the vocoder's samples for N_i frames (480 N_i unless given: Vocoder.out_len)
      pp_rows / pp_row0   F_i = min(1 + Tp_i // 480, 1 + T_i // 480) frames of the post-processing STFT, and their first row
    Everything is back to back.  A clip too short for the reflect pad of the front end is refused as LogMel refuses it
    (check_mel=False: the resampler alone takes any length).  sr_in: one rate for the list, or one rate per clip."""
    len_in = [int(n) for n in lengths_in]
    if not len_in:
        raise ValueError("empty clip list")
    rates = clip_rates(sr_in, len(len_in))
    len_out = [tables.resample_out_len(n, sr_out, r) for n, r in zip(len_in, rates)]
    mel_rows = [t // HOP for t in len_out]
    for t, n in zip(len_out, mel_rows):
        if check_mel and (n < 1 or t <= (N_FFT - HOP) // 2):
            raise ValueError(f"clip of {t} samples is too short for the mel front end")
    pred_len = [HOP * n for n in mel_rows] if pred_lens is None else [int(n) for n in pred_lens]
    if len(pred_len) != len(len_in):
        raise ValueError("one pred length per clip")
    pp_rows = [min(1 + tp // HOP, 1 + t // HOP) for tp, t in zip(pred_len, len_out)]

    def starts(v):
        return [int(x) for x in np.cumsum([0] + list(v[:-1]))]
    return dict(len_in=len_in, in_off=starts(len_in), len_out=len_out, out_off=starts(len_out), mel_rows=mel_rows,
                mel_row0=starts(mel_rows), pred_len=pred_len, pp_rows=pp_rows, pp_row0=starts(pp_rows))


def _ptr(t):
    return t.data_ptr()


def upload_tables(parts, device):
    """Descriptor arrays and segment tables of a call (ctypes arrays / int32 numpy arrays) as ONE pinned buffer and one copy;
    returns (device uint8 tensor that owns them, device address of every part), parts 16-byte aligned."""
    blobs, offs, pos = [], [], 0
    for part in parts:
        b = part.tobytes() if isinstance(part, np.ndarray) else bytes(part)
        offs.append(pos)
        b += bytes(-len(b) % 16)
        blobs.append(b)
        pos += len(b)
    host = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8)
    dev = host.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else host
    return dev, [dev.data_ptr() + o for o in offs]


def clip_array(src=None, dst=None, len_in=None, len_out=None, row0=None, rows=None, n=None):
    """hip.Clip array from per-clip lists (a field left out is zero: the entry that takes the array does not read it)."""
    n = n if n is not None else len(next(v for v in (src, dst, len_in, len_out, row0, rows) if v is not None))
    z = [0] * n
    cols = [v if v is not None else z for v in (src, dst, len_in, len_out, row0, rows)]
    return (hip.Clip * n)(*[hip.Clip(*[int(c[i]) for c in cols]) for i in range(n)])


def seg_table(row0, rows):
    return np.array([[a, b] for a, b in zip(row0, rows)], dtype=np.int32)


def _views(packed, offs, lens):
    return [packed[o:o + n] for o, n in zip(offs, lens)]


def _flat(ts):
    return [t.reshape(-1) for t in ts]


class LogMel:
    def __init__(self, device):
        self.device = hip.norm_device(device)
        self.c = _Const.get(self.device)
        self._ws = hip.ShapeCache()

    @hip.on_device
    def __call__(self, audio):
        """audio [B, T] on device -> log-mel [B*N, 256] (token-major rows), N = T // 480."""
        B, T = audio.shape
        N = T // HOP
        if N < 1 or T <= (N_FFT - HOP) // 2:
            raise ValueError(f"clip of {T} samples is too short for the mel front end")
        key = (B, T)
        if key not in self._ws:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._ws[key] = (torch.empty(B * N, N_FFT, **f32), torch.empty(B * N, MAG_WIDTH, **f32))
        frames, mag = self._ws[key]
        L, st = hip.lib(), hip.stream()
        audio = audio.contiguous()
        hip.check(L.fh_frame_f32(audio.data_ptr(), self.c["hann"].data_ptr(), frames.data_ptr(), B, T, N,
                                 N_FFT, HOP, (N_FFT - HOP) // 2, 0, st), "fh_frame_f32")
        if _USE_FFT:
            hip.check(L.fh_rfft2048_f32(frames.data_ptr(), self.c["tw"].data_ptr(), mag.data_ptr(), B * N, 1, st),
                      "fh_rfft2048_f32")
        else:
            hip.gemm(frames, self.c["w_fwd"], mag, B * N, P_WIDTH, N_FFT, epilogue=hip.EPI_MAG)
        mel = torch.empty(B * N, N_MELS, dtype=torch.float32, device=self.device)
        hip.gemm(mag, self.c["w_mel"], mel, B * N, N_MELS, MAG_WIDTH, epilogue=hip.EPI_LOGCLAMP)
        return mel

    @hip.on_device
    def ragged(self, conds):
        """conds: list of [T_i] device clips (48 kHz) -> (log-mel [sum N_i, 256] of all clips packed back to back, list of the
        clips' [N_i, 256] views), every clip's rows the bits of __call__ on that clip alone.  Three launches for the list.
        The result belongs to the workspace of this mix of lengths (overwritten by the next call of the same mix)."""
        conds = _flat(conds)
        tab = ragged_clip_tables([c.shape[0] for c in conds], 48000)
        key = tuple(tab["len_out"])
        ptrs = tuple(_ptr(c) for c in conds)
        M = sum(tab["mel_rows"])
        if key not in self._ws:
            f32 = dict(dtype=torch.float32, device=self.device)
            mel = torch.empty(M, N_MELS, **f32)
            self._ws[key] = dict(frames=torch.empty(M, N_FFT, **f32), mag=torch.empty(M, MAG_WIDTH, **f32), mel=mel,
                                 views=_views(mel, tab["mel_row0"], tab["mel_rows"]), ptrs=None)
        w = self._ws[key]
        if w["ptrs"] != ptrs:             # (clips at other addresses than last time: the descriptors go up again, one copy)
            w["desc"], (w["clips"],) = upload_tables([clip_array(src=ptrs, len_in=tab["len_out"], row0=tab["mel_row0"],
                                                                 rows=tab["mel_rows"])], self.device)
            w["ptrs"] = ptrs
        L, st = hip.lib(), hip.stream()
        frames, mag, mel = w["frames"], w["mag"], w["mel"]
        hip.check(L.fh_frame_seg_f32(w["clips"], len(conds), max(tab["mel_rows"]), min(tab["len_out"]), self.c["hann"].data_ptr(),
                                     frames.data_ptr(), N_FFT, HOP, (N_FFT - HOP) // 2, 0, st), "fh_frame_seg_f32")
        if _USE_FFT:
            hip.check(L.fh_rfft2048_f32(frames.data_ptr(), self.c["tw"].data_ptr(), mag.data_ptr(), M, 1, st), "fh_rfft2048_f32")
        else:
            hip.gemm(frames, self.c["w_fwd"], mag, M, P_WIDTH, N_FFT, epilogue=hip.EPI_MAG)
        hip.gemm(mag, self.c["w_mel"], mel, M, N_MELS, MAG_WIDTH, epilogue=hip.EPI_LOGCLAMP)
        return mel, w["views"]


class PostProcessor:
    def __init__(self, device):
        self.device = hip.norm_device(device)
        self.c = _Const.get(self.device)
        self._ws = hip.ShapeCache()

    @hip.on_device
    def __call__(self, pred, src, length, return_cr=False):
        """pred [B, Tp], src [B, T] -> [B, length]; per-clip cutoff, splice, iSTFT, 0.99 peak."""
        B, Tp = pred.shape
        T = src.shape[1]
        F = min(1 + Tp // HOP, 1 + T // HOP)
        key = (B, Tp, T, length)
        if key not in self._ws:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._ws[key] = dict(frames=torch.empty(B * F, N_FFT, **f32), sp=torch.empty(B * F, P_WIDTH, **f32),
                                 ss=torch.empty(B * F, P_WIDTH, **f32), energy=torch.empty(B, 1025, **f32),
                                 cr=torch.empty(B, dtype=torch.int32, device=self.device),
                                 peak=torch.empty(B, dtype=torch.int32, device=self.device))
        w = self._ws[key]
        L, st = hip.lib(), hip.stream()
        hann = self.c["hann"].data_ptr()
        pred, src = pred.contiguous(), src.contiguous()
        for sig, n, spec in ((pred, Tp, w["sp"]), (src, T, w["ss"])):
            hip.check(L.fh_frame_f32(sig.data_ptr(), hann, w["frames"].data_ptr(), B, n, F, N_FFT, HOP,
                                     N_FFT // 2, 1, st), "fh_frame_f32")
            if _USE_FFT:
                hip.check(L.fh_rfft2048_f32(w["frames"].data_ptr(), self.c["tw"].data_ptr(), spec.data_ptr(), B * F,
                                            0, st), "fh_rfft2048_f32")
            else:
                hip.gemm(w["frames"], self.c["w_fwd"], spec, B * F, P_WIDTH, N_FFT)
        hip.check(L.fh_spec_energy_f32(w["ss"].data_ptr(), w["energy"].data_ptr(), B, F, st), "fh_spec_energy_f32")
        hip.check(L.fh_cutoff_index_f32(w["energy"].data_ptr(), w["cr"].data_ptr(), B, 1025, 0.99, st), "fh_cutoff_index_f32")
        hip.check(L.fh_spec_splice_f32(w["sp"].data_ptr(), w["ss"].data_ptr(), w["cr"].data_ptr(),
                                       w["sp"].data_ptr(), B, F, st), "fh_spec_splice_f32")
        if _USE_FFT:
            hip.check(L.fh_irfft2048_f32(w["sp"].data_ptr(), self.c["tw"].data_ptr(), w["frames"].data_ptr(), B * F, st),
                      "fh_irfft2048_f32")
        else:
            hip.gemm(w["sp"], self.c["w_inv"], w["frames"], B * F, N_FFT, P_WIDTH)
        out = torch.empty(B, length, dtype=torch.float32, device=self.device)
        w["peak"].zero_()
        hip.check(L.fh_istft_ola_f32(w["frames"].data_ptr(), hann, out.data_ptr(), w["peak"].data_ptr(), B, F,
                                     length, N_FFT, HOP, st), "fh_istft_ola_f32")
        hip.check(L.fh_peak_scale_f32(out.data_ptr(), w["peak"].data_ptr(), B, length, 0.99, st), "fh_peak_scale_f32")
        return (out, w["cr"]) if return_cr else out

    @hip.on_device
    def ragged(self, preds, srcs, lengths, return_cr=False):
        """preds: list of [Tp_i] (or [1, Tp_i]) vocoder waveforms, srcs: list of [T_i] conditioning clips, lengths: samples to
        return per clip -> (output packed [sum length_i], list of the clips' [length_i] views[, cr int32 [n]]), every clip the
        bits of __call__(pred_i[None], src_i[None], length_i): per-clip cutoff, splice, iSTFT, 0.99 peak.  11 launches for the
        list.  The results belong to the workspace of this mix of lengths: a caller that keeps them clones them."""
        preds, srcs = _flat(preds), _flat(srcs)
        lengths = [int(n) for n in lengths]
        n = len(preds)
        if len(srcs) != n or len(lengths) != n or n < 1:
            raise ValueError("one pred, one src and one length per clip")
        Tp, T = [p.shape[0] for p in preds], [s_.shape[0] for s_ in srcs]
        F = [min(1 + a // HOP, 1 + b // HOP) for a, b in zip(Tp, T)]
        key = (tuple(Tp), tuple(T), tuple(lengths))
        ptrs = tuple(_ptr(t) for t in preds + srcs)
        R = sum(F)
        if key not in self._ws:
            f32 = dict(dtype=torch.float32, device=self.device)
            out = torch.empty(sum(lengths), **f32)
            off = [int(x) for x in np.cumsum([0] + lengths[:-1])]
            self._ws[key] = dict(frames=torch.empty(R, N_FFT, **f32), sp=torch.empty(R, P_WIDTH, **f32),
                                 ss=torch.empty(R, P_WIDTH, **f32), energy=torch.empty(n, 1025, **f32),
                                 cr=torch.empty(n, dtype=torch.int32, device=self.device),
                                 peak=torch.empty(n, dtype=torch.int32, device=self.device), out=out, off=off,
                                 views=_views(out, off, lengths), ptrs=None)
        w = self._ws[key]
        if w["ptrs"] != ptrs:
            row0 = [int(x) for x in np.cumsum([0] + F[:-1])]
            outs = [w["out"].data_ptr() + 4 * o for o in w["off"]]
            w["desc"], (w["c_pred"], w["c_src"], w["seg"]) = upload_tables(
                [clip_array(src=ptrs[:n], len_in=Tp, row0=row0, rows=F),
                 clip_array(src=ptrs[n:], len_in=T, row0=row0, rows=F, dst=outs, len_out=lengths), seg_table(row0, F)], self.device)
            w["ptrs"] = ptrs
        L, st = hip.lib(), hip.stream()
        hann = self.c["hann"].data_ptr()
        for clips, lens, spec in ((w["c_pred"], Tp, w["sp"]), (w["c_src"], T, w["ss"])):
            hip.check(L.fh_frame_seg_f32(clips, n, max(F), min(lens), hann, w["frames"].data_ptr(), N_FFT, HOP, N_FFT // 2, 1, st),
                      "fh_frame_seg_f32")
            if _USE_FFT:
                hip.check(L.fh_rfft2048_f32(w["frames"].data_ptr(), self.c["tw"].data_ptr(), spec.data_ptr(), R, 0, st),
                          "fh_rfft2048_f32")
            else:
                hip.gemm(w["frames"], self.c["w_fwd"], spec, R, P_WIDTH, N_FFT)
        hip.check(L.fh_spec_energy_seg_f32(w["ss"].data_ptr(), w["energy"].data_ptr(), w["seg"], n, st), "fh_spec_energy_seg_f32")
        hip.check(L.fh_cutoff_index_f32(w["energy"].data_ptr(), w["cr"].data_ptr(), n, 1025, 0.99, st), "fh_cutoff_index_f32")
        hip.check(L.fh_spec_splice_seg_f32(w["sp"].data_ptr(), w["ss"].data_ptr(), w["cr"].data_ptr(), w["sp"].data_ptr(),
                                           w["seg"], n, max(F), st), "fh_spec_splice_seg_f32")
        if _USE_FFT:
            hip.check(L.fh_irfft2048_f32(w["sp"].data_ptr(), self.c["tw"].data_ptr(), w["frames"].data_ptr(), R, st),
                      "fh_irfft2048_f32")
        else:
            hip.gemm(w["sp"], self.c["w_inv"], w["frames"], R, N_FFT, P_WIDTH)
        w["peak"].zero_()
        hip.check(L.fh_istft_ola_seg_f32(w["frames"].data_ptr(), hann, w["c_src"], n, max(lengths), w["peak"].data_ptr(),
                                         N_FFT, HOP, st), "fh_istft_ola_seg_f32")
        hip.check(L.fh_peak_scale_seg_f32(w["c_src"], n, max(lengths), w["peak"].data_ptr(), 0.99, st), "fh_peak_scale_seg_f32")
        return (w["out"], w["views"], w["cr"]) if return_cr else (w["out"], w["views"])


class Resampler:
    """Device polyphase resampler + peak normalise (the reference does this on the host in numpy)."""

    def __init__(self, device):
        self.device = hip.norm_device(device)
        self._taps = {}
        self._banks = {}                  # (sr_out, distinct input rates ...) -> (device tap bank, hip.Rate rows)
        self._ws = hip.ShapeCache()

    @hip.on_device
    def __call__(self, x, sr_in, sr_out=48000):
        """x [B, T_in] float32 on device -> [B, T_out], each clip divided by its max |.|."""
        B, n_in = x.shape
        plan = tables.resample_poly_plan(sr_out, sr_in)
        L, st = hip.lib(), hip.stream()
        if plan is None:
            y = x.clone()
        else:
            taps, pre, up, down = plan
            key = (sr_out, sr_in)
            if key not in self._taps:
                self._taps[key] = taps.to(self.device)
            n_out = tables.resample_out_len(n_in, sr_out, sr_in)
            y = torch.empty(B, n_out, dtype=torch.float32, device=self.device)
            x = x.contiguous()
            hip.check(L.fh_resample_poly_f32(x.data_ptr(), self._taps[key].data_ptr(), y.data_ptr(), B, n_in,
                                             n_out, up, down, self._taps[key].numel(), pre, st), "fh_resample_poly_f32")
        peak = torch.zeros(B, dtype=torch.int32, device=self.device)
        hip.check(L.fh_peak_abs_f32(y.data_ptr(), peak.data_ptr(), B, y.shape[1], st), "fh_peak_abs_f32")
        hip.check(L.fh_peak_scale_f32(y.data_ptr(), peak.data_ptr(), B, y.shape[1], 1.0, st), "fh_peak_scale_f32")
        return y

    def _fill(self, buf, xs):
        """list of 1-D float32 clips -> the packed device buffer `buf`.  Host arrays go up as one pinned buffer and one copy."""
        if all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in xs):
            torch.cat([x.reshape(-1).to(torch.float32) for x in xs], out=buf)
            return
        xs = [x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]
        host = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in xs]))
        buf.copy_(host.pin_memory() if buf.is_cuda else host, non_blocking=True)

    @hip.on_device
    def ragged(self, xs, sr_in, sr_out=48000):
        """xs: list of 1-D float32 clips at sr_in (host arrays: packed and uploaded with one copy; or device tensors) ->
        (the 48 kHz clips packed back to back [sum T_i], list of their [T_i] views), each resampled and divided by its
        max |.| with the bits of __call__ on that clip alone.  Four launches for the list.  The result belongs to the
        workspace of this mix of lengths: its address is the same at every call of the mix.
        sr_in may be one rate per clip: clips of different rates still run as one resampling launch, every clip with the
        polyphase filter of its own rate (fh_resample_poly_rates_seg_f32); the workspace then belongs to the mix of
        (length, rate) pairs."""
        rates = clip_rates(sr_in, len(xs))
        if len(set(rates)) > 1:
            return self._ragged_rates(xs, rates, sr_out)
        sr_in = rates[0] if rates else sr_in
        tab = ragged_clip_tables([int(np.prod(x.shape)) for x in xs], sr_in, sr_out, check_mel=False)
        n = len(xs)
        plan = tables.resample_poly_plan(sr_out, sr_in)
        key = (sr_in, sr_out, tuple(tab["len_in"]))
        if key not in self._ws:           # (input, output and descriptors belong to the mix: a mix seen before uploads only its samples)
            f32 = dict(dtype=torch.float32, device=self.device)
            x, y = torch.empty(sum(tab["len_in"]), **f32), torch.empty(sum(tab["len_out"]), **f32)
            desc, (clips,) = upload_tables(
                [clip_array(src=[x.data_ptr() + 4 * o for o in tab["in_off"]], len_in=tab["len_in"],
                            dst=[y.data_ptr() + 4 * o for o in tab["out_off"]], len_out=tab["len_out"])], self.device)
            self._ws[key] = dict(x=x, y=y, views=_views(y, tab["out_off"], tab["len_out"]), desc=desc, clips=clips,
                                 peak=torch.empty(n, dtype=torch.int32, device=self.device))
        w = self._ws[key]
        self._fill(w["x"], xs)
        L, st = hip.lib(), hip.stream()
        if plan is None:
            taps, n_taps, pre, up, down = 0, 0, 0, 1, 1
        else:
            taps_t, pre, up, down = plan
            tk = (sr_out, sr_in)
            if tk not in self._taps:
                self._taps[tk] = taps_t.to(self.device)
            taps, n_taps = self._taps[tk].data_ptr(), self._taps[tk].numel()
        max_len = max(tab["len_out"])
        hip.check(L.fh_resample_poly_seg_f32(w["clips"], n, max_len, taps, up, down, n_taps, pre, st), "fh_resample_poly_seg_f32")
        w["peak"].zero_()
        hip.check(L.fh_peak_abs_seg_f32(w["clips"], n, max_len, w["peak"].data_ptr(), st), "fh_peak_abs_seg_f32")
        hip.check(L.fh_peak_scale_seg_f32(w["clips"], n, max_len, w["peak"].data_ptr(), 1.0, st), "fh_peak_scale_seg_f32")
        return w["y"], w["views"]

    def _ragged_rates(self, xs, rates, sr_out):
        """ragged() for clips of more than one input rate: one resampling launch over per-clip filter rows, then the two
        peak launches.  The clip descriptors, the filter rows and every clip's row index go up as one buffer, once per
        mix; the tap bank is kept on the device per tuple of distinct rates."""
        tab = ragged_clip_tables([int(np.prod(x.shape)) for x in xs], rates, sr_out, check_mel=False)
        n = len(xs)
        distinct = tuple(dict.fromkeys(rates))
        bk = (sr_out,) + distinct
        if bk not in self._banks:
            bank, rows, _ = rate_tables(distinct, sr_out)
            self._banks[bk] = (torch.from_numpy(bank).to(self.device), rows)
        bank, rows = self._banks[bk]
        key = (tuple(rates), sr_out, tuple(tab["len_in"]))
        if key not in self._ws:
            f32 = dict(dtype=torch.float32, device=self.device)
            x, y = torch.empty(sum(tab["len_in"]), **f32), torch.empty(sum(tab["len_out"]), **f32)
            rate_of = np.array([distinct.index(r) for r in rates], dtype=np.int32)
            desc, (clips, rows_dev, rate_of_dev) = upload_tables(
                [clip_array(src=[x.data_ptr() + 4 * o for o in tab["in_off"]], len_in=tab["len_in"],
                            dst=[y.data_ptr() + 4 * o for o in tab["out_off"]], len_out=tab["len_out"]), rows, rate_of],
                self.device)
            self._ws[key] = dict(x=x, y=y, views=_views(y, tab["out_off"], tab["len_out"]), desc=desc, clips=clips,
                                 rows=rows_dev, rate_of=rate_of_dev, peak=torch.empty(n, dtype=torch.int32, device=self.device))
        w = self._ws[key]
        self._fill(w["x"], xs)
        L, st = hip.lib(), hip.stream()
        max_len = max(tab["len_out"])
        hip.check(L.fh_resample_poly_rates_seg_f32(w["clips"], w["rate_of"], n, max_len, w["rows"], len(distinct),
                                                   bank.data_ptr() if bank.numel() else 0, bank.numel(), st),
                  "fh_resample_poly_rates_seg_f32")
        w["peak"].zero_()
        hip.check(L.fh_peak_abs_seg_f32(w["clips"], n, max_len, w["peak"].data_ptr(), st), "fh_peak_abs_seg_f32")
        hip.check(L.fh_peak_scale_seg_f32(w["clips"], n, max_len, w["peak"].data_ptr(), 1.0, st), "fh_peak_scale_seg_f32")
        return w["y"], w["views"]

    @hip.on_device
    def upload_packed(self, conds):
        """conds: list of 1-D float32 host clips that are 48 kHz already (resampled and normalised on the host,
        upsampling_method='scipy') -> (packed device tensor [sum T_i], views): one pinned buffer, one copy, into the
        workspace of this mix of lengths."""
        lens = [int(np.prod(c.shape)) for c in conds]
        key = ("host",) + tuple(lens)
        if key not in self._ws:
            y = torch.empty(sum(lens), dtype=torch.float32, device=self.device)
            self._ws[key] = dict(y=y, views=_views(y, [int(v) for v in np.cumsum([0] + lens[:-1])], lens))
        w = self._ws[key]
        self._fill(w["y"], conds)
        return w["y"], w["views"]
