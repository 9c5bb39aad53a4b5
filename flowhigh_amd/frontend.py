"""Log-mel front end, STFT-domain post-processing and the resampling pre-step on the HIP kernels.

  LogMel          MelVoco.encode                   models/melvoco.py:56-86 (paths under the reference's src/flowhigh/)
  PostProcessor   PostProcessing.post_processing   postprocessing.py:5-41
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


# ---- ragged calls: clips of different lengths through the segment-form entries (fh_*_seg_f32, csrc/frontend.hip) ----------
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


def rate_index(rates):
    """(the distinct rates of a clip list in order of first appearance, int32 numpy array: every clip's index among them)."""
    distinct = list(dict.fromkeys(rates))
    return distinct, np.array([distinct.index(r) for r in rates], dtype=np.int32)


def rate_tables(rates, sr_out=48000):
    """Host side of the per-clip filters of fh_resample_poly_rates_seg_f32 for clips at `rates` (one per clip) ->
      bank      float32 numpy array: the taps of every distinct rate's tables.resample_poly_plan back to back
      rows      hip.Rate array, one row per distinct rate in order of first appearance (a rate equal to sr_out: n_taps = 0,
                up = down = 1: the copy)
      rate_of   int32 numpy array, the row of every clip."""
    distinct, rate_of = rate_index(clip_rates(rates, len(rates)))
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
    return bank, (hip.Rate * len(rows))(*rows), rate_of


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


def _launch(name, *args):
    """One library entry on the current stream."""
    hip.check(getattr(hip.lib(), name)(*args, hip.stream()), name)


def _starts(lens):
    return [int(x) for x in np.cumsum([0] + list(lens[:-1]))]


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


def resample_clip_array(tab, x_ptr, y_ptr):
    """The resampler's descriptors for the clips of `tab` (ragged_clip_tables), packed back to back at x_ptr (input) and
    y_ptr (output): the same for one input rate and for a rate per clip."""
    return clip_array(src=[x_ptr + 4 * o for o in tab["in_off"]], len_in=tab["len_in"],
                      dst=[y_ptr + 4 * o for o in tab["out_off"]], len_out=tab["len_out"])


def seg_table(row0, rows):
    return np.array([[a, b] for a, b in zip(row0, rows)], dtype=np.int32)


def _views(packed, offs, lens):
    return [packed[o:o + n] for o, n in zip(offs, lens)]


def _flat(ts):
    return [t.reshape(-1) for t in ts]


def _rfft(c, frames, out, rows, mag):
    """frames [rows, 2048] -> out [rows, .]: the P-layout spectrum, or (mag) its magnitude.  c: the device's _Const."""
    if _USE_FFT:
        _launch("fh_rfft2048_f32", _ptr(frames), _ptr(c["tw"]), _ptr(out), rows, int(mag))
    else:
        hip.gemm(frames, c["w_fwd"], out, rows, P_WIDTH, N_FFT, epilogue=hip.EPI_MAG if mag else hip.EPI_LINEAR)


def _irfft(c, spec, frames, rows):
    """P-layout spectrum [rows, .] -> frames [rows, 2048]."""
    if _USE_FFT:
        _launch("fh_irfft2048_f32", _ptr(spec), _ptr(c["tw"]), _ptr(frames), rows)
    else:
        hip.gemm(spec, c["w_inv"], frames, rows, N_FFT, P_WIDTH)


class LogMel:
    def __init__(self, device):
        self.device = hip.norm_device(device)
        self.c = _Const.get(self.device)
        self._ws = hip.ShapeCache()

    def _buffers(self, rows):
        f32 = dict(dtype=torch.float32, device=self.device)
        return torch.empty(rows, N_FFT, **f32), torch.empty(rows, MAG_WIDTH, **f32)

    def _project(self, frames, mag, mel, rows):
        """The framed clips -> log-mel rows: |STFT|, then the mel projection with its log."""
        _rfft(self.c, frames, mag, rows, mag=True)
        hip.gemm(mag, self.c["w_mel"], mel, rows, N_MELS, MAG_WIDTH, epilogue=hip.EPI_LOGCLAMP)
        return mel

    @hip.on_device
    def __call__(self, audio):
        """audio [B, T] on device -> log-mel [B*N, 256] (token-major rows), N = T // 480."""
        B, T = audio.shape
        N = T // HOP
        if N < 1 or T <= (N_FFT - HOP) // 2:
            raise ValueError(f"clip of {T} samples is too short for the mel front end")
        key = (B, T)
        if key not in self._ws:
            self._ws[key] = self._buffers(B * N)
        frames, mag = self._ws[key]
        audio = audio.contiguous()
        _launch("fh_frame_f32", _ptr(audio), _ptr(self.c["hann"]), _ptr(frames), B, T, N, N_FFT, HOP, (N_FFT - HOP) // 2, 0)
        return self._project(frames, mag, torch.empty(B * N, N_MELS, dtype=torch.float32, device=self.device), B * N)

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
            frames, mag = self._buffers(M)
            mel = torch.empty(M, N_MELS, dtype=torch.float32, device=self.device)
            self._ws[key] = dict(frames=frames, mag=mag, mel=mel, views=_views(mel, tab["mel_row0"], tab["mel_rows"]), ptrs=None)
        w = self._ws[key]
        if w["ptrs"] != ptrs:             # (clips at other addresses than last time: the descriptors go up again, one copy)
            w["desc"], (w["clips"],) = upload_tables([clip_array(src=ptrs, len_in=tab["len_out"], row0=tab["mel_row0"],
                                                                 rows=tab["mel_rows"])], self.device)
            w["ptrs"] = ptrs
        _launch("fh_frame_seg_f32", w["clips"], len(conds), max(tab["mel_rows"]), min(tab["len_out"]), _ptr(self.c["hann"]),
                _ptr(w["frames"]), N_FFT, HOP, (N_FFT - HOP) // 2, 0)
        return self._project(w["frames"], w["mag"], w["mel"], M), w["views"]


class _BatchedPost:
    """PostProcessor's own launches for B equal-length clips: pred [B, Tp], src [B, T] -> out [B, length], F frames each."""

    def __init__(self, pred, src, out, F):
        self.sig, self.out, self.B, self.F = dict(pred=pred, src=src), out, out.shape[0], F

    def frame(self, which, hann, frames):
        x = self.sig[which]
        _launch("fh_frame_f32", _ptr(x), hann, _ptr(frames), self.B, x.shape[1], self.F, N_FFT, HOP, N_FFT // 2, 1)

    def spec_energy(self, ss, energy):
        _launch("fh_spec_energy_f32", _ptr(ss), _ptr(energy), self.B, self.F)

    def spec_splice(self, sp, ss, cr):
        _launch("fh_spec_splice_f32", _ptr(sp), _ptr(ss), _ptr(cr), _ptr(sp), self.B, self.F)

    def istft_ola(self, frames, hann, peak):
        _launch("fh_istft_ola_f32", _ptr(frames), hann, _ptr(self.out), _ptr(peak), self.B, self.F, self.out.shape[1], N_FFT, HOP)

    def peak_scale(self, peak):
        _launch("fh_peak_scale_f32", _ptr(self.out), _ptr(peak), self.B, self.out.shape[1], 0.99)

    def row_gain(self, gains):
        _launch("fh_row_gain_f32", _ptr(self.out), _ptr(gains), self.B, self.out.shape[1])


class _SegmentPost:
    """The same launches for n clips of different lengths: w holds the device tables (c_pred, c_src: fh_clip arrays, seg: the
    row table); Tp, T, F, lengths are per clip."""

    def __init__(self, w, Tp, T, F, lengths):
        self.clips, self.min_len = dict(pred=w["c_pred"], src=w["c_src"]), dict(pred=min(Tp), src=min(T))
        self.seg, self.n, self.max_rows, self.max_len = w["seg"], len(F), max(F), max(lengths)

    def frame(self, which, hann, frames):
        _launch("fh_frame_seg_f32", self.clips[which], self.n, self.max_rows, self.min_len[which], hann, _ptr(frames), N_FFT, HOP,
                N_FFT // 2, 1)

    def spec_energy(self, ss, energy):
        _launch("fh_spec_energy_seg_f32", _ptr(ss), _ptr(energy), self.seg, self.n)

    def spec_splice(self, sp, ss, cr):
        _launch("fh_spec_splice_seg_f32", _ptr(sp), _ptr(ss), _ptr(cr), _ptr(sp), self.seg, self.n, self.max_rows)

    def istft_ola(self, frames, hann, peak):
        _launch("fh_istft_ola_seg_f32", _ptr(frames), hann, self.clips["src"], self.n, self.max_len, _ptr(peak), N_FFT, HOP)

    def peak_scale(self, peak):
        _launch("fh_peak_scale_seg_f32", self.clips["src"], self.n, self.max_len, _ptr(peak), 0.99)

    def row_gain(self, gains):
        _launch("fh_row_gain_seg_f32", self.clips["src"], self.n, self.max_len, _ptr(gains))


class PostProcessor:
    def __init__(self, device):
        self.device = hip.norm_device(device)
        self.c = _Const.get(self.device)
        self._ws = hip.ShapeCache()

    def _workspace(self, key, rows, n, **more):
        """The buffers of a shape (rows STFT frames of n clips), made once per key; more: what else the entry starts with."""
        if key not in self._ws:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._ws[key] = dict(frames=torch.empty(rows, N_FFT, **f32), sp=torch.empty(rows, P_WIDTH, **f32),
                                 ss=torch.empty(rows, P_WIDTH, **f32), energy=torch.empty(n, 1025, **f32),
                                 cr=torch.empty(n, dtype=torch.int32, device=self.device),
                                 peak=torch.empty(n, dtype=torch.int32, device=self.device), **more)
        return self._ws[key]

    def _level_args(self, n, gains, groups):
        """gains= / groups= of __call__ and ragged, checked: device float32 [n] / int32 [n] of this device."""
        if gains is None:
            if groups is not None:
                raise ValueError("groups= goes with gains=: the joint peak of a group is that of its rows at their own levels")
            return
        for name, t, dtype in (("gains", gains, torch.float32), ("groups", groups, torch.int32)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,)
                                  or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"{name} must be a contiguous {dtype} [{n}] on {self.device}")

    def _run(self, w, form, rows, n, gains=None, groups=None):
        """The launch sequence of both forms: per-clip cutoff, splice, iSTFT, 0.99 peak.  form: _BatchedPost or _SegmentPost.
        gains (float32 [n], every row's input peak): the iSTFT output times its row's gain instead, the signal at the input's
        level; with groups (int32 [n], non-decreasing) then scaled to 0.99 of the joint peak of every group of rows."""
        hann = _ptr(self.c["hann"])
        for which, spec in (("pred", w["sp"]), ("src", w["ss"])):
            form.frame(which, hann, w["frames"])
            _rfft(self.c, w["frames"], spec, rows, mag=False)
        form.spec_energy(w["ss"], w["energy"])
        _launch("fh_cutoff_index_f32", _ptr(w["energy"]), _ptr(w["cr"]), n, 1025, 0.99)
        form.spec_splice(w["sp"], w["ss"], w["cr"])
        _irfft(self.c, w["sp"], w["frames"], rows)
        w["peak"].zero_()
        form.istft_ola(w["frames"], hann, w["peak"])
        if gains is None:
            form.peak_scale(w["peak"])
            return
        form.row_gain(gains)
        if groups is not None:
            _launch("fh_group_peak_f32", _ptr(w["peak"]), _ptr(gains), _ptr(groups), n)
            form.peak_scale(w["peak"])

    @hip.on_device
    def __call__(self, pred, src, length, return_cr=False, gains=None, groups=None):
        """pred [B, Tp], src [B, T] -> [B, length]; per-clip cutoff, splice, iSTFT, 0.99 peak.
        gains=, groups= (_run): the rows at their inputs' levels, or at 0.99 of their group's joint peak."""
        B, Tp = pred.shape
        self._level_args(B, gains, groups)
        T = src.shape[1]
        F = min(1 + Tp // HOP, 1 + T // HOP)
        w = self._workspace((B, Tp, T, length), B * F, B)
        out = torch.empty(B, length, dtype=torch.float32, device=self.device)
        self._run(w, _BatchedPost(pred.contiguous(), src.contiguous(), out, F), B * F, B, gains, groups)
        return (out, w["cr"]) if return_cr else out

    @hip.on_device
    def ragged(self, preds, srcs, lengths, return_cr=False, gains=None, groups=None):
        """preds: list of [Tp_i] (or [1, Tp_i]) vocoder waveforms, srcs: list of [T_i] conditioning clips, lengths: samples to
        return per clip -> (output packed [sum length_i], list of the clips' [length_i] views[, cr int32 [n]]), every clip the
        bits of __call__(pred_i[None], src_i[None], length_i): per-clip cutoff, splice, iSTFT, 0.99 peak.  11 launches for the
        list.  The results belong to the workspace of this mix of lengths: a caller that keeps them clones them.
        gains=, groups= as in __call__ (one launch more than the 11, or two)."""
        preds, srcs = _flat(preds), _flat(srcs)
        lengths = [int(n) for n in lengths]
        n = len(preds)
        self._level_args(n, gains, groups)
        if len(srcs) != n or len(lengths) != n or n < 1:
            raise ValueError("one pred, one src and one length per clip")
        Tp, T = [p.shape[0] for p in preds], [s_.shape[0] for s_ in srcs]
        F = [min(1 + a // HOP, 1 + b // HOP) for a, b in zip(Tp, T)]
        key = (tuple(Tp), tuple(T), tuple(lengths))
        ptrs = tuple(_ptr(t) for t in preds + srcs)
        if key not in self._ws:
            out = torch.empty(sum(lengths), dtype=torch.float32, device=self.device)
            off = _starts(lengths)
            self._workspace(key, sum(F), n, out=out, off=off, views=_views(out, off, lengths), ptrs=None)
        w = self._ws[key]
        if w["ptrs"] != ptrs:
            row0 = _starts(F)
            outs = [w["out"].data_ptr() + 4 * o for o in w["off"]]
            w["desc"], (w["c_pred"], w["c_src"], w["seg"]) = upload_tables(
                [clip_array(src=ptrs[:n], len_in=Tp, row0=row0, rows=F),
                 clip_array(src=ptrs[n:], len_in=T, row0=row0, rows=F, dst=outs, len_out=lengths), seg_table(row0, F)], self.device)
            w["ptrs"] = ptrs
        self._run(w, _SegmentPost(w, Tp, T, F, lengths), sum(F), n, gains, groups)
        return (w["out"], w["views"], w["cr"]) if return_cr else (w["out"], w["views"])


class Resampler:
    """Device polyphase resampler + peak normalise (the reference does this on the host in numpy)."""

    def __init__(self, device):
        self.device = hip.norm_device(device)
        self._taps = {}
        self._banks = {}                  # (sr_out, distinct input rates ...) -> (device tap bank, hip.Rate rows)
        self._ws = hip.ShapeCache()

    def _filter(self, sr_out, sr_in):
        """(device address of the taps, n_taps, n_pre_remove, up, down) of one input rate; None: equal rates."""
        plan = tables.resample_poly_plan(sr_out, sr_in)
        if plan is None:
            return None
        taps, pre, up, down = plan
        key = (sr_out, sr_in)
        if key not in self._taps:
            self._taps[key] = taps.to(self.device)
        return self._taps[key].data_ptr(), self._taps[key].numel(), pre, up, down

    def _bank(self, distinct, sr_out):
        """(device tap bank, hip.Rate rows) of a tuple of distinct input rates, kept on the device per tuple."""
        key = (sr_out,) + tuple(distinct)
        if key not in self._banks:
            bank, rows, _ = rate_tables(distinct, sr_out)
            self._banks[key] = (torch.from_numpy(bank).to(self.device), rows)
        return self._banks[key]

    def _gains(self, peak, n):
        """fh_channel_peaks_f32 between the peak and the division: float32 [n] = the peaks (the caller's own tensor); a silent
        clip's slot becomes 1.0, so its samples stay exact zeros."""
        gains = torch.empty(n, dtype=torch.float32, device=self.device)
        _launch("fh_channel_peaks_f32", _ptr(peak), _ptr(gains), n)
        return gains

    @hip.on_device
    def __call__(self, x, sr_in, sr_out=48000, gains=False):
        """x [B, T_in] float32 on device -> [B, T_out], each clip divided by its max |.|.
        gains=True -> (that, float32 [B] on the device: the peaks the clips were divided by), with a silent clip left as zeros
        (its gain is 0) where the default divides 0 by 0."""
        B, n_in = x.shape
        flt = self._filter(sr_out, sr_in)
        if flt is None:
            y = x.clone()
        else:
            taps, n_taps, pre, up, down = flt
            n_out = tables.resample_out_len(n_in, sr_out, sr_in)
            y = torch.empty(B, n_out, dtype=torch.float32, device=self.device)
            x = x.contiguous()
            _launch("fh_resample_poly_f32", _ptr(x), taps, _ptr(y), B, n_in, n_out, up, down, n_taps, pre)
        peak = torch.zeros(B, dtype=torch.int32, device=self.device)
        _launch("fh_peak_abs_f32", _ptr(y), _ptr(peak), B, y.shape[1])
        g = self._gains(peak, B) if gains else None
        _launch("fh_peak_scale_f32", _ptr(y), _ptr(peak), B, y.shape[1], 1.0)
        return (y, g) if gains else y

    def _fill(self, buf, xs):
        """list of 1-D float32 clips -> the packed device buffer `buf`.  Host arrays go up as one pinned buffer and one copy."""
        if all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in xs):
            torch.cat([x.reshape(-1).to(torch.float32) for x in xs], out=buf)
            return
        xs = [x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]
        host = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in xs]))
        buf.copy_(host.pin_memory() if buf.is_cuda else host, non_blocking=True)

    @hip.on_device
    def ragged(self, xs, sr_in, sr_out=48000, gains=False):
        """xs: list of 1-D float32 clips at sr_in (host arrays: packed and uploaded with one copy; or device tensors) ->
        (the 48 kHz clips packed back to back [sum T_i], list of their [T_i] views), each resampled and divided by its
        max |.| with the bits of __call__ on that clip alone.  Four launches for the list.  The result belongs to the
        workspace of this mix of lengths: its address is the same at every call of the mix.
        sr_in may be one rate per clip: clips of different rates still run as one resampling launch, every clip with the
        polyphase filter of its own rate (fh_resample_poly_rates_seg_f32: the filter rows and every clip's row index go up
        with the clip descriptors, the tap bank is kept per tuple of distinct rates); the workspace then belongs to the mix
        of (length, rate) pairs.
        gains=True -> (packed, views, float32 [n] on the device) as in __call__; the gains are the caller's own tensor."""
        rates = clip_rates(sr_in, len(xs))
        tab = ragged_clip_tables([int(np.prod(x.shape)) for x in xs], rates, sr_out, check_mel=False)
        n, max_len = len(xs), max(tab["len_out"])
        distinct, rate_of = rate_index(rates)
        mixed = len(distinct) > 1
        key = (tuple(rates) if mixed else rates[0], sr_out, tuple(tab["len_in"]))
        if key not in self._ws:           # (input, output and descriptors belong to the mix: a mix seen before uploads only its samples)
            f32 = dict(dtype=torch.float32, device=self.device)
            x, y = torch.empty(sum(tab["len_in"]), **f32), torch.empty(sum(tab["len_out"]), **f32)
            parts = [resample_clip_array(tab, x.data_ptr(), y.data_ptr())] + ([self._bank(distinct, sr_out)[1], rate_of] if mixed else [])
            desc, (clips, *rate_tabs) = upload_tables(parts, self.device)
            self._ws[key] = dict(x=x, y=y, views=_views(y, tab["out_off"], tab["len_out"]), desc=desc, clips=clips,
                                 rate_tabs=rate_tabs, peak=torch.empty(n, dtype=torch.int32, device=self.device))
        w = self._ws[key]
        self._fill(w["x"], xs)
        if mixed:
            bank, (rows, rate_of_dev) = self._bank(distinct, sr_out)[0], w["rate_tabs"]
            _launch("fh_resample_poly_rates_seg_f32", w["clips"], rate_of_dev, n, max_len, rows, len(distinct),
                    bank.data_ptr() if bank.numel() else 0, bank.numel())
        else:
            taps, n_taps, pre, up, down = self._filter(sr_out, rates[0]) or (0, 0, 0, 1, 1)
            _launch("fh_resample_poly_seg_f32", w["clips"], n, max_len, taps, up, down, n_taps, pre)
        w["peak"].zero_()
        _launch("fh_peak_abs_seg_f32", w["clips"], n, max_len, _ptr(w["peak"]))
        g = self._gains(w["peak"], n) if gains else None
        _launch("fh_peak_scale_seg_f32", w["clips"], n, max_len, _ptr(w["peak"]), 1.0)
        return (w["y"], w["views"], g) if gains else (w["y"], w["views"])

    @hip.on_device
    def upload_packed(self, conds):
        """conds: list of 1-D float32 host clips that are 48 kHz already (resampled and normalised on the host,
        upsampling_method='scipy') -> (packed device tensor [sum T_i], views): one pinned buffer, one copy, into the
        workspace of this mix of lengths."""
        lens = [int(np.prod(c.shape)) for c in conds]
        key = ("host",) + tuple(lens)
        if key not in self._ws:
            y = torch.empty(sum(lens), dtype=torch.float32, device=self.device)
            self._ws[key] = dict(y=y, views=_views(y, _starts(lens), lens))
        w = self._ws[key]
        self._fill(w["y"], conds)
        return w["y"], w["views"]
