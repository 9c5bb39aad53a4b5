"""Delivery: what generate*(output_rate=, pcm=, dither=, interleaved=) do to the post-processed 48 kHz result, on the device.

  48 kHz rows -> resample_poly to the output rate (the input side's kernels with the (R, 48000) plan)
              -> level='peak': 0.99 of the clip's own peak again, jointly over its channels (the 48 kHz path's peak kernels)
              -> loudness=L:  the clip put at L LUFS at the delivered rate (csrc/loudness.hip; loudness.py is the definition):
                              the rows' peaks, the K-weighted sub-block energies, the gate and gain, the row gain
              -> true_peak=T: the clip held under T dBTP (csrc/truepeak.hip; truepeak.py is the definition): one gain from its
                              4x oversampled peak, or with limiter='lookahead' the oversampled envelope and the look-ahead
                              limiter (behind the UNCAPPED loudness gain where loudness= is given as well)
              -> pcm='int16': one launch of fh_pcm_i16_f32 / fh_pcm_i16_seg_f32 (csrc/pcm.hip; pcm.py is the definition)
                 pcm='s24', 's24in32': one launch of fh_pcm_s24_f32 / fh_pcm_s24_seg_f32: 24-bit samples packed in 3 bytes
                              (uint8 [..., 3], the pcm_s24le layout) or sign-extended in an int32

`batch` runs the batched entries over clips of one length, `ragged` the segment forms over a group of clips of different
lengths; rows are read where the post-processor left them, and a clip gets the same bits from either.  With every keyword at
its default nothing here runs.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from . import hip, tables
from . import loudness as _loudness
from . import pcm as _pcm_def
from . import quality as _quality
from . import truepeak as _truepeak
from .frontend import _launch, _ptr, clip_array, upload_tables
from .prior import expand_seed

MAX_RATE_FACTOR = 640             # max(up, down) of the reduced output_rate / 48000: the filter has 20 * that + 1 taps
# pcm -> (the result's dtype, bytes per sample, the entries' stem); the 24-bit entries take the bytes per sample as `container`
PCM_FORMATS = {"int16": (torch.int16, 2, "i16"), "s24": (torch.uint8, 3, "s24"), "s24in32": (torch.int32, 4, "s24")}
assert tuple(PCM_FORMATS) == _pcm_def.FORMATS
_PCM = (None, *PCM_FORMATS)
_DITHER = (None, "tpdf")
_PCM_ENTRIES = {"batched": "fh_pcm_{}_f32", "segment": "fh_pcm_{}_seg_f32", "stream mono": "fh_stream_pcm_{}_f32",
                "stream rows": "fh_stream_pcm_{}_rows_f32"}


@functools.lru_cache(maxsize=None)
def pcm_entry(pcm, form):
    """The encode launch of a format in one of its forms ('batched', 'segment', 'stream mono', 'stream rows') -> (the entry's
    name, the arguments behind `interleaved`: the 24-bit entries' container).  The 24-bit formats have no mono stream entry: a
    mono stream is a group of one job of 'stream rows'."""
    _, size, stem = PCM_FORMATS[pcm]
    name = _PCM_ENTRIES[form].format(stem)
    if name not in hip.EXPORTS:
        raise ValueError(f"pcm={pcm!r} has no {form} entry")
    return name, ((size,) if stem == "s24" else ())


def pcm_buffer(pcm, samples, device):
    """The encoder's output buffer for `samples` samples: int16 / int32 [samples], or uint8 [3 * samples]."""
    dtype, size, _ = PCM_FORMATS[pcm]
    return torch.empty(samples * size // dtype.itemsize, dtype=dtype, device=device)


def pcm_shape(pcm, *shape):
    """The shape of an encoded block of `shape` samples: 's24' holds a sample as a last axis of 3 bytes."""
    return tuple(shape) + ((3,) if pcm == "s24" else ())


def resolve_output_rate(output_rate):
    """output_rate= -> None (48 kHz: nothing to do) or the rate R as an int.  R is a positive integer whose reduced ratio
    up / down = R / 48000 has max(up, down) <= 640 (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 88200, 96000, ...)."""
    if output_rate is None:
        return None
    r = output_rate
    if isinstance(r, (bool, str, bytes)) or not isinstance(r, (int, np.integer, float)) or r != r or int(r) != r or int(r) <= 0:
        raise ValueError(f"output_rate must be None or a positive integer, got {output_rate!r}")
    r = int(r)
    if r == 48000:
        return None
    g = math.gcd(r, 48000)
    if max(r // g, 48000 // g) > MAX_RATE_FACTOR:
        raise ValueError(f"output_rate={r}: {r} / 48000 reduces to {r // g} / {48000 // g}; the larger of the two must be "
                         f"at most {MAX_RATE_FACTOR} (e.g. 8000, 16000, 22050, 32000, 44100, 96000)")
    return r


def resolve_delivery(n_clips, output_rate=None, pcm=None, dither=None, dither_seed=0, interleaved=False, *, loudness=None,
                     level="peak", true_peak=None, limiter=None):
    """The delivery keywords of a call over n_clips clips, checked (ValueError, before any GPU work) ->
    None when they are all at their defaults, else dict(rate: None | R, pcm, keys: None | one (seed, stream) per clip,
    interleaved), with the key "loudness" (the target in LUFS) only when loudness= is given, and the keys "true_peak" (the ceiling
    in dBTP) and "limiter" only when true_peak= is given.  level: the call's level=, which loudness= has to agree with
    (true_peak= goes with either level: its rule only attenuates)."""
    rate = resolve_output_rate(output_rate)
    target = _loudness.resolve_loudness(loudness)
    ceiling, limiter = _truepeak.resolve_true_peak(true_peak, limiter, 48000 if rate is None else rate)
    if target is not None:
        if level == "input":
            raise ValueError("loudness= and level='input' are two rules for one gain: loudness= goes with level='peak'")
        _loudness.geometry(48000 if rate is None else rate)
    if pcm not in _PCM:
        raise ValueError(f"pcm must be one of {_PCM}, got {pcm!r}")
    if dither not in _DITHER:
        raise ValueError(f"dither must be one of {_DITHER}, got {dither!r}")
    if dither is not None and pcm is None:
        raise ValueError("dither= goes with pcm=: a float result is not quantised")
    if interleaved not in (False, True):
        raise ValueError(f"interleaved must be a bool, got {interleaved!r}")
    if interleaved and pcm is None:
        raise ValueError("interleaved=True goes with pcm=: the float result is planar")
    keys = None
    if dither is not None:
        try:
            keys = expand_seed(dither_seed, n_clips)
        except TypeError as e:
            raise ValueError(f"dither_seed: {e}") from e
    if rate is None and pcm is None and target is None and ceiling is None:
        return None
    opt = dict(rate=rate, pcm=pcm, keys=keys, interleaved=bool(interleaved))
    if target is not None:
        opt["loudness"] = target
    if ceiling is not None:
        opt["true_peak"] = ceiling
        opt["limiter"] = limiter
    return opt


def delivered_len(t48, output_rate=None):
    """Samples per channel of a delivered clip whose 48 kHz result has t48."""
    rate = resolve_output_rate(output_rate)
    return int(t48) if rate is None else tables.resample_out_len(int(t48), rate, 48000)


class Delivery:
    def __init__(self, device, resampler):
        self.device = hip.norm_device(device)
        self.resampler = resampler            # its tap cache holds the (R, 48000) filters beside the input side's
        self._windows = {}                    # half window H -> the limiter's device double [2 H + 1]
        self._fft = None                      # measure_quality's window and twiddles

    def _keys(self, opt, which):
        """Device int64 [n, 2] of the clips `which` of the call, or None without dither."""
        if opt["keys"] is None:
            return None
        host = np.array([[opt["keys"][i][0], opt["keys"][i][1]] for i in which], dtype=np.uint64).view(np.int64)
        return torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)

    def _rows(self, t):
        if t.dtype != torch.float32 or t.ndim != 2 or t.device != self.device:
            raise ValueError(f"delivery takes float32 [rows, T] on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t if t.stride(1) == 1 or t.shape[1] == 1 else t.contiguous()

    @hip.on_device
    def batch(self, rows, chans, level, opt, which, packed=False):
        """rows [R, T48]: the channels of len(chans) clips of one length, in clip order; which: the clips' indices in the
        call (their dither keys).  -> list of the clips' results, [C_i, T] float32 / int16, or [T, C_i] int16 interleaved:
        views of one buffer in clip order.  packed (mono clips only): that buffer instead, [R, T], or [R, T, 1] interleaved.
        pcm='s24in32': int32 in the int16 shapes; pcm='s24': uint8 with a last axis of 3 bytes ([C_i, T, 3], [T, C_i, 3])."""
        rows = self._rows(rows).contiguous()
        R, n = rows.shape[0], len(chans)
        if sum(chans) != R or (packed and R != n):
            raise ValueError(f"{R} rows for clips of {chans} channels")
        y = rows
        if opt["rate"] is not None:
            taps, n_taps, pre, up, down = self.resampler._filter(opt["rate"], 48000)
            T = tables.resample_out_len(rows.shape[1], opt["rate"], 48000)
            y = torch.empty(R, T, dtype=torch.float32, device=self.device)
            _launch("fh_resample_poly_f32", _ptr(rows), taps, _ptr(y), R, rows.shape[1], T, up, down, n_taps, pre)
            if level == "peak":
                peak = torch.zeros(R, dtype=torch.int32, device=self.device)
                _launch("fh_peak_abs_f32", _ptr(y), _ptr(peak), R, T)
                self._group_peak(peak, chans)
                _launch("fh_peak_scale_f32", _ptr(y), _ptr(peak), R, T, 0.99)
        T = y.shape[1]
        target, ceiling = opt.get("loudness"), opt.get("true_peak")
        if (target is not None or ceiling is not None) and y is rows:
            y = rows.clone()                 # (the rows belong to the post-processor's plan: the gain goes onto the caller's own copy)
        rate = opt["rate"] or 48000
        lufs = peak = None
        if target is not None:
            peak = torch.zeros(R, dtype=torch.int32, device=self.device)
            _launch("fh_peak_abs_f32", _ptr(y), _ptr(peak), R, T)
            hop, energies = self._energies(rate, R, T)
            _launch("fh_kweight_energy_f32", _ptr(y), _coef(rate), _ptr(energies), R, T, hop)
            # (with true_peak= the gate only measures: the gain is composed by fh_delivery_gain_f32)
            lufs, gains = self._gate(energies, [T] * R, chans, hop, None if ceiling is not None else target, peak)
            if ceiling is None:
                _launch("fh_row_gain_f32", _ptr(y), _ptr(gains), R, T)
        if ceiling is not None:
            group = self._group(chans)
            if opt["limiter"] is None:
                tp = torch.zeros(R, dtype=torch.int32, device=self.device)
                _launch("fh_true_peak_f32", _ptr(y), self._tp_taps(), _ptr(tp), R, T)
                gains = self._delivery_gain(lufs, target, peak, tp, group, R, n, ceiling, False)
                _launch("fh_row_gain_f32", _ptr(y), _ptr(gains), R, T)
            else:
                if target is not None:
                    gains = self._delivery_gain(lufs, target, None, None, group, R, n, ceiling, True)
                    _launch("fh_row_gain_f32", _ptr(y), _ptr(gains), R, T)
                H, c32 = _truepeak.half_window(rate), float(np.float32(_truepeak.ceiling(ceiling)))
                m = torch.empty(n, T, dtype=torch.float32, device=self.device)
                if len(set(chans)) == 1:
                    _launch("fh_tp_envelope_f32", _ptr(y), self._tp_taps(), _ptr(m), n, chans[0], T)
                    _launch("fh_limit_f32", _ptr(y), _ptr(y), _ptr(m), self._window(H), 0, n, chans[0], T, H, c32)
                else:                  # clips of different channel counts: the segment forms, in place
                    table = (hip.PcmClip * n)(*[hip.PcmClip(y.data_ptr() + 4 * T * r, 0, T, c, T) for r, c in zip(_starts(chans), chans)])
                    desc, (clips,) = upload_tables([table], self.device)
                    _launch("fh_tp_envelope_seg_f32", clips, n, T, self._tp_taps(), _ptr(m))
                    _launch("fh_limit_seg_f32", clips, n, T, _ptr(m), self._window(H), 0, H, c32)
        if opt["pcm"] is None:
            return y if packed else list(y.split(chans))
        out = pcm_buffer(opt["pcm"], R * T, self.device)
        keys = self._keys(opt, which)
        if len(set(chans)) == 1:
            entry, tail = pcm_entry(opt["pcm"], "batched")
            _launch(entry, _ptr(y), _ptr(out), hip.ptr(keys), n, chans[0], T, int(opt["interleaved"]), *tail)
        else:                      # clips of different channel counts: the segment form, the rows still where they are
            self._pcm_seg([y.data_ptr() + 4 * T * r for r in _starts(chans)], [T] * n, chans, [T] * n, out, keys, opt)
        if packed:
            return out.view(pcm_shape(opt["pcm"], R, T, 1) if opt["interleaved"] else pcm_shape(opt["pcm"], R, T))
        return _clip_views(out, chans, [T] * n, opt["interleaved"], opt["pcm"])

    def _group_peak(self, peak, chans):
        """The rows' peak slots -> the joint peak of every clip in all of its rows' slots; a silent clip's becomes 1.0, so the
        scaling leaves its zeros (fh_group_peak_f32 with every gain 1: fl(q * 1) = q)."""
        R = sum(chans)
        group = self._group(chans)
        _launch("fh_group_peak_f32", _ptr(peak), _ptr(torch.ones(R, dtype=torch.float32, device=self.device)), _ptr(group), R)

    def _group(self, chans):
        """Device int32 [rows]: the clip of every row."""
        return torch.from_numpy(np.repeat(np.arange(len(chans), dtype=np.int32), chans)).pin_memory().to(self.device, non_blocking=True)

    def _tp_taps(self):
        """The device taps of the 4x oversampling: the resampler's own (4, 1) filter, from its tap cache."""
        taps, n_taps, pre, up, down = self.resampler._filter(4 * 48000, 48000)
        assert (n_taps, pre, up, down) == (_truepeak.N_TAPS + 1, 4 * _truepeak.HALF + 1, 4, 1)
        return taps

    def _window(self, H):
        """The limiter's Hann weights for the half window H as a device double [2 H + 1], made once per H."""
        if H not in self._windows:
            self._windows[H] = torch.from_numpy(_truepeak.window(H)).to(self.device)
        return self._windows[H].data_ptr()

    def _delivery_gain(self, lufs, target, peak, tp, group, R, n, ceiling, uncapped, dbtp=None):
        """fh_delivery_gain_f32 -> gains [R] (None when only dbtp is asked for); ceiling in dBTP; group: a device int32 [R] tensor or
        its address."""
        gains = None if dbtp is not None else torch.empty(R, dtype=torch.float32, device=self.device)
        _launch("fh_delivery_gain_f32", hip.ptr(lufs), float("nan") if target is None else float(target), hip.ptr(peak), hip.ptr(tp),
                group if isinstance(group, int) else _ptr(group), R, n, 1.0 if ceiling is None else _truepeak.ceiling(ceiling),
                int(uncapped), hip.ptr(gains), hip.ptr(dbtp))
        return gains

    def _energies(self, rate, rows, max_len):
        hop, _ = _loudness.geometry(rate)
        return hop, torch.empty(rows, -(-max_len // hop), dtype=torch.float64, device=self.device)

    def _gate(self, energies, row_len, chans, hop, target, peak):
        """fh_loudness_gate_f32 over rows that are chans[i] per clip -> (lufs [n_clips], gains [rows]); target None: measure."""
        R, n = len(row_len), len(chans)
        host = np.concatenate([np.asarray(row_len, dtype=np.int32), np.repeat(np.arange(n, dtype=np.int32), chans)])
        tab = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
        lufs = torch.empty(n, dtype=torch.float32, device=self.device)
        gains = torch.empty(R, dtype=torch.float32, device=self.device)
        _launch("fh_loudness_gate_f32", _ptr(energies), energies.shape[1], _ptr(tab[:R]), _ptr(tab[R:]), R, n, hop,
                float("nan") if target is None else float(target), _ptr(peak), _ptr(lufs), _ptr(gains))
        return lufs, gains

    def _loudness_seg(self, srcs, pitches, chans, lens, rate, target, row_table=None):
        """The segment forms over clips read where they are (clip i: chans[i] rows of lens[i] floats, pitches[i] apart, from
        srcs[i]) -> (lufs, gains); row_table: the fh_clip per row (dst, len_out) the peak entry takes, made here when None."""
        seg = self._seg_tables(srcs, pitches, chans, lens, row_table)
        lufs, gains, _ = self._loudness_on(seg, chans, lens, rate, target)
        return (lufs, gains), seg["rows"]

    def _seg_tables(self, srcs, pitches, chans, lens, row_table=None):
        """The device tables of a group of clips read where they are -> dict(keep, clips: the fh_pcm_clip table (dst NULL), group:
        int32 [rows], rows: the fh_clip per row, row_len)."""
        n = len(chans)
        row_len = [t for t, c in zip(lens, chans) for _ in range(c)]
        group = np.repeat(np.arange(n, dtype=np.int32), chans)
        pcm_table = (hip.PcmClip * n)(*[hip.PcmClip(int(s), 0, int(p), int(c), int(t))
                                        for s, p, c, t in zip(srcs, pitches, chans, lens)])
        tables_ = [pcm_table, group]
        if row_table is None:
            tables_.append(clip_array(dst=[s + 4 * p * r for s, p, c in zip(srcs, pitches, chans) for r in range(c)], len_out=row_len))
        desc, ptrs = upload_tables(tables_, self.device)
        return dict(keep=desc, clips=ptrs[0], group=ptrs[1], rows=ptrs[2] if len(ptrs) == 3 else row_table, row_len=row_len)

    def _loudness_on(self, seg, chans, lens, rate, target):
        """The loudness launches over _seg_tables' tables -> (lufs, gains, the rows' peak slots)."""
        R, n, max_len = sum(chans), len(chans), max(lens)
        peak = torch.zeros(R, dtype=torch.int32, device=self.device)
        _launch("fh_peak_abs_seg_f32", seg["rows"], R, max_len, _ptr(peak))
        hop, energies = self._energies(rate, R, max_len)
        _launch("fh_kweight_energy_seg_f32", seg["clips"], seg["group"], n, R, max_len, _coef(rate), _ptr(energies), hop)
        return (*self._gate(energies, seg["row_len"], chans, hop, target, peak), peak)

    @hip.on_device
    def measure(self, rows, chans=None, rate=48000):
        """FlowHighSR.measure_loudness: float32 [R, T] rows (chans[i] per clip; None: every row a clip) or a list of [C_i, T_i]
        tensors -> float32 [n_clips] LUFS on the device: the kernels of loudness= with no target."""
        hop, _ = _loudness.geometry(rate)            # (any integer rate with a sub-block of 16 samples or more, not only output rates)
        rate = int(rate)
        if isinstance(rows, torch.Tensor):
            rows = self._rows(rows).contiguous()
            R, T = rows.shape
            chans = [1] * R if chans is None else [int(c) for c in chans]
            if sum(chans) != R or min(chans, default=0) < 1 or T < 1:
                raise ValueError(f"{R} rows of {T} samples for clips of {chans} channels")
            peak = torch.zeros(R, dtype=torch.int32, device=self.device)
            _launch("fh_peak_abs_f32", _ptr(rows), _ptr(peak), R, T)
            hop, energies = self._energies(rate, R, T)
            _launch("fh_kweight_energy_f32", _ptr(rows), _coef(rate), _ptr(energies), R, T, hop)
            return self._gate(energies, [T] * R, chans, hop, None, peak)[0]
        if chans is not None:
            raise ValueError("chans= goes with one [R, T] tensor: a list holds one [C_i, T_i] tensor per clip")
        clips = [self._rows(c) for c in rows]
        if not clips or min(min(c.shape) for c in clips) < 1:
            raise ValueError("measure_loudness takes at least one clip, every clip at least one sample")
        (lufs, _), _ = self._loudness_seg([c.data_ptr() for c in clips], [c.stride(0) for c in clips], [c.shape[0] for c in clips],
                                         [c.shape[1] for c in clips], rate, None)
        return lufs

    def _report(self, energies, row_len, chans, hop):
        """fh_loudness_report_f32 over rows that are chans[i] per clip -> float32 [n_clips, 6] (meter.FIELDS)."""
        R, n = len(row_len), len(chans)
        host = np.concatenate([np.asarray(row_len, dtype=np.int32), np.repeat(np.arange(n, dtype=np.int32), chans)])
        tab = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
        report = torch.empty(n, 6, dtype=torch.float32, device=self.device)
        _launch("fh_loudness_report_f32", _ptr(energies), energies.shape[1], _ptr(tab[:R]), _ptr(tab[R:]), R, n, hop, _ptr(report))
        return report

    @hip.on_device
    def measure_report(self, rows, chans=None, rate=48000):
        """FlowHighSR.measure_loudness_report: rows, chans and rate as measure() takes them -> float32 [n_clips, 6] on the device:
        integrated, momentary maximum, short-term maximum, range, last momentary, last short-term (meter.py is the definition).
        Column 0 has the bits of measure()."""
        hop, _ = _loudness.geometry(rate)
        rate = int(rate)
        if isinstance(rows, torch.Tensor):
            rows = self._rows(rows).contiguous()
            R, T = rows.shape
            chans = [1] * R if chans is None else [int(c) for c in chans]
            if sum(chans) != R or min(chans, default=0) < 1 or T < 1:
                raise ValueError(f"{R} rows of {T} samples for clips of {chans} channels")
            hop, energies = self._energies(rate, R, T)
            _launch("fh_kweight_energy_f32", _ptr(rows), _coef(rate), _ptr(energies), R, T, hop)
            return self._report(energies, [T] * R, chans, hop)
        if chans is not None:
            raise ValueError("chans= goes with one [R, T] tensor: a list holds one [C_i, T_i] tensor per clip")
        clips = [self._rows(c) for c in rows]
        if not clips or min(min(c.shape) for c in clips) < 1:
            raise ValueError("measure_loudness_report takes at least one clip, every clip at least one sample")
        chans, lens = [c.shape[0] for c in clips], [c.shape[1] for c in clips]
        seg = self._seg_tables([c.data_ptr() for c in clips], [c.stride(0) for c in clips], chans, lens, row_table=0)
        hop, energies = self._energies(rate, sum(chans), max(lens))
        _launch("fh_kweight_energy_seg_f32", seg["clips"], seg["group"], len(chans), sum(chans), max(lens), _coef(rate),
                _ptr(energies), hop)
        return self._report(energies, seg["row_len"], chans, hop)

    @hip.on_device
    def measure_true_peak(self, rows, chans=None, rate=48000):
        """FlowHighSR.measure_true_peak: rows as measure() takes them -> float32 [n_clips] dBTP on the device (-inf for silence):
        fh_true_peak_f32 / fh_true_peak_seg_f32 and the joint maximum of fh_delivery_gain_f32."""
        if isinstance(rate, (bool, str, bytes)) or int(rate) != rate or int(rate) <= 0:
            raise ValueError(f"rate must be a positive integer, got {rate!r}")          # (the factor is 4 at every rate)
        if isinstance(rows, torch.Tensor):
            rows = self._rows(rows).contiguous()
            R, T = rows.shape
            chans = [1] * R if chans is None else [int(c) for c in chans]
            if sum(chans) != R or min(chans, default=0) < 1 or T < 1:
                raise ValueError(f"{R} rows of {T} samples for clips of {chans} channels")
            tp = torch.zeros(R, dtype=torch.int32, device=self.device)
            _launch("fh_true_peak_f32", _ptr(rows), self._tp_taps(), _ptr(tp), R, T)
            group = self._group(chans)
        else:
            if chans is not None:
                raise ValueError("chans= goes with one [R, T] tensor: a list holds one [C_i, T_i] tensor per clip")
            clips = [self._rows(c) for c in rows]
            if not clips or min(min(c.shape) for c in clips) < 1:
                raise ValueError("measure_true_peak takes at least one clip, every clip at least one sample")
            chans, lens = [c.shape[0] for c in clips], [c.shape[1] for c in clips]
            R = sum(chans)
            seg = self._seg_tables([c.data_ptr() for c in clips], [c.stride(0) for c in clips], chans, lens, row_table=0)
            tp = torch.zeros(R, dtype=torch.int32, device=self.device)
            _launch("fh_true_peak_seg_f32", seg["clips"], seg["group"], len(chans), R, max(lens), self._tp_taps(), _ptr(tp))
            group = seg["group"]
        dbtp = torch.empty(len(chans), dtype=torch.float32, device=self.device)
        self._delivery_gain(None, None, None, tp, group, R, len(chans), None, False, dbtp=dbtp)
        return dbtp

    def _fft_tables(self):
        """(the device Hann window, the device twiddles) of the quality report's STFT, uploaded once."""
        if self._fft is None:
            self._fft = (tables.hann_window().to(self.device), tables.fft_twiddles().to(self.device))
        return self._fft[0].data_ptr(), self._fft[1].data_ptr()

    @hip.on_device
    def measure_quality(self, rows, ref_rows, chans=None, rate=48000, cutoff_hz=None):
        """FlowHighSR.measure_quality: an estimate and its reference, float32 [R, T] rows (chans[i] per clip; None: every row a
        clip) or two lists of [C_i, T_i] tensors of equal shapes pair by pair -> float32 [n_clips, 4] on the device: lsd, lsd_low,
        lsd_high, snr_db (quality.py is the definition).  cutoff_hz: None, one positive number, or one per clip.  Everything is
        checked before the first launch.  Rows of one length and one cutoff run the batched entry, anything else the segment
        form, read where the rows are; a clip gets the same bits from either."""
        batched = isinstance(rows, torch.Tensor) or isinstance(ref_rows, torch.Tensor)
        if batched:
            if not (isinstance(rows, torch.Tensor) and isinstance(ref_rows, torch.Tensor)):
                raise ValueError("measure_quality takes two [R, T] tensors or two lists of [C_i, T_i] tensors")
            est, ref = [rows], [ref_rows]
        else:
            if chans is not None:
                raise ValueError("chans= goes with two [R, T] tensors: a list holds one [C_i, T_i] tensor per clip")
            est, ref = list(rows), list(ref_rows)
            if not est or len(est) != len(ref):
                raise ValueError(f"measure_quality takes at least one clip and a reference for every clip, got {len(est)} and {len(ref)}")
        for e, r in zip(est, ref):
            for t in (e, r):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 2 or t.device != self.device:
                    raise ValueError(f"measure_quality takes float32 [rows, T] on {self.device}, got "
                                     f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
            if e.shape != r.shape or min(e.shape) < 1:
                raise ValueError(f"an estimate and its reference have one shape of at least one row and one sample, got "
                                 f"{tuple(e.shape)} and {tuple(r.shape)}")
        if batched:
            R, T = rows.shape
            chans = [1] * R if chans is None else [int(c) for c in chans]
            if sum(chans) != R or min(chans, default=0) < 1:
                raise ValueError(f"{R} rows of {T} samples for clips of {chans} channels")
            lens = [T] * len(chans)
        else:
            chans, lens = [e.shape[0] for e in est], [e.shape[1] for e in est]
        n, R, max_len = len(chans), sum(chans), max(lens)
        if R > 65535 or max_len > 2 ** 30:
            raise ValueError(f"measure_quality takes up to 65535 rows of up to 2^30 samples, got {R} rows, {max_len} samples")
        kcs = _quality_bins(cutoff_hz, rate, n)
        window, tw = self._fft_tables()
        F = _quality.n_frames(max_len)
        frames = torch.empty(R, F, 5, dtype=torch.float64, device=self.device)
        row_len = np.repeat(np.asarray(lens, dtype=np.int32), chans)
        group = np.repeat(np.arange(n, dtype=np.int32), chans)
        if batched and len(set(kcs)) == 1:
            e, r = rows.contiguous(), ref_rows.contiguous()
            desc, (p_len, p_group) = upload_tables([row_len, group], self.device)
            _launch("fh_quality_frames_f32", _ptr(e), _ptr(r), window, tw, _ptr(frames), R, max_len, kcs[0])
        else:
            if batched:                                # (one cutoff per clip: the clips as views of the two tensors)
                est, ref = list(rows.split(chans)), list(ref_rows.split(chans))
            est, ref = [self._rows(e) for e in est], [self._rows(r) for r in ref]
            table = (hip.QualityClip * n)(*[hip.QualityClip(e.data_ptr(), r.data_ptr(), e.stride(0), r.stride(0), c, t, k, 0)
                                            for e, r, c, t, k in zip(est, ref, chans, lens, kcs)])
            desc, (p_clips, p_len, p_group) = upload_tables([table, row_len, group], self.device)
            _launch("fh_quality_frames_seg_f32", p_clips, ctypes.addressof(table), p_group, n, R, max_len, window, tw, _ptr(frames))
        report = torch.empty(n, 4, dtype=torch.float32, device=self.device)
        _launch("fh_quality_report_f32", _ptr(frames), F, p_len, p_group, R, n, _ptr(report))
        return report

    def _pcm_seg(self, srcs, pitches, chans, lens, out, keys, opt):
        size, (entry, tail) = PCM_FORMATS[opt["pcm"]][1], pcm_entry(opt["pcm"], "segment")
        off = _starts([c * t for c, t in zip(chans, lens)])
        table = (hip.PcmClip * len(chans))(*[hip.PcmClip(int(s), out.data_ptr() + size * o, int(p), int(c), int(t))
                                            for s, o, p, c, t in zip(srcs, off, pitches, chans, lens)])
        desc, (clips,) = upload_tables([table], self.device)
        _launch(entry, clips, len(chans), max(chans), max(lens), hip.ptr(keys), int(opt["interleaved"]), *tail)

    @hip.on_device
    def ragged(self, clips, level, opt, which):
        """clips: list of [C_i, T48_i] device tensors (any row pitch: views of the post-processor's buffers) -> list of the
        clips' results as in `batch`, each the bits of batch() on that clip alone.  One launch per step for the group."""
        clips = [self._rows(c) for c in clips]
        chans, n = [c.shape[0] for c in clips], len(clips)
        srcs, pitches, lens = [c.data_ptr() for c in clips], [c.stride(0) for c in clips], [c.shape[1] for c in clips]
        if opt["rate"] is not None:
            flt = self.resampler._filter(opt["rate"], 48000)
            taps, n_taps, pre, up, down = flt
            out_lens = [tables.resample_out_len(t, opt["rate"], 48000) for t in lens]
            row_in = [s + 4 * p * r for s, p, c in zip(srcs, pitches, chans) for r in range(c)]
            row_len_in = [t for t, c in zip(lens, chans) for _ in range(c)]
            row_len = [t for t, c in zip(out_lens, chans) for _ in range(c)]
            y = torch.empty(sum(row_len), dtype=torch.float32, device=self.device)
            row_off = _starts(row_len)
            desc, (table,) = upload_tables([clip_array(src=row_in, len_in=row_len_in, len_out=row_len,
                                                       dst=[y.data_ptr() + 4 * o for o in row_off])], self.device)
            R, max_len = len(row_len), max(row_len)
            _launch("fh_resample_poly_seg_f32", table, R, max_len, taps, up, down, n_taps, pre)
            if level == "peak":
                peak = torch.zeros(R, dtype=torch.int32, device=self.device)
                _launch("fh_peak_abs_seg_f32", table, R, max_len, _ptr(peak))
                self._group_peak(peak, chans)
                _launch("fh_peak_scale_seg_f32", table, R, max_len, _ptr(peak), 0.99)
            first = _starts(chans)
            srcs, pitches, lens = [y.data_ptr() + 4 * row_off[r] for r in first], out_lens, out_lens
        target, ceiling = opt.get("loudness"), opt.get("true_peak")
        if target is not None or ceiling is not None:
            if opt["rate"] is None:
                # (views of the post-processor's buffers: the gain goes onto the caller's own copy, one buffer for the group)
                y = torch.cat([c.reshape(-1) for c in clips])
                row_off = _starts([t for t, c in zip(lens, chans) for _ in range(c)])
                first = _starts(chans)
                srcs, pitches, table = [y.data_ptr() + 4 * row_off[r] for r in first], lens, None
            R, max_len, rate = sum(chans), max(lens), opt["rate"] or 48000
            seg = self._seg_tables(srcs, pitches, chans, lens, table)
            lufs = peak = None
            if target is not None:
                lufs, gains, peak = self._loudness_on(seg, chans, lens, rate, None if ceiling is not None else target)
                if ceiling is None:
                    _launch("fh_row_gain_seg_f32", seg["rows"], R, max_len, _ptr(gains))
            if ceiling is not None and opt["limiter"] is None:
                tp = torch.zeros(R, dtype=torch.int32, device=self.device)
                _launch("fh_true_peak_seg_f32", seg["clips"], seg["group"], n, R, max_len, self._tp_taps(), _ptr(tp))
                gains = self._delivery_gain(lufs, target, peak, tp, seg["group"], R, n, ceiling, False)
                _launch("fh_row_gain_seg_f32", seg["rows"], R, max_len, _ptr(gains))
            elif ceiling is not None:
                if target is not None:
                    gains = self._delivery_gain(lufs, target, None, None, seg["group"], R, n, ceiling, True)
                    _launch("fh_row_gain_seg_f32", seg["rows"], R, max_len, _ptr(gains))
                H, c32 = _truepeak.half_window(rate), float(np.float32(_truepeak.ceiling(ceiling)))
                m = torch.empty(n, max_len, dtype=torch.float32, device=self.device)
                _launch("fh_tp_envelope_seg_f32", seg["clips"], n, max_len, self._tp_taps(), _ptr(m))
                _launch("fh_limit_seg_f32", seg["clips"], n, max_len, _ptr(m), self._window(H), 0, H, c32)
        if opt["rate"] is not None or target is not None or ceiling is not None:
            if opt["pcm"] is None:
                return [y[row_off[r]:row_off[r] + c * t].view(c, t) for r, c, t in zip(first, chans, lens)]
        out = pcm_buffer(opt["pcm"], sum(c * t for c, t in zip(chans, lens)), self.device)
        self._pcm_seg(srcs, pitches, chans, lens, out, self._keys(opt, which), opt)
        return _clip_views(out, chans, lens, opt["interleaved"], opt["pcm"])


_COEF = {}


def _coef(rate):
    """The K-weighting of `rate` as the host double [10] the energy entries read during the call (kept: the address is passed)."""
    if rate not in _COEF:
        _COEF[rate] = (ctypes.c_double * 10)(*_loudness.coefficients(rate))
    return ctypes.addressof(_COEF[rate])


def _starts(lens):
    return [int(x) for x in np.cumsum([0] + list(lens[:-1]))]


def _quality_bins(cutoff_hz, rate, n_clips):
    """measure_quality's cutoff_hz (None, one number, or one per clip) -> the cutoff bin of every clip, -1 without a cutoff."""
    if cutoff_hz is None or np.ndim(cutoff_hz) == 0:
        cut = [cutoff_hz] * n_clips
    else:
        cut = list(cutoff_hz)
        if len(cut) != n_clips:
            raise ValueError(f"one cutoff_hz per clip: {len(cut)} for {n_clips} clips")
    for c in cut:
        if c is not None and (isinstance(c, (bool, str, bytes)) or not isinstance(c, (int, float, np.integer, np.floating))):
            raise ValueError(f"cutoff_hz must be None or finite and positive, got {c!r}")
    return [-1 if c is None else _quality.cutoff_bin(c, rate) for c in cut]


def _clip_views(out, chans, lens, interleaved, pcm="int16"):
    """The clips of a packed result buffer: [C, T] planar, [T, C] interleaved; 's24' (uint8, 3 bytes a sample): [C, T, 3], [T, C, 3]."""
    views, o, k = [], 0, 3 if pcm == "s24" else 1
    for c, t in zip(chans, lens):
        v = out[o:o + k * c * t]
        views.append(v.view(pcm_shape(pcm, t, c) if interleaved else pcm_shape(pcm, c, t)))
        o += k * c * t
    return views
