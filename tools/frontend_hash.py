"""sha256 of every output of a fixed, seeded list of launches of the front / back end entries (csrc/frontend.hip): run once per
library (FH_LIB_PATH) in a fresh process and compare the two listings -- a refactor of these kernels must not move a bit.
    python tools/frontend_hash.py [out_file]            one line per output: <name> <sha256>
  b3.*     every batched entry on a batch of 3 equal-length clips: 2401 samples at 48 kHz (5 mel frames, 6 post-processing
           frames), the resampler on 601 samples at 12 kHz and 22 050 Hz, spec_energy over 70 rows, the mel entries at d = 256 / 40
  seg3.*   the segment entries on a table that describes the same three clips
  seg5.*   the segment entries on five clips of 600 / 1500 / 2401 / 2401 / 3000 samples at 12 kHz (the list of
           tests/test_hip_ragged_ends.py), the resampler also at 22 050 Hz, at 48 kHz (the copy) and with a rate per clip
  peak.*   both peak_abs entries past the 1024-block cap of their grid
  model.*  one generate() and one generate_many(ends='ragged') on TINY_CFG
Outputs are NaN-filled before the launch and hashed whole, guard included."""
import hashlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth, tables      # noqa: E402
from flowhigh_amd import frontend as FE                                # noqa: E402
from flowhigh_amd.tables import HOP, N_FFT, P_WIDTH                    # noqa: E402

LINES, KEEP = [], []
GUARD = 64
LENS5, RATES5 = [600, 1500, 2401, 2401, 3000], [12000, 22050, 48000, 8000, 22050]


def rnd(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def p(t, first=0):
    return t.data_ptr() + 4 * first


def call(name, *args):
    hip.check(getattr(hip.lib(), name)(*args, hip.stream()), name)


def dev(*parts):
    buf, addrs = FE.upload_tables(list(parts), torch.device("cuda"))
    KEEP.append(buf)
    return addrs


def emit(name, *outs):
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        LINES.append(f"{name}{'.' + str(i) if len(outs) > 1 else ''} {hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest()}")


def starts(v):
    return [sum(v[:i]) for i in range(len(v))]


def clip_set(tag, lens, seed):
    """Every clip-wise entry on clips of `lens` samples at 48 kHz: tag 'b3' = the batched entries (equal lengths), else the
    segment entries."""
    n, batched = len(lens), tag == "b3"
    T = lens[0]
    hann = FE._Const.get("cuda")["hann"]
    off = starts(lens)
    x = rnd(sum(lens), seed, 0.3)
    mel_rows, pp_rows = [t // HOP for t in lens], [1 + t // HOP for t in lens]
    for mode, pad, pm, rows in (("reflect", (N_FFT - HOP) // 2, 0, mel_rows), ("zero", N_FFT // 2, 1, pp_rows)):
        f = nan(sum(rows) + 1, N_FFT)
        if batched:
            call("fh_frame_f32", p(x), p(hann), p(f), n, T, rows[0], N_FFT, HOP, pad, pm)
        else:
            (clips,) = dev(FE.clip_array(src=[p(x, o) for o in off], len_in=lens, row0=starts(rows), rows=rows))
            call("fh_frame_seg_f32", clips, n, max(rows), min(lens), p(hann), p(f), N_FFT, HOP, pad, pm)
        emit(f"{tag}.frame.{mode}", f)
    # spectra: the post-processing rows, and 70 rows per clip for the energy sum
    rows = pp_rows
    R = sum(rows)
    (seg,) = dev(FE.seg_table(starts(rows), rows))
    erows = [70 + 9 * i for i in range(n)] if not batched else [70] * n
    (eseg,) = dev(FE.seg_table(starts(erows), erows))
    spec = rnd(sum(erows) * P_WIDTH, seed + 1).view(-1, P_WIDTH)
    e = nan(n + 1, 1025)
    if batched:
        call("fh_spec_energy_f32", p(spec), p(e), n, erows[0])
    else:
        call("fh_spec_energy_seg_f32", p(spec), p(e), eseg, n)
    emit(f"{tag}.spec_energy", e)
    cr = torch.tensor([31, 300, 777, 0, 1025][:n], dtype=torch.int32, device="cuda")
    pred, src, o = rnd(R * P_WIDTH, seed + 2).view(R, P_WIDTH), rnd(R * P_WIDTH, seed + 3).view(R, P_WIDTH), nan(R + 1, P_WIDTH)
    if batched:
        call("fh_spec_splice_f32", p(pred), p(src), p(cr), p(o), n, rows[0])
    else:
        call("fh_spec_splice_seg_f32", p(pred), p(src), p(cr), p(o), seg, n, max(rows))
    emit(f"{tag}.spec_splice", o)
    fr, y, peak = rnd(R * N_FFT, seed + 4).view(R, N_FFT), nan(sum(lens) + GUARD), torch.zeros(n, dtype=torch.int32, device="cuda")
    (clips,) = dev(FE.clip_array(dst=[p(y, o_) for o_ in off], len_out=lens, row0=starts(rows), rows=rows))
    if batched:
        call("fh_istft_ola_f32", p(fr), p(hann), p(y), p(peak), n, rows[0], T, N_FFT, HOP)
    else:
        call("fh_istft_ola_seg_f32", p(fr), p(hann), clips, n, max(lens), p(peak), N_FFT, HOP)
    emit(f"{tag}.istft_ola", y, peak)
    y, peak = torch.cat([x, nan(GUARD)]), torch.zeros(n, dtype=torch.int32, device="cuda")
    (clips,) = dev(FE.clip_array(dst=[p(y, o_) for o_ in off], len_out=lens))
    if batched:
        call("fh_peak_abs_f32", p(y), p(peak), n, T)
        call("fh_peak_scale_f32", p(y), p(peak), n, T, 0.99)
    else:
        call("fh_peak_abs_seg_f32", clips, n, max(lens), p(peak))
        call("fh_peak_scale_seg_f32", clips, n, max(lens), p(peak), 0.99)
    emit(f"{tag}.peak", y, peak)
    for d in (256, 40):
        rows = mel_rows
        R = sum(rows)
        (seg,) = dev(FE.seg_table(starts(rows), rows))
        low, high = rnd(R * d, seed + 5).view(R, d), rnd(R * d, seed + 6).view(R, d)
        cut = torch.tensor([3, 17, 39, 0, 40][:n], dtype=torch.int32, device="cuda")
        e, o = nan(n + 1, d), nan(R + 1, d)
        if batched:
            call("fh_mel_energy_f32", p(low), p(e), n, rows[0], d)
            call("fh_mel_splice_f32", p(low), p(high), p(cut), p(o), n, rows[0], d)
        else:
            call("fh_mel_energy_seg_f32", p(low), p(e), seg, n, d)
            call("fh_mel_splice_seg_f32", p(low), p(high), p(cut), p(o), seg, n, max(rows), d)
        emit(f"{tag}.mel.d{d}", e, o)


def resample(tag, lens, rates, seed, form):
    """form 'b': fh_resample_poly_f32 (equal lengths, one rate), 'seg': the one-rate segment entry, 'rates': a filter per clip."""
    n = len(lens)
    tab = FE.ragged_clip_tables(lens, rates, check_mel=False)
    x, y = rnd(sum(lens), seed, 0.2), nan(sum(tab["len_out"]) + GUARD)
    clip_tab = FE.clip_array(src=[p(x, o) for o in tab["in_off"]], len_in=tab["len_in"], dst=[p(y, o) for o in tab["out_off"]],
                             len_out=tab["len_out"])
    if form == "rates":
        bank, rows, rate_of = FE.rate_tables(rates)
        bank = torch.from_numpy(bank).cuda()
        clips, rows_dev, rate_of_dev = dev(clip_tab, rows, rate_of)
        call("fh_resample_poly_rates_seg_f32", clips, rate_of_dev, n, max(tab["len_out"]), rows_dev, len(rows), p(bank), bank.numel())
    else:
        plan = tables.resample_poly_plan(48000, rates[0])
        taps, pre, up, down = (plan[0].cuda(), *plan[1:]) if plan is not None else (None, 0, 1, 1)
        if form == "b":
            call("fh_resample_poly_f32", p(x), p(taps), p(y), n, lens[0], tab["len_out"][0], up, down, taps.numel(), pre)
        else:
            (clips,) = dev(clip_tab)
            call("fh_resample_poly_seg_f32", clips, n, max(tab["len_out"]), p(taps) if taps is not None else 0, up, down,
                 taps.numel() if taps is not None else 0, pre)
    emit(tag, y)


def capped_peak():
    lens = [1024 * 256 + 300, 300]
    xs = [rnd(n, 70 + i, 0.3) for i, n in enumerate(lens)]
    (clips,) = dev(FE.clip_array(dst=[p(v) for v in xs], len_out=lens))
    peak, ref = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    call("fh_peak_abs_seg_f32", clips, 2, max(lens), p(peak))
    for i, v in enumerate(xs):
        call("fh_peak_abs_f32", p(v), p(ref, i), 1, v.numel())
    emit("peak.capped", peak, ref)


def model():
    m = FlowHighSR(FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda"), torchdiffeq_ode_method="euler",
                   upsampling_method="hip")
    secs = [0.5, 1.31, 0.2, 0.7713, 0.05]
    clips = [synth.lowres_clip(140 + i, s_, 12000) for i, s_ in enumerate(secs)]
    noise = [synth.prior_noise(140 + i, (len(c) * 4) // 480) for i, c in enumerate(clips)]
    emit("model.generate", m.generate(clips[1], 12000, 48000, 1, noise=noise[1]))
    emit("model.generate_many.ragged_ends", *m.generate_many(clips, 12000, 48000, 1, noise=noise, ends="ragged"))
    rates = [12000, 16000, 12000, 24000, 8000]
    noise = [synth.prior_noise(150 + i, tables.resample_out_len(len(c), 48000, r) // 480) for i, (c, r) in enumerate(zip(clips, rates))]
    emit("model.generate_many.ragged_ends.rates", *m.generate_many(clips, rates, 48000, 1, noise=noise, ends="ragged"))


def main():
    clip_set("b3", [2401] * 3, 100)
    clip_set("seg3", [2401] * 3, 100)
    clip_set("seg5", FE.ragged_clip_tables(LENS5, 12000)["len_out"], 200)
    for sr in (12000, 22050):
        resample(f"b3.resample.{sr}", [601] * 3, [sr] * 3, 300, "b")
        resample(f"seg3.resample.{sr}", [601] * 3, [sr] * 3, 300, "seg")
    for sr in (12000, 22050, 48000):
        resample(f"seg5.resample.{sr}", LENS5, [sr] * 5, 400, "seg")
    resample("seg5.resample.rates", LENS5, RATES5, 400, "rates")
    capped_peak()
    model()
    text = "\n".join(LINES) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text)
    print(text + f"{len(LINES)} outputs, all: {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
