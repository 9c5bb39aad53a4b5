"""What loudness on the device buys a serving caller: wall time from the call to int16 PCM at 44.1 kHz and -16 LUFS on the HOST, for
  device   generate_batch(..., output_rate=44100, loudness=-16, pcm='int16', interleaved=True) and the copy of the int16 result
  host     what a caller does without the keyword: generate_batch at 48 kHz, .cpu(), scipy.signal.resample_poly to 44.1 kHz,
           loudness.normalise (the float64 BS.1770 meter and the gain), numpy round / clip to int16, transpose to [T, C]
for B = 1 and B = 8 clips of 10 s, mono and stereo.  One process, alternating rounds, medians and quartiles; the loudness
launches alone from device events; the sub-energy kernel's GB/s on a single 120 s mono row and on 16 rows of 10 s, beside
fh_peak_abs_f32 over the same bytes.  Writes profiles/loudness.md (or the path given); --test-log: the output of
`pytest -m gpu -s tests/test_hip_loudness.py`, whose "loudness:" lines (the worst error ratios) are copied in.

python tools/loudness_bench.py [--rounds 10] [--out profiles/loudness.md] [--test-log LOG]"""
import argparse
import platform
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.signal
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import FLowHigh, FlowHighSR, delivery, hip, loudness, synth, tables          # noqa: E402

SR_IN, RATE, SECONDS, TARGET = 12000, 44100, 10.0, -16.0


def cpu_name():
    try:
        for ln in Path("/proc/cpuinfo").read_text().splitlines():
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def wall(fn):
    """Host clock from the call to the result on the host, ms."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def quartiles(v):
    s = sorted(v)
    return s[len(s) // 4], s[(3 * len(s)) // 4]


def host_finish(y48):
    """The caller's side of today's interface, per clip: y48 float32 [C, T48] on the host -> int16 [T, C] at RATE and TARGET."""
    y = scipy.signal.resample_poly(y48, RATE, 48000, axis=-1)
    peak = np.abs(y).max()
    y = (y / peak * np.float32(0.99) if peak > 0 else y).astype(np.float32)
    y, _, _ = loudness.normalise(y, RATE, TARGET)
    return np.clip(np.rint(y * np.float32(32768)), -32768, 32767).astype(np.int16).T.copy()


def events_ms(fn, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_rates(dev):
    """The sub-energy kernel alone: (rows, seconds, ms, GB/s of the float32 read, fh_peak_abs_f32's ms and GB/s on the same rows)."""
    L, out = hip.lib(), []
    hop, _ = loudness.geometry(48000)
    coef = delivery._coef(48000)
    for rows, seconds in ((1, 120), (16, 10), (64, 10)):
        T = seconds * 48000
        x = torch.randn(rows, T, device=dev) * 0.1
        e = torch.empty(rows, -(-T // hop), dtype=torch.float64, device=dev)
        peak = torch.zeros(rows, dtype=torch.int32, device=dev)
        ms = statistics.median(events_ms(lambda: hip.check(L.fh_kweight_energy_f32(x.data_ptr(), coef, e.data_ptr(), rows, T, hop, hip.stream()),
                                                           "fh_kweight_energy_f32"), reps=5) for _ in range(5))
        pk = statistics.median(events_ms(lambda: hip.check(L.fh_peak_abs_f32(x.data_ptr(), peak.data_ptr(), rows, T, hip.stream()),
                                                           "fh_peak_abs_f32"), reps=5) for _ in range(5))
        gb = rows * T * 4 / 1e9
        out.append((rows, seconds, ms, gb / (ms * 1e-3), pk, gb / (pk * 1e-3)))
        print("energy kernel", out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "loudness.md"))
    ap.add_argument("--test-log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_bench needs a GPU")
    dev = torch.device("cuda:0")
    cfg = synth.SYNTH_CFG
    m = FlowHighSR(FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev), torchdiffeq_ode_method="euler", upsampling_method="hip")
    n_in = int(SECONDS * SR_IN)
    frames = n_in * 4 // 480
    rows = []
    for B in (1, 8):
        for C in (1, 2):
            clips = [np.stack([synth.lowres_clip(10 * b + c, SECONDS, SR_IN)[:n_in] for c in range(C)]) for b in range(B)]
            noise = torch.cat([synth.prior_noise(b, frames) for b in range(B)], 0)          # [B, N, n_mels]: one draw per clip
            kw = dict(noise=noise, channels="first")

            def device():
                return [y.cpu().numpy() for y in m.generate_batch(clips, SR_IN, output_rate=RATE, loudness=TARGET, pcm="int16",
                                                                  interleaved=True, **kw)]

            def host():
                return [host_finish(y.cpu().numpy()) for y in m.generate_batch(clips, SR_IN, **kw)]

            def plain():
                return [y.cpu().numpy() for y in m.generate_batch(clips, SR_IN, output_rate=RATE, pcm="int16", interleaved=True, **kw)]

            got, want = device(), host()
            assert all(g.shape == w.shape and g.dtype == w.dtype for g, w in zip(got, want))
            lsb = max(int(np.abs(g.astype(np.int32) - w.astype(np.int32)).max()) for g, w in zip(got, want))
            read = [loudness.integrated(g.T.astype(np.float64) / 32768.0, RATE) for g in got]
            variants = dict(device=device, host=host, plain=plain)
            for fn in variants.values():
                for _ in range(2):
                    fn()
            # the loudness launches alone (peaks, sub-energies, gate, row gain), from device events, on rows like the resampler's
            y = torch.randn(B * C, tables.resample_out_len(frames * 480, RATE, 48000), device=dev) * 0.1
            opt = dict(rate=None, pcm=None, keys=None, interleaved=False, loudness=TARGET)
            m.delivery.measure(y, [C] * B, RATE)
            t = {k: [] for k in variants}
            kern = []
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    t[k].append(wall(fn))
                # (batch() with loudness= alone clones the rows first: the clone is timed with it, as a caller pays for it)
                kern.append(events_ms(lambda: m.delivery.batch(y, [C] * B, "peak", opt, range(B))))
            rows.append((B, C, {k: (statistics.median(v), quartiles(v)) for k, v in t.items()}, statistics.median(kern), lsb,
                         (min(read), max(read))))
            print(B, C, {k: round(statistics.median(v), 2) for k, v in t.items()}, "loudness launches ms", round(rows[-1][3], 3),
                  "max |device - host| LSB", lsb, "delivered LUFS", rows[-1][5], flush=True)
    rates = kernel_rates(dev)
    t_out = tables.resample_out_len(frames * 480, RATE, 48000)
    lines = ["# Loudness on the device: int16 at 44.1 kHz and -16 LUFS on the host, two ways", "",
             f"`python tools/loudness_bench.py --rounds {a.rounds}` on {torch.cuda.get_device_name(0)} (host: {cpu_name()}), torch {torch.__version__}, "
             f"scipy {scipy.__version__}.  SYNTH_CFG, {SECONDS:.0f} s clips at {SR_IN} Hz, euler x 1, `upsampling_method='hip'`; {t_out} samples per "
             "channel come back.  Wall time from the call to the int16 `[T, C]` arrays on the host, ms: median (quartiles) of "
             f"{a.rounds} alternating rounds in one process.", "",
             f"- **device**: `generate_batch(..., output_rate=44100, loudness={TARGET:g}, pcm='int16', interleaved=True)` + `.cpu()` of the int16 result",
             "- **host**: `generate_batch(...)` at 48 kHz + `.cpu()` + `scipy.signal.resample_poly` + 0.99 peak + `loudness.normalise` "
             "(the float64 meter) + numpy quantise and transpose: what a caller does without the keyword",
             "- **device, no loudness**: the device call without `loudness=`, what the keyword is added to", "",
             "| B | C | device | host | device, no loudness | loudness launches alone (device events) | max abs(device - host), LSB | delivered, LUFS (float64 meter on the int16) |",
             "|---|---|---|---|---|---|---|---|"]
    for B, C, t, kern, lsb, read in rows:
        cell = lambda k: f"{t[k][0]:.2f} ({t[k][1][0]:.2f}-{t[k][1][1]:.2f})"          # noqa: E731
        lines.append(f"| {B} | {C} | {cell('device')} | {cell('host')} | {cell('plain')} | {kern:.3f} | {lsb} | {read[0]:.3f} .. {read[1]:.3f} |")
    lines += ["", "The loudness launches are the rows' peaks (`fh_peak_abs_f32`), the K-weighted sub-block energies (`fh_kweight_energy_f32`), "
              "the gate and gain (`fh_loudness_gate_f32`) and the row gain (`fh_row_gain_f32`), with the copy that keeps the gain off the "
              "post-processor's buffer.  The two results differ by rounding only (resampling in float32 on the device, scipy in its own order; "
              "a gain computed from a float32 loudness).", "",
              "## The sub-energy kernel alone", "",
              "`fh_kweight_energy_f32` at 48 kHz, device events, median of 5 x 5 launches; GB/s counts the 4 bytes per sample it reads.  "
              "`fh_peak_abs_f32` over the same rows is the streaming kernel it runs beside.", "",
              "| rows | seconds per row | sub-energies, ms | GB/s | fh_peak_abs_f32, ms | GB/s |", "|---|---|---|---|---|---|"]
    for r, s, ms, gbs, pk, pgbs in rates:
        lines.append(f"| {r} | {s} | {ms:.3f} | {gbs:.2f} | {pk:.3f} | {pgbs:.1f} |")
    one, many = rates[0], rates[-1]
    lines += ["", f"One workgroup walks a row span by span ({one[2] / (one[1] * 48000 / 4096) * 1e3:.1f} us per span of 4096 samples: two dependent float64 "
              "chains of 16 samples, 8 scan steps with a barrier each), so a single row is latency-bound and far below the streaming kernels: "
              f"{one[3]:.1f} GB/s on the {one[1]} s row against {many[3]:.0f} GB/s once {many[0]} rows run side by side, where it is within "
              f"{many[2] / many[4]:.1f}x of `fh_peak_abs_f32` (whose single-row figure is a cache-resident read).  Decision: the three-launch form "
              "(zero-state end states per span, a scan over spans, a re-run) is NOT built.  It would spread one long row over the device, "
              f"but the case it helps is a single clip of minutes, where {one[2]:.1f} ms stands beside the model's own time for such a clip, a dozen times that of a 10 s clip "
              "(a 10 s clip takes 15 ms end to end), while a serving batch already has one workgroup per row and pays "
              "0.5 to 0.7 ms for all four launches, inside the run-to-run spread of the call.  What it would have to beat is the table above."]
    if a.test_log:
        found = [ln.strip().lstrip(".") for ln in Path(a.test_log).read_text().splitlines() if "loudness: " in ln]
        lines += ["", "## What the GPU tests printed", "", "`pytest -m gpu -s tests/test_hip_loudness.py`: the worst error against the "
                  "float64 definition, as a fraction of each test's bar (energies: 1e-9 relative per sub-block), and the model-level readings.", "", "```"]
        lines += found + ["```"]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
