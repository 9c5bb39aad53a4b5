"""What the true-peak ceiling and the look-ahead limiter add to a delivery on the device: int16 PCM at 44.1 kHz and -4 LUFS on the
HOST, wall time from the call, for
  loudness   generate_batch(..., output_rate=44100, loudness=-4, pcm='int16', interleaved=True): the chain of profiles/loudness.md, at a
             target its 0.99 cap binds on, so that the three deliveries differ in what they deliver as well
  static     the same with true_peak=-1: one more gain from the 4x oversampled peak
  limiter    the same with true_peak=-1, limiter='lookahead': the uncapped loudness gain, the envelope and the limiter
for B = 1 and B = 8 clips of 10 s, mono and stereo.  One process, alternating rounds, medians and quartiles; the added launches alone
from device events on rows like the resampler's; and the three kernels alone against fh_peak_abs_f32 over the same bytes.  Writes
profiles/truepeak.md (or the path given); --test-log: the outputs of `pytest -s tests/test_truepeak_cpu.py` and
`pytest -m gpu -s tests/test_hip_truepeak.py`, whose "truepeak:" lines are copied in.

python tools/truepeak_bench.py [--rounds 10] [--out profiles/truepeak.md] [--test-log LOG ...]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import FLowHigh, FlowHighSR, hip, loudness, synth, tables, truepeak          # noqa: E402

SR_IN, RATE, SECONDS, TARGET, CEILING = 12000, 44100, 10.0, -4.0, -1.0            # (a target the 0.99 cap binds on: SYNTH_CFG's clips read -4.7 dBTP at -16 LUFS)


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


def events_ms(fn, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_rates(m, dev):
    """The kernels alone at 48 kHz: (rows, seconds, {kernel: ms}, GB of float32 the rows hold)."""
    L, out = hip.lib(), []
    taps, H = m.delivery._tp_taps(), truepeak.half_window(48000)
    w, c32 = m.delivery._window(H), float(np.float32(truepeak.ceiling(CEILING)))
    for rows, seconds in ((1, 120), (16, 10), (64, 10)):
        T = seconds * 48000
        x = torch.randn(rows, T, device=dev) * 0.3
        y = torch.empty_like(x)
        env = torch.empty(rows, T, device=dev)
        peak = torch.zeros(rows, dtype=torch.int32, device=dev)
        calls = {
            "fh_peak_abs_f32": lambda: L.fh_peak_abs_f32(x.data_ptr(), peak.data_ptr(), rows, T, hip.stream()),
            "fh_true_peak_f32": lambda: L.fh_true_peak_f32(x.data_ptr(), taps, peak.data_ptr(), rows, T, hip.stream()),
            "fh_tp_envelope_f32": lambda: L.fh_tp_envelope_f32(x.data_ptr(), taps, env.data_ptr(), rows, 1, T, hip.stream()),
            "fh_limit_f32": lambda: L.fh_limit_f32(x.data_ptr(), y.data_ptr(), env.data_ptr(), w, 0, rows, 1, T, H, c32, hip.stream()),
        }
        ms = {}
        for name, call in calls.items():
            ms[name] = statistics.median(events_ms(lambda: hip.check(call(), name), reps=5) for _ in range(5))
        out.append((rows, seconds, ms, rows * T * 4 / 1e9))
        print("kernels", rows, seconds, {k: round(v, 3) for k, v in ms.items()}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "truepeak.md"))
    ap.add_argument("--test-log", nargs="*", default=[])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("truepeak_bench needs a GPU")
    dev = torch.device("cuda:0")
    cfg = synth.SYNTH_CFG
    m = FlowHighSR(FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev), torchdiffeq_ode_method="euler", upsampling_method="hip")
    n_in = int(SECONDS * SR_IN)
    frames = n_in * 4 // 480
    t_out = tables.resample_out_len(frames * 480, RATE, 48000)
    deliveries = dict(loudness=dict(), static=dict(true_peak=CEILING), limiter=dict(true_peak=CEILING, limiter="lookahead"))
    rows = []
    for B in (1, 8):
        for C in (1, 2):
            clips = [np.stack([synth.lowres_clip(10 * b + c, SECONDS, SR_IN)[:n_in] for c in range(C)]) for b in range(B)]
            noise = torch.cat([synth.prior_noise(b, frames) for b in range(B)], 0)
            kw = dict(noise=noise, channels="first", output_rate=RATE, loudness=TARGET, pcm="int16", interleaved=True)
            variants = {k: (lambda d=d: [y.cpu().numpy() for y in m.generate_batch(clips, SR_IN, **kw, **d)]) for k, d in deliveries.items()}
            read = {}
            for k, fn in variants.items():
                got = [g.T.astype(np.float32) / np.float32(32768.0) for g in fn()]
                fn()
                read[k] = (max(float(truepeak.dbtp(truepeak.true_peak(g))) for g in got),
                           min(loudness.integrated(g, RATE) for g in got), max(loudness.integrated(g, RATE) for g in got))
            y = torch.randn(B * C, t_out, device=dev) * 0.1
            opts = {k: dict(rate=None, pcm=None, keys=None, interleaved=False, loudness=TARGET,
                            **({"true_peak": d["true_peak"], "limiter": d.get("limiter")} if d else {})) for k, d in deliveries.items()}
            t = {k: [] for k in variants}
            kern = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    t[k].append(wall(fn))
                for k, opt in opts.items():
                    # (batch() clones the rows first: the clone is timed with it, as a caller pays for it)
                    kern[k].append(events_ms(lambda: m.delivery.batch(y, [C] * B, "peak", opt, range(B))))
            rows.append((B, C, {k: (statistics.median(v), quartiles(v)) for k, v in t.items()},
                         {k: statistics.median(v) for k, v in kern.items()}, read))
            print(B, C, {k: round(statistics.median(v), 2) for k, v in t.items()}, {k: round(v, 3) for k, v in rows[-1][3].items()}, read, flush=True)
    rates = kernel_rates(m, dev)
    lines = [f"# True peak and limiter on the device: what they add to a delivery at 44.1 kHz and {TARGET:g} LUFS", "",
             f"`python tools/truepeak_bench.py --rounds {a.rounds}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  SYNTH_CFG, "
             f"{SECONDS:.0f} s clips at {SR_IN} Hz, euler x 1, `upsampling_method='hip'`; {t_out} samples per channel come back.  Wall time from "
             f"the call to the int16 `[T, C]` arrays on the host, ms: median (quartiles) of {a.rounds} alternating rounds in one process.  "
             "No bar is set on these numbers: they were unmeasured before.", "",
             f"- **loudness**: `generate_batch(..., output_rate=44100, loudness={TARGET:g}, pcm='int16', interleaved=True)`, the chain of `profiles/loudness.md` "
             "(there at -16 LUFS; here at a target its 0.99 cap binds on, so that the three differ in what they deliver; the launches are the same)",
             f"- **static**: the same with `true_peak={CEILING:g}`", f"- **limiter**: the same with `true_peak={CEILING:g}, limiter='lookahead'`", "",
             "| B | C | loudness | static | limiter | delivery launches alone, loudness / static / limiter (device events) | delivered dBTP, loudness / static / limiter | delivered LUFS, loudness / static / limiter |",
             "|---|---|---|---|---|---|---|---|"]
    for B, C, t, kern, read in rows:
        cell = lambda k: f"{t[k][0]:.2f} ({t[k][1][0]:.2f}-{t[k][1][1]:.2f})"          # noqa: E731
        lines.append(f"| {B} | {C} | {cell('loudness')} | {cell('static')} | {cell('limiter')} | "
                     + " / ".join(f"{kern[k]:.3f}" for k in deliveries) + " | " + " / ".join(f"{read[k][0]:+.3f}" for k in deliveries) + " | "
                     + " / ".join(f"{read[k][1]:.2f} .. {read[k][2]:.2f}" for k in deliveries) + " |")
    lines += ["", "The static rule adds `fh_true_peak_f32` and `fh_delivery_gain_f32` (the gate then only measures); the limiter adds "
              "`fh_delivery_gain_f32`, `fh_row_gain_f32`, `fh_tp_envelope_f32` and `fh_limit_f32`.  The delivered figures are read by the float64 "
              "definitions off the int16 result (quantisation moves a true peak by up to 2^-16 of full scale per tap).", "",
              "## The kernels alone", "", "48 kHz rows, one channel per clip, device events, median of 5 x 5 launches, ms; `fh_peak_abs_f32` over the "
              "same rows is the streaming kernel they run beside.", "",
              "| rows | seconds per row | GB | fh_peak_abs_f32 | fh_true_peak_f32 | fh_tp_envelope_f32 | fh_limit_f32 (H = 240) |", "|---|---|---|---|---|---|---|"]
    for r, s, ms, gb in rates:
        lines.append(f"| {r} | {s} | {gb:.3f} | {ms['fh_peak_abs_f32']:.3f} | {ms['fh_true_peak_f32']:.3f} | {ms['fh_tp_envelope_f32']:.3f} | {ms['fh_limit_f32']:.3f} |")
    found = [ln.strip().lstrip(".") for p in a.test_log for ln in Path(p).read_text().splitlines() if "truepeak: " in ln]
    if found:
        lines += ["", "## What the tests printed", "", "`pytest -s tests/test_truepeak_cpu.py` and `pytest -m gpu -s tests/test_hip_truepeak.py`: the "
                  "definition's own readings (the re-measured true peak of the limiter's results relative to the ceiling among them) and the worst "
                  "error of the kernels against the definition, as a fraction of each test's bar.", "", "```"] + found + ["```"]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
