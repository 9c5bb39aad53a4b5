"""What delivery on the device buys a serving caller: wall time from the call to int16 PCM at 44.1 kHz on the HOST, for
  device   generate_batch(..., output_rate=44100, pcm='int16', interleaved=True) and the device-to-host copy of the int16 result
  host     what a caller does on the interface without the keywords: generate_batch at 48 kHz, .cpu(), scipy.signal.resample_poly
           to 44.1 kHz, 0.99 peak, numpy scale / round / clip to int16, transpose to [T, C]
for B = 1 and B = 8 clips of 10 s, mono and stereo.  One process, alternating rounds, medians and quartiles; the encoder's and the
output resampler's own time from device events.  Writes profiles/delivery.md (or the path given).

python tools/delivery_bench.py [--rounds 20] [--out profiles/delivery.md]"""
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
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth, tables          # noqa: E402

SR_IN, RATE, SECONDS = 12000, 44100, 10.0


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
    """The caller's side of today's interface, per clip: y48 float32 [C, T48] on the host -> int16 [T, C] at RATE."""
    y = scipy.signal.resample_poly(y48, RATE, 48000, axis=-1)
    peak = np.abs(y).max()
    y = y / peak * np.float32(0.99) if peak > 0 else y
    return np.clip(np.rint(y * np.float32(32768)), -32768, 32767).astype(np.int16).T.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "delivery.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("delivery_bench needs a GPU")
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
                return [y.cpu().numpy() for y in m.generate_batch(clips, SR_IN, output_rate=RATE, pcm="int16", interleaved=True, **kw)]

            def host():
                return [host_finish(y.cpu().numpy()) for y in m.generate_batch(clips, SR_IN, **kw)]

            def plain():
                return [y.cpu() for y in m.generate_batch(clips, SR_IN, **kw)]

            got, want = device(), host()
            assert all(g.shape == w.shape and g.dtype == w.dtype for g, w in zip(got, want))
            lsb = max(int(np.abs(g.astype(np.int32) - w.astype(np.int32)).max()) for g, w in zip(got, want))
            variants = dict(device=device, host=host, plain=plain)
            for fn in variants.values():
                for _ in range(2):
                    fn()
            # the delivery launches alone, from device events, on rows like the post-processor's
            y48 = torch.randn(B * C, frames * 480, device=dev) * 0.1
            opt = dict(rate=RATE, pcm="int16", keys=None, interleaved=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def kernels_ms(reps=10):
                e0.record()
                for _ in range(reps):
                    m.delivery.batch(y48, [C] * B, "peak", opt, range(B))
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps
            kernels_ms()
            t = {k: [] for k in variants}
            kern = []
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    t[k].append(wall(fn))
                kern.append(kernels_ms())
            rows.append((B, C, {k: (statistics.median(v), quartiles(v)) for k, v in t.items()}, statistics.median(kern), lsb))
            print(B, C, {k: round(statistics.median(v), 2) for k, v in t.items()}, "delivery launches ms", round(rows[-1][3], 3),
                  "max |device - host| LSB", lsb, flush=True)
    t_out = tables.resample_out_len(frames * 480, RATE, 48000)
    lines = ["# Delivery on the device: int16 at 44.1 kHz on the host, two ways", "",
             f"`python tools/delivery_bench.py --rounds {a.rounds}` on {torch.cuda.get_device_name(0)} (host: {cpu_name()}), torch {torch.__version__}, "
             f"scipy {scipy.__version__}.  SYNTH_CFG, {SECONDS:.0f} s clips at {SR_IN} Hz, euler x 1, `upsampling_method='hip'`; {t_out} samples per "
             "channel come back.  Wall time from the call to the int16 `[T, C]` arrays on the host, ms: median (quartiles) of "
             f"{a.rounds} alternating rounds in one process.", "",
             "- **device**: `generate_batch(..., output_rate=44100, pcm='int16', interleaved=True)` + `.cpu()` of the int16 result",
             "- **host**: `generate_batch(...)` at 48 kHz + `.cpu()` + `scipy.signal.resample_poly` + 0.99 peak + numpy quantise and transpose",
             "- **48 kHz float**: `generate_batch(...)` + `.cpu()` alone, what both start from", "",
             "| B | C | device | host | 48 kHz float | delivery launches alone (device events) | max abs(device - host), LSB |", "|---|---|---|---|---|---|---|"]
    for B, C, t, kern, lsb in rows:
        cell = lambda k: f"{t[k][0]:.2f} ({t[k][1][0]:.2f}-{t[k][1][1]:.2f})"          # noqa: E731
        lines.append(f"| {B} | {C} | {cell('device')} | {cell('host')} | {cell('plain')} | {kern:.3f} | {lsb} |")
    lines += ["", "The two results differ by rounding only (the device resamples in float32 with fused multiply-adds, scipy in its "
              "own order): the last column is the largest difference in int16 steps."]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
