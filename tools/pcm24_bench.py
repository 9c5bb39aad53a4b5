"""The encode launch of delivery in its three formats, alone, from device events:
  int16     fh_pcm_i16_f32 / fh_pcm_i16_seg_f32 (unchanged by the 24-bit work: the launch as it was)
  s24       fh_pcm_s24_f32 / fh_pcm_s24_seg_f32 with container 3: 3 bytes a sample
  s24in32   the same with container 4: an int32 a sample
on one 10 s clip at 48 kHz (batched entry) and on 24 such clips (segment entry), C = 2, planar and interleaved, with and without
dither.  One process, the three alternating in every round; medians and quartiles over the rounds, each round the mean of `reps`
back-to-back launches.  Beside it the whole step: generate(...) with and without pcm='s24' on SYNTH_CFG.
Writes profiles/pcm24.md (or the path given).

python tools/pcm24_bench.py [--rounds 20] [--out profiles/pcm24.md]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth                  # noqa: E402
from flowhigh_amd.delivery import PCM_FORMATS, pcm_entry                   # noqa: E402
from flowhigh_amd.frontend import upload_tables                            # noqa: E402

T, C, SECONDS = 480000, 2, 10.0
FORMATS = tuple(PCM_FORMATS)


def quartiles(v):
    s = sorted(v)
    return s[len(s) // 4], s[(3 * len(s)) // 4]


def launcher(n_clips, fmt, interleaved, dither, x, keys):
    """-> a function that queues the encode launch of n_clips clips [C, T] in the format, and its output buffer."""
    name, size = fmt, PCM_FORMATS[fmt][1]
    entry, tail = pcm_entry(name, "batched" if n_clips == 1 else "segment")
    call = getattr(hip.lib(), entry)
    out = torch.empty(n_clips * C * T * size, dtype=torch.uint8, device=x.device)
    kp = keys.data_ptr() if dither else 0
    if n_clips == 1:
        return (lambda: hip.check(call(x.data_ptr(), out.data_ptr(), kp, 1, C, T, interleaved, *tail, hip.stream()), name)), out
    table = (hip.PcmClip * n_clips)(*[hip.PcmClip(x.data_ptr() + 4 * C * T * b, out.data_ptr() + size * C * T * b, T, C, T)
                                      for b in range(n_clips)])
    keep, (clips,) = upload_tables([table], x.device)
    return (lambda keep=keep: hip.check(call(clips, n_clips, C, T, kp, interleaved, *tail, hip.stream()), name)), out


def launch_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pcm24.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcm24_bench needs a GPU")
    dev = torch.device("cuda:0")
    rows = []
    for n_clips in (1, 24):
        x = (torch.rand(n_clips, C, T, device=dev) * 1.8 - 0.9).contiguous()
        keys = torch.from_numpy(np.array([[7, b] for b in range(n_clips)], dtype=np.uint64).view(np.int64)).to(dev)
        for interleaved in (0, 1):
            for dither in (True, False):
                fns = {fmt: launcher(n_clips, fmt, interleaved, dither, x, keys) for fmt in FORMATS}
                for fn, _ in fns.values():
                    launch_us(fn, 3)
                # the two 24-bit containers hold one integer
                wide = fns["s24in32"][1].view(torch.int32)
                packed = fns["s24"][1].view(-1, 3).to(torch.int32)
                low = wide.reshape(-1) & 0xFFFFFF
                assert torch.equal(packed[:, 0] | (packed[:, 1] << 8) | (packed[:, 2] << 16), low)
                t = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for k, (fn, _) in fns.items():
                        t[k].append(launch_us(fn, a.reps))
                rows.append((n_clips, interleaved, dither, {k: (statistics.median(v), quartiles(v)) for k, v in t.items()}))
                print(n_clips, "interleaved" if interleaved else "planar", "dither" if dither else "plain",
                      {k: round(statistics.median(v), 1) for k, v in t.items()}, flush=True)
    # the whole step
    cfg = synth.SYNTH_CFG
    m = FlowHighSR(FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev), torchdiffeq_ode_method="euler", upsampling_method="hip")
    sr = 12000
    n_in = int(SECONDS * sr)
    clip = np.stack([synth.lowres_clip(c, SECONDS, sr)[:n_in] for c in range(C)])
    kw = dict(noise=synth.prior_noise(0, n_in * 4 // 480), channels="first")
    steps = dict(float=lambda: m.generate(clip, sr, **kw),
                 int16=lambda: m.generate(clip, sr, pcm="int16", dither="tpdf", interleaved=True, **kw),
                 s24=lambda: m.generate(clip, sr, pcm="s24", dither="tpdf", interleaved=True, **kw))
    for fn in steps.values():
        for _ in range(2):
            fn()
    ts = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            ts[k].append(wall(fn))
    step = {k: (statistics.median(v), quartiles(v)) for k, v in ts.items()}
    print({k: round(v[0], 2) for k, v in step.items()}, flush=True)

    cell = lambda v: f"{v[0]:.1f} ({v[1][0]:.1f}-{v[1][1]:.1f})"          # noqa: E731
    lines = ["# 24-bit PCM delivery: the encode launch in its three formats", "",
             f"`python tools/pcm24_bench.py --rounds {a.rounds} --reps {a.reps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  "
             f"Clips of {SECONDS:.0f} s at 48 kHz, C = {C} ({C * T} samples a clip); 1 clip through the batched entry, 24 through the "
             f"segment entry.  Device events around {a.reps} back-to-back launches, microseconds per launch: median (quartiles) of "
             f"{a.rounds} rounds, the three formats alternating in every round of one process.  The int16 kernel is unchanged, so "
             "its column is the launch as it was.", "",
             "Bytes moved per sample: 4 + 2 (int16), 4 + 3 (s24), 4 + 4 (s24in32); the 24-bit encoders add two float64 operations a "
             "sample, and their interleaved form draws one Philox block per sample where the planar form and the int16 kernel draw one per two.", "",
             "| clips | layout | dither | int16 | s24 | s24in32 | s24 / int16 | bytes 7 / 6 |", "|---|---|---|---|---|---|---|---|"]
    for n_clips, interleaved, dither, t in rows:
        lines.append(f"| {n_clips} | {'interleaved' if interleaved else 'planar'} | {'tpdf' if dither else 'none'} | {cell(t['int16'])} | "
                     f"{cell(t['s24'])} | {cell(t['s24in32'])} | {t['s24'][0] / t['int16'][0]:.2f} | 1.17 |")
    lines += ["", f"Whole step, `generate` of one {SECONDS:.0f} s stereo clip at {sr} Hz on SYNTH_CFG (euler x 1), wall ms, median (quartiles):", "",
              "| float32 | pcm='int16', tpdf, interleaved | pcm='s24', tpdf, interleaved |", "|---|---|---|",
              f"| {cell(step['float'])} | {cell(step['int16'])} | {cell(step['s24'])} |"]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
