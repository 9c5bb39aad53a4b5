"""Streaming sessions measured (flowhigh_amd/stream.py, streaming.py): the numbers of profiles/streaming.md.

  --mode stream     ms per push and per window of FlowHighSR.stream_push: windows of 0.5 / 1 / 2 s (overlap 20 % of the window, guard 5 % rounded
                    down to 10 ms), 1 / 8 / 32 sessions in one push, every push making one window per session runnable; and the ratio
                    of the RMS difference of two windows over their overlap with the session's shared prior to that with
                    independent keys (full-size synthetic model, 1 s windows).
  --mode generate   the yardstick: the SAME windows as separate generate(window, sr, level='input', seed=) calls, one per
                    window.  Uses nothing this feature added, so it runs on the parent commit's tree as well: that run is the
                    one the profile compares against.
(The profile's CPU-side tables -- stitched windows against the whole-clip run through the oracle -- come from
tests/tools/stream_quality.py.)  Every mode prints one JSON line; --out appends it to a file.  SYNTH_CFG (the full-size synthetic checkpoint of bench.py),
12 kHz input, euler x 1, upsampling_method='hip', prior='device'; host clock around a synchronised call, medians over --rounds.

python tools/stream_bench.py --mode stream|generate [--rounds 20] [--out file.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SR = 12000
WINDOWS_MS = (500, 1000, 2000)
SESSIONS = (1, 8, 32)


def plan_ms(window_ms):
    return dict(window_ms=window_ms, overlap_ms=window_ms // 5, guard_ms=window_ms // 200 * 10)          # 500: 100 / 20, 1000: 200 / 50, 2000: 400 / 100


def wall(torch, fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def gpu_model():
    import torch
    from flowhigh_amd import FLowHigh, FlowHighSR, synth
    cfg = synth.SYNTH_CFG
    sd = synth.make_state_dict(cfg, 0)
    return torch, synth, FlowHighSR(FLowHigh(sd, cfg, "cuda"), torchdiffeq_ode_method="euler", upsampling_method="hip", prior="device")


def mode_stream(rounds):
    torch, synth, m = gpu_model()
    from flowhigh_amd import stream as S
    rows = []
    for w_ms in WINDOWS_MS:
        p = S.StreamPlan(SR, **plan_ms(w_ms))
        for n in SESSIONS:
            clips = [synth.lowres_clip(500 + i, (p.W + (rounds + 2) * p.H) / SR, SR) for i in range(n)]
            sessions = [m.stream(SR, seed=i, **plan_ms(w_ms)) for i in range(n)]
            m.stream_push(sessions, [c[:p.W] for c in clips])                       # window 0: plans, workspaces
            m.stream_push(sessions, [c[p.W:p.W + p.H] for c in clips])              # window 1: the first seam
            ts = []
            for r in range(rounds):
                a = p.W + (r + 1) * p.H
                blocks = [c[a:a + p.H] for c in clips]
                ts.append(wall(torch, lambda: m.stream_push(sessions, blocks)))
            for s in sessions:
                s.flush()
            t = statistics.median(ts)
            rows.append(dict(window_ms=w_ms, sessions=n, ms_per_push=round(t, 3), ms_per_window=round(t / n, 3),
                             audio_ms_per_push=n * (p.H * 1000 // SR), q1=round(sorted(ts)[len(ts) // 4], 3),
                             q3=round(sorted(ts)[3 * len(ts) // 4], 3)))
            print(rows[-1], file=sys.stderr, flush=True)
    # what the shared prior buys, on this model: windows 0 and 1 of a 1 s plan over their overlap
    p = S.StreamPlan(SR, **plan_ms(1000))
    x = synth.lowres_clip(600, (p.W + p.H) / SR, SR)
    rms = {}
    for name, keys in (("shared", [(7, 0, 0), (7, 0, p.first_frame(1))]), ("independent", [(7, 0, 0), (7, 1, 0)])):
        w = []
        for (seed, stream, first), (a, b) in zip(keys, p.spans(len(x))):
            z = m.draw_prior(p.window_frames, seed, stream=stream, first_frame=first)
            w.append(m.generate(x[a:b], SR, level="input", noise=z)[0].double().cpu().numpy())
        d = w[0][-p.O48:] - w[1][:p.O48]
        rms[name] = float(np.sqrt(np.mean(d * d)))
    rms["signal"] = float(np.sqrt(np.mean(w[0][-p.O48:] ** 2)))
    return dict(mode="stream", rounds=rounds, rows=rows, overlap_rms=rms, device=torch.cuda.get_device_name(0))


def mode_generate(rounds):
    """One generate() per window: spans by plain arithmetic, so that this runs on a tree without flowhigh_amd/stream.py."""
    torch, synth, m = gpu_model()
    rows = []
    for w_ms in WINDOWS_MS:
        W = w_ms * SR // 1000
        H = W - (w_ms // 5) * SR // 1000
        for n in SESSIONS:
            clips = [synth.lowres_clip(500 + i, (W + (rounds + 2) * H) / SR, SR) for i in range(n)]
            for c in clips[:2]:
                m.generate(c[:W], SR, level="input", seed=1)
            ts = []
            for r in range(rounds):
                a = (r + 2) * H
                ts.append(wall(torch, lambda: [m.generate(c[a:a + W], SR, level="input", seed=i) for i, c in enumerate(clips)]))
            t = statistics.median(ts)
            rows.append(dict(window_ms=w_ms, sessions=n, ms_per_push=round(t, 3), ms_per_window=round(t / n, 3),
                             q1=round(sorted(ts)[len(ts) // 4], 3), q3=round(sorted(ts)[3 * len(ts) // 4], 3)))
            print(rows[-1], file=sys.stderr, flush=True)
    return dict(mode="generate", rounds=rounds, rows=rows, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("stream", "generate"), required=True)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = (mode_stream if a.mode == "stream" else mode_generate)(a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
