"""Where the prior noise is drawn: wall time of generate() with prior='reference' (host draw + upload, the default), with
prior='device' (fh_prior_normal_f32) and with a pre-drawn host noise=, per clip length; the host time of the reference draw alone;
the prior kernel's time from device events; the 24-clip generate_many mix of tools/serve_bench.py under both priors.
One process, alternating rounds, medians.  Writes profiles/device_prior.md (or the path given).

python tools/prior_bench.py [--rounds 30] [--out profiles/device_prior.md]"""
import argparse
import os
import platform
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth                 # noqa: E402
from flowhigh_amd.flowhighsr import reference_prior_draw                   # noqa: E402

SR_IN = 12000
CLIPS = [("BASELINE configs[0]: 2 s", 2.0), ("BASELINE configs[1]: 10 s", 10.0), ("30 s", 30.0)]


def cpu_name():
    try:
        for ln in Path("/proc/cpuinfo").read_text().splitlines():
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def wall(fn):
    """Host clock from the call to the synchronised result, ms."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def med(v):
    return statistics.median(v)


def spread(v):
    s = sorted(v)
    return s[len(s) // 4], s[(3 * len(s)) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "device_prior.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prior_bench needs a GPU")
    dev = torch.device("cuda:0")
    cfg = synth.SYNTH_CFG
    fh = FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev)
    kw = dict(torchdiffeq_ode_method="euler", upsampling_method="hip")
    m_ref, m_dev = FlowHighSR(fh, **kw), FlowHighSR(fh, prior="device", **kw)
    rows = []
    for ci, (label, secs) in enumerate(CLIPS):
        clip = synth.lowres_clip(ci, secs, SR_IN)
        n = len(clip) * 4 // 480
        z = synth.prior_noise(ci, n)
        variants = {"reference": lambda: m_ref.generate(clip, SR_IN),
                    "device": lambda: m_dev.generate(clip, SR_IN),
                    "noise=": lambda: m_ref.generate(clip, SR_IN, noise=z)}
        keys = torch.tensor([[1234 + ci, 0]], dtype=torch.int64, device=dev)
        buf = torch.empty(n, 256, dtype=torch.float32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def kernel_ms(reps=20):
            e0.record()
            for _ in range(reps):
                hip.check(hip.lib().fh_prior_normal_f32(buf.data_ptr(), keys.data_ptr(), 0, 1, n, 256, hip.stream(dev)),
                          "fh_prior_normal_f32")
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        for fn in variants.values():                 # plans, workspaces, pinned staging: every shape once before the clock
            for _ in range(3):
                fn()
        kernel_ms()
        t = {k: [] for k in variants}
        draw, kern = [], []
        for _ in range(a.rounds):                    # alternating: every variant once per round
            for k, fn in variants.items():
                t[k].append(wall(fn))
            t0 = time.perf_counter()
            reference_prior_draw(n, 256)
            draw.append((time.perf_counter() - t0) * 1e3)
            kern.append(kernel_ms())
        same = torch.equal(m_dev.generate(clip, SR_IN, seed=5), m_dev.generate(clip, SR_IN, noise=m_dev.draw_prior(n, 5)))
        rows.append((label, n, {k: (med(v), spread(v)) for k, v in t.items()}, med(draw), med(kern), same))
        print(label, {k: round(med(v), 2) for k, v in t.items()}, "draw", round(med(draw), 2), "kernel us", round(med(kern) * 1e3, 1), flush=True)

    # the serving mix of tools/serve_bench.py: 24 clips of 0.5 .. 4 s, one ragged launch sequence
    rng = np.random.default_rng(0)
    lens = [int(rng.integers(5, 41)) * 1200 for _ in range(24)]
    clips = [synth.lowres_clip(i, L / SR_IN, SR_IN) for i, L in enumerate(lens)]
    audio_s = sum(lens) / SR_IN
    mix = {"reference": lambda: m_ref.generate_many(clips, SR_IN, ragged=True),
           "device": lambda: m_dev.generate_many(clips, SR_IN, ragged=True)}
    for fn in mix.values():
        for _ in range(2):
            fn()
    tm = {k: [] for k in mix}
    for _ in range(a.rounds):
        for k, fn in mix.items():
            tm[k].append(wall(fn))
    print("mix", {k: round(med(v), 1) for k, v in tm.items()}, flush=True)

    out = ["# Prior noise on the host and on the device", "",
           f"`python tools/prior_bench.py --rounds {a.rounds}`: one process, {a.rounds} alternating rounds (every variant once per round), medians "
           "(quartiles in brackets).  SYNTH_CFG weights, B = 1, 12 -> 48 kHz, euler x 1, default conv form "
           f"(`{fh.conv_form}`), `upsampling_method='hip'`.",
           f"GPU: {torch.cuda.get_device_name(0)}.  Host CPU: {cpu_name()}, {os.cpu_count()} logical CPUs, {torch.get_num_threads()} torch threads; torch {torch.__version__}.",
           "", "Wall time of `generate(clip, sr)`, from the call to the synchronised result, ms:", "",
           "| clip | frames | `prior='reference'`, no noise (baseline) | `prior='device'` | pre-drawn host `noise=` | `reference_prior_draw` alone (host) | prior kernel (events) | `seed=` == `noise=draw_prior` bitwise |",
           "|---|---|---|---|---|---|---|---|"]
    for label, n, t, d, k, same in rows:
        cell = lambda x: f"{x[0]:.2f} [{x[1][0]:.2f}, {x[1][1]:.2f}]"      # noqa: E731
        out.append(f"| {label} | {n} x 256 | {cell(t['reference'])} | {cell(t['device'])} | {cell(t['noise='])} | {d:.2f} | {k * 1e3:.1f} us | {same} |")
    out += ["", f"`generate_many` over the serving mix of `tools/serve_bench.py` (24 clips, {audio_s:.1f} s of audio, {len(set(lens))} lengths, one ragged launch "
            "sequence), ms per list:", "", "| prior | ms | x real time |", "|---|---|---|"]
    for k, v in tm.items():
        lo, hi = spread(v)
        out.append(f"| `'{k}'` | {med(v):.1f} [{lo:.1f}, {hi:.1f}] | {audio_s / med(v) * 1e3:.0f} |")
    worst = max(t["device"][0] / t["reference"][0] for _, _, t, _, _, _ in rows)
    out += ["", f"Device form / baseline, worst length: {worst:.3f}; the mix: {med(tm['device']) / med(tm['reference']):.3f}."
            "  The host figures depend on the host CPU named above; the kernel's do not.", ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
