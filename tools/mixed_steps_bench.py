"""A serving window whose requests ask for different step counts: ONE generate_many call with the counts as a list ("mixed":
one ragged sequence with a time per clip) against one generate_many call per distinct count back to back ("per_count": what a
server that groups a window by step count does, BatchingServer(mix_steps=False)).
python tools/mixed_steps_bench.py [n_clips] [--rounds R] [--ends per_clip|ragged] [--out profiles/mixed_steps.md]
The window: n clips (default 24) of the lengths of serve_bench.py's window (0.5 .. 4 s at 12 kHz, seed 0), step counts drawn from
{1, 2, 4} (seed 1), on euler and on midpoint.  A second window is all timestep=1, run with the int and with the list of ones: the
list must cost nothing.  Method: the forms alternate within every round in one process, R rounds (default 15) after two warm-up
calls per form; a time is the host clock around a call that ends in a device synchronise.  Median, fastest, slowest and the
library calls per form, as a markdown table on stdout and in --out."""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n_clips", nargs="?", type=int, default=24)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--ends", choices=["per_clip", "ragged"], default="ragged")
ap.add_argument("--out", default=None)
args = ap.parse_args()
n = args.n_clips
dev = torch.device("cuda:0")
cfg = synth.SYNTH_CFG
net = FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev)
rng = np.random.default_rng(0)
lens = [int(rng.integers(5, 41)) * 1200 for _ in range(n)]          # (serve_bench.py's window: multiples of 0.1 s)
steps = [int(s) for s in np.random.default_rng(1).choice([1, 2, 4], n)]
clips = [synth.lowres_clip(i, L / 12000, 12000) for i, L in enumerate(lens)]
noise = [synth.prior_noise(i, L * 4 // 480) for i, L in enumerate(lens)]
audio_s = sum(lens) / 12000
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def count_library_calls(fn):
    real, count = hip.check, [0]

    def check(rc, what=""):
        count[0] += 1
        return real(rc, what)
    hip.check = check
    try:
        fn()
    finally:
        hip.check = real
    return count[0]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def compare(title, forms, ref, n_calls):
    for name, fn in forms.items():                                   # plans, workspaces, descriptors of every mix
        for _ in range(2):
            _, out = timed(fn)
        assert all(torch.equal(a, b) for a, b in zip(ref, out)), f"{title}, {name}: not bit-identical to generate() per clip"
    calls = {name: count_library_calls(fn) for name, fn in forms.items()}
    times = {name: [] for name in forms}
    order = list(forms)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):          # (the order within a round alternates too)
            times[name].append(timed(forms[name])[0])
    say(f"### {title}")
    say()
    say("| form | generate_many calls | median ms | fastest ms | slowest ms | x real time (median) | library calls |")
    say("|---|---|---|---|---|---|---|")
    for name in forms:
        t = times[name]
        med = statistics.median(t)
        say(f"| {name} | {n_calls[name]} | {med:.2f} | {min(t):.2f} | {max(t):.2f} | {audio_s / med * 1e3:.0f} | {calls[name]} |")
    a, b = order
    d = statistics.median(times[b]) - statistics.median(times[a])
    say()
    say(f"median({b}) - median({a}) = {d:+.2f} ms ({d / statistics.median(times[b]) * 100:+.1f} % of {b}); slowest {a} round below "
        f"fastest {b} round: {max(times[a]) < min(times[b])}; bit-identical to generate() per clip: True (both forms)")
    say()
    say("all rounds, ms: " + "; ".join(f"{name}: " + " ".join(f"{v:.1f}" for v in times[name]) for name in forms))
    say()


say("# Mixed step counts in one ragged sequence: tools/mixed_steps_bench.py")
say()
arch = str(getattr(torch.cuda.get_device_properties(0), "gcnArchName", "gfx950")).split(":")[0]
say(f"Box: one MI355X ({arch}; torch names the device \"{torch.cuda.get_device_name(0)}\"), torch {torch.__version__}, HIP {torch.version.hip}; one process, one GPU.  Model: synth.SYNTH_CFG, "
    f"seed 0, upsampling_method='hip', ends={args.ends!r}.")
say(f"Window: {n} clips, {audio_s:.1f} s of audio, {len(set(lens))} lengths (0.5 .. 4 s at 12 kHz, serve_bench.py's window); step counts "
    f"from {{1, 2, 4}}: {steps.count(1)} x 1, {steps.count(2)} x 2, {steps.count(4)} x 4 (in list order: {' '.join(map(str, steps))}).")
say(f"Method: two warm-up calls per form, then {args.rounds} rounds with the forms alternating inside every round (the order flips every "
    "round); a time is the host clock around the call(s) of a form, ending in a device synchronise.  Every form's results are compared "
    "with generate() per clip at its own count first (torch.equal).")
say()
by_count = {s: [i for i in range(n) if steps[i] == s] for s in sorted(set(steps))}
for method in ("euler", "midpoint"):
    model = FlowHighSR(net, torchdiffeq_ode_method=method, upsampling_method="hip")
    kw = dict(ragged=True, ends=args.ends)
    ref = [model.generate(c, 12000, 48000, s, noise=z).clone() for c, s, z in zip(clips, steps, noise)]

    def mixed():
        return model.generate_many(clips, 12000, 48000, steps, noise=noise, **kw)

    def per_count():
        out = [None] * n
        for s, idx in by_count.items():
            for i, y in zip(idx, model.generate_many([clips[i] for i in idx], 12000, 48000, s, noise=[noise[i] for i in idx], **kw)):
                out[i] = y
        return out
    compare(f"{method}: one mixed call against one call per step count", dict(mixed=mixed, per_count=per_count), ref,
            dict(mixed=1, per_count=len(by_count)))

model = FlowHighSR(net, torchdiffeq_ode_method="euler", upsampling_method="hip")
ref = [model.generate(c, 12000, 48000, 1, noise=z).clone() for c, z in zip(clips, noise)]
compare("euler, every clip at timestep=1: the list of ones against the int",
        dict(list_of_ones=lambda: model.generate_many(clips, 12000, 48000, [1] * n, noise=noise, ragged=True, ends=args.ends),
             int_one=lambda: model.generate_many(clips, 12000, 48000, 1, noise=noise, ragged=True, ends=args.ends)), ref,
        dict(list_of_ones=1, int_one=1))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
