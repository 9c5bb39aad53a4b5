"""Serving mix: N clips of random lengths (0.5 .. 4 s, 12 kHz) through generate_many -- bucketed by length
(ragged=False: one batch per distinct length) against ONE ragged launch sequence (ragged=True).
python tools/serve_bench.py [n_clips] [profile] [--ends per_clip|ragged|compare] [--rounds R]
--ends per_clip | ragged: how the front and back end of the ragged sequence run (generate_many(ends=); default: the library's).
--ends compare: the two forms alternating in one process, R rounds (default 15): median, fastest and slowest wall time of
generate_many per form, and the library calls per generate_many (counted by wrapping hip.check).  profiles/ragged_ends.md is
this mode's output.
--rates 8000,12000,16000,24000: the clips are dealt round-robin over these input rates (same durations) and the tool compares, R
rounds alternating in one process, ONE generate_many with the list of rates ("mixed") against one generate_many per distinct rate
in a row ("per_rate": what a server that groups a window by input rate does); --ends per_clip | ragged selects the ends of both.
Median, fastest and slowest wall time and the library calls per form; profiles/mixed_rates.md is this mode's output."""
import argparse, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, '.')
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth

ap = argparse.ArgumentParser()
ap.add_argument("n_clips", nargs="?", type=int, default=24)
ap.add_argument("profile", nargs="?", default=None)
ap.add_argument("--ends", choices=["per_clip", "ragged", "compare"], default=None)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--rates", default=None, help="comma-separated input rates: compare one mixed-rate call with one call per rate")
args = ap.parse_args()
if args.rates and args.ends == "compare":
    ap.error("--rates compares mixed against per-rate calls: give --ends per_clip or --ends ragged")
n = args.n_clips
dev = torch.device("cuda:0")
cfg = synth.SYNTH_CFG
model = FlowHighSR(FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev), torchdiffeq_ode_method="euler",
                   upsampling_method="hip")
rng = np.random.default_rng(0)
lens = [int(rng.integers(5, 41)) * 1200 for _ in range(n)]          # multiples of 0.1 s


def count_library_calls(fn):
    """Library calls of fn(): every one goes through hip.check."""
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


def compare_rates():
    from flowhigh_amd import tables
    rate_list = [int(r) for r in args.rates.split(",")]
    rates = [rate_list[i % len(rate_list)] for i in range(n)]
    secs = [L / 12000 for L in lens]
    clips = [synth.lowres_clip(i, s_, sr) for i, (s_, sr) in enumerate(zip(secs, rates))]
    t48 = [tables.resample_out_len(len(c), 48000, sr) for c, sr in zip(clips, rates)]
    noise = [synth.prior_noise(i, t // 480) for i, t in enumerate(t48)]
    audio_s = sum(t48) / 48000
    ref = [model.generate(c, sr, noise=z).clone() for c, sr, z in zip(clips, rates, noise)]
    by_rate = {sr: [i for i in range(n) if rates[i] == sr] for sr in dict.fromkeys(rates)}
    kw = dict(ragged=True, ends=args.ends)

    def mixed():
        return model.generate_many(clips, rates, noise=noise, **kw)

    def per_rate():
        out = [None] * n
        for sr, idx in by_rate.items():
            for i, y in zip(idx, model.generate_many([clips[i] for i in idx], sr, noise=[noise[i] for i in idx], **kw)):
                out[i] = y
        return out
    forms = dict(mixed=mixed, per_rate=per_rate)

    def timed_form(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out
    for name, fn in forms.items():                                   # plans, workspaces, descriptors of every mix
        for _ in range(2):
            _, out = timed_form(fn)
        assert all(torch.equal(a, b) for a, b in zip(ref, out)), f"{name}: not bit-identical to generate() per clip"
    calls = {name: count_library_calls(fn) for name, fn in forms.items()}
    times = {name: [] for name in forms}
    order = list(forms)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):          # (the order within a round alternates too)
            times[name].append(timed_form(forms[name])[0])
    print(f"{n} clips, {audio_s:.1f} s of audio at 48 kHz, input rates {rate_list} round-robin ({len(by_rate)} distinct), "
          f"{len(set(zip(map(len, clips), rates)))} (length, rate) shapes, ends={model_ends(args.ends)}, {args.rounds} rounds, forms "
          "alternating; bit-identical to generate() per clip: True (both forms)")
    print("| form | generate_many calls | median ms | fastest ms | slowest ms | spread (slowest - fastest) ms | x real time (median) | library calls |")
    print("|---|---|---|---|---|---|---|---|")
    for name in forms:
        t = times[name]
        med = statistics.median(t)
        print(f"| {name} | {1 if name == 'mixed' else len(by_rate)} | {med:.2f} | {min(t):.2f} | {max(t):.2f} | {max(t) - min(t):.2f} | "
              f"{audio_s / med * 1e3:.0f} | {calls[name]} |")
    d = statistics.median(times["per_rate"]) - statistics.median(times["mixed"])
    apart = max(times["mixed"]) < min(times["per_rate"])
    print(f"median(per_rate) - median(mixed) = {d:+.2f} ms; slowest mixed round below fastest per_rate round: {apart}")
    print("all rounds, ms: " + "; ".join(f"{name}: " + " ".join(f"{v:.1f}" for v in times[name]) for name in forms))


def model_ends(ends):
    from flowhigh_amd.flowhighsr import resolve_ends
    return resolve_ends(ends)


if args.rates:
    compare_rates()
    sys.exit(0)
clips = [synth.lowres_clip(i, L / 12000, 12000) for i, L in enumerate(lens)]
noise = [synth.prior_noise(i, L * 4 // 480) for i, L in enumerate(lens)]
audio_s = sum(lens) / 12000
ref = [model.generate(c, 12000, noise=z).clone() for c, z in zip(clips, noise)]


def timed(**kw):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = model.generate_many(clips, 12000, noise=noise, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def library_calls(**kw):
    """Library calls of one generate_many."""
    return count_library_calls(lambda: model.generate_many(clips, 12000, noise=noise, **kw))


if args.ends == "compare":
    forms = ("per_clip", "ragged")
    for f in forms:                                                  # plans, workspaces, descriptors of the mix
        for _ in range(2):
            dt, out = timed(ragged=True, ends=f)
        assert all(torch.equal(a, b) for a, b in zip(ref, out)), f"ends={f}: not bit-identical to generate() per clip"
    calls = {f: library_calls(ragged=True, ends=f) for f in forms}
    times = {f: [] for f in forms}
    for r in range(args.rounds):
        for f in (forms if r % 2 == 0 else forms[::-1]):             # (the order within a round alternates too)
            times[f].append(timed(ragged=True, ends=f)[0] * 1e3)
    print(f"{n} clips, {audio_s:.1f} s of audio, {len(set(lens))} lengths, {args.rounds} rounds, forms alternating; "
          "bit-identical to generate() per clip: True (both forms)")
    print("| ends | median ms | fastest ms | slowest ms | spread (slowest - fastest) ms | x real time (median) | library calls per generate_many |")
    print("|---|---|---|---|---|---|---|")
    for f in forms:
        t = times[f]
        med = statistics.median(t)
        print(f"| {f} | {med:.2f} | {min(t):.2f} | {max(t):.2f} | {max(t) - min(t):.2f} | {audio_s / med * 1e3:.0f} | {calls[f]} |")
    d = statistics.median(times["per_clip"]) - statistics.median(times["ragged"])
    print(f"median(per_clip) - median(ragged) = {d:+.2f} ms")
    print("all rounds, ms: " + "; ".join(f"{f}: " + " ".join(f"{v:.1f}" for v in times[f]) for f in forms))
    sys.exit(0)

for ragged in (False, True, False, True, True):
    model.generate_many(clips, 12000, noise=noise, ragged=ragged, ends=args.ends)           # plans for every shape
    dt, out = timed(ragged=ragged, ends=args.ends)
    same = all(torch.equal(a, b) for a, b in zip(ref, out))
    print(f"{n} clips, {audio_s:.1f} s of audio, {len(set(lens))} lengths, ragged={ragged}: {dt * 1e3:7.1f} ms "
          f"= {audio_s / dt:6.1f} x real time, bit-identical to generate() per clip: {same}")
# a new mix of the same lengths (merged plan rebuilt from cached per-clip plans: the serving case)
perm = rng.permutation(n)
c2, z2 = [clips[i] for i in perm], [noise[i] for i in perm]
torch.cuda.synchronize()
t = time.perf_counter()
model.generate_many(c2, 12000, noise=z2, ragged=True, ends=args.ends)
torch.cuda.synchronize()
print(f"new order of the same clips (merge rebuilt): {(time.perf_counter() - t) * 1e3:7.1f} ms")
if args.profile:
    import cProfile, pstats
    pr = cProfile.Profile(); pr.enable()
    model.generate_many(clips, 12000, noise=noise, ragged=True, ends=args.ends)
    torch.cuda.synchronize(); pr.disable()
    pstats.Stats(pr).sort_stats("tottime").print_stats(25)
