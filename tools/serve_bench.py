"""Serving mix: N clips of random lengths (0.5 .. 4 s, 12 kHz) through generate_many -- bucketed by length
(ragged=False: one batch per distinct length) against ONE ragged launch sequence (ragged=True).
python tools/serve_bench.py [n_clips] [profile] [--ends per_clip|ragged|compare] [--rounds R]
--ends per_clip | ragged: how the front and back end of the ragged sequence run (generate_many(ends=); default: the library's).
--ends compare: the two forms alternating in one process, R rounds (default 15): median, fastest and slowest wall time of
generate_many per form, and the library calls per generate_many (counted by wrapping hip.check).  profiles/ragged_ends.md is
this mode's output."""
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
args = ap.parse_args()
n = args.n_clips
dev = torch.device("cuda:0")
cfg = synth.SYNTH_CFG
model = FlowHighSR(FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev), torchdiffeq_ode_method="euler",
                   upsampling_method="hip")
rng = np.random.default_rng(0)
lens = [int(rng.integers(5, 41)) * 1200 for _ in range(n)]          # multiples of 0.1 s
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
    """Library calls of one generate_many: every one goes through hip.check."""
    real, count = hip.check, [0]

    def check(rc, what=""):
        count[0] += 1
        return real(rc, what)
    hip.check = check
    try:
        model.generate_many(clips, 12000, noise=noise, **kw)
    finally:
        hip.check = real
    return count[0]


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
