"""Banded attention (attn_window=) against full attention, random data, 16 heads x 64.
    python tools/attn_band_bench.py [kernels [f32 | bf16x6 | ab]] | e2e
kernels (default, both forms): at (B, N) = (1, 3000) (1, 12000) (1, 30000) (1, 60000) the full entry, the banded entry at R = 250, 500,
  1000 and the banded entry at R = N, alternated in one process: after a warm-up, SAMPLES samples of each, a sample = device events around
  enough launches to last at least MIN_SAMPLE_S.  Per entry the median, the spread (max - min) of its samples, and beside every banded
  time the count model it should follow: 64-key iterations per block, counted exactly from the kernels' tile range (mean over the
  blocks; about (2 R + Q_block) / 64 + 1) against the full kernel's N / 64.  Ends with the two conditions:
    band faster than full  banded (N = 12000, R = 500): every sample below every sample of the full entry;
    wide band costs nothing  banded R = N: its samples overlap the full entry's, or its median is within the full entry's spread.
e2e: one 600 s clip end to end (SYNTH_CFG, generate_from_device, 12 -> 48 kHz, euler x 1) with attn_window=None and =500: peak device
  memory of a call (each model alone in the process), then the time per call, the two models alternated."""
import sys, time, torch
sys.path.insert(0, '.')
from flowhigh_amd import hip

DEV = torch.device("cuda:0")
SHAPES = ((1, 3000), (1, 12000), (1, 30000), (1, 60000))
RADII = (250, 500, 1000)
ENTRY = {"f32": ("fh_attention_f32", "fh_attention_band_f32"), "bf16x6": ("fh_attention_bf16x6_f32", "fh_attention_bf16x6_band_f32")}
MIN_SAMPLE_S = 0.2
SAMPLES = 5


def runner(form, R, qkv, out, B, N):
    """R None: the full entry."""
    name = ENTRY[form][R is not None]
    fn = getattr(hip.lib(), name)
    if R is None:
        return lambda: hip.check(fn(qkv.data_ptr(), out.data_ptr(), B, N, 16, 10.0, hip.stream()), name)
    return lambda: hip.check(fn(qkv.data_ptr(), out.data_ptr(), B, N, 16, R, 10.0, hip.stream()), name)


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per launch


def reps_for(run):
    for _ in range(2):
        run()
    return max(2, int(MIN_SAMPLE_S * 1e6 / timed(run, 2)) + 1)


def iterations(B, N, R):
    """Mean 64-key iterations per block: attention_softmax.h's launch rule and tile range (R None: the full kernel)."""
    qb = 128 if -(-N // 128) * 16 * B >= 512 else 64
    if R is None:
        return -(-N // 64), qb
    R = min(R, N)
    its = [-(-(min(N, q0 + qb + R) - max(0, q0 - R) // 64 * 64) // 64) for q0 in range(0, N, qb)]
    return sum(its) / len(its), qb


def kernels(forms):
    ok = {}
    for B, N in SHAPES:
        qkv = torch.randn(B * N, 3072, device=DEV) * 0.3
        out = torch.empty(B * N, 1024, device=DEV)
        full_it, qb = iterations(B, N, None)
        print(f"B={B} N={N} ({qb} queries per block, full kernel: {full_it} iterations per block)", flush=True)
        for form in forms:
            cases = [("full", None)] + [(f"R={R}", R) for R in RADII] + [("R=N", N)]
            runs = {k: runner(form, R, qkv, out, B, N) for k, R in cases}
            reps = {k: reps_for(runs[k]) for k, _ in cases}
            us = {k: [] for k, _ in cases}
            for _ in range(SAMPLES):
                for k, _ in cases:                      # alternated: full, R = 250, 500, 1000, N, full, ...
                    us[k].append(timed(runs[k], reps[k]))
            med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
            for k, R in cases:
                s = sorted(us[k])
                line = f"  {form:6s} {k:7s} {med[k]:10.1f} us  spread {s[-1] - s[0]:8.1f}  ({reps[k]} launches per sample)"
                if R is not None:
                    it, _ = iterations(B, N, R)
                    line += (f"  full / band = {med['full'] / med[k]:6.2f}   count model: {it:7.1f} iterations per block "
                             f"(~ (2 R + {qb}) / 64 + 1 = {(2 * min(R, N) + qb) / 64 + 1:.1f}), full / band = {full_it / it:6.2f}")
                print(line, flush=True)
            if N == 12000:
                ok[f"{form}: band faster than full (N = 12000, R = 500)"] = max(us["R=500"]) < min(us["full"])
            a, b = sorted(us["full"]), sorted(us["R=N"])
            within = (b[0] <= a[-1] and a[0] <= b[-1]) or abs(med["R=N"] - med["full"]) <= a[-1] - a[0]
            ok[f"{form}: wide band costs nothing (N = {N}, R = N within the full entry's spread)"] = within
            print(f"  {form:6s} R=N / full = {med['R=N'] / med['full']:.4f}", flush=True)
    for k, v in ok.items():
        print(f"{'HOLDS' if v else 'FAILS'}  {k}")
    return all(ok.values())


def e2e():
    from flowhigh_amd import FLowHigh, FlowHighSR, synth
    cfg, secs = synth.SYNTH_CFG, 600.0
    sd = synth.make_state_dict(cfg, 0)
    n_in, N = int(secs * 12000), int(secs * 100)
    x = torch.from_numpy(synth.lowres_clip(0, secs, 12000))[None].to(DEV)
    noise = synth.prior_noise(0, N).to(DEV).reshape(N, -1).contiguous()
    make = lambda w: FlowHighSR(FLowHigh(sd, cfg, DEV, attn_window=w), torchdiffeq_ode_method="euler", upsampling_method="hip")

    def call(m):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = m.generate_from_device(x, 12000, 1, noise=noise)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    print(f"one {secs:.0f} s clip (N = {N} frames), SYNTH_CFG, generate_from_device, 12 -> 48 kHz, euler x 1", flush=True)
    for w in (None, 500):                              # memory: each model alone
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        m = make(w)
        ms, out = call(m)
        print(f"attn_window={w}: first call {ms:9.1f} ms, peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB, "
              f"output {tuple(out.shape)} finite {bool(torch.isfinite(out).all())}", flush=True)
        del m, out
    models = {w: make(w) for w in (None, 500)}
    for m in models.values():
        call(m)
    ms = {w: [] for w in models}
    for _ in range(3):
        for w, m in models.items():                    # alternated
            ms[w].append(call(m)[0])
    for w, v in ms.items():
        s = sorted(v)
        print(f"attn_window={w}: {s[1]:9.1f} ms per call (samples {' '.join(f'{t:.1f}' for t in v)}) = {secs * 1e3 / s[1]:6.1f} x real time", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "e2e":
        e2e()
    elif mode == "kernels":
        form = sys.argv[2] if len(sys.argv) > 2 else "ab"
        if form not in ("f32", "bf16x6", "ab"):
            sys.exit(__doc__)
        sys.exit(0 if kernels(("f32", "bf16x6") if form == "ab" else (form,)) else 1)
    else:
        sys.exit(__doc__)
