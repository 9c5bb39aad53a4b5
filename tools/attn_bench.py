"""The attention entries (16 heads x 64) at the transformer's shapes, random data.
    python tools/attn_bench.py [f32 | bf16x6 | ab]
f32 / bf16x6: one form (fh_attention_f32 / fh_attention_bf16x6_f32).  ab (default): both forms alternated per shape in one
process -- three samples of each, a sample = device events around enough launches to last at least 0.2 s -- and the ratio
f32 / bf16x6 of the medians next to the spread (max - min) of each form's samples."""
import sys, torch
sys.path.insert(0, '.')
from flowhigh_amd import hip
DEV = torch.device("cuda:0")
SHAPES = ((1, 50), (1, 1000), (8, 1000), (32, 1000), (1, 3000), (8, 3000))
ENTRY = {"f32": "fh_attention_f32", "bf16x6": "fh_attention_bf16x6_f32"}
MIN_SAMPLE_S = 0.2


def runner(form, qkv, out, B, N):
    fn = getattr(hip.lib(), ENTRY[form])
    return lambda: hip.check(fn(qkv.data_ptr(), out.data_ptr(), B, N, 16, 10.0, hip.stream()), ENTRY[form])


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per launch


def reps_for(run):
    for _ in range(3):
        run()
    return max(10, int(MIN_SAMPLE_S * 1e6 / timed(run, 10)) + 1)


def main(mode):
    forms = ("f32", "bf16x6") if mode == "ab" else (mode,)
    for B, N in SHAPES:
        qkv = torch.randn(B * N, 3072, device=DEV) * 0.3
        outs = {f: torch.empty(B * N, 1024, device=DEV) for f in forms}
        runs = {f: runner(f, qkv, outs[f], B, N) for f in forms}
        reps = {f: reps_for(runs[f]) for f in forms}
        us = {f: [] for f in forms}
        for _ in range(3):
            for f in forms:                           # alternated: f32, bf16x6, f32, ...
                us[f].append(timed(runs[f], reps[f]))
        flop = 4.0 * B * 16 * N * N * 64
        line = f"B={B:2d} N={N:5d}:"
        for f in forms:
            s = sorted(us[f])
            line += f"  {f} {s[1]:9.1f} us (spread {s[2] - s[0]:6.1f}, {flop / s[1] / 1e6:6.1f} TFLOP/s)"
        if mode == "ab":
            a, b = sorted(us["f32"]), sorted(us["bf16x6"])
            verdict = "faster" if b[2] < a[0] else "slower" if b[0] > a[2] else "within the spread"
            line += f"  f32 / bf16x6 = {a[1] / b[1]:.3f} ({verdict})  max |difference| {(outs['f32'] - outs['bf16x6']).abs().max().item():.2e}"
        print(line, flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    if mode not in ("f32", "bf16x6", "ab"):
        sys.exit(__doc__)
    main(mode)
