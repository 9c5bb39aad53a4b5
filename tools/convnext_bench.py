"""The ConvNeXt vector field (FLowHigh(architecture='convnext')) beside the transformer's, and its two kernels alone.
    python tools/convnext_bench.py [out.md]
At (B, N) = (1, 1000) (8, 1000) (1, 12000), synthetic weights (dim 1024, 8 blocks / depth 2), conv_form 'winograd' (fp32 linears):
  field    one vector-field evaluation (net.forward, 39 launches) of ConvNextNet beside FlowNet's (21 launches);
  kernels  one launch of fh_dwconv_ln_f32 with the 7-tap conv, one without (the final LayerNorm), one of fh_gelu_f32 over the
           [B N, 3072] hidden rows, with the bytes/s they reach against what they must move (2 x 4 KB per row for the fused
           kernel: a row read once, a row written; the GELU 2 x 12 KB per row).
Method as in profiles/attention_band.md: the entries of a shape alternate in one process; after a warm-up, SAMPLES samples of each,
a sample = device events around enough calls to last at least MIN_SAMPLE_S; per entry the median and the spread (max - min).
Prints markdown tables (and writes them to out.md): profiles/convnext.md holds a run."""
import sys, torch
sys.path.insert(0, '.')
from flowhigh_amd import convnext, flow, hip, synth

DEV = torch.device("cuda:0")
SHAPES = ((1, 1000), (8, 1000), (1, 12000))
MIN_SAMPLE_S = 0.1
SAMPLES = 5
DIM, DIM_IN, INNER = 1024, 256, 3072


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def reps_for(run):
    for _ in range(2):
        run()
    return max(2, int(MIN_SAMPLE_S * 1e6 / timed(run, 2)) + 1)


def measure(runs):
    """{name: callable} -> {name: (median us, spread us, calls per sample)}, the entries alternated."""
    reps = {k: reps_for(r) for k, r in runs.items()}
    us = {k: [] for k in runs}
    for _ in range(SAMPLES):
        for k, r in runs.items():
            us[k].append(timed(r, reps[k]))
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v), reps[k]) for k, v in us.items()}


def main(out_path=None):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    L = hip.lib()
    nets = {"convnext (8 blocks, 39 launches)": convnext.ConvNextNet(synth.make_convnext_state_dict(0), DEV),
            "transformer (depth 2, 21 launches)": flow.FlowNet(synth.make_flow_state_dict(0), DEV)}
    g = torch.Generator().manual_seed(1)
    say("| (B, N) | entry | median us | spread (max - min of 5) us | calls per sample | GB/s moved (must move) |")
    say("|---|---|---|---|---|---|")
    for B, N in SHAPES:
        M = B * N
        x = torch.randn(M, DIM_IN, generator=g).to(DEV)
        cond = (torch.randn(M, DIM_IN, generator=g) * 2.0 - 3.0).to(DEV)
        out = torch.empty_like(x)
        for net in nets.values():
            net.set_cond(cond, B, N)
        runs = {k: (lambda net=net: net.forward(x, 0.3, out, B, N, alpha=0.5, res=x)) for k, net in nets.items()}
        rows = torch.randn(M, DIM, generator=g).to(DEV)
        y = torch.empty_like(rows)
        hid = torch.randn(M, INNER, generator=g).to(DEV)
        w, v = (torch.randn(7, DIM, generator=g) * 0.3).to(DEV), torch.randn(DIM, generator=g).to(DEV)
        st = hip.stream()
        runs["fh_dwconv_ln_f32, k = 7"] = lambda: hip.check(L.fh_dwconv_ln_f32(
            rows.data_ptr(), w.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), y.data_ptr(), B, N, DIM, 7, 1e-6, st), "fh_dwconv_ln_f32")
        runs["fh_dwconv_ln_f32, no conv"] = lambda: hip.check(L.fh_dwconv_ln_f32(
            rows.data_ptr(), 0, 0, v.data_ptr(), v.data_ptr(), y.data_ptr(), B, N, DIM, 1, 1e-6, st), "fh_dwconv_ln_f32")
        hid2 = torch.empty_like(hid)
        runs["fh_gelu_f32, [B N, 3072]"] = lambda: hip.check(L.fh_gelu_f32(hid.data_ptr(), hid2.data_ptr(), M * INNER, st), "fh_gelu_f32")
        must = {"fh_dwconv_ln_f32, k = 7": 2 * 4 * DIM * M, "fh_dwconv_ln_f32, no conv": 2 * 4 * DIM * M,
                "fh_gelu_f32, [B N, 3072]": 2 * 4 * INNER * M}
        res = measure(runs)
        for k, (med, spread, reps) in res.items():
            bw = f"{must[k] / med / 1e3:.0f} ({must[k] / 1e6:.1f} MB)" if k in must else ""
            say(f"| ({B}, {N}) | {k} | {med:.1f} | {spread:.1f} | {reps} | {bw} |")
        names = list(nets)
        say(f"| ({B}, {N}) | transformer / convnext evaluation | {res[names[1]][0] / res[names[0]][0]:.2f} | | | |")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
