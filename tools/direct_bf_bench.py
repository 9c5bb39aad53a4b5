"""A/B of conv_form='direct_bf16x6' against 'direct' (and the default 'bf16x6') on one GPU, in one process.
    python tools/direct_bf_bench.py [reps=30] [out.md]
1. Per launch: the conv launches of the SYNTH_CFG vocoder's plan for B = 1 x 1000 frames (a 10 s clip), timed in place with HIP
   events (Vocoder.conv_timing) while the whole plan runs, the two forms alternating run by run; median us per launch of both
   kernels, the ratio, and the fraction of the 2.5 PFLOP/s bf16 peak the bf16 x 6 launch issues (6 bf16 FLOPs per fp32 FLOP).
2. Whole step: BASELINE configs[1] (B = 1, 10 s, 12 -> 48 kHz, euler x 1, upsampling_method='hip') through generate_from_device in
   the three forms, the order rotated every round; ms per step (median, min), x real time, and the waveform's max-abs distance
   from the 'direct' form.
Random data everywhere (zeros would flatter the matrix pipe's clock)."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowhigh_amd import FLowHigh, FlowHighSR, synth      # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
out_md = Path(sys.argv[2]) if len(sys.argv) > 2 else None
FORMS = ("direct", "direct_bf16x6", "bf16x6")
BF16_PEAK = 2.5e15
cfg = synth.SYNTH_CFG
sd = synth.make_state_dict(cfg, 0)
models = {f: FlowHighSR(FLowHigh(sd, cfg, "cuda", conv_form=f), torchdiffeq_ode_method="euler", upsampling_method="hip") for f in FORMS}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


# ---- 1. per launch ---------------------------------------------------------------------------------------------------------
N = 1000
vocs = {f: models[f].flowhigh.vocoder for f in FORMS[:2]}
plans = {f: v.plan(1, N) for f, v in vocs.items()}
mel = (torch.randn(1, cfg["num_mels"], N, generator=torch.Generator().manual_seed(1)) * 2.0 - 3.0).cuda()
for p in plans.values():
    p["mel_in"].copy_(mel)
times = {f: [] for f in vocs}
for r in range(5 + reps):
    for f in (FORMS[:2] if r % 2 == 0 else FORMS[1::-1]):
        vocs[f].conv_timing = []
        vocs[f].run(plans[f])
        torch.cuda.synchronize()
        if r >= 5:
            times[f].append([a.elapsed_time(b) * 1e3 for a, b in vocs[f].conv_timing])
        vocs[f].conv_timing = None
med = {f: [statistics.median(col) for col in zip(*times[f])] for f in vocs}


def describe(plan):
    """(position key, kind, channels in -> out, taps per group, n_len) of every conv-family launch."""
    out = []
    for s, (key, structs) in zip(plan["steps"], plan["meta"]):
        if s.kind in ("conv", "convt"):
            g = structs[0]
            taps = "/".join(str(sum(gr.seg[i].ntaps for i in range(gr.nseg))) for gr in structs)
            out.append((key, s.kind, f"{g.seg[0].cin}->{g.cout}", f"{len(structs)}g k={taps}", s.n_len))
        elif s.kind == "amp":
            out.append((key, "narrow", f"{s.c}->{s.c}", f"{s.ng}g", structs[0].len))
    return out


say(f"## Per launch, as the two plans run them: SYNTH_CFG, B = 1 x {N} frames, median of {reps} alternating runs (us)")
say()
say("Each launch is timed in place while its whole plan runs (activations between the convs, caches as in a real step).  Rows of family")
say("`direct_bf16x6` compare `fh_conv_grouped_f32` with `fh_conv_grouped_bf16x6_f32` on the same descriptors and tile; rows of family")
say("`narrow_bf16x6` compare the 'direct' plan's fp32 conv (8- or 16-channel chunks) with `narrow_bf.hip`; `direct` rows are the same")
say("fp32 phase-fused launch in both plans.")
say()
say("| position | launch | channels | groups, taps | n | family | fp32 `direct` | `direct_bf16x6` | fp32 / new | of bf16 peak |")
say("|---|---|---|---|---|---|---|---|---|---|")
tot = {"direct": 0.0, "direct_bf16x6": 0.0}
for i, (d_old, d_new) in enumerate(zip(describe(plans["direct"]), describe(plans["direct_bf16x6"]))):
    fam, ex, _ = plans["direct_bf16x6"]["conv_launches"][i]
    a, b = med["direct"][i], med["direct_bf16x6"][i]
    tot["direct"] += a
    tot["direct_bf16x6"] += b
    peak = f"{6.0 * ex / (b * 1e-6) / BF16_PEAK:.3f}" if fam == "direct_bf16x6" else "-"
    say(f"| {d_new[0]} | {d_old[1]} -> {d_new[1]} | {d_new[2]} | {d_new[3]} | {d_new[4]} | {fam} | {a:.1f} | {b:.1f} | {a / b:.2f} | {peak} |")
say(f"| all conv launches | | | | | | {tot['direct']:.0f} | {tot['direct_bf16x6']:.0f} | {tot['direct'] / tot['direct_bf16x6']:.2f} | |")
say()

# ---- 2. whole step ----------------------------------------------------------------------------------------------------------
secs, sr_in = 10.0, 12000
x = torch.from_numpy(synth.lowres_clip(0, secs, sr_in)[None]).cuda()
noise = synth.prior_noise(0, int(secs * 100)).cuda().reshape(int(secs * 100), -1).contiguous()
wav, ms = {}, {f: [] for f in FORMS}
for f in FORMS:
    for _ in range(3):
        wav[f] = models[f].generate_from_device(x, sr_in, 1, noise=noise).clone()
torch.cuda.synchronize()
for r in range(reps):
    for j in range(len(FORMS)):
        f = FORMS[(r + j) % len(FORMS)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        models[f].generate_from_device(x, sr_in, 1, noise=noise)
        e1.record()
        torch.cuda.synchronize()
        ms[f].append(e0.elapsed_time(e1))
say(f"## Whole step: BASELINE configs[1] (B = 1, {secs:.0f} s, 12 -> 48 kHz, euler x 1, upsampling 'hip'), {reps} rounds, order rotated")
say()
say("| conv_form | ms per step (median) | min | x real time (median) | max abs distance to 'direct' |")
say("|---|---|---|---|---|")
for f in FORMS:
    m_ = statistics.median(ms[f])
    say(f"| {f} | {m_:.2f} | {min(ms[f]):.2f} | {secs * 1e3 / m_:.0f} | {(wav[f] - wav['direct']).abs().max().item():.2e} |")
say()
# ---- 3. host cost of a launch call (the bf16 x 6 entry asks the runtime where its descriptor array lives) ---------------------------
import time                                              # noqa: E402
from flowhigh_amd import hip                             # noqa: E402
from flowhigh_amd import vocoder as V                    # noqa: E402
c_, n_ = 32, 64
xs_, out_ = torch.randn(1, c_, n_).cuda(), torch.empty(1, c_, n_).cuda()
host_us = {}
for bf in (False, True):
    w_ = torch.randn(c_, c_, 3) * 0.1
    wp_ = (V.pack_conv_bf_weight(w_, 32) if bf else V.pack_conv_weight(w_, 32, 16)).cuda()
    g_ = V.make_conv_group([V.make_conv_seg(xs_, wp_, c_, [-1, 0, 1])], None, [], out_, c_, 32, n_, n_, n_)
    d_ = hip.to_device_struct_array([g_], "cuda")
    L_, st_ = hip.lib(), hip.stream()
    call = (lambda: L_.fh_conv_grouped_bf16x6_f32(d_.data_ptr(), 1, 1, 32, n_, 4, st_)) if bf else \
        (lambda: L_.fh_conv_grouped_f32(d_.data_ptr(), 1, 1, 32, n_, 4, 16, st_))
    best = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            call()
        best.append((time.perf_counter() - t0) / 500 * 1e6)
        torch.cuda.synchronize()
    host_us[bf] = min(best)
say(f"## Host time of one launch call (500 back-to-back calls of a one-block conv, best of 5): fh_conv_grouped_f32 {host_us[False]:.2f} us, "
    f"fh_conv_grouped_bf16x6_f32 {host_us[True]:.2f} us")
say()
say(f"device: {torch.cuda.get_device_name(0)}; peak |wav| {wav['direct'].abs().max().item():.3f}")
if out_md is not None:
    out_md.parent.mkdir(parents=True, exist_ok=True)
    out_md.write_text("\n".join(lines) + "\n")
