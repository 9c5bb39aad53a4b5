"""A/B of conv_form='direct_bf16x3' against 'direct_bf16x6' (and 'direct' and the default 'bf16x6') on one GPU, in one process.
    python tools/direct_bf3_bench.py [reps=30] [out.md]
1. Per launch: the conv launches of the SYNTH_CFG vocoder's plan for B = 1 x 1000 frames (a 10 s clip), timed in place with HIP
   events (Vocoder.conv_timing) while the whole plan runs, the plans of 'direct_bf16x6', 'direct_bf16x3' and 'bf16x6' taking turns
   run by run, the order rotated; median us per launch of the six-pair and the three-pair kernel, their ratio, the ratio to the
   default form's launch at the same position of the model (where that form has exactly one conv launch there), and the fraction
   of the 2.5 PFLOP/s bf16 peak the three-pair launch issues (3 bf16 FLOPs per fp32 FLOP).
2. Whole step: BASELINE configs[1] (B = 1, 10 s, 12 -> 48 kHz, euler x 1, upsampling_method='hip') through generate_from_device in
   the four forms, the order rotated every round; ms per step (median, min), x real time, the ratios, and the waveforms' max-abs
   distances between the forms.
Random data everywhere (zeros would flatter the matrix pipe's clock)."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowhigh_amd import FLowHigh, FlowHighSR, synth      # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
out_md = Path(sys.argv[2]) if len(sys.argv) > 2 else None
OLD, NEW, DEFAULT = "direct_bf16x6", "direct_bf16x3", "bf16x6"
FORMS = ("direct", OLD, NEW, DEFAULT)
LAUNCH_FORMS = (OLD, NEW, DEFAULT)
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
vocs = {f: models[f].flowhigh.vocoder for f in LAUNCH_FORMS}
plans = {f: v.plan(1, N) for f, v in vocs.items()}
mel = (torch.randn(1, cfg["num_mels"], N, generator=torch.Generator().manual_seed(1)) * 2.0 - 3.0).cuda()
for p in plans.values():
    p["mel_in"].copy_(mel)
times = {f: [] for f in vocs}
for r in range(5 + reps):
    for j in range(len(LAUNCH_FORMS)):
        f = LAUNCH_FORMS[(r + j) % len(LAUNCH_FORMS)]
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
        elif s.kind == "wino":
            out.append((key, "wino", "", "", s.length))
    return out


# the default form's launches by position: a position with one conv launch there has a time to compare with
by_key = {}
for (key, *_), t in zip(describe(plans[DEFAULT]), med[DEFAULT]):
    by_key.setdefault(key, []).append(t)

say(f"## Per launch, as the plans run them: SYNTH_CFG, B = 1 x {N} frames, median of {reps} rotating runs (us)")
say()
say("Each launch is timed in place while its whole plan runs (activations between the convs, caches as in a real step).  Rows of family")
say(f"`{NEW}` compare `fh_conv_grouped_bf16x6_f32` with `fh_conv_grouped_bf16x3_f32` on the same descriptors and tile; rows of family")
say("`narrow_bf16x3` compare `fh_narrow_conv_bf16x6_f32` with `fh_narrow_conv_bf16x3_f32`; `direct` rows are the same fp32 phase-fused")
say(f"launch in both plans.  `{DEFAULT}` is the default form's conv launch at the same position of the model (Winograd F(5,4) / F(4,3) in")
say("the wide stages, the six-pair narrow kernel below; `-` where that form has no single launch there).  Of bf16 peak: 3 MFMA FLOPs")
say("per algorithmic FLOP over the launch time, against 2.5 PFLOP/s.")
say()
say(f"| position | launch | channels | groups, taps | n | family | `{OLD}` | `{NEW}` | six-pair / three-pair | `{DEFAULT}` | default / three-pair | of bf16 peak |")
say("|---|---|---|---|---|---|---|---|---|---|---|---|")
tot = {OLD: 0.0, NEW: 0.0}
slower = []
for i, (d_old, d_new) in enumerate(zip(describe(plans[OLD]), describe(plans[NEW]))):
    fam, ex, _ = plans[NEW]["conv_launches"][i]
    a, b = med[OLD][i], med[NEW][i]
    tot[OLD] += a
    tot[NEW] += b
    peak = f"{3.0 * ex / (b * 1e-6) / BF16_PEAK:.3f}" if fam == NEW else "-"
    dflt = by_key.get(d_new[0], [])
    dcol = (f"{dflt[0]:.1f}", f"{dflt[0] / b:.2f}") if len(dflt) == 1 else ("-", "-")
    if fam != "direct" and b > a:
        slower.append((d_new[0], fam, a, b))
    say(f"| {d_new[0]} | {d_new[1]} | {d_new[2]} | {d_new[3]} | {d_new[4]} | {fam} | {a:.1f} | {b:.1f} | {a / b:.2f} | {dcol[0]} | {dcol[1]} | {peak} |")
say(f"| all conv launches | | | | | | {tot[OLD]:.0f} | {tot[NEW]:.0f} | {tot[OLD] / tot[NEW]:.2f} | {sum(med[DEFAULT]):.0f} | {sum(med[DEFAULT]) / tot[NEW]:.2f} | |")
say()
say("Launches of the new entries that are slower than their six-pair twin: " +
    ("none." if not slower else "; ".join(f"{k} ({fam}: {a:.1f} -> {b:.1f} us)" for k, fam, a, b in slower) + "."))
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
mm = {f: statistics.median(ms[f]) for f in FORMS}
say(f"| conv_form | ms per step (median) | min | x real time (median) | time / `{NEW}` | max abs distance to 'direct' | to `{OLD}` | to `{DEFAULT}` |")
say("|---|---|---|---|---|---|---|---|")
dist = lambda a, b: f"{(wav[a] - wav[b]).abs().max().item():.2e}"
for f in FORMS:
    say(f"| {f} | {mm[f]:.2f} | {min(ms[f]):.2f} | {secs * 1e3 / mm[f]:.0f} | {mm[f] / mm[NEW]:.3f} | {dist(f, 'direct')} | {dist(f, OLD)} | {dist(f, DEFAULT)} |")
say()
say(f"device: {torch.cuda.get_device_name(0)}; peak |wav| {wav['direct'].abs().max().item():.3f}")
if out_md is not None:
    out_md.parent.mkdir(parents=True, exist_ok=True)
    out_md.write_text("\n".join(lines) + "\n")
