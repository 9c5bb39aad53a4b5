"""Model-level A/B of attn_form at a BASELINE configuration (default configs[4]: B = 8 x 30 s, 24 -> 48 kHz, midpoint x 4,
conv_form='bf16x6'): two models from one synthetic state dict that differ only in attn_form, alternated in one process.
    python tools/attn_form_ab.py [B secs sr_in method steps [samples]]"""
import sys, time
import torch
sys.path.insert(0, '.')
from flowhigh_amd import FLowHigh, FlowHighSR, synth

a = sys.argv[1:]
B, secs, sr_in, method, steps = (int(a[0]), float(a[1]), int(a[2]), a[3], int(a[4])) if len(a) >= 5 else (8, 30.0, 24000, "midpoint", 4)
samples = int(a[5]) if len(a) > 5 else 3
dev = torch.device("cuda:0")
cfg = synth.SYNTH_CFG
sd = synth.make_state_dict(cfg, 0)
models = {f: FlowHighSR(FLowHigh(sd, cfg, dev, conv_form="bf16x6", attn_form=f), torchdiffeq_ode_method=method, upsampling_method="hip")
          for f in ("f32", "bf16x6")}
n = int(secs * 100)
x = torch.stack([torch.from_numpy(synth.lowres_clip(i, secs, sr_in)) for i in range(B)]).to(dev)
noise = torch.cat([synth.prior_noise(i, n) for i in range(B)], 0).to(dev).contiguous()
outs = {}
for f, m in models.items():
    for _ in range(2):
        outs[f] = m.generate_from_device(x, sr_in, steps, noise=noise).clone()
torch.cuda.synchronize()
ms = {f: [] for f in models}
for _ in range(samples):
    for f, m in models.items():                        # alternated
        t = time.perf_counter()
        m.generate_from_device(x, sr_in, steps, noise=noise)
        torch.cuda.synchronize()
        ms[f].append((time.perf_counter() - t) * 1e3)
for f in models:
    s = sorted(ms[f])
    print(f"attn_form={f:7s}: {s[len(s) // 2]:8.1f} ms per batch (samples {' '.join(f'{v:.1f}' for v in ms[f])}) = "
          f"{B * secs / (s[len(s) // 2] * 1e-3):.1f} x real time")
print(f"B={B} x {secs:g} s, {sr_in}->48000 Hz, {method} x {steps}: f32 / bf16x6 = "
      f"{sorted(ms['f32'])[samples // 2] / sorted(ms['bf16x6'])[samples // 2]:.4f}; "
      f"max |waveform difference| {(outs['f32'] - outs['bf16x6']).abs().max().item():.2e}")
