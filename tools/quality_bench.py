"""What the spectral quality report costs on the device, and the table it is for.
  time      FlowHighSR.measure_quality's launches (fh_quality_frames_f32 + fh_quality_report_f32) for 1 x 10 s and 32 x 10 s mono
            pairs at 48 kHz beside a path COMPOSED here from the existing entries: fh_frame_f32 and fh_rfft2048_f32 on both
            signals, then torch for the powers, the log, the band means and the SNR.  Device events, one warm-up call, the
            median and the quartiles of 9 x 10 calls; the workspace of each path in bytes.
  variants  the synthetic SYNTH_CFG checkpoint, one 10 s clip from 16 kHz: measure_quality of each variant's output against the
            default's (attn_window 100 / 250 / 500, attn_form 'bf16x6', conv_form 'winograd' / 'direct_bf16x3', and
            midpoint x 1 against midpoint x 4), cutoff 8 kHz.  Synthetic weights: distances between computations, not
            perceptual quality.
Writes the tables to profiles/quality.md (or the path given) under the heading "## Measurements"; what stands above that heading
in the file is kept.

python tools/quality_bench.py [--out profiles/quality.md] [--skip-variants]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import FLowHigh, FlowHighSR, hip, quality, synth, tables          # noqa: E402

RATE = 48000
HEADING = "## Measurements"
KC = 341


def events_ms(fn, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread_ms(fn):
    fn()
    torch.cuda.synchronize()
    v = sorted(events_ms(fn) for _ in range(9))
    return statistics.median(v), v[2], v[6]


def composed(e, r, window, tw, ws):
    """The same figures from fh_frame_f32 + fh_rfft2048_f32 on both signals and torch behind them -> float64 [R, 4]."""
    L = hip.lib()
    R, T = e.shape
    F = quality.n_frames(T)
    specs = []
    for x, frames, spec in ((e, ws["fe"], ws["se"]), (r, ws["fr"], ws["sr"])):
        hip.check(L.fh_frame_f32(x.data_ptr(), window.data_ptr(), frames.data_ptr(), R, T, F, 2048, 480, 1024, 1, hip.stream()), "frame")
        hip.check(L.fh_rfft2048_f32(frames.data_ptr(), tw.data_ptr(), spec.data_ptr(), R * F, 0, hip.stream()), "rfft")
        s = spec.view(R, F, 33, 2, 32).double()
        re, im = s[:, :, :, 0].reshape(R, F, 1056)[..., :1025], s[:, :, :, 1].reshape(R, F, 1056)[..., :1025]
        specs.append(torch.log10(torch.clamp(re * re + im * im, min=quality.FLOOR)))
    d2 = (specs[1] - specs[0]) ** 2
    lsd = [d2.mean(-1).sqrt().mean(-1), d2[..., :KC].mean(-1).sqrt().mean(-1), d2[..., KC:].mean(-1).sqrt().mean(-1)]
    e64, r64 = e.double(), r.double()
    snr = 10.0 * torch.log10((r64 * r64).sum(-1) / ((r64 - e64) ** 2).sum(-1))
    return torch.stack([*lsd, snr], dim=1)


def time_rows(dev):
    m = FlowHighSR(FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, dev), prior="device", torchdiffeq_ode_method="euler")
    window, tw = tables.hann_window().to(dev), tables.fft_twiddles().to(dev)
    out = []
    for R in (1, 32):
        T = 10 * RATE
        F = quality.n_frames(T)
        g = torch.Generator(device=dev).manual_seed(R)
        r = (torch.rand(R, T, device=dev, generator=g) * 2 - 1) * 0.1
        e = r + (torch.rand(R, T, device=dev, generator=g) * 2 - 1) * 0.01
        ws = dict(fe=torch.empty(R * F, 2048, device=dev), fr=torch.empty(R * F, 2048, device=dev),
                  se=torch.empty(R * F, 2112, device=dev), sr=torch.empty(R * F, 2112, device=dev))
        fused = m.measure_quality(e, r, cutoff_hz=8000.0)
        comp = composed(e, r, window, tw, ws)
        torch.cuda.synchronize()
        diff = (fused.double() - comp).abs().max().item()
        row = dict(R=R, frames=R * F, fused=spread_ms(lambda: m.measure_quality(e, r, cutoff_hz=8000.0)),
                   composed=spread_ms(lambda: composed(e, r, window, tw, ws)), fused_bytes=R * F * 40,
                   composed_bytes=sum(t.numel() * 4 for t in ws.values()), diff=diff, figures=[round(v, 4) for v in fused[0].tolist()])
        out.append(row)
        print("time", row, flush=True)
        del ws
    return out


def variant_rows(dev):
    cfg, sd = synth.SYNTH_CFG, synth.make_state_dict(synth.SYNTH_CFG, 0)
    sr_in = 16000
    audio = synth.lowres_clip(0, 10.0, sr_in)

    def run(method="euler", steps=1, **kw):
        m = FlowHighSR(FLowHigh(sd, cfg, dev, **kw), prior="device", torchdiffeq_ode_method=method)
        y = m.generate(audio, sr_in, 48000, steps, seed=0).clone()
        return m, y

    m0, base = run()
    rows = []
    for name, kw in (("attn_window=100", dict(attn_window=100)), ("attn_window=250", dict(attn_window=250)),
                     ("attn_window=500", dict(attn_window=500)), ("attn_form='bf16x6'", dict(attn_form="bf16x6")),
                     ("conv_form='winograd'", dict(conv_form="winograd")), ("conv_form='direct_bf16x3'", dict(conv_form="direct_bf16x3"))):
        _, y = run(**kw)
        q = m0.measure_quality(y, base, cutoff_hz=sr_in / 2)[0].tolist()
        rows.append((name, "the default, euler x 1", q, (y - base).abs().max().item()))
        print("variant", rows[-1], flush=True)
        torch.cuda.empty_cache()
    _, y4 = run("midpoint", 4)
    _, y1 = run("midpoint", 1)
    q = m0.measure_quality(y1, y4, cutoff_hz=sr_in / 2)[0].tolist()
    rows.append(("midpoint, timestep=1", "midpoint, timestep=4", q, (y1 - y4).abs().max().item()))
    print("variant", rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quality.md"))
    ap.add_argument("--skip-variants", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench needs a GPU")
    dev = torch.device("cuda:0")
    times = time_rows(dev)
    lines = [HEADING, "", f"`python tools/quality_bench.py` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.", "",
             "Mono pairs of 10 s at 48 kHz (noise of amplitude 0.1 against itself plus noise of 0.01), cutoff 8 kHz.  `fused`: "
             "`measure_quality` as a caller runs it (the table upload, `fh_quality_frames_f32`, `fh_quality_report_f32`); `composed`: "
             "`fh_frame_f32` + `fh_rfft2048_f32` on both signals into buffers allocated once, then torch in float64.  Device events "
             "around 10 calls, one warm-up call, ms per call: the median (2nd - 3rd quartile) of 9 such groups.  Workspace: what a "
             "path holds besides the two signals and the result (the composed path's torch temporaries, several times its float "
             "tensors in float64, are not counted).", "",
             "| pairs | frames | fused ms | composed ms | composed / fused | fused workspace | composed workspace | largest difference of a figure |",
             "|---|---|---|---|---|---|---|---|"]
    for r in times:
        f, c = r["fused"], r["composed"]
        lines.append(f"| {r['R']} | {r['frames']} | {f[0]:.3f} ({f[1]:.3f}-{f[2]:.3f}) | {c[0]:.3f} ({c[1]:.3f}-{c[2]:.3f}) | {c[0] / f[0]:.1f} | "
                     f"{r['fused_bytes'] / 1e6:.2f} MB | {r['composed_bytes'] / 1e6:.1f} MB | {r['diff']:.1e} |")
    if not a.skip_variants:
        lines += ["", "`measure_quality(variant, baseline, cutoff_hz=8000)` on one 10 s clip from 16 kHz, the synthetic SYNTH_CFG "
                  "checkpoint, device prior with seed 0.  **Synthetic weights give distances between computations, not perceptual "
                  "quality.**", "",
                  "| variant | against | lsd | lsd_low | lsd_high | snr_db | waveform max-abs |", "|---|---|---|---|---|---|---|"]
        for name, base, q, mx in variant_rows(dev):
            lines.append(f"| `{name}` | {base} | {q[0]:.3e} | {q[1]:.3e} | {q[2]:.3e} | {q[3]:.2f} | {mx:.2e} |")
    path = Path(a.out)
    head = path.read_text().split(HEADING)[0] if path.exists() else "# The spectral quality report on the device\n\n"
    path.write_text(head + "\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
