"""What the loudness meter costs on the device.
  report   fh_loudness_report_f32 for ONE stereo clip of 10 s, 60 s and 600 s at 48 kHz beside fh_loudness_gate_f32 on the same
           energies (device events, the median of 5 x 10 launches), and the report's share per part: the same launch over clips
           cut so that a part has nothing to do (no short-term window: the gate and the momentary maximum alone)
  stream   FlowHighSR.delivery_push of 8 mono streams, 100 ms blocks at 48 kHz, output_rate=44100 + the limiter + int16 with
           dither, with meter=True against the same push without it (host clock around push + synchronize, the median of the
           pushes of 20 s of stream), and loudness() of one of them
Writes the tables to profiles/meter.md (or the path given) under the heading "## Measurements"; what stands above that heading
in the file is kept.

python tools/meter_bench.py [--out profiles/meter.md]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import FLowHigh, FlowHighSR, delivery, hip, loudness, synth          # noqa: E402

RATE = 48000
HEADING = "## Measurements"


def events_ms(fn, reps=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def median_ms(fn):
    return statistics.median(events_ms(fn) for _ in range(5))


def report_rows(dev):
    L = hip.lib()
    hop, _ = loudness.geometry(RATE)
    out = []
    for seconds in (10, 60, 600):
        T, C = seconds * RATE, 2
        level = 0.02 + 0.3 * (torch.arange(T, device=dev) // (5 * RATE) % 3 == 0)           # (steps of 24 dB every 5 s: a range to select)
        x = torch.randn(C, T, device=dev) * level
        n_sub = -(-T // hop)
        e = torch.empty(C, n_sub, dtype=torch.float64, device=dev)
        hip.check(L.fh_kweight_energy_f32(x.data_ptr(), delivery._coef(RATE), e.data_ptr(), C, T, hop, hip.stream()), "energies")
        lens = torch.full((C,), T, dtype=torch.int32, device=dev)
        momentary_only = torch.full((C,), 29 * hop, dtype=torch.int32, device=dev)              # (no short-term window)
        group = torch.zeros(C, dtype=torch.int32, device=dev)
        peak = torch.zeros(C, dtype=torch.int32, device=dev)
        lufs, gains = torch.empty(1, device=dev), torch.empty(C, device=dev)
        rep = torch.empty(1, 6, device=dev)

        def gate(ln=lens):
            hip.check(L.fh_loudness_gate_f32(e.data_ptr(), n_sub, ln.data_ptr(), group.data_ptr(), C, 1, hop, float("nan"), peak.data_ptr(),
                                             lufs.data_ptr(), gains.data_ptr(), hip.stream()), "gate")

        def report(ln=lens):
            hip.check(L.fh_loudness_report_f32(e.data_ptr(), n_sub, ln.data_ptr(), group.data_ptr(), C, 1, hop, rep.data_ptr(), hip.stream()),
                      "report")

        row = dict(seconds=seconds, n_sub=n_sub, windows=n_sub - 29, gate_ms=median_ms(gate), report_ms=median_ms(report),
                   fixed_ms=median_ms(lambda: report(momentary_only)), figures=[round(v, 3) for v in rep[0].tolist()])
        report()
        torch.cuda.synchronize()
        row["figures"] = [round(v, 3) for v in rep[0].tolist()]
        out.append(row)
        print("report", row, flush=True)
    return out


def stream_rows(dev):
    cfg = synth.TINY_CFG
    m = FlowHighSR(FLowHigh(synth.make_state_dict(cfg, 0), cfg, dev), prior="device", torchdiffeq_ode_method="euler")
    kw = dict(output_rate=44100, true_peak=-1.0, limiter="lookahead", pcm="int16", dither="tpdf")
    n, block, pushes = 8, RATE // 10, 200
    x = torch.randn(n, 1, block * pushes, device=dev) * 0.3
    out = {}
    for name, extra in (("plain", {}), ("metered", dict(meter=True)), ("plain again", {})):
        streams = [m.delivery_stream(dither_seed=i, **kw, **extra) for i in range(n)]
        t = []
        for k in range(pushes):
            blocks = [x[i, :, k * block:(k + 1) * block] for i in range(n)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.delivery_push(streams, blocks)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        t = sorted(t[10:])
        out[name] = (statistics.median(t), t[len(t) // 4], t[3 * len(t) // 4])
        if extra:
            out["loudness()"] = median_ms(streams[0].loudness)
            out["measured"] = streams[0].meter.measured
        print("stream", name, out[name], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "meter.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meter_bench needs a GPU")
    dev = torch.device("cuda:0")
    rep, stream = report_rows(dev), stream_rows(dev)
    lines = [HEADING, "", f"`python tools/meter_bench.py` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.", "",
             "One stereo clip at 48 kHz, noise whose level steps by 24 dB every 5 s; one launch, device events, the median of 5 x 10 "
             "launches, ms.  `fixed`: the report launch with the clip's length set to 2.9 s, where no short-term window exists: the "
             "row search, the gate and the momentary maximum of a clip that short.", "",
             "| clip | sub-blocks | short-term windows | fh_loudness_gate_f32 | fh_loudness_report_f32 | report / gate | fixed | I, M_max, S_max, LRA, M, S |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rep:
        lines.append(f"| {r['seconds']} s | {r['n_sub']} | {r['windows']} | {r['gate_ms']:.3f} | {r['report_ms']:.3f} | "
                     f"{r['report_ms'] / r['gate_ms']:.1f} | {r['fixed_ms']:.3f} | {r['figures']} |")
    lines += ["", "`delivery_push` of 8 mono streams, one 100 ms block each (4800 samples at 48 kHz), `output_rate=44100, true_peak=-1, "
              "limiter='lookahead', pcm='int16', dither='tpdf'`: host clock around the push and a synchronize, ms, median (quartiles) "
              "of 190 pushes; the plain streams are timed before and after the metered ones.", "",
              "| streams | ms per push |", "|---|---|"]
    for name in ("plain", "metered", "plain again"):
        med, q1, q3 = stream[name]
        lines.append(f"| {name} | {med:.3f} ({q1:.3f}-{q3:.3f}) |")
    lines += ["", f"`loudness()` of one of the metered streams behind its 20 s ({stream['measured']} samples measured): "
              f"{stream['loudness()']:.3f} ms per call (device events; one small table upload and the report launch)."]
    path = Path(a.out)
    head = path.read_text().split(HEADING)[0] if path.exists() else "# The loudness meter on the device\n\n"
    path.write_text(head + "\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
