"""What streams of channels cost per push: 1 and 16 stereo streams (n_channels=2), each pushed 0.8 s blocks at 48 kHz through the
full chain (44.1 kHz, look-ahead limiter at -1 dBTP, dithered int16, planar) by FlowHighSR.delivery_push's launch sequence, beside
  - the one-shot Delivery.batch(level='input') on one [2, n] block per stream (the yardstick of profiles/stream_delivery.md: no
    carry, a clip's edge rules at both ends, not the same result), and
  - twice as many mono streams pushed the same blocks (the mono path: the entries and the host code a stream without n_channels
    runs, which this tool's tree leaves as they were; not the same result either: two envelopes, channel 0's dither for both).
And the linked limiter launch alone, fh_stream_limit_linked_f32 on n groups of 2 jobs, against fh_stream_limit_f32 on the same 2 n
jobs, in a 48 kHz stream's steady state.  Wall time per call with a synchronise behind it and device events; alternating rounds
in one process.  Needs no model.  Writes profiles/stream_channels.md (or the path given).

python tools/stream_channels_bench.py [--rounds 9] [--channels 2] [--out profiles/stream_channels.md]"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from flowhigh_amd import delivery_stream as DS, hip, truepeak                          # noqa: E402
from flowhigh_amd.delivery import Delivery, resolve_delivery                           # noqa: E402
from flowhigh_amd.frontend import Resampler, upload_tables                             # noqa: E402
from stream_delivery_bench import (BLOCK, CEILING, CHAIN, LAUNCHES, PUSHES, RATE, count_launches, events_ms, quartiles,  # noqa: E402
                                   wall_ms)


def med(v):
    return statistics.median(v), quartiles(v)


def limiter_launches(D, n, C, dev, rounds):
    """fh_stream_limit_linked_f32 on n groups of C jobs against fh_stream_limit_f32 on the same n C jobs (steady state of a 48 kHz
    stream: a carry of 2 D samples, a fresh block, as many outputs as came in): ms per launch from device events."""
    L, H = hip.lib(), truepeak.half_window(48000)
    Dl, c32 = 2 * H + truepeak.HALF, float(np.float32(truepeak.ceiling(CEILING)))
    taps, w = D._tp_taps(), D._window(H)
    R = n * C
    carry, fresh = torch.randn(R, 2 * Dl, device=dev) * 0.4, torch.randn(R, BLOCK, device=dev) * 0.4
    outs = [torch.empty(R, BLOCK, device=dev) for _ in range(2)]
    keeps = [torch.empty(R, 2 * Dl, device=dev) for _ in range(2)]
    base = 10 * BLOCK
    tables = []
    for out, keep_buf in zip(outs, keeps):
        jobs = [hip.StreamJob(carry[i].data_ptr(), fresh[i].data_ptr(), out[i].data_ptr(), keep_buf[i].data_ptr(), base, base + Dl,
                              2 * Dl, BLOCK, BLOCK, 2 * Dl, 0, 0) for i in range(R)]
        tables.append((hip.StreamJob * R)(*jobs))
    keep, (jm, jl, gp) = upload_tables(tables + [np.arange(0, R + 1, C, dtype=np.int32)], dev)

    def mono():
        hip.check(L.fh_stream_limit_f32(jm, R, BLOCK, taps, w, H, c32, hip.stream()), "fh_stream_limit_f32")

    def linked():
        hip.check(L.fh_stream_limit_linked_f32(jl, R, gp, n, BLOCK, taps, w, H, c32, hip.stream()), "fh_stream_limit_linked_f32")
    mono()
    linked()
    torch.cuda.synchronize()
    assert torch.equal(keeps[0], keeps[1]) and (C > 1 or torch.equal(outs[0], outs[1])), "the two launches carry different tails"
    mo, li = [], []
    for _ in range(rounds):                                              # alternating
        mo.append(events_ms(mono, LAUNCHES))
        li.append(events_ms(linked, LAUNCHES))
    return dict(mono=med(mo), linked=med(li), ratio=med([a / b for a, b in zip(li, mo)]), spread=(max(mo) - min(mo)) / statistics.median(mo))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stream_channels.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_channels_bench needs a GPU")
    C = a.channels
    dev = torch.device("cuda:0")
    D = Delivery(dev, Resampler(dev))
    opt = resolve_delivery(1, level="input", **CHAIN)
    rows = []
    for n in (1, 16):
        blocks = [torch.randn(C, BLOCK, device=dev) * 0.4 for _ in range(n)]
        mono_blocks = [b[c:c + 1] for b in blocks for c in range(C)]
        whole = torch.cat(blocks, 0).contiguous()
        streams = [DS.DeliveryStream(DS.resolve(CHAIN, None, C)) for _ in range(n)]
        monos = [DS.DeliveryStream(DS.resolve(CHAIN)) for _ in range(n * C)]
        opt_n = dict(opt, keys=[opt["keys"][0]] * n)
        calls = dict(push=lambda: DS.push(D, streams, blocks), mono=lambda: DS.push(D, monos, mono_blocks),
                     one=lambda: D.batch(whole, [C] * n, "input", opt_n, range(n)))
        for _ in range(5):                                               # warm: the carries fill, every shape has run
            for fn in calls.values():
                fn()
        launches = {k: count_launches(fn) for k, fn in calls.items()}
        t = {f"{k}{s}": [] for k in calls for s in ("", "_ev")}
        for _ in range(a.rounds):                                        # alternating, one process
            for k, fn in calls.items():
                t[k].append(wall_ms(fn, PUSHES))
                t[k + "_ev"].append(events_ms(fn, PUSHES))
        lim = limiter_launches(D, n, C, dev, a.rounds)
        rows.append((n, {k: med(v) for k, v in t.items()}, launches, lim))
        print(n, {k: round(statistics.median(v), 4) for k, v in t.items()}, lim, flush=True)
    cell = lambda v: f"{v[0]:.3f} ({v[1][0]:.3f}-{v[1][1]:.3f})"                        # noqa: E731
    c4 = lambda v: f"{v[0]:.4f} ({v[1][0]:.4f}-{v[1][1]:.4f})"                          # noqa: E731
    H48 = truepeak.half_window(48000)
    lines = ["# Streams of channels: what a push costs", "",
             f"`python tools/stream_channels_bench.py --rounds {a.rounds} --channels {C}` on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}.  Every stream has {C} channels (`n_channels={C}`) and is pushed blocks of {BLOCK} samples (0.8 s at 48 kHz) "
             f"through the full chain: {RATE} Hz, `limiter='lookahead'` at {CEILING:g} dBTP, dithered int16, planar.  ms per call: median "
             f"(quartiles) of {a.rounds} alternating rounds of {PUSHES} calls in one process, all three calls in every round; **wall** is a "
             "host clock around the calls with a synchronise behind them, **device events** bracket the same calls; a timed window is "
             "40-150 ms.  No bar is set on these numbers.", "",
             f"- **push**: `delivery_push` of the streams of {C} channels: `{'`, `'.join(rows[0][2]['push'])}`",
             f"- **one-shot**: `Delivery.batch(level='input')` on one `[{C}, n]` block per stream, the yardstick of `profiles/stream_delivery.md`: "
             f"no carry, a clip's edge rules at both ends of every block, not the same result: `{'`, `'.join(rows[0][2]['one'])}`",
             f"- **mono x {C}**: `delivery_push` of {C} times as many mono streams on the same samples -- the entries and host code of a stream "
             f"opened without `n_channels`, which are the parent commit's -- and not the same result ({C} envelopes, channel 0's dither for "
             f"every row): `{'`, `'.join(rows[0][2]['mono'])}`", "",
             f"| streams | push, wall | one-shot, wall | push / one-shot | mono x {C}, wall | push / mono x {C} | push, device events | mono x {C}, device events |",
             "|---|---|---|---|---|---|---|---|"]
    for n, t, launches, lim in rows:
        lines.append(f"| {n} | {cell(t['push'])} | {cell(t['one'])} | {t['push'][0] / t['one'][0]:.2f} | {cell(t['mono'])} | "
                     f"{t['push'][0] / t['mono'][0]:.2f} | {cell(t['push_ev'])} | {cell(t['mono_ev'])} |")
    lines += ["", "## The linked limiter launch against the mono launch with as many jobs", "",
              f"`fh_stream_limit_linked_f32` on n groups of {C} jobs against `fh_stream_limit_f32` on the same {C} n jobs, a 48 kHz stream's steady "
              f"state (H = {H48}: a carry of {2 * (2 * H48 + 10)} samples and a fresh block of {BLOCK}, {BLOCK} outputs per job); the carried tails "
              f"are compared bit for bit before timing.  Device events around {LAUNCHES} launches, ms per launch: median (quartiles) of {a.rounds} "
              "alternating rounds; the ratio is taken round by round; the margin is the mono launch's own spread over the rounds, (max - min) / median.", "",
              f"| streams | fh_stream_limit_f32, {C} n jobs | fh_stream_limit_linked_f32, n groups | linked / mono, per round | spread of the mono launch |",
              "|---|---|---|---|---|"]
    for n, t, launches, lim in rows:
        lines.append(f"| {n} | {c4(lim['mono'])} | {c4(lim['linked'])} | {lim['ratio'][0]:.3f} ({lim['ratio'][1][0]:.3f}-{lim['ratio'][1][1]:.3f}) | "
                     f"{lim['spread']:.1%} |")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
