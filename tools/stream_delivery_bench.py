"""What streaming delivery costs per push: 1, 4 and 16 streams, each pushed 0.8 s blocks at 48 kHz through the full chain (44.1 kHz,
look-ahead limiter at -1 dBTP, dithered int16) by FlowHighSR.delivery_push's launch sequence, beside the one-shot
Delivery.batch(level='input') on one block of the same size per stream (no carry, a clip's edge rules at both ends: what a caller
without streaming delivery would run per block, and not the same result).  Wall time per call with a synchronise behind it and the
launches alone from device events; launches counted per push; and the fused limiter kernel against the two launches it stands
for, on the same samples.  Needs no model.  Writes profiles/stream_delivery.md (or the path given).

python tools/stream_delivery_bench.py [--rounds 10] [--out profiles/stream_delivery.md]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import delivery_stream as DS, hip, truepeak                          # noqa: E402
from flowhigh_amd.delivery import Delivery, resolve_delivery                           # noqa: E402
from flowhigh_amd.frontend import Resampler, upload_tables                             # noqa: E402

BLOCK, RATE, CEILING = 38400, 44100, -1.0                                              # 0.8 s at 48 kHz
CHAIN = dict(output_rate=RATE, pcm="int16", dither="tpdf", dither_seed=9, true_peak=CEILING, limiter="lookahead")
TILE = 1024                                                                            # csrc/stream_delivery.hip, csrc/truepeak.hip
PUSHES = 500                                                                           # calls per timed window: 40-150 ms
LAUNCHES = 2000                                                                        # launch sets per timed window of the limiter alone: 50-100 ms


def quartiles(v):
    s = sorted(v)
    return s[len(s) // 4], s[(3 * len(s)) // 4]


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def count_launches(fn):
    """The library entries `fn` goes through, by name."""
    seen, check = [], hip.check

    def counting(rc, what=""):
        seen.append(what)
        return check(rc, what)
    hip.check = DS.hip.check = counting
    try:
        fn()
    finally:
        hip.check = DS.hip.check = check
    return seen


def limiter_alone(D, n, dev, rounds):
    """fh_stream_limit_f32 in the steady state of a 48 kHz stream (a carry of 2 D samples, a fresh block, as many outputs as came
    in) against fh_tp_envelope_f32 + fh_limit_f32 on rows of the same samples: ms per launch set from device events."""
    L, H = hip.lib(), truepeak.half_window(48000)
    Dl, c32 = 2 * H + truepeak.HALF, float(np.float32(truepeak.ceiling(CEILING)))
    taps, w = D._tp_taps(), D._window(H)
    carry = torch.randn(n, 2 * Dl, device=dev) * 0.4
    fresh = torch.randn(n, BLOCK, device=dev) * 0.4
    out, keep_buf = torch.empty(n, BLOCK, device=dev), torch.empty(n, 2 * Dl, device=dev)
    base = 10 * BLOCK
    jobs = [hip.StreamJob(carry[i].data_ptr(), fresh[i].data_ptr(), out[i].data_ptr(), keep_buf[i].data_ptr(), base, base + Dl,
                          2 * Dl, BLOCK, BLOCK, 2 * Dl, 0, 0) for i in range(n)]
    keep, (jp,) = upload_tables([(hip.StreamJob * n)(*jobs)], dev)
    rows = torch.cat([carry, fresh], 1).contiguous()
    T = rows.shape[1]
    m, y = torch.empty(n, T, device=dev), torch.empty(n, T, device=dev)

    def fused():
        hip.check(L.fh_stream_limit_f32(jp, n, BLOCK, taps, w, H, c32, hip.stream()), "fh_stream_limit_f32")

    def two():
        hip.check(L.fh_tp_envelope_f32(rows.data_ptr(), taps, m.data_ptr(), n, 1, T, hip.stream()), "fh_tp_envelope_f32")
        hip.check(L.fh_limit_f32(rows.data_ptr(), y.data_ptr(), m.data_ptr(), w, 0, n, 1, T, H, c32, hip.stream()), "fh_limit_f32")
    fused()
    two()
    torch.cuda.synchronize()
    # the fused kernel's outputs are the two launches' at the same absolute samples (first = base + D is row index D)
    assert torch.equal(out, y[:, Dl:Dl + BLOCK]), "the fused limiter and the two launches differ"
    fu, tw = [], []
    for _ in range(rounds):                                              # alternating
        fu.append(events_ms(fused, LAUNCHES))
        tw.append(events_ms(two, LAUNCHES))
    ratio = [a / b for a, b in zip(fu, tw)]
    return {k: (statistics.median(v), quartiles(v)) for k, v in dict(fused=fu, two=tw, ratio=ratio).items()}, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stream_delivery.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_delivery_bench needs a GPU")
    dev = torch.device("cuda:0")
    D = Delivery(dev, Resampler(dev))
    opt = resolve_delivery(1, level="input", **CHAIN)
    rows = []
    for n in (1, 4, 16):
        blocks = [torch.randn(1, BLOCK, device=dev) * 0.4 for _ in range(n)]
        whole = torch.cat(blocks, 0).contiguous()
        streams = [DS.DeliveryStream(DS.resolve(CHAIN)) for _ in range(n)]
        opt_n = dict(opt, keys=[opt["keys"][0]] * n)

        def push():
            return DS.push(D, streams, blocks)

        def one_shot():
            return D.batch(whole, [1] * n, "input", opt_n, range(n))
        for _ in range(5):                                               # warm: the carries fill, every shape has run
            push()
            one_shot()
        launches = count_launches(push)
        launches_one = count_launches(one_shot)
        out_len = [int(y.shape[1]) for y in push()]
        t = dict(push=[], one=[], push_ev=[], one_ev=[])
        for _ in range(a.rounds):                                        # alternating, one process
            t["push"].append(wall_ms(push, PUSHES))
            t["one"].append(wall_ms(one_shot, PUSHES))
            t["push_ev"].append(events_ms(push, PUSHES))
            t["one_ev"].append(events_ms(one_shot, PUSHES))
        lim, T = limiter_alone(D, n, dev, a.rounds)
        rows.append((n, {k: (statistics.median(v), quartiles(v)) for k, v in t.items()}, launches, launches_one, out_len, lim, T))
        print(n, {k: round(statistics.median(v), 4) for k, v in t.items()}, launches, launches_one, out_len[0], lim, flush=True)
    H441, H48 = truepeak.half_window(RATE), truepeak.half_window(48000)
    cell = lambda v: f"{v[0]:.3f} ({v[1][0]:.3f}-{v[1][1]:.3f})"                        # noqa: E731
    lines = ["# Streaming delivery: what a push costs", "",
             f"`python tools/stream_delivery_bench.py --rounds {a.rounds}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  "
             f"Every stream is pushed blocks of {BLOCK} samples (0.8 s at 48 kHz) through the full chain: {RATE} Hz, `limiter='lookahead'` at "
             f"{CEILING:g} dBTP, dithered int16.  ms per call: median (quartiles) of {a.rounds} alternating rounds of {PUSHES} calls in one "
             "process; **wall** is a host clock around the calls with a synchronise behind them, **device events** bracket the same calls "
             "(with so little work per launch both are the host's enqueue time, not kernel time); a timed window is 40-150 ms.  No bar is set on these numbers: "
             "they were unmeasured before.", "",
             "- **push**: `delivery_push(streams, blocks)`: the carried delivery, whose blocks add up to the one-shot delivery of the whole stream",
             "- **one-shot**: `Delivery.batch(block, level='input')` on one block per stream: no carry, a clip's edge rules at both ends of "
             "every block -- what a caller ran per block before, and not the same result", "",
             "| streams | push, wall | one-shot, wall | push / one-shot | push, device events | one-shot, device events | launches per push | launches per one-shot | delivered samples per push |",
             "|---|---|---|---|---|---|---|---|---|"]
    for n, t, launches, launches_one, out_len, lim, T in rows:
        lines.append(f"| {n} | {cell(t['push'])} | {cell(t['one'])} | {t['push'][0] / t['one'][0]:.2f} | {cell(t['push_ev'])} | {cell(t['one_ev'])} | "
                     f"{len(launches)} | {len(launches_one)} | {out_len[0]} |")
    lines += ["", f"Launches of a push: {', '.join('`' + k + '`' for k in rows[0][2])}; of the one-shot: "
              f"{', '.join('`' + k + '`' for k in rows[0][3])}.  A push also uploads the stages' job tables and the dither keys as one buffer.  "
              "What a push costs over the one-shot is host time: one schedule step, its consistency asserts and one job record per stream "
              "and stage in Python (48 for 16 streams), where the one-shot passes four sets of scalars whatever the number of rows; the "
              "kernels themselves take what the one-shot's take (below).", "",
              "## The fused limiter against the two launches", "",
              f"`fh_stream_limit_f32` in a 48 kHz stream's steady state (H = {H48}: a carry of {2 * (2 * H48 + 10)} samples and a fresh block "
              f"of {BLOCK}, {BLOCK} outputs) against `fh_tp_envelope_f32` + `fh_limit_f32` on rows of the same {rows[0][6]} samples; the "
              f"outputs are compared bit for bit before timing.  Device events around {LAUNCHES} launch sets, ms per set: median (quartiles) of "
              f"{a.rounds} alternating rounds; the ratio is taken round by round.", "",
              "| streams | fh_stream_limit_f32 | fh_tp_envelope_f32 + fh_limit_f32 | fused / two, per round |", "|---|---|---|---|"]
    for n, t, launches, launches_one, out_len, lim, T in rows:
        c4 = lambda v: f"{v[0]:.4f} ({v[1][0]:.4f}-{v[1][1]:.4f})"                      # noqa: E731
        lines.append(f"| {n} | {c4(lim['fused'])} | {c4(lim['two'])} | {lim['ratio'][0]:.3f} ({lim['ratio'][1][0]:.3f}-{lim['ratio'][1][1]:.3f}) |")
    lines += ["", f"The fused kernel computes the envelope over tile +- 2 H: (TILE + 4 H) / TILE = {(TILE + 4 * H48) / TILE:.3f} of the envelope "
              f"work at 48 kHz (H = {H48}) and {(TILE + 4 * H441) / TILE:.3f} at {RATE} Hz (H = {H441}) with TILE = {TILE}; the recomputed "
              f"share of its envelope work is 4 H / (TILE + 4 H) = {4 * H48 / (TILE + 4 * H48):.1%} and {4 * H441 / (TILE + 4 * H441):.1%}.  "
              "That buys one launch instead of two and no round trip of m through memory."]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
