"""GPU: the loudness meter -- fh_loudness_report_f32 on planted double energies and FlowHighSR.measure_loudness_report end to end
against flowhigh_amd/meter.py, fh_stream_kweight_energy_f32 against fh_kweight_energy_f32 bit for bit, LoudnessMeter / meter_push
against measure_loudness_report bit for bit, and delivery_stream(meter=True).

Bars (those of test_hip_loudness.py).  Any LUFS / LU figure against the float64 definition: 1e-5 LU -- a float32 below 64 in
magnitude rounds by at most 3.8e-6, the double arithmetic error is negligible; -inf and a range of 0 exactly.  Where two runs of
this project are compared the test is bitwise.  Inputs are asserted, from the definition alone, to keep every window 1e-6
relative away from a gate threshold and the two selected percentiles 1e-9 relative away from their neighbours.

Low rates make long series of few samples: rate 160 has hop 16, block 64 and 480 samples to a short-term window.  Through the
K-weighting itself, though, 160 Hz is a rate at which loudness.k_weighting's re-designed shelf is UNSTABLE (its poles lie at radius
1.056: the shelf's 1682 Hz are far above that Nyquist), so noise of 4096 samples measures +1900 LUFS and 8193 samples overflow
float64 in the definition itself.  The end-to-end test keeps the rate, with the bar that float32 allows there -- 1e-5 LU times
|value| / 64 above 64, a float32's spacing growing with its magnitude -- and exact equality where the definition gives an
infinity; rate 165 (hop 17, poles at 0.45) stands beside it as the low rate at which the figures are ordinary."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, loudness, meter, synth     # noqa: E402

GUARD = 16
SENT32 = 0x7fc12345
SPAN = 4096
NOTHING = (-math.inf, -math.inf, -math.inf, 0.0, -math.inf, -math.inf)
_STATE = {}


def st():
    return hip.stream()


def coef(rate):
    key = ("coef", rate)
    if key not in _STATE:
        _STATE[key] = (ctypes.c_double * 10)(*loudness.coefficients(rate))
    return ctypes.addressof(_STATE[key])


def model():
    if "model" not in _STATE:
        fh = FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda")
        _STATE["model"] = FlowHighSR(fh, prior="device", torchdiffeq_ode_method="euler")
    return _STATE["model"]


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def bar(want):
    return 1e-5 * max(1.0, abs(want) / 64.0)


def close(got, want, what):
    """One report row against the definition's six floats; -> the worst error over its bar."""
    worst = 0.0
    for name, g, w in zip(meter.FIELDS, (float(v) for v in got), want):
        if math.isinf(w) or w == 0.0:
            assert g == w, (what, name, g, w)
        else:
            worst = max(worst, abs(g - w) / bar(w))
            assert abs(g - w) <= bar(w), (what, name, g, w)
    return worst


def clear_of_the_gates(e, T, rate):
    """From the definition alone: no block or window within 1e-6 relative of a gate threshold, the selected percentiles not
    within 1e-9 relative of their neighbours."""
    for z, rel in ((meter.momentary(e, T, rate), loudness.REL_GATE), (meter.short_term(e, T, rate), meter.LRA_REL_GATE)):
        z = z[np.isfinite(z)]
        assert (np.abs(z - loudness.ZA) > 1e-6 * loudness.ZA).all()
        absolute = z > loudness.ZA
        if absolute.any():
            thr = rel * z[absolute].mean()
            assert (np.abs(z - thr) > 1e-6 * thr).all()
    zs = meter.short_term(e, T, rate)
    v = np.sort(zs[meter.range_gate(zs)])
    for k in meter.percentile_ranks(v.size) if v.size else ():
        for other in (k - 1, k + 1):
            assert not 0 <= other < v.size or abs(v[other] - v[k]) > 1e-9 * v[k]


# ---- 1. the report kernel on planted energies -----------------------------------------------------------------------------------
def planted_clips():
    """-> (rate, [(name, e [C, n_sub], T)]): K = 1 .. 5000 complete sub-blocks (ns = K - 29 windows: none, 1, 2, and either side of
    one sweep of 256), some with a partial sub-block behind them, C = 1, 2 and 8; the gates' cases."""
    rate, hop = 160, 16
    rng = np.random.default_rng(7)
    clips = []
    for n, (K, C, partial) in enumerate([(1, 1, 0), (29, 2, 5), (30, 8, 0), (31, 1, 3), (284, 2, 0), (285, 8, 0), (286, 1, 15),
                                         (287, 2, 0), (5000, 8, 0), (5000, 1, 9)]):
        level = np.where((np.arange(K + 1) // 40) % 3 == 1, 0.05, 1.0)            # (steps of 13 dB: the range has something to read)
        e = rng.uniform(20.0, 60.0, (C, K + 1)) * level
        clips.append((f"K{K}C{C}", e[:, :K + (partial > 0)], K * hop + partial))
    clips.append(("silent", np.zeros((2, 40)), 40 * hop))
    clips.append(("absolute", rng.uniform(0.1, 0.9, (2, 60)) * loudness.ZA * hop / 2, 60 * hop))       # every window under -70 LUFS
    e = rng.uniform(20.0, 60.0, (1, 200))
    e[:, :100] *= 1e-4                           # the quiet half is 40 dB down: the relative gate (-20 LU) takes its windows out
    clips.append(("relative", e, 200 * hop))
    return rate, clips


def run_report(rate, clips, with_gate=True):
    hop, _ = loudness.geometry(rate)
    rows = sum(e.shape[0] for _, e, _ in clips)
    n_sub = max(e.shape[1] for _, e, _ in clips)
    host = np.full((rows, n_sub), np.nan)
    lens, group, r = [], [], 0
    for i, (_, e, T) in enumerate(clips):
        host[r:r + e.shape[0], :e.shape[1]] = e
        r += e.shape[0]
        lens += [T] * e.shape[0]
        group += [i] * e.shape[0]
    ed = torch.from_numpy(host).cuda()
    ld, gd = torch.tensor(lens, dtype=torch.int32).cuda(), torch.tensor(group, dtype=torch.int32).cuda()
    n = len(clips)
    out = torch.full((GUARD + 6 * n + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    L = hip.lib()
    hip.check(L.fh_loudness_report_f32(ed.data_ptr(), n_sub, ld.data_ptr(), gd.data_ptr(), rows, n, hop, out[GUARD:].data_ptr(), st()),
              "fh_loudness_report_f32")
    assert bool((out[:GUARD] == SENT32).all()) and bool((out[GUARD + 6 * n:] == SENT32).all())
    report = out[GUARD:GUARD + 6 * n].view(torch.float32).view(n, 6)
    if with_gate:
        lufs, gains = torch.empty(n, device="cuda"), torch.empty(rows, device="cuda")
        peaks = torch.zeros(rows, dtype=torch.int32, device="cuda")
        hip.check(L.fh_loudness_gate_f32(ed.data_ptr(), n_sub, ld.data_ptr(), gd.data_ptr(), rows, n, hop, math.nan, peaks.data_ptr(),
                                         lufs.data_ptr(), gains.data_ptr(), st()), "fh_loudness_gate_f32")
        assert same_bits(report[:, 0], lufs)
    return report.cpu().numpy()


def test_the_report_kernel_against_the_definition_on_planted_energies():
    rate, clips = planted_clips()
    want = {}
    for name, e, T in clips:
        clear_of_the_gates(e, T, rate)
        want[name] = meter.report_from_energies(e, T, rate)
    # the cases are what they are planted as
    assert want["silent"] == NOTHING and want["K1C1"][2] == -math.inf and want["K29C2"][2] == -math.inf
    assert want["absolute"][0] == -math.inf and want["absolute"][3] == 0.0 and -90 < want["absolute"][2] < -70
    zs = meter.short_term(clips[-1][1], clips[-1][2], rate)
    gated = meter.range_gate(zs)
    assert zs.size == 171 and 60 < gated.sum() < 110 and not gated[:60].any() and 0.0 < want["relative"][3] < 10.0
    assert want["K5000C8"][3] > 3.0 and want["K31C1"][3] >= 0.0
    got = run_report(rate, clips)                                        # every clip in ONE launch
    worst = max(close(got[i], want[name], name) for i, (name, _, _) in enumerate(clips))
    print(f"meter: report on planted energies: worst error / bar {worst:.2e}")
    # a clip alone, and in another place of another table, has the bits it has in company
    for i in (3, 8, len(clips) - 1):
        alone = run_report(rate, [clips[i]], with_gate=False)
        pair = run_report(rate, [clips[0], clips[i]], with_gate=False)
        assert np.array_equal(alone[0].view(np.int32), got[i].view(np.int32)), clips[i][0]
        assert np.array_equal(pair[1].view(np.int32), got[i].view(np.int32)), clips[i][0]


# ---- 2. measure_loudness_report end to end ----------------------------------------------------------------------------------------
def stepped_noise(rows, T, seed):
    """Noise at 0.3 whose second half is 20 dB down, every row at a level of its own."""
    x = torch.randn(rows, T, generator=torch.Generator().manual_seed(seed)).numpy() * 0.3
    x *= np.where(np.arange(T) < T // 2, 1.0, 0.1) * (0.5 + 0.5 * np.arange(1, rows + 1)[:, None] / rows)
    return x.astype(np.float32)


@pytest.mark.parametrize("rate", [160, 165, 8000, 48000])
def test_measure_loudness_report_against_the_definition(rate):
    m = model()
    hop, _ = loudness.geometry(rate)
    worst = 0.0
    for T in (SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1, 30 * hop - 1, 30 * hop, 30 * hop + 1, 45 * hop + 7):
        x = stepped_noise(3, T, seed=rate + T)
        xd = torch.from_numpy(x).cuda()
        clips = [x[:2], x[2:]]
        with np.errstate(over="ignore", invalid="ignore"):
            want = [meter.report(c, rate) for c in clips]
            for c in clips:
                if rate != 160:                      # (at 160 the energies are 1e190 and more: no gate is anywhere near)
                    clear_of_the_gates(loudness.sub_energies(loudness.k_weight(c, rate), rate), T, rate)
        got = m.measure_loudness_report(xd, chans=[2, 1], rate=rate)
        assert got.shape == (2, 6) and got.dtype == torch.float32 and got.is_cuda
        assert same_bits(got[:, 0], m.measure_loudness(xd, chans=[2, 1], rate=rate))
        for i in range(2):
            worst = max(worst, close(got[i].cpu().numpy(), want[i], (rate, T, i)))
        # a list of clips of different lengths: the segment form of the energies
        half = xd[2:, :T // 2]
        listed = m.measure_loudness_report([xd[:2], half], rate=rate)
        assert same_bits(listed[0], got[0])
        assert same_bits(listed[:, 0], m.measure_loudness([xd[:2], half], rate=rate))
        with np.errstate(over="ignore", invalid="ignore"):
            worst = max(worst, close(listed[1].cpu().numpy(), meter.report(x[2:, :T // 2], rate), (rate, T, "listed")))
        assert same_bits(m.measure_loudness_report(xd[2:], rate=rate)[0], got[1])             # (chans=None: every row a clip)
    print(f"meter: measure_loudness_report rate {rate}: worst error / bar {worst:.2e}")


def test_measure_loudness_report_refusals():
    m = model()
    x = torch.zeros(3, 100, device="cuda")
    for bad in (dict(rate=100), dict(rate=44100.5), dict(chans=[2, 2])):
        with pytest.raises(ValueError):
            m.measure_loudness_report(x, **bad)
    with pytest.raises(ValueError):
        m.measure_loudness_report([x], chans=[3])
    with pytest.raises(ValueError):
        m.measure_loudness_report(x[:, :0])


# ---- 3. the stream entry against the batched one ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [16, 800])
def test_the_stream_energies_are_the_batched_energies(hop):
    """A stream of 3 spans + 17 samples in the blocks [1, 4095, 1, 4096, rest], then ended: its log has the bits of
    fh_kweight_energy_f32 on the whole rows, sub-block by sub-block, and the two existing entries are those they were."""
    L, rate, rows = hip.lib(), 8000, 2                   # (the filter of 8 kHz at either hop: the entries take them apart)
    assert L.fh_loudness_span_len() == SPAN == meter.SPAN
    T = 3 * SPAN + 17
    x = torch.from_numpy(stepped_noise(rows, T, seed=hop)).cuda()
    n_sub = -(-T // hop)
    want = torch.empty(rows, n_sub, dtype=torch.float64, device="cuda")
    hip.check(L.fh_kweight_energy_f32(x.data_ptr(), coef(rate), want.data_ptr(), rows, T, hop, st()), "fh_kweight_energy_f32")
    cap = n_sub + 3
    log = torch.full((rows, cap), math.nan, dtype=torch.float64, device="cuda")
    state = torch.zeros(rows, 5, dtype=torch.float64, device="cuda")
    kept = [torch.full((rows, SPAN), math.nan, device="cuda") for _ in range(2)]
    arrived = processed = cur = 0
    for n, ended in [(1, 0), (4095, 0), (1, 0), (4096, 0), (T - 8193, 0), (0, 1)]:
        block = x[:, arrived:arrived + n].contiguous()
        n_kept = arrived - processed
        jobs = (hip.MeterJob * rows)(*[hip.MeterJob(kept[cur][r].data_ptr(), block.data_ptr() + 4 * r * n, kept[cur ^ 1][r].data_ptr(),
                                                    state[r].data_ptr(), log[r].data_ptr(), processed, n_kept, n, cap, ended)
                                       for r in range(rows)])
        dev = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).cuda()
        hip.check(L.fh_stream_kweight_energy_f32(dev.data_ptr(), ctypes.addressof(jobs), rows, coef(rate), hop, st()), "stream energies")
        arrived += n
        processed = arrived if ended else arrived // SPAN * SPAN
        cur ^= 1
        done = processed // hop                          # the complete sub-blocks are final from the push that completes them
        assert torch.equal(log[:, :done].view(torch.int64), want[:, :done].view(torch.int64)), (hop, arrived)
    assert processed == T and torch.equal(log[:, :n_sub].view(torch.int64), want.view(torch.int64))
    assert bool(torch.isnan(log[:, n_sub:]).all())       # nothing behind the stream's last sub-block is written
    # the segment form on the same rows: the third instantiation did not move the other two
    clips = (hip.PcmClip * 1)(hip.PcmClip(x.data_ptr(), 0, T, rows, T))
    table = torch.frombuffer(bytearray(bytes(clips)), dtype=torch.uint8).cuda()
    group = torch.zeros(rows, dtype=torch.int32, device="cuda")
    seg = torch.empty_like(want)
    hip.check(L.fh_kweight_energy_seg_f32(table.data_ptr(), group.data_ptr(), 1, rows, T, coef(rate), seg.data_ptr(), hop, st()), "seg")
    assert torch.equal(seg.view(torch.int64), want.view(torch.int64))
    ref = loudness.sub_energies(loudness.k_weight(x.cpu().numpy(), rate), rate) if hop == 800 else None
    if ref is not None:                                  # (and they are right: test_hip_loudness.py's bar)
        assert (np.abs(want.cpu().numpy() - ref) <= 1e-9 * ref).all()


# ---- 4. LoudnessMeter -----------------------------------------------------------------------------------------------------------
LENS = [1, 4095, 1, 4096, 8197, 0]


def stream_input(channels, rate, seed, extra=3001):
    T = sum(LENS) + extra
    return torch.from_numpy(stepped_noise(channels, T, seed)).cuda(), LENS + [extra]


def reading(m, lm, x):
    """read() against measure_loudness_report of what it covers, bit for bit; -> the row."""
    got = lm.read()
    assert got.shape == (6,) and got.dtype == torch.float32 and got.is_cuda
    if lm.measured == 0:
        assert tuple(got.tolist()) == NOTHING
    else:
        assert same_bits(got, m.measure_loudness_report(x[:, :lm.measured], chans=[x.shape[0]], rate=lm.rate)[0]), lm.measured
    return got


@pytest.mark.parametrize("channels, rate", [(None, 165), (2, 165), (1, 8000)])
def test_a_meter_reads_what_measure_loudness_report_reads(channels, rate):
    m = model()
    x, lens = stream_input(channels or 1, rate, seed=rate + (channels or 0))
    hop, _ = loudness.geometry(rate)
    lm = m.loudness_meter(rate, channels)
    reading(m, lm, x)
    at = 0
    for n in lens:
        block = x[:, at:at + n]
        assert lm.push(block[0] if channels is None and n % 2 else block) is None          # ([n] and [1, n] are one thing)
        at += n
        assert lm.measured == meter.measured(at // SPAN * SPAN, hop)
        reading(m, lm, x)
    assert at == x.shape[1] and 0 < lm.measured < at
    lm.flush()
    assert lm.measured == at and lm.closed
    last = reading(m, lm, x)
    want = meter.report(x.cpu().numpy(), rate)
    assert close(last.cpu().numpy(), want, (channels, rate)) <= 1.0
    assert want[3] > 1.0 or rate != 165              # (at 165 Hz the stream is two minutes long: a range to read)
    with pytest.raises(RuntimeError, match="closed"):
        lm.push(x[:, :10])


def test_meters_pushed_together_are_the_meters_alone():
    """Two meters of one rate with different block lengths and channel counts, and one of another rate, in one meter_push."""
    m = model()
    xa, _ = stream_input(1, 165, seed=1)
    xb, _ = stream_input(2, 165, seed=2, extra=777)
    xc, _ = stream_input(1, 8000, seed=3)
    specs = [(xa, 165, None, [5000, 0, 3300, 9000]), (xb, 165, 2, [1, 8191, 4097, 2000]), (xc, 8000, None, [4096, 4096, 10, 7000])]

    def run(which, together):
        meters = [m.loudness_meter(rate, ch) for _, rate, ch, _ in which]
        at, reads = [0] * len(which), []
        for k in range(4):
            blocks = [x[:, a:a + cuts[k]] for (x, _, _, cuts), a in zip(which, at)]
            at = [a + cuts[k] for (_, _, _, cuts), a in zip(which, at)]
            if together:
                m.meter_push(meters, blocks)
            else:
                for lm, b in zip(meters, blocks):
                    lm.push(b)
            reads.append([lm.read() for lm in meters])
        rest = [x[:, a:] for (x, _, _, _), a in zip(which, at)]
        m.meter_push(meters, rest, final=True) if together else [m.meter_push([lm], [b], final=True) for lm, b in zip(meters, rest)]
        reads.append([lm.read() for lm in meters])
        return reads

    together = run(specs, True)
    for i, spec in enumerate(specs):
        alone = run([spec], False)
        for a, b in zip(alone, together):
            assert same_bits(a[0], b[i]), i
        x, rate, ch, _ = spec
        assert same_bits(together[-1][i], m.measure_loudness_report(x, chans=[x.shape[0]], rate=rate)[0])
    # refusals leave every meter as it was
    a, b = m.loudness_meter(165), m.loudness_meter(165, 2)
    with pytest.raises(ValueError):
        m.meter_push([a, b], [xa[:, :10], xa[:, :10]])       # (b takes [2, n])
    with pytest.raises(ValueError):
        m.meter_push([a, a], [xa[:, :10], xa[:, :10]])
    with pytest.raises(ValueError):
        m.meter_push([a], [xa[:, :10].double()])
    assert a.counters.arrived == b.counters.arrived == 0
    for bad in (dict(n_channels=9), dict(rate=100), dict(log_capacity=0)):
        with pytest.raises(ValueError):
            m.loudness_meter(**bad)


def test_the_log_grows_by_doubling_with_the_same_bits():
    """64 sub-blocks at rate 160 (hop 16): the first span needs 256 of them -- two doublings --, the end a third, which copies
    what the log holds.  (Rate 160: the figures are astronomic, see above, and finite up to 6400 samples; the test is bitwise.)"""
    m, rate = model(), 160
    x = torch.from_numpy(stepped_noise(2, SPAN + 1500, seed=5)).cuda()
    small, roomy = m.loudness_meter(rate, 2, log_capacity=64), m.loudness_meter(rate, 2)
    caps = []
    for a, b in ((0, 3000), (3000, 4596), (4596, x.shape[1])):
        for lm in (small, roomy):
            lm.push(x[:, a:b])
        caps.append(small.capacity)
        assert same_bits(small.read(), roomy.read()) and small.measured == roomy.measured
    small.flush(), roomy.flush()
    caps.append(small.capacity)
    assert caps == [64, 256, 256, 512] and roomy.capacity == 4096
    got = small.read()
    assert same_bits(got, roomy.read()) and bool(torch.isfinite(got).all())
    assert same_bits(got, m.measure_loudness_report(x, chans=[2], rate=rate)[0])


# ---- 5. delivery_stream(meter=True) -----------------------------------------------------------------------------------------------
FULL = dict(output_rate=16000, true_peak=-1.0, limiter="lookahead", pcm="int16", dither="tpdf")
CUTS48 = [1, 4801, 4802, 19000, 19000, 33333]


def through(ds, x, mid=None):
    """x [C, T] in the blocks of CUTS48 (and the rest), then flushed -> the blocks; mid(k): called behind push k."""
    outs, prev = [], 0
    for k, c in enumerate(CUTS48 + [x.shape[1]]):
        outs.append(ds.push(x[:, prev:c]))
        prev = c
        if mid is not None:
            mid(k)
    outs.append(ds.flush())
    return outs


@pytest.mark.parametrize("channels", [None, 2])
def test_a_metered_delivery_stream(channels):
    m = model()
    rows = channels or 1
    x = torch.from_numpy(stepped_noise(rows, 48000, seed=11 + rows) * np.float32(2.5)).cuda()          # (peaks over the ceiling)
    kw = dict(FULL, dither_seed=4)
    plain = through(m.delivery_stream(n_channels=channels, **kw), x)
    floats = through(m.delivery_stream(n_channels=channels, **{k: v for k, v in kw.items() if k not in ("pcm", "dither", "dither_seed")}), x)
    whole = torch.cat(floats, 1)
    assert whole.dtype == torch.float32 and whole.shape == (rows, 16000) and float(whole.abs().max()) < 0.9
    ds = m.delivery_stream(n_channels=channels, meter=True, **kw)
    mids = []
    metered = through(ds, x, lambda k: mids.append((ds.meter.measured, ds.loudness())))
    assert len(metered) == len(plain) and all(same_bits(a, b) for a, b in zip(metered, plain)) and metered[0].dtype == torch.int16
    got = ds.loudness()
    assert ds.meter.measured == 16000 and same_bits(got, m.measure_loudness_report(whole, chans=[rows], rate=16000)[0])
    assert close(got.cpu().numpy(), meter.report(whole.cpu().numpy(), 16000), channels) <= 1.0
    assert [n for n, _ in mids] == sorted(n for n, _ in mids) and 0 < mids[-1][0] < 16000 and mids[0][0] == 0
    for n, row in mids:                                  # mid-stream: the report of the floats delivered so far, in whole sub-blocks
        if n:
            assert same_bits(row, m.measure_loudness_report(whole[:, :n], chans=[rows], rate=16000)[0]), n
        else:
            assert tuple(row.tolist()) == NOTHING
    with pytest.raises(RuntimeError, match="no meter"):
        m.delivery_stream(n_channels=channels, **kw).loudness()


def test_a_stream_with_nothing_but_the_meter():
    m = model()
    x = torch.from_numpy(stepped_noise(1, 48000, seed=21)).cuda()
    ds = m.delivery_stream(meter=True)
    outs = through(ds, x)
    assert same_bits(torch.cat(outs, 1), x) and outs[-1].shape == (1, 0)
    assert same_bits(ds.loudness(), m.measure_loudness_report(x, rate=48000)[0])
    with pytest.raises(ValueError, match="nothing to deliver"):
        m.delivery_stream(meter=False)
    with pytest.raises(ValueError, match="meter must be a bool"):
        m.delivery_stream(meter="yes")
    with pytest.raises(ValueError, match="statistic of the whole stream"):
        m.delivery_stream(meter=True, loudness=-23.0)


# ---- 6. arguments -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_not_crashed():
    L = hip.lib()
    assert L.fh_sizeof_meter_state() == ctypes.sizeof(hip.MeterState) == 40
    assert L.fh_sizeof_meter_job() == ctypes.sizeof(hip.MeterJob) == 64
    p = 256                                              # a fake non-null pointer is enough for the argument checks
    report = lambda *a: L.fh_loudness_report_f32(*a, 0)                           # noqa: E731
    for args, word in (((0, 10, p, p, 1, 1, 16, p), "null"), ((p, 10, 0, p, 1, 1, 16, p), "null"), ((p, 10, p, 0, 1, 1, 16, p), "null"),
                       ((p, 10, p, p, 1, 1, 16, 0), "null"), ((p, (1 << 20) + 1, p, p, 1, 1, 16, p), "n_sub"),
                       ((p, 0, p, p, 1, 1, 16, p), "n_sub"), ((p, 10, p, p, 1, 1, 15, p), "hop"), ((p, 10, p, p, 1, 2, 16, p), "clips"),
                       ((p + 4, 10, p, p, 1, 1, 16, p), "aligned")):
        assert report(*args) == -1 and b"fh_loudness_report_f32" in L.fh_last_error() and word.encode() in L.fh_last_error(), args

    def job(**kw):
        j = dict(kept=p, fresh=p, keep=p, state=p, log=p, base=0, n_kept=0, n_fresh=100, log_len=64, ended=0)
        j.update(kw)
        return (hip.MeterJob * 1)(hip.MeterJob(*[j[name] for name, _ in hip.MeterJob._fields_]))

    def stream(jobs, dev=p, n=1, c=None, hop=16):
        return L.fh_stream_kweight_energy_f32(dev, 0 if jobs is None else ctypes.addressof(jobs), n, coef(8000) if c is None else c, hop, 0)

    good = job()
    for kw, word in ((dict(jobs=good, dev=0), "null"), (dict(jobs=None), "null"), (dict(jobs=good, n=0), "jobs"), (dict(jobs=good, hop=15), "hop"),
                     (dict(jobs=job(base=100)), "multiple of the span"), (dict(jobs=job(base=-SPAN)), "multiple of the span"),
                     (dict(jobs=job(n_kept=SPAN)), "n_kept"), (dict(jobs=job(n_fresh=-1)), "n_fresh"),
                     (dict(jobs=job(log_len=(1 << 20) + 1)), "log_len"), (dict(jobs=job(state=0)), "null"), (dict(jobs=job(log=0)), "null"),
                     (dict(jobs=job(fresh=0)), "null"), (dict(jobs=job(keep=0)), "null"), (dict(jobs=job(log=p + 4)), "aligned")):
        assert stream(**kw) == -1, (kw, word)
        assert b"fh_stream_kweight_energy_f32" in L.fh_last_error() and word.encode() in L.fh_last_error(), (word, L.fh_last_error())
    bad = (ctypes.c_double * 10)(*([1.0] * 9 + [math.inf]))
    assert stream(good, c=ctypes.addressof(bad)) == -1 and b"finite" in L.fh_last_error()


# ---- 7. a session whose delivery is metered -----------------------------------------------------------------------------------------
def test_a_session_with_a_metered_delivery():
    """stream(delivery=dict(meter=True)) and generate_long with it: the session's blocks are those of the plain session, the
    meter has read them."""
    m, sr, plan = model(), 12000, dict(window_ms=200, overlap_ms=60, guard_ms=10)
    x = synth.lowres_clip(400, 0.75, sr)
    plain = m.generate_long(x, sr, seed=5, **plan)
    s = m.stream(sr, seed=5, delivery=dict(meter=True), **plan)
    outs = [s.push(x[a:a + 2400]) for a in range(0, len(x), 2400)] + [s.flush()]
    assert same_bits(torch.cat(outs, 1), plain)
    got = s.delivery.loudness()
    assert s.delivery.meter.measured == plain.shape[1] and same_bits(got, m.measure_loudness_report(plain, rate=48000)[0])
    assert math.isfinite(float(got[0])) and float(got[2]) == -math.inf               # (0.75 s: no short-term window)
    assert same_bits(m.generate_long(x, sr, seed=5, delivery=dict(meter=True), **plan), plain)
