"""CPU: the loudness meter's definition (flowhigh_amd/meter.py) against the EBU's own test signals and by hand, the schedule of a
metered stream, and the refusals."""
import math

import numpy as np
import pytest

from flowhigh_amd import loudness, meter


def _tone(rate, parts, freq=1000.0, channels=2):
    """A stereo sine whose level steps through `parts` = [(dBFS, seconds)], the phase running through."""
    amp = np.concatenate([np.full(int(round(sec * rate)), 10.0 ** (db / 20.0)) for db, sec in parts])
    x = amp * np.sin(2.0 * np.pi * freq * np.arange(amp.size) / rate)
    return np.repeat(x[None], channels, 0).astype(np.float32)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_tech_3341_case_1(rate):
    """-23 dBFS for 20 s: I = M_max = S_max = -23 LUFS within the EBU's 0.1 LU."""
    I, M_max, S_max, LRA, M_last, S_last = meter.report(_tone(rate, [(-23.0, 20.0)]), rate)
    for v in (I, M_max, S_max, M_last, S_last):
        assert abs(v + 23.0) <= 0.1, v
    assert 0.0 <= LRA < 1e-9


@pytest.mark.parametrize("rate", [8000, 48000])
@pytest.mark.parametrize("parts, want", [([(-20.0, 20.0), (-30.0, 20.0)], 10.0), ([(-20.0, 20.0), (-15.0, 20.0)], 5.0),
                                         ([(-40.0, 20.0), (-20.0, 20.0)], 20.0),
                                         ([(-50.0, 20.0), (-35.0, 20.0), (-20.0, 20.0), (-35.0, 20.0), (-50.0, 20.0)], 15.0)],
                         ids=["3342-1", "3342-2", "3342-3", "3342-4"])
def test_tech_3342_cases(rate, parts, want):
    """The range of the EBU's four level-step signals within its 1 LU."""
    LRA = meter.report(_tone(rate, parts), rate)[3]
    assert abs(LRA - want) <= 1.0, LRA


def test_percentile_ranks_by_hand():
    # n - 1 = 0, 1, 10, 20, 100: 10 % and 95 % of that, rounded to the nearest rank (half up)
    assert meter.percentile_ranks(1) == (0, 0)
    assert meter.percentile_ranks(2) == (0, 1)            # 0.1 -> 0, 0.95 -> 1
    assert meter.percentile_ranks(11) == (1, 10)          # 1.0, 9.5 -> 10
    assert meter.percentile_ranks(21) == (2, 19)          # 2.0, 19.0
    assert meter.percentile_ranks(101) == (10, 95)
    assert meter.loudness_range(np.zeros(0)) == 0.0
    assert meter.loudness_range(np.full(7, loudness.ZA)) == 0.0            # (the absolute gate is strict: n = 0)
    # 101 windows 1, 2, .. 101 (all pass: the relative gate is at 0.51): lo = 11, hi = 96
    assert meter.loudness_range(np.arange(1.0, 102.0)[::-1]) == 10.0 * math.log10(96.0 / 11.0)
    # the relative gate takes the quiet half out: 10 windows at 1, 10 at 1e-3 -> mean 0.5005, gate 0.005005
    z = np.concatenate([np.full(10, 1e-3), np.linspace(1.0, 1.9, 10)])
    assert meter.range_gate(z).tolist() == [False] * 10 + [True] * 10
    assert meter.loudness_range(z) == 10.0 * math.log10(z[10 + 9] / z[10 + 1])        # ranks (1, 9) of 10


@pytest.mark.parametrize("K, ns", [(29, 0), (30, 1), (31, 2)])
def test_short_term_window_count(K, ns):
    rate, hop = 160, 16
    rng = np.random.default_rng(K)
    T = K * hop + 5                                       # (a partial sub-block behind them is in no window)
    e = rng.uniform(0.5, 1.5, (2, K + 1))
    zs = meter.short_term(e, T, rate)
    assert zs.shape == (ns,) and meter.n_short_term(T, hop) == ns
    s = e[0] + e[1]
    for j in range(ns):                                   # one addition at a time, in ascending order
        acc = s[j]
        for i in range(1, 30):
            acc = acc + s[j + i]
        assert zs[j] == acc / (30 * hop)
    rep = meter.report_from_energies(e, T, rate)
    if ns == 0:
        assert rep[2] == -math.inf and rep[5] == -math.inf and rep[3] == 0.0
    else:
        assert rep[2] == meter.lufs(zs).max() and rep[5] == meter.lufs(zs)[-1]


def test_short_clip_is_one_momentary_block():
    rate, hop = 160, 16
    x = np.random.default_rng(0).standard_normal((2, 3 * hop + 7)).astype(np.float32) * 0.1
    I, M_max, S_max, LRA, M_last, S_last = meter.report(x, rate)
    e = loudness.sub_energies(loudness.k_weight(x, rate), rate)
    assert meter.momentary(e, x.shape[1], rate).shape == (1,)
    want = -0.691 + 10.0 * math.log10(e.sum() / x.shape[1])
    assert I == M_max == M_last and abs(I - want) < 1e-12
    assert S_max == S_last == -math.inf and LRA == 0.0
    assert meter.report(np.zeros((1, 0), np.float32), rate) == (-math.inf, -math.inf, -math.inf, 0.0, -math.inf, -math.inf)
    silent = meter.report(np.zeros((1, 40 * hop), np.float32), rate)
    assert silent == (-math.inf, -math.inf, -math.inf, 0.0, -math.inf, -math.inf)


def test_measured_and_counters():
    assert [meter.measured(P, 16) for P in (0, 15, 16, 4096, 4100)] == [0, 0, 16, 4096, 4096]
    assert meter.measured(4096, 4800) == 0 and meter.measured(8192, 4800) == 4800
    c = meter.Counters(48000)
    assert c.step(4095) == dict(base=0, n_kept=0, n_fresh=4095, n_keep=4095, ended=False, log_need=0)
    assert c.step(2) == dict(base=0, n_kept=4095, n_fresh=2, n_keep=1, ended=False, log_need=1)
    assert (c.processed, c.kept, c.measured) == (4096, 1, 0)
    assert c.step(4096 * 2) == dict(base=4096, n_kept=1, n_fresh=8192, n_keep=1, ended=False, log_need=3)
    assert c.measured == 2 * 4800
    assert c.step(0, True) == dict(base=3 * 4096, n_kept=1, n_fresh=0, n_keep=0, ended=True, log_need=3)
    assert c.measured == 3 * 4096 + 1
    with pytest.raises(RuntimeError, match="closed"):
        c.step(1)
    # the log's bound: the push that would begin sub-block 2^20 + 1 is refused and leaves the counters as they were
    c = meter.Counters(160)
    c.step(meter.MAX_SUB * 16 - 10)
    before = (c.arrived, c.processed, c.ended)
    assert c.log_need(10) == meter.MAX_SUB
    with pytest.raises(RuntimeError, match="2\\^20"):
        c.step(4096 + 10)
    assert (c.arrived, c.processed, c.ended) == before


@pytest.mark.parametrize("channels", [None, 2])
def test_stream_meter_follows_the_schedule(channels):
    rate, hop = 165, 17                                   # (a low rate makes a long series of few samples; 165 is the lowest whose
    assert loudness.geometry(rate)[0] == hop              # re-designed shelf is stable: at 160 its poles lie at radius 1.06)
    lens = [1, 4095, 1, 4096, 8197, 0]
    T = sum(lens) + 3001
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((channels or 1, T)) * np.where(np.arange(T) < T // 2, 0.05, 0.4)).astype(np.float32)
    m = meter.StreamMeter(rate, channels)
    assert m.measured == 0 and m.read() == (-math.inf, -math.inf, -math.inf, 0.0, -math.inf, -math.inf)
    at = 0
    for n in lens + [T - sum(lens)]:
        m.push(x[:, at:at + n] if channels else x[0, at:at + n])
        at += n
        assert m.measured == meter.measured(at // 4096 * 4096, hop)
        assert m.read() == meter.report(x[:, :m.measured], rate)
    assert at == T and m.measured < T
    m.flush()
    assert m.measured == T and m.read() == meter.report(x, rate)
    assert m.read()[3] > 1.0                              # (the level step gives the range something to measure)


def test_refusals():
    for bad in (0, 9, 2.0, True, "2"):
        with pytest.raises(ValueError, match="n_channels"):
            meter.StreamMeter(48000, bad)
    with pytest.raises(ValueError, match="rate"):
        meter.StreamMeter(100)                            # (a sub-block shorter than the kernels' chunk)
    m = meter.StreamMeter(48000, 2)
    with pytest.raises(ValueError, match=r"\[2, n\]"):
        m.push(np.zeros((1, 10), np.float32))
    with pytest.raises(ValueError, match=r"\[2, n\]"):
        m.push(np.zeros(10, np.float32))
    with pytest.raises(ValueError, match="float32"):
        m.push(np.zeros((2, 10), np.float64))
    assert m.counters.arrived == 0                        # (a refused block moves nothing)
    m.push(np.zeros((2, 10), np.float32))
    m.flush()
    with pytest.raises(RuntimeError, match="closed"):
        m.push(np.zeros((2, 10), np.float32))
    with pytest.raises(RuntimeError, match="closed"):
        m.flush()


def test_meter_is_a_key_of_a_streams_delivery():
    from flowhigh_amd import delivery_stream as DS
    from flowhigh_amd import streaming
    assert DS.resolve({}) is None and DS.resolve(dict(meter=False)) is None
    assert DS.resolve(dict(meter=True)) == dict(rate=None, true_peak=None, pcm=None, key=None, meter=True)        # non-default by itself
    plan = DS.resolve(dict(meter=True, output_rate=16000, pcm="int16"), None, 2)
    assert plan["meter"] is True and plan["channels"] == 2 and plan["rate"] == 16000
    assert "meter" not in DS.resolve(dict(output_rate=16000))                     # (a plan without it is the plan it always was)
    with pytest.raises(ValueError, match="meter must be a bool"):
        DS.resolve(dict(meter="yes"))
    with pytest.raises(ValueError, match="two encoders"):
        DS.resolve(dict(meter=True), "int16")
    # the refusals stay, with a pointer to the meter
    with pytest.raises(ValueError, match="statistic of the whole stream.*meter=True"):
        DS.resolve(dict(meter=True, loudness=-23.0))
    with pytest.raises(ValueError, match="of a whole clip.*meter=True"):
        streaming.check_not_built(loudness=-23.0)
