"""GPU: true peak and the look-ahead limiter on the device -- fh_true_peak_* / fh_tp_envelope_* against flowhigh_amd/truepeak.py on
the same float32 input, fh_limit_* fed the definition's float32 envelope, fh_delivery_gain_f32 on planted values, and
generate*(true_peak=, limiter=) / measure_true_peak on TINY_CFG: clips of 0.33 to 0.7 s at 12 and 16 kHz.

Bars.  Envelope and true peak: 22 * 2^-24 * 2.2415 * peak per value (2.9e-6 of the row's or clip's peak) -- a chain of 21 float32 FMAs
and the rounding of the definition's float64 value, each at most 2^-24 of sum |h x| <= 2.2415 peak, the largest per-phase sum |h|.
Limiter: g within 1 float32 ulp of the definition (a float64 sum of 2 H + 1 terms in another order moves it by 1e-13 relative), y
within 2^-23 |x| (the ulp of g, and the product's own rounding), max |y| <= c32 exactly.  fh_delivery_gain_f32: 1 float32 ulp.
Where two runs of this project are compared the test is bitwise.  Output buffers are framed by sentinels that must keep their bits."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, loudness, synth, truepeak     # noqa: E402
from flowhigh_amd import frontend as FE                                          # noqa: E402

GUARD = 16
SENT32 = 0x7fc12345
U = 2.0 ** -24
TP_BAR = 22 * U * 2.2415
_STATE = {}
f32 = np.float32


def st():
    return hip.stream()


def tile():
    return hip.lib().fh_tp_tile_len()


def taps():
    if "taps" not in _STATE:
        from flowhigh_amd import tables
        _STATE["taps"] = tables.resample_poly_plan(4, 1)[0].cuda()
        assert _STATE["taps"].numel() == 82
    return _STATE["taps"].data_ptr()


def window(H):
    if ("w", H) not in _STATE:
        _STATE["w", H] = torch.from_numpy(truepeak.window(H)).cuda()
    return _STATE["w", H].data_ptr()


def put(x, lead):
    """x [rows, T] float32 on the device, its first float `lead` floats past a 16-byte boundary, NaN sentinels around it."""
    n = x.size
    buf = torch.full((8 + n + 8,), SENT32, dtype=torch.int32).view(torch.float32).cuda()
    assert buf.data_ptr() % 16 == 0
    xd = buf[4 + lead:4 + lead + n]
    xd.copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)))
    return buf, xd


def framed(n, lead=0):
    buf = torch.full((GUARD + lead + n + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD + lead:GUARD + lead + n]


def intact(buf, n, lead=0):
    return bool((buf[:GUARD + lead] == SENT32).all()) and bool((buf[GUARD + lead + n:] == SENT32).all())


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def planted_rows(rows, T, seed):
    """Noise at 0.1 with peaks of 0.9 (alternating sign) at the first sample, the last one and both sides of every tile boundary."""
    x = (torch.randn(rows, T, generator=torch.Generator().manual_seed(seed)) * 0.1).numpy()
    at = sorted({0, T - 1} | {n for k in range(1, T // tile() + 2) for n in (k * tile() - 1, k * tile()) if n < T})
    for i, n in enumerate(at):
        x[i % rows, n] = 0.9 * (-1) ** i
    return x


def lengths():
    t = tile()
    return [1, 19, 20, 21, t - 1, t, t + 1, 2 * t + 5]


# ---- the meter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
def test_true_peak_and_envelope_against_the_definition(rows):
    L = hip.lib()
    worst = 0.0
    for T in lengths():
        x = planted_rows(rows, T, seed=11 * T + rows)
        m_ref = truepeak.envelope(x).astype(np.float64)
        tp_ref = np.array([float(truepeak.true_peak(x[r])) for r in range(rows)])
        row_peak = np.abs(x).max(1).astype(np.float64)
        for lead in range(4):
            keep, xd = put(x, lead)
            pbuf, peak = framed(rows)
            peak.zero_()
            hip.check(L.fh_true_peak_f32(xd.data_ptr(), taps(), peak.data_ptr(), rows, T, st()), "fh_true_peak_f32")
            got = peak.view(torch.float32).cpu().numpy().astype(np.float64)
            ratio = float((np.abs(got - tp_ref) / (TP_BAR * row_peak)).max())
            assert intact(pbuf, rows) and ratio <= 1.0, (rows, T, lead, ratio)
            mbuf, m = framed(T, lead=(lead + 1) % 4)
            hip.check(L.fh_tp_envelope_f32(xd.data_ptr(), taps(), m.data_ptr(), 1, rows, T, st()), "fh_tp_envelope_f32")
            gm = m.view(torch.float32).cpu().numpy().astype(np.float64)
            ratio_m = float((np.abs(gm - m_ref) / (TP_BAR * row_peak.max())).max())
            assert intact(mbuf, T, (lead + 1) % 4) and ratio_m <= 1.0, (rows, T, lead, ratio_m)
            assert (gm >= np.abs(x).max(0)).all()                   # the |x[n]| term, exactly
            worst = max(worst, ratio, ratio_m)
            if lead == 0:
                first = (got, gm)
            else:                                                   # the values do not depend on the alignment
                assert np.array_equal(got, first[0]) and np.array_equal(gm, first[1]), (rows, T, lead)
    print(f"truepeak: true peak and envelope, {rows} rows: worst error / bar {worst:.3f}")


def test_a_silent_row_reads_zero_and_rows_are_independent():
    L = hip.lib()
    T = tile() + 7
    x = planted_rows(3, T, seed=5)
    x[1] = 0
    keep, xd = put(x, 1)
    peak = torch.zeros(3, dtype=torch.int32, device="cuda")
    hip.check(L.fh_true_peak_f32(xd.data_ptr(), taps(), peak.data_ptr(), 3, T, st()), "fh_true_peak_f32")
    got = peak.cpu()
    assert int(got[1]) == 0 and int(got[0]) > 0
    for r in (0, 2):
        keep1, x1 = put(x[r:r + 1], 3)
        one = torch.zeros(1, dtype=torch.int32, device="cuda")
        hip.check(L.fh_true_peak_f32(x1.data_ptr(), taps(), one.data_ptr(), 1, T, st()), "fh_true_peak_f32")
        assert int(one[0]) == int(got[r]), r


def test_the_segment_forms_give_every_clip_the_bits_of_the_batched_entries():
    """Clips of (C, T) = (1, tile - 1), (2, 2 tile + 5), (3, 21), (1, 1) in one launch, their rows at pitches of their own in wider
    buffers filled with NaN, at odd alignments: torch.equal to the batched entries on each clip alone."""
    L = hip.lib()
    t = tile()
    shapes = [(1, t - 1), (2, 2 * t + 5), (3, 21), (1, 1)]
    pitches = [t - 1, 2 * t + 8, 26, 3]
    xs = [planted_rows(c, T, seed=700 + T) for c, T in shapes]
    alone_tp, alone_m = [], []
    for x, (c, T) in zip(xs, shapes):
        keep, xd = put(x, 0)
        peak = torch.zeros(c, dtype=torch.int32, device="cuda")
        m = torch.empty(T, dtype=torch.float32, device="cuda")
        hip.check(L.fh_true_peak_f32(xd.data_ptr(), taps(), peak.data_ptr(), c, T, st()), "fh_true_peak_f32")
        hip.check(L.fh_tp_envelope_f32(xd.data_ptr(), taps(), m.data_ptr(), 1, c, T, st()), "fh_tp_envelope_f32")
        alone_tp.append(peak.clone())
        alone_m.append(m.clone())
    srcs = []
    for i, (x, (c, T), p) in enumerate(zip(xs, shapes, pitches)):
        wide = torch.full((c * p + 3,), float("nan"))
        v = wide[i % 4:i % 4 + c * p].view(c, p)
        v[:, :T] = torch.from_numpy(x)
        dev = wide.cuda()
        srcs.append((dev, dev.data_ptr() + 4 * (i % 4)))
    n, R, max_len = len(shapes), sum(c for c, _ in shapes), max(T for _, T in shapes)
    table = (hip.PcmClip * n)(*[hip.PcmClip(s[1], 0, p, c, T) for s, p, (c, T) in zip(srcs, pitches, shapes)])
    group = np.repeat(np.arange(n, dtype=np.int32), [c for c, _ in shapes])
    keep, (clips, grp) = FE.upload_tables([table, group], torch.device("cuda"))
    pbuf, peak = framed(R)
    peak.zero_()
    hip.check(L.fh_true_peak_seg_f32(clips, grp, n, R, max_len, taps(), peak.data_ptr(), st()), "fh_true_peak_seg_f32")
    mbuf, m = framed(n * max_len)
    hip.check(L.fh_tp_envelope_seg_f32(clips, n, max_len, taps(), m.data_ptr(), st()), "fh_tp_envelope_seg_f32")
    assert intact(pbuf, R) and intact(mbuf, n * max_len)
    assert torch.equal(peak, torch.cat(alone_tp))
    m = m.view(n, max_len)
    for i, (c, T) in enumerate(shapes):
        assert torch.equal(m[i, :T].view(torch.float32), alone_m[i]), (c, T)
        assert bool((m[i, T:] == SENT32).all()), (c, T)             # (a shorter clip's tail is not written)


# ---- the limiter ----------------------------------------------------------------------------------------------------------------
def limiter_case(C, T, H, seed):
    """Noise at 0.2 (under the -1 dBTP ceiling but for its crests) with spikes of 3 at 0, T - 1, 1023, 1024, 1024 +- H, 1024 +- 2 H."""
    x = (torch.randn(C, T, generator=torch.Generator().manual_seed(seed)) * 0.2).numpy()
    at = sorted({n for n in (0, T - 1, 1023, 1024, 1024 - H, 1024 + H, 1024 - 2 * H, 1024 + 2 * H) if 0 <= n < T})
    for i, n in enumerate(at):
        x[i % C, n] = 3.0 * (-1) ** i
    return x


@pytest.mark.parametrize("H", [40, 221, 240, 512])
def test_the_limiter_against_the_definition(H):
    L = hip.lib()
    db = -1.0
    c32 = float(f32(truepeak.ceiling(db)))
    worst_g, worst_y, cases = 0, 0.0, []
    for T in (1, H, 2 * H + 1, 1023, 1024, 1025, 1024 + 4 * H + 3):
        for C in (1, 2, 3):
            x = limiter_case(C, T, H, seed=H + 13 * T + C)
            m = truepeak.envelope(x)
            g_ref, r = truepeak.limiter_gain(m, H, db)
            y_ref = np.clip((x * g_ref[None]).astype(np.float32), -f32(c32), f32(c32))
            assert (g_ref <= r).all() and (g_ref < 1).any()
            lead = (T + C) % 4
            keep, xd = put(x, lead)
            md = torch.from_numpy(m).cuda()
            ybuf, y = framed(C * T, lead=(lead + 1) % 4)
            gbuf, g = framed(T)
            hip.check(L.fh_limit_f32(xd.data_ptr(), y.data_ptr(), md.data_ptr(), window(H), g.data_ptr(), 1, C, T, H, c32, st()),
                      "fh_limit_f32")
            assert intact(ybuf, C * T, (lead + 1) % 4) and intact(gbuf, T), (H, T, C)
            gg = g.view(torch.float32).cpu().numpy()
            gy = y.view(torch.float32).cpu().numpy().reshape(C, T)
            worst_g = max(worst_g, int(ulps(gg, g_ref).max()))
            assert ulps(gg, g_ref).max() <= 1, (H, T, C)
            err = np.abs(gy.astype(np.float64) - y_ref.astype(np.float64))
            assert (err <= 2.0 ** -23 * np.abs(x)).all(), (H, T, C, float(err.max()))
            worst_y = max(worst_y, float((err / np.maximum(2.0 ** -23 * np.abs(x), 1e-300)).max()))
            assert float(np.abs(gy).max()) <= c32, (H, T, C)
            assert (gg <= r).all()
            # in place: the same bits, nothing outside the rows
            hip.check(L.fh_limit_f32(xd.data_ptr(), xd.data_ptr(), md.data_ptr(), window(H), 0, 1, C, T, H, c32, st()), "fh_limit_f32")
            assert torch.equal(xd, y.view(torch.float32)), (H, T, C)
            assert bool((keep[:4 + lead].view(torch.int32) == SENT32).all()) and bool((keep[4 + lead + C * T:].view(torch.int32) == SENT32).all())
            cases.append((x, md, y.view(torch.float32).clone(), g.view(torch.float32).clone()))
    print(f"truepeak: limiter H {H}: worst gain error {worst_g} ulp, worst |y - definition| / bar {worst_y:.3f}")
    # the segment form over all of these clips in one launch: rows at pitches of their own, half of the clips in place
    n = len(cases)
    max_len = max(c[0].shape[1] for c in cases)
    m_all = torch.zeros(n, max_len, device="cuda")
    holders, rows_, dsts, table = [], [], [], []
    for i, (x, md, y, g) in enumerate(cases):
        C, T = x.shape
        p = T + (i % 3)
        wide = torch.full((C * p + 3,), float("nan"))
        wide[i % 4:i % 4 + C * p].view(C, p)[:, :T] = torch.from_numpy(x)
        dev = wide.cuda()
        holders.append(dev)
        src = dev.data_ptr() + 4 * (i % 4)
        m_all[i, :T] = md
        dbuf = None
        if i % 2:
            dbuf = framed(C * T, lead=i % 4)
        dsts.append(dbuf)
        rows_.append(dev[i % 4:i % 4 + C * p].view(C, p))
        table.append(hip.PcmClip(src, dbuf[1].data_ptr() if dbuf else 0, p, C, T))
    keep, (clips,) = FE.upload_tables([(hip.PcmClip * n)(*table)], torch.device("cuda"))
    gbuf, g_all = framed(n * max_len)
    hip.check(L.fh_limit_seg_f32(clips, n, max_len, m_all.data_ptr(), window(H), g_all.data_ptr(), H, c32, st()), "fh_limit_seg_f32")
    assert intact(gbuf, n * max_len)
    g_all = g_all.view(n, max_len)
    for i, (x, md, y, g) in enumerate(cases):
        C, T = x.shape
        assert torch.equal(g_all[i, :T].view(torch.float32), g), i
        if dsts[i]:
            assert intact(dsts[i][0], C * T, i % 4) and torch.equal(dsts[i][1].view(torch.float32), y), i
            assert np.array_equal(rows_[i][:, :T].cpu().numpy(), x), i                  # (the source is left as it was)
        else:
            assert torch.equal(rows_[i][:, :T].reshape(-1), y), i
            assert bool(torch.isnan(rows_[i][:, T:]).all()), i                         # (nothing behind a row's end)


def test_a_clip_under_the_ceiling_comes_back_bit_for_bit():
    L = hip.lib()
    T, H = 2 * tile() + 9, 240
    x = (torch.randn(2, T, generator=torch.Generator().manual_seed(2)) * 0.05).numpy()
    m = truepeak.envelope(x)
    assert float(m.max()) < truepeak.ceiling(-1.0)
    keep, xd = put(x, 2)
    before = xd.clone()
    g = torch.empty(T, device="cuda")
    hip.check(L.fh_limit_f32(xd.data_ptr(), xd.data_ptr(), torch.from_numpy(m).cuda().data_ptr(), window(H), g.data_ptr(), 1, 2, T, H,
                             float(f32(truepeak.ceiling(-1.0))), st()), "fh_limit_f32")
    assert torch.equal(xd, before) and bool((g == 1).all())


# ---- the gain -------------------------------------------------------------------------------------------------------------------
def test_the_delivery_gain_kernel_on_planted_values():
    """Clips of 1, 2, 3 and 2 rows: a plain one, one whose cap binds, one whose largest true peak is in its last row, a silent one."""
    L = hip.lib()
    chans = [1, 2, 3, 2]
    lufs = f32([-20.5, -30.25, -12.125, -math.inf])
    peak = f32([0.5, 0.9, 0.2, 0.7, 0.3, 0.99, 0.0, 0.0])
    tp = f32([0.55, 0.95, 0.25, 0.72, 0.35, 1.07, 0.0, 0.0])
    group = np.repeat(np.arange(4, dtype=np.int32), chans)
    R, n = 8, 4
    dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.float32 else a).cuda()      # noqa: E731
    ld, pd, td, gd = dev(lufs), dev(peak), dev(tp), dev(group)
    starts = np.cumsum([0] + chans[:-1])
    c = truepeak.ceiling(-1.0)
    for target, uncapped, with_tp in ((math.nan, 0, True), (-16.0, 0, True), (-16.0, 0, False), (-16.0, 1, False), (math.nan, 1, False)):
        gbuf, g = framed(R)
        dbuf, d = framed(n)
        hip.check(L.fh_delivery_gain_f32(ld.data_ptr(), target, pd.data_ptr(), td.data_ptr() if with_tp else 0, gd.data_ptr(), R, n, c,
                                         uncapped, g.data_ptr(), d.data_ptr() if with_tp else 0, st()), "fh_delivery_gain_f32")
        assert intact(gbuf, R) and intact(dbuf, n)
        got = g.view(torch.float32).cpu().numpy()
        for i, (s, ch) in enumerate(zip(starts, chans)):
            pk, TP = float(peak[s:s + ch].max()), float(tp[s:s + ch].max())
            t = None if math.isnan(target) else target
            if uncapped:
                want = truepeak.uncapped_gain(lufs[i], t)
            else:
                g_l = f32(1.0) if t is None else loudness.gain(lufs[i], t, pk)
                want = truepeak.static_gain(TP, -1.0, g_l) if with_tp else g_l
            for r in range(s, s + ch):
                assert ulps(got[r], want) <= 1, (target, uncapped, with_tp, i, r, float(got[r]), float(want))
            if with_tp:
                db = float(d.view(torch.float32)[i])
                assert db == -math.inf if TP == 0 else abs(db - float(truepeak.dbtp(TP))) <= 1e-5, (i, db)
    # what the planted values exercise, from the definition: the cap binds in clip 1, the ceiling in clips 1 and 2 (its last row), not 0
    assert loudness.gain(lufs[1], -16.0, 0.9) == f32(0.99 / float(f32(0.9))) and truepeak.static_gain(0.55, -1.0) == 1
    assert truepeak.static_gain(1.07, -1.0) < 1 and tp[3:6].argmax() == 2 and truepeak.static_gain(0.0, -1.0) == 1


# ---- the model ------------------------------------------------------------------------------------------------------------------
def model(prior="reference"):
    if "fh" not in _STATE:
        _STATE["fh"] = FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda")
    if prior not in _STATE:
        _STATE[prior] = FlowHighSR(_STATE["fh"], torchdiffeq_ode_method="euler", upsampling_method="hip", prior=prior)
    return _STATE[prior]


CLIPS = dict(M=(1, 3960, 12000, 33), S=(2, 3960, 12000, 33), L=(1, 4800, 12000, 40), W=(1, 5400, 16000, 33), X=(2, 8400, 12000, 70))


def clip(name):
    """'M': mono, 3960 samples at 12 kHz (0.33 s, 33 frames); 'S': stereo of that length; 'L': mono, 0.4 s; 'W': mono, 5400 samples
    at 16 kHz (0.34 s); 'X': stereo, 8400 samples at 12 kHz (0.7 s).  -> ([C, T] array, its rate)"""
    chans, n, sr, _ = CLIPS[name]
    scale = (1.0, 0.45)
    x = np.stack([synth.lowres_clip(900 + ord(name) + c, n / sr, sr)[:n] * np.float32(scale[c]) for c in range(chans)])
    assert x.shape == (chans, n) and np.abs(x).max() <= 1
    return x, sr


def noise(name):
    return synth.prior_noise(800 + ord(name), CLIPS[name][3])


def run(name, **kw):
    x, sr = clip(name)
    return model().generate(x, sr, noise=noise(name), channels="first", **kw)


def run48(name):
    if ("y48", name) not in _STATE:
        _STATE["y48", name] = run(name).clone()
    return _STATE["y48", name]


def y_bar(peak, limiter, extra=0.0):
    """|device - definition| per sample as a fraction of the |x| the gain multiplies, x of sample peak `peak`, ceiling -1 dBTP.
    Static rule: the true peak is within TP_BAR peak <= TP_BAR TP, so is the gain; its rounding and the product's on either side:
    2^-22.  Limiter: m is within TP_BAR peak, so r = c / m (m > c) within c TP_BAR peak / m^2 <= TP_BAR peak / c, q and g (a
    weighted mean of q) with it.  extra: what x itself differs by, relative (it reaches y through x and through g)."""
    c = truepeak.ceiling(-1.0)
    return TP_BAR * (max(1.0, peak / c) if limiter else 1.0) + 2.0 ** -22 + 2 * extra


def test_true_peak_none_is_the_call_without_the_keyword():
    m = model()
    (M, _), (L_, _) = clip("M"), clip("L")
    assert torch.equal(run("S", true_peak=None, limiter=None), run48("S"))
    assert torch.equal(m.generate(M[0], 12000, noise=noise("M"), true_peak=None), m.generate(M[0], 12000, noise=noise("M")))
    kw = dict(noise=[noise("M"), noise("L")], ends="ragged", output_rate=44100, pcm="int16")
    a, b = m.generate_many([M[0], L_[0]], 12000, true_peak=None, **kw), m.generate_many([M[0], L_[0]], 12000, **kw)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("name", ["M", "S", "X"])
def test_true_peak_is_the_definition_on_the_48k_result(name):
    """generate(true_peak=-1) and generate(true_peak=-1, limiter='lookahead') against truepeak.deliver on the same call's result
    without the keyword; measure_true_peak against the definition, and of both results at or under -1 dBTP + 0.01 dB."""
    y48 = run48(name)
    host = y48.cpu().numpy()
    C = host.shape[0]
    tp_dev = model().measure_true_peak(y48, chans=[C])
    assert tp_dev.dtype == torch.float32 and tp_dev.is_cuda and tuple(tp_dev.shape) == (1,)
    tp_def = float(truepeak.true_peak(host))
    assert abs(10.0 ** (float(tp_dev[0]) / 20.0) - tp_def) <= (TP_BAR + U) * float(np.abs(host).max())
    assert tp_def > truepeak.ceiling(-1.0)                          # (the 0.99 sample peak: both rules have something to do)
    for limiter in (None, "lookahead"):
        got = run(name, true_peak=-1.0, limiter=limiter)
        want = truepeak.deliver(host, 48000, -1.0, limiter=limiter)
        assert got.dtype == torch.float32 and got.shape == y48.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        bar = y_bar(float(np.abs(host).max()), limiter) * np.abs(host)
        ratio = float((err / np.maximum(bar, 1e-300)).max())
        back = float(model().measure_true_peak(got, chans=[C])[0])
        print(f"truepeak: clip {name} limiter {limiter}: worst |device - definition| / bar {ratio:.3f}; delivered {back:+.4f} dBTP "
              f"(definition {float(truepeak.dbtp(truepeak.true_peak(got.cpu().numpy()))):+.4f}) from {float(tp_dev[0]):+.4f}")
        assert (err <= bar).all(), (name, limiter, ratio)
        assert back <= -1.0 + 0.01
        if limiter is not None:
            assert float(got.abs().max()) <= float(f32(truepeak.ceiling(-1.0)))
            assert not torch.equal(got, run(name, true_peak=-1.0))
    # a list of clips goes through the segment form
    listed = model().measure_true_peak([y48, y48[:1, :5000]])
    assert float(listed[0]) == float(tp_dev[0])
    assert abs(10.0 ** (float(listed[1]) / 20.0) - float(truepeak.true_peak(host[:1, :5000]))) <= (TP_BAR + U) * float(np.abs(host).max())


def test_measure_true_peak_shapes_and_errors():
    m = model()
    x = (torch.randn(3, 3001, generator=torch.Generator().manual_seed(1)) * 0.2)
    x[2] = 0
    xd = x.cuda()
    got = m.measure_true_peak(xd, chans=[2, 1], rate=44100).cpu().numpy()
    assert abs(10.0 ** (got[0] / 20.0) - float(truepeak.true_peak(x[:2].numpy()))) <= (TP_BAR + U) * float(x.abs().max())
    assert got[1] == -math.inf and tuple(m.measure_true_peak(xd).shape) == (3,)
    for bad in (dict(rate=0), dict(rate=44100.5), dict(chans=[2, 2])):
        with pytest.raises(ValueError):
            m.measure_true_peak(xd, **bad)
    with pytest.raises(ValueError):
        m.measure_true_peak([xd], chans=[3])
    with pytest.raises(ValueError):
        m.measure_true_peak(xd.double())


def peaky_clip():
    """A mono 12 kHz clip and an output rate at which the cap of loudness=-16 binds by 3 dB or more, chosen on the CPU from the
    model's own delivered result: a quiet floor with three clicks, the quietest floor first.  The vocoder of TINY_CFG fills the band
    above the input's with dense noise whatever the input (crest 13 dB: -16.5 LUFS at 48 kHz, the cap does not bind), so the clip is
    delivered at 8 or 16 kHz, where the input's own band is what is left.
    -> (clip [1, T], noise, rate, y [1, T_rate] on the device, L, peak)"""
    if "peaky" not in _STATE:
        n, frames = 8400, 70
        for rate in (8000, 16000, 48000):
            for floor in (0.003, 0.01, 0.03):
                rng = np.random.default_rng(17)
                x = (rng.standard_normal(n) * floor).astype(np.float32)
                x[[1500, 4100, 6900]] = [0.9, -0.8, 0.85]
                z = synth.prior_noise(4242, frames)
                y = model().generate(x[None], 12000, noise=z, channels="first", output_rate=rate).clone()
                host = y.cpu().numpy()
                L, peak = loudness.integrated(host, rate), float(np.abs(host).max())
                print(f"truepeak: peaky candidate floor {floor} at {rate} Hz: {L:.2f} LUFS at peak {peak:.3f}")
                if "peaky" not in _STATE and math.isfinite(L) and 10.0 ** ((-16.0 - L) / 20.0) >= 10.0 ** (3.0 / 20.0) * 0.99 / peak:
                    _STATE["peaky"] = (x[None], z, rate, y, L, peak)
            if "peaky" in _STATE:
                break
        assert "peaky" in _STATE, "no candidate clip on which the cap of loudness=-16 binds by 3 dB"
    return _STATE["peaky"]


def test_the_limiter_lifts_the_cap_of_loudness():
    x, z, rate, y, L, peak = peaky_clip()
    m = model()
    kw = dict(noise=z, channels="first", output_rate=rate)
    capped = m.generate(x, 12000, loudness=-16.0, **kw)
    got = m.generate(x, 12000, loudness=-16.0, true_peak=-1.0, limiter="lookahead", **kw)
    l_capped, l_got = (float(m.measure_loudness(t, chans=[1], rate=rate)[0]) for t in (capped, got))
    tp = float(m.measure_true_peak(got, chans=[1], rate=rate)[0])
    print(f"truepeak: loudness=-16 on the peaky clip ({L:.2f} LUFS at {rate} Hz): capped {l_capped:.3f} LUFS, with the limiter "
          f"{l_got:.3f} LUFS at {tp:+.4f} dBTP")
    assert l_capped <= -16.0 - 3.0 + 1e-3
    assert abs(l_got + 16.0) < abs(l_capped + 16.0) and l_got <= -16.0 + 1e-3
    assert tp <= -1.0 + 0.01 and float(got.abs().max()) <= float(f32(truepeak.ceiling(-1.0)))
    host = y.cpu().numpy()
    want = truepeak.deliver(host, rate, -1.0, limiter="lookahead", loudness=-16.0)
    g_u = float(truepeak.uncapped_gain(L, -16.0))
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    # (the uncapped gain is made from the device's float32 loudness, within 1e-5 LU of the definition's: 1.2e-6 relative, and rounded)
    bar = y_bar(g_u * peak, "lookahead", extra=1.2e-6 + U) * g_u * np.abs(host)
    print(f"truepeak: peaky clip, loudness and limiter: worst |device - definition| / bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
    assert (err <= bar).all()
    # the static rule with loudness=: the capped gain, then the ceiling
    static = m.generate(x, 12000, loudness=-16.0, true_peak=-1.0, **kw)
    assert float(m.measure_true_peak(static, chans=[1], rate=rate)[0]) <= -1.0 + 0.01
    assert float(m.measure_loudness(static, chans=[1], rate=rate)[0]) < l_capped


@pytest.mark.parametrize("deliver", [dict(true_peak=-1.0), dict(true_peak=-1.0, limiter="lookahead"),
                                     dict(true_peak=-1.0, limiter="lookahead", loudness=-12.0, output_rate=44100, pcm="int16"),
                                     dict(true_peak=-2.0, loudness=-12.0, output_rate=44100, pcm="int16", interleaved=True)])
def test_a_clip_gets_the_same_bits_alone_in_a_batch_and_in_a_ragged_group(deliver):
    """The stereo clip S alone = beside a second clip of its length in generate_batch = beside clips of other lengths and another
    input rate in generate_many under both `ends` and without the ragged sequence (one bucket per shape)."""
    m = model()
    (S, _), (M, _), (L_, _), (W, _) = clip("S"), clip("M"), clip("L"), clip("W")
    S2 = S[::-1] * np.float32(0.5)
    kw = dict(channels="first", **deliver)
    alone = m.generate(S, 12000, noise=noise("S"), **kw)
    batch = m.generate_batch([S, S2], 12000, noise=[noise("S"), noise("S")], **kw)
    assert torch.equal(batch[0], alone) and batch[1].shape == alone.shape and batch[1].dtype == alone.dtype
    both = m.generate_batch([S, M], 12000, noise=[noise("S"), noise("M")], **kw)          # (2 and 1 channels: the segment forms)
    assert torch.equal(both[0], alone)
    mono = m.generate(M, 12000, noise=noise("M"), **kw)
    wide = m.generate(W, 16000, noise=noise("W"), **kw)
    assert torch.equal(both[1], mono)
    for how in (dict(ends="per_clip"), dict(ends="ragged"), dict(ragged=False)):
        outs = m.generate_many([S, L_, M, W], [12000, 12000, 12000, 16000], noise=[noise(n) for n in "SLMW"], **how, **kw)
        assert torch.equal(outs[0], alone), how
        assert torch.equal(outs[2], mono), how
        assert torch.equal(outs[3], wide), how
    assert alone.any() and mono.any() and wide.any()
    assert alone.dtype == (torch.int16 if deliver.get("pcm") else torch.float32)


def test_mono_clips_without_channels_and_both_ends():
    m = model()
    M, L_ = clip("M")[0][0], clip("L")[0][0]
    kw = dict(true_peak=-1.0, limiter="lookahead")
    a = m.generate(M, 12000, noise=noise("M"), **kw)
    b = m.generate(L_, 12000, noise=noise("L"), **kw)
    assert a.shape == (1, 15840) and b.shape == (1, 19200) and a.dtype == torch.float32
    for ends in ("per_clip", "ragged"):
        outs = m.generate_many([M, L_], 12000, noise=[noise("M"), noise("L")], ends=ends, **kw)
        assert torch.equal(outs[0], a) and torch.equal(outs[1], b), ends
    two = m.generate_batch([M, M * np.float32(0.5)], 12000, noise=torch.cat([noise("M"), noise("M")]), **kw)
    assert two.shape == (2, 15840) and torch.equal(two[:1], a)
    # level='input' goes with true_peak=: the rule only attenuates
    c = m.generate(M, 12000, noise=noise("M"), level="input", true_peak=-6.0)
    assert float(m.measure_true_peak(c)[0]) <= -6.0 + 0.01


def test_a_true_peak_call_scales_no_buffer_the_next_call_reads():
    """The post-processor's rows are plan-owned: after a true_peak= call the same call without the keyword gives what it gave
    before, alone, in a batch and in a ragged group."""
    m = model()
    (S, _), (M, _), (L_, _) = clip("S"), clip("M"), clip("L")
    before = run48("S").clone()
    for kw in (dict(true_peak=-6.0), dict(true_peak=-6.0, limiter="lookahead")):
        got = run("S", **kw)
        assert torch.equal(run("S"), before) and not torch.equal(got, before)
        assert torch.equal(got, run("S", **kw))
        for ends in ("per_clip", "ragged"):
            mk = dict(noise=[noise("M"), noise("L")], ends=ends)
            ref = [y.clone() for y in m.generate_many([M[0], L_[0]], 12000, **mk)]
            m.generate_many([M[0], L_[0]], 12000, **kw, **mk)
            again = m.generate_many([M[0], L_[0]], 12000, **mk)
            assert all(torch.equal(p, q) for p, q in zip(ref, again)), ends
        two = torch.cat([noise("M"), noise("M")])
        ref = m.generate_batch([M[0], M[0]], 12000, noise=two).clone()
        m.generate_batch([M[0], M[0]], 12000, noise=two, **kw)
        assert torch.equal(m.generate_batch([M[0], M[0]], 12000, noise=two), ref)
