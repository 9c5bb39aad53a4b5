"""GPU: loudness on the device -- fh_kweight_energy_f32 / fh_kweight_energy_seg_f32 against flowhigh_amd/loudness.py on the
float64 lfilter of the same float32 input, fh_loudness_gate_f32 on planted double energies against the definition's gate and
gain, and generate*(loudness=) / measure_loudness on TINY_CFG: clips of 0.33 to 0.7 s at 12 and 16 kHz.

Bars.  Energies: 1e-9 relative per sub-block -- two float64 orderings of this filter differ by 1.4e-12, the high-pass's all-pole
noise gain is 2.0e6 in power, so double rounding through it is about 2e-13; a wrong hand-over state or coefficient costs at least
1e-3.  lufs: 1e-5 LU -- a float32 below 64 in magnitude rounds by at most 3.8e-6, the double arithmetic error is negligible.
gains: 1 float32 ulp of loudness.gain.  Where two runs of this project are compared the test is bitwise.  Output buffers are
framed by sentinels that must keep their bits."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, loudness, pcm, synth     # noqa: E402
from flowhigh_amd import frontend as FE                                     # noqa: E402

GUARD = 16
SENT64 = 0x7ff8_0000_5A17_5A17            # a NaN no kernel writes: an element that was written loses these bits
SENT32 = 0x7fc12345
RATES = [8000, 11025, 44100, 48000]
_STATE = {}


def st():
    return hip.stream()


def span():
    return hip.lib().fh_loudness_span_len()


def coef(rate):
    import ctypes
    key = ("coef", rate)
    if key not in _STATE:
        _STATE[key] = (ctypes.c_double * 10)(*loudness.coefficients(rate))
    return ctypes.addressof(_STATE[key])


def noise_rows(rows, T, seed):
    return (torch.randn(rows, T, generator=torch.Generator().manual_seed(seed)) * 0.3).numpy()


def framed64(n):
    buf = torch.full((GUARD + n + GUARD,), SENT64, dtype=torch.int64, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float64)


def intact64(buf, n):
    return bool((buf[:GUARD] == SENT64).all()) and bool((buf[GUARD + n:] == SENT64).all())


def put(x, lead):
    """x [rows, T] float32 on the device, its first float `lead` floats past a 16-byte boundary, NaN around it."""
    n = x.size
    buf = torch.full((8 + n + 8,), SENT32, dtype=torch.int32).view(torch.float32).cuda()
    assert buf.data_ptr() % 16 == 0
    xd = buf[4 + lead:4 + lead + n]
    xd.copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)))
    return buf, xd


def energies(x, rate, lead=0):
    """fh_kweight_energy_f32 on x [rows, T] -> (float64 [rows, n_sub] on the host, sentinels intact)."""
    rows, T = x.shape
    hop, _ = loudness.geometry(rate)
    n_sub = -(-T // hop)
    keep, xd = put(x, lead)
    buf, e = framed64(rows * n_sub)
    hip.check(hip.lib().fh_kweight_energy_f32(xd.data_ptr(), coef(rate), e.data_ptr(), rows, T, hop, st()), "fh_kweight_energy_f32")
    return e.cpu().view(rows, n_sub).numpy().copy(), intact64(buf, rows * n_sub)


def lengths(rate):
    hop, block = loudness.geometry(rate)
    S = span()
    return [1, hop - 1, hop, block - 1, block, block + hop - 1, block + hop, S - 1, S, S + 1, 2 * S + 1]


# ---- the energies ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("rate", RATES)
def test_sub_block_energies_against_the_float64_definition(rate, rows):
    """Every length either side of a sub-block, of a block and of a span, the input on the 16-byte grid and one float past it:
    1e-9 relative per sub-block of loudness.sub_energies on the float64 lfilter of the same float32 input."""
    worst = 0.0
    for T in lengths(rate):
        x = noise_rows(rows, T, seed=rate + 7 * T + rows)
        ref = loudness.sub_energies(loudness.k_weight(x, rate), rate)
        assert ref.shape == (rows, -(-T // loudness.geometry(rate)[0])) and (ref > 0).all()
        for lead in (0, 1):
            got, intact = energies(x, rate, lead)
            ratio = float((np.abs(got - ref) / ref).max()) / 1e-9
            worst = max(worst, ratio)
            assert intact and np.isfinite(got).all() and ratio <= 1.0, (rate, rows, T, lead, ratio)
    print(f"loudness: energies rate {rate} rows {rows}: worst error / bar {worst:.2e}")


def test_sub_block_energies_of_a_low_frequency_heavy_row():
    """A 20 Hz tone at 0.5 plus 1e-3 noise, 1 s at 48 kHz: the input on which a float32 recursion loses 5e-4 of a sub-block."""
    T, rate = 48000, 48000
    x = (0.5 * np.sin(2 * np.pi * 20.0 * np.arange(T) / rate) + 1e-3 * noise_rows(1, T, 20)[0] / 0.3).astype(np.float32)[None]
    ref = loudness.sub_energies(loudness.k_weight(x, rate), rate)
    got, intact = energies(x, rate)
    ratio = float((np.abs(got - ref) / ref).max()) / 1e-9
    print(f"loudness: energies of the 20 Hz row: worst error / bar {ratio:.2e}")
    assert intact and ratio <= 1.0


def test_a_row_s_energies_depend_on_the_row_alone():
    """Row r of a 3-row launch = the 1-row launch, bit for bit; the first k sub-blocks of a longer row = those of its prefix of
    k hop samples (the spans are counted from the row's sample 0, and what follows a sub-block adds exact zeros to it)."""
    rate = 44100
    hop, block = loudness.geometry(rate)
    T = 2 * span() + 1
    x = noise_rows(3, T, seed=99)
    three, _ = energies(x, rate)
    for r in range(3):
        one, _ = energies(x[r:r + 1], rate, lead=r % 2)
        assert np.array_equal(one[0], three[r]), r
    T = block + hop + 17
    x = noise_rows(1, T, seed=98)
    whole, _ = energies(x, rate)
    for k in (1, 2, 4, 5):
        part, _ = energies(x[:, :k * hop], rate)
        assert part.shape == (1, k) and np.array_equal(part[0], whole[0, :k]), k
    assert whole.shape == (1, 6)


def test_the_segment_form_gives_every_clip_the_bits_of_the_batched_entry():
    """Clips of (C, T) = (1, block - 1), (2, SPAN + 1), (3, hop) in one launch, their rows at pitches of their own in wider
    buffers filled with NaN: every row torch.equal to fh_kweight_energy_f32 on that clip alone."""
    L = hip.lib()
    rate = 8000
    hop, block = loudness.geometry(rate)
    shapes = [(1, block - 1), (2, span() + 1), (3, hop)]
    pitches = [block - 1, span() + 14, hop + 3]
    xs = [noise_rows(c, t, seed=300 + t) for c, t in shapes]
    alone = [energies(x, rate)[0] for x in xs]
    srcs = []
    for x, (c, t), p in zip(xs, shapes, pitches):
        wide = torch.full((c, p), float("nan"))
        wide[:, :t] = torch.from_numpy(x)
        srcs.append(wide.cuda())
    table = (hip.PcmClip * 3)(*[hip.PcmClip(s.data_ptr(), 0, p, c, t) for s, p, (c, t) in zip(srcs, pitches, shapes)])
    group = np.repeat(np.arange(3, dtype=np.int32), [c for c, _ in shapes])
    keep, (clips, grp) = FE.upload_tables([table, group], torch.device("cuda"))
    max_len = max(t for _, t in shapes)
    n_sub = -(-max_len // hop)
    buf, e = framed64(6 * n_sub)
    hip.check(L.fh_kweight_energy_seg_f32(clips, grp, 3, 6, max_len, coef(rate), e.data_ptr(), hop, st()), "fh_kweight_energy_seg_f32")
    got = e.cpu().view(torch.int64).view(6, n_sub)
    r = 0
    for a, (c, t) in zip(alone, shapes):
        k = -(-t // hop)
        for ch in range(c):
            assert np.array_equal(got[r, :k].view(torch.float64).numpy(), a[ch]), (c, t, ch)
            assert bool((got[r, k:] == SENT64).all()), (c, t, ch)          # (a shorter row's tail is not written)
            r += 1
    assert intact64(buf, 6 * n_sub)


# ---- the gate -------------------------------------------------------------------------------------------------------------------
def tie_energy(block):
    """A sub-block energy E with E / block == ZA exactly, and the next double above it."""
    E = loudness.ZA * block
    for _ in range(8):
        if E / block == loudness.ZA:
            break
        E = np.nextafter(E, math.inf if E / block < loudness.ZA else -math.inf)
    assert E / block == loudness.ZA
    up = E
    while up / block <= loudness.ZA:
        up = np.nextafter(up, math.inf)
    return float(E), float(up)


def planted_clips():
    """(name, e [C, n_sub], T, peaks [C]) at 48 kHz: groups of 1, 2 and 3 rows, a clip shorter than a block, clips the absolute and
    the relative gate take blocks from, an all-silent clip, a block exactly at ZA and one a double above it, a loud peak (the cap)."""
    rate = 48000
    hop, block = loudness.geometry(rate)
    rng = np.random.default_rng(5)
    clips = []
    for name, C, T in (("one", 1, 3 * rate), ("two", 2, 2 * rate + 17), ("three", 3, block + hop + 5), ("short", 2, block - 1)):
        clips.append((name, rng.uniform(20.0, 60.0, (C, -(-T // hop))), T, rng.uniform(0.2, 0.6, C).astype(np.float32)))
    e = rng.uniform(20.0, 60.0, (2, 30))
    e[:, 8:20] = rng.uniform(1e-7, 2e-5, (2, 12))                       # blocks around ZA * block = 2.25e-3: the absolute gate decides
    clips.append(("absolute", e, 30 * hop, np.float32([0.5, 0.1])))
    x = np.concatenate([noise_rows(1, rate, 61)[0], noise_rows(1, rate, 62)[0] * 0.01, np.zeros(rate, dtype=np.float32)])[None]
    clips.append(("relative", loudness.sub_energies(loudness.k_weight(x, rate), rate), 3 * rate, np.float32([np.abs(x).max()])))
    clips.append(("silent", np.zeros((2, 12)), 12 * hop, np.float32([0.0, 0.0])))
    E, up = tie_energy(block)
    clips.append(("tie", np.array([[E, 0, 0, 0, 0, 0.0]]), 6 * hop, np.float32([0.3])))
    clips.append(("above", np.array([[up, 0, 0, 0, 0, 0.0]]), 6 * hop, np.float32([1e-4])))
    clips.append(("cap", rng.uniform(0.5, 1.0, (1, 20)), 20 * hop, np.float32([0.9])))
    return rate, clips


def run_gate(rate, clips, target):
    hop, _ = loudness.geometry(rate)
    rows = sum(e.shape[0] for _, e, _, _ in clips)
    n_sub = max(e.shape[1] for _, e, _, _ in clips)
    host = np.full((rows, n_sub), np.nan)
    lens, group, peaks, r = [], [], [], 0
    for i, (_, e, T, pk) in enumerate(clips):
        host[r:r + e.shape[0], :e.shape[1]] = e
        r += e.shape[0]
        lens += [T] * e.shape[0]
        group += [i] * e.shape[0]
        peaks += list(pk)
    ed = torch.from_numpy(host).cuda()
    ld, gd = torch.tensor(lens, dtype=torch.int32).cuda(), torch.tensor(group, dtype=torch.int32).cuda()
    pd = torch.from_numpy(np.float32(peaks).view(np.int32)).cuda()
    lufs = torch.full((GUARD + len(clips) + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    gains = torch.full((GUARD + rows + GUARD,), SENT32, dtype=torch.int32, device="cuda")
    hip.check(hip.lib().fh_loudness_gate_f32(ed.data_ptr(), n_sub, ld.data_ptr(), gd.data_ptr(), rows, len(clips), hop, target,
                                             pd.data_ptr(), lufs[GUARD:].data_ptr(), gains[GUARD:].data_ptr(), st()),
              "fh_loudness_gate_f32")
    for buf, n in ((lufs, len(clips)), (gains, rows)):
        assert bool((buf[:GUARD] == SENT32).all()) and bool((buf[GUARD + n:] == SENT32).all())
    return (lufs[GUARD:GUARD + len(clips)].view(torch.float32).cpu().numpy(), gains[GUARD:GUARD + rows].view(torch.float32).cpu().numpy())


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_the_gate_kernel_against_the_definition_on_planted_energies():
    rate, clips = planted_clips()
    seen = {}
    for name, e, T, pk in clips:
        # from the definition alone: no planted block within 1e-6 relative of the relative threshold (ties are planted against
        # ZA only, which is a constant)
        z = loudness.block_energies(e, T, rate)
        absolute = z > loudness.ZA
        if absolute.any():
            thr = loudness.REL_GATE * z[absolute].mean()
            assert (np.abs(z - thr) > 1e-6 * thr).all(), name
        L, both = loudness.gate(z)
        seen[name] = (len(z), int((~absolute).sum()), int((absolute & ~both).sum()), L)
    assert seen["short"][0] == 1 and seen["three"][0] == 2
    assert seen["absolute"][1] >= 5 and seen["relative"][:3] == (27, 7, 10) and abs(seen["relative"][3] + 8.01) < 0.05
    assert seen["silent"][3] == -math.inf and seen["tie"][3] == -math.inf and abs(seen["above"][3] + 70.0) < 1e-9
    for target in (-23.0, 0.0, math.nan):
        lufs, gains = run_gate(rate, clips, target)
        r, worst = 0, 0.0
        for i, (name, e, T, pk) in enumerate(clips):
            L = seen[name][3]
            if math.isinf(L):
                assert lufs[i] == -math.inf, name
            else:
                worst = max(worst, abs(float(lufs[i]) - L))
                assert abs(float(lufs[i]) - L) <= 1e-5, (name, float(lufs[i]), L)
            want = np.float32(1.0) if math.isnan(target) else loudness.gain(L, target, pk.max())
            for c in range(e.shape[0]):
                assert ulps(gains[r], want) <= 1, (name, target, c, float(gains[r]), float(want))
                r += 1
        print(f"loudness: gate target {target}: worst |lufs - definition| {worst:.2e} LU")
    # the cap bound where it should: target 0 on the loud-peaked clips, not at -23 on the quiet ones
    cap = dict((n, (loudness.gain(seen[n][3], 0.0, pk.max()), pk.max())) for n, _, _, pk in clips)
    assert cap["cap"][0] == np.float32(0.99 / 0.9) and cap["silent"][0] == 1.0 and cap["tie"][0] == 1.0
    assert loudness.gain(seen["one"][3], -23.0, 0.3) < np.float32(0.99 / 0.3)


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
    at 16 kHz (0.34 s); 'X': stereo, 8400 samples at 12 kHz (0.7 s: four 400 ms blocks at 48 kHz).  -> ([C, T] array, its rate)"""
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


@pytest.mark.parametrize("name", ["M", "S", "X"])
def test_loudness_is_the_48k_result_times_the_device_gain(name):
    """generate(loudness=-23) = fl32(y48 * g) bit for bit, y48 the same call without the keyword and g the device's gain, restated
    from measure_loudness through loudness.gain; g within 1 ulp of the definition's gain on y48; and the float64 definition reads
    the target off the delivered clip within 1e-4 LU where it says that neither the cap binds nor a block lies within the applied
    gain of the absolute gate (asserted first, from the definition)."""
    target = -23.0
    y48 = run48(name)
    host = y48.cpu().numpy()
    C = host.shape[0]
    got = run(name, loudness=target)
    assert got.dtype == torch.float32 and got.shape == y48.shape
    L_dev = model().measure_loudness(y48, chans=[C])
    assert L_dev.dtype == torch.float32 and L_dev.is_cuda and tuple(L_dev.shape) == (1,)
    peak = float(np.abs(host).max())
    g = loudness.gain(float(L_dev[0]), target, peak)
    assert np.array_equal(got.cpu().numpy(), (host * g).astype(np.float32))
    L_def = loudness.integrated(host, 48000)
    g_def = loudness.gain(L_def, target, peak)
    print(f"loudness: clip {name}: device {float(L_dev[0]):.6f} LUFS, definition {L_def:.6f}, gain {float(g):.7f} ({ulps(g, g_def)} ulp)")
    assert abs(float(L_dev[0]) - L_def) <= 1e-5 and ulps(g, g_def) <= 1
    # the definition's two conditions
    assert 10.0 ** ((target - L_def) / 20.0) < 0.99 / peak
    z = loudness.block_energies(loudness.sub_energies(loudness.k_weight(host, 48000), 48000), host.shape[1], 48000)
    lo, hi = sorted((loudness.ZA, loudness.ZA / float(g) ** 2))
    assert not ((z > lo * (1 - 1e-3)) & (z < hi * (1 + 1e-3))).any()
    delivered = loudness.integrated(got.cpu().numpy(), 48000)
    print(f"loudness: clip {name}: delivered {delivered:.6f} LUFS for {target}")
    assert abs(delivered - target) <= 1e-4
    # what was delivered, read back on the device: a list of clips goes through the segment forms
    back = model().measure_loudness([got, y48])
    assert abs(float(back[0]) - target) <= 1e-4 and float(back[1]) == float(L_dev[0])


def test_the_cap_binds_at_0_lufs():
    """Target 0 LUFS needs more than 0.99 / peak: the delivered peak is 0.99 within 2 ulp and the loudness stays below the target."""
    y48 = run48("S")
    got = run("S", loudness=0.0)
    L = float(model().measure_loudness(y48, chans=[2])[0])
    peak = float(y48.abs().max())
    assert 10.0 ** ((0.0 - L) / 20.0) > 0.99 / peak
    assert abs(float(got.abs().max()) - 0.99) <= 2 * 2.0 ** -24
    assert np.array_equal(got.cpu().numpy(), (y48.cpu().numpy() * loudness.gain(L, 0.0, peak)).astype(np.float32))
    assert float(model().measure_loudness(got, chans=[2])[0]) < -1.0


def test_stereo_takes_one_gain_for_both_rows():
    y48, got = run48("X").cpu().numpy(), run("X", loudness=-30.0).cpu().numpy()
    L = float(model().measure_loudness(run48("X"), chans=[2])[0])
    g = loudness.gain(L, -30.0, float(np.abs(y48).max()))
    for c in range(2):
        assert np.array_equal(got[c], (y48[c] * g).astype(np.float32)), c
    # ... and it is not the gain either row would get alone
    alone = model().measure_loudness(run48("X"))
    assert tuple(alone.shape) == (2,) and float(alone[0]) != L and float(alone[1]) != L


def test_measure_loudness_at_other_rates_and_its_errors():
    """Rows at 16 kHz and at 22 kHz (not an output rate: any rate with a sub-block of 16 samples or more is measured), a tensor with
    chans= and a list of clips, against the definition within 1e-5 LU; the shapes and rates it refuses."""
    m = model()
    for rate, T in ((16000, 9001), (22000, 30011)):
        x = noise_rows(3, T, seed=rate)
        x[2] *= 0.05
        xd = torch.from_numpy(x).cuda()
        got = m.measure_loudness(xd, chans=[2, 1], rate=rate).cpu().numpy()
        want = [loudness.integrated(x[:2], rate), loudness.integrated(x[2:], rate)]
        assert np.abs(got - want).max() <= 1e-5, (rate, got, want)
        listed = m.measure_loudness([xd[:2], xd[2:, :T // 2]], rate=rate).cpu().numpy()
        assert listed[0] == got[0] and abs(listed[1] - loudness.integrated(x[2:, :T // 2], rate)) <= 1e-5
    assert float(m.measure_loudness(torch.zeros(1, 5000, device="cuda"))[0]) == -math.inf
    for bad in (dict(rate=100), dict(rate=44100.5), dict(chans=[2, 2])):
        with pytest.raises(ValueError):
            m.measure_loudness(xd, **bad)
    with pytest.raises(ValueError):
        m.measure_loudness([xd], chans=[3])
    with pytest.raises(ValueError):
        m.measure_loudness(xd.double())


@pytest.mark.parametrize("deliver", [dict(), dict(output_rate=16000), dict(pcm="int16", dither="tpdf", dither_seed=5, interleaved=True),
                                     dict(output_rate=44100, pcm="int16")])
def test_a_clip_gets_the_same_bits_alone_in_a_batch_and_in_a_ragged_group(deliver):
    """The stereo clip S alone = beside a second clip of its length in generate_batch = beside clips of other lengths and another
    input rate in generate_many under both `ends` and without the ragged sequence.  Clip i of a call dithers with (seed, i)."""
    m = model()
    (S, _), (M, _), (L_, _), (W, _) = clip("S"), clip("M"), clip("L"), clip("W")
    S2 = S[::-1] * np.float32(0.5)
    kw = dict(channels="first", loudness=-23.0, **deliver)

    def at(i):
        return dict(kw, dither_seed=[(5, i)]) if "dither_seed" in kw else kw
    alone = m.generate(S, 12000, noise=noise("S"), **at(0))
    batch = m.generate_batch([S, S2], 12000, noise=[noise("S"), noise("S")], **kw)
    assert torch.equal(batch[0], alone) and batch[1].shape == alone.shape and batch[1].dtype == alone.dtype
    mono = m.generate(M, 12000, noise=noise("M"), **at(2))
    wide = m.generate(W, 16000, noise=noise("W"), **at(3))
    for how in (dict(ends="per_clip"), dict(ends="ragged"), dict(ragged=False)):
        outs = m.generate_many([S, L_, M, W], [12000, 12000, 12000, 16000], noise=[noise(n) for n in "SLMW"], **how, **kw)
        assert torch.equal(outs[0], alone), how
        assert torch.equal(outs[2], mono), how
        assert torch.equal(outs[3], wide), how
    assert alone.any() and mono.any() and wide.any()
    if not deliver:
        # the float result against the call without the keyword: the gains differ per clip, S2 is 6 dB down and comes up again
        assert not torch.equal(alone, run48("S"))
        b = m.measure_loudness(torch.cat(list(batch)), chans=[2, 2])
        assert abs(float(b[0]) + 23.0) <= 1e-3 and abs(float(b[1]) + 23.0) <= 1e-3
    if deliver.get("pcm") and "output_rate" not in deliver:
        f = m.generate(S, 12000, noise=noise("S"), channels="first", loudness=-23.0).cpu().numpy()
        assert np.array_equal(alone.cpu().numpy(), pcm.encode(f, key=(5, 0), interleaved=True))


def test_mono_clips_without_channels_and_both_ends():
    """The default path's clips (no channels=): [1, T48] alone, [B, T48] from generate_batch, a ragged group of two lengths."""
    m = model()
    M, L_ = clip("M")[0][0], clip("L")[0][0]
    a = m.generate(M, 12000, noise=noise("M"), loudness=-16.0)
    b = m.generate(L_, 12000, noise=noise("L"), loudness=-16.0)
    assert a.shape == (1, 15840) and b.shape == (1, 19200) and a.dtype == torch.float32
    for ends in ("per_clip", "ragged"):
        outs = m.generate_many([M, L_], 12000, noise=[noise("M"), noise("L")], ends=ends, loudness=-16.0)
        assert torch.equal(outs[0], a) and torch.equal(outs[1], b), ends
    two = m.generate_batch([M, M * np.float32(0.5)], 12000, noise=torch.cat([noise("M"), noise("M")]), loudness=-16.0)
    assert two.shape == (2, 15840) and torch.equal(two[:1], a)


def test_loudness_none_is_the_call_without_the_keyword():
    m = model()
    (S, _), (M, _), (L_, _) = clip("S"), clip("M"), clip("L")
    assert torch.equal(m.generate(S, 12000, noise=noise("S"), channels="first", loudness=None), run48("S"))
    assert torch.equal(m.generate(M[0], 12000, noise=noise("M"), loudness=None), m.generate(M[0], 12000, noise=noise("M")))
    kw = dict(noise=[noise("M"), noise("L")], ends="ragged", output_rate=44100, pcm="int16")
    a, b = m.generate_many([M[0], L_[0]], 12000, loudness=None, **kw), m.generate_many([M[0], L_[0]], 12000, **kw)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_a_loudness_call_scales_no_buffer_the_next_call_reads():
    """The post-processor's rows are plan-owned: after a loudness= call the same call without the keyword gives what it gave
    before, alone, in a batch and in a ragged group, and the loudness= results do not alias each other."""
    m = model()
    (S, _), (M, _), (L_, _) = clip("S"), clip("M"), clip("L")
    before = run48("S").clone()
    quiet = run("S", loudness=-40.0)
    assert torch.equal(run("S"), before)
    loud = run("S", loudness=-20.0)
    assert torch.equal(run("S"), before) and not torch.equal(quiet, loud)
    assert torch.equal(quiet, run("S", loudness=-40.0))
    for ends in ("per_clip", "ragged"):
        kw = dict(noise=[noise("M"), noise("L")], ends=ends)
        ref = [y.clone() for y in m.generate_many([M[0], L_[0]], 12000, **kw)]
        m.generate_many([M[0], L_[0]], 12000, loudness=-40.0, **kw)
        again = m.generate_many([M[0], L_[0]], 12000, **kw)
        assert all(torch.equal(p, q) for p, q in zip(ref, again)), ends
    two = torch.cat([noise("M"), noise("M")])
    ref = m.generate_batch([M[0], M[0]], 12000, noise=two).clone()
    m.generate_batch([M[0], M[0]], 12000, noise=two, loudness=-40.0)
    assert torch.equal(m.generate_batch([M[0], M[0]], 12000, noise=two), ref)
