"""GPU: multichannel clips and level-true output -- the four entries of csrc/level.hip against tests/ref_level.py, bit for bit,
and generate*(channels=, level=) on TINY_CFG at 12 kHz: clips of 3000 and 3960 samples (25 and 33 frames), C in {1, 2, 3}.

The kernels do single correctly rounded float32 operations, so their tests are torch.equal / equal bits and their outputs are
framed by sentinels that must keep their bits.  The model tests are bitwise where two runs of this project are compared (a clip
alone, in a batch, in a ragged group, under either `ends`) and 1e-4 max-abs, the project's bar for a waveform, against the
oracle, which is composed here from ref_cpu's public pieces per channel and finished by ref_level's six rules."""
import numpy as np
import pytest
import scipy.signal
import torch

pytestmark = pytest.mark.gpu

import ref_frontend                                                        # noqa: E402
import ref_level                                                           # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth                 # noqa: E402
from flowhigh_amd import frontend as FE                                    # noqa: E402
from oracle import ref_cpu                                                 # noqa: E402

SR = 12000
TOL_WAVEFORM = 1e-4
GUARD = 64
SENTINEL = 0x7fc12345          # a NaN with a payload: an element that was written, by anything, loses these bits
_STATE = {}


def st():
    return hip.stream()


def framed(x, lead=GUARD):
    """(buffer = lead sentinels, x, GUARD sentinels; the view of x in it).  lead % 4 != 0 puts x off the 16-byte grid."""
    buf = torch.full((lead + x.numel() + GUARD,), SENTINEL, dtype=torch.int32).view(torch.float32).cuda()
    view = buf[lead:lead + x.numel()]
    view.copy_(x.reshape(-1))
    return buf, view


def sentinels_intact(buf, lead, n):
    b = buf.view(torch.int32)
    return bool((b[:lead] == SENTINEL).all()) and bool((b[lead + n:] == SENTINEL).all())


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024, 1025])
def test_row_gain_is_one_float32_multiply_per_sample(n, batch):
    """Every length at every alignment of the first row (lead 64 .. 61 elements; the later rows move with b * n): the slots
    that overlap a row's ends go element by element, the others as 16-byte accesses."""
    L = hip.lib()
    x = rnd(batch, n, seed=n + batch)
    gains = torch.tensor([0.37, 0.0, 1.0][:batch])
    want = x * gains[:, None]                                       # the host's float32 product
    g_dev = gains.cuda()
    for lead in (64, 63, 62, 61):
        buf, view = framed(x, lead)
        hip.check(L.fh_row_gain_f32(view.data_ptr(), g_dev.data_ptr(), batch, n, st()), "fh_row_gain_f32")
        assert torch.equal(view.cpu().view(batch, n), want), (n, batch, lead)
        assert sentinels_intact(buf, lead, batch * n), (n, batch, lead)


def test_row_gain_seg_works_over_the_clip_table():
    L = hip.lib()
    lens = [1, 1025, 4]
    xs = [rnd(n, seed=70 + n) for n in lens]
    gains = torch.tensor([0.5, 0.37, 3.0])
    packed = []
    for i, x in enumerate(xs):                                      # clip i behind 61 + i sentinels of its own
        packed += [torch.full((61 + i,), SENTINEL, dtype=torch.int32).view(torch.float32), x]
    packed.append(torch.full((GUARD,), SENTINEL, dtype=torch.int32).view(torch.float32))
    buf = torch.cat(packed).cuda()
    offs, pos = [], 0
    for i, n in enumerate(lens):
        pos += 61 + i
        offs.append(pos)
        pos += n
    keep, (clips,) = FE.upload_tables([FE.clip_array(dst=[buf.data_ptr() + 4 * o for o in offs], len_out=lens)], torch.device("cuda"))
    g_dev = gains.cuda()
    hip.check(L.fh_row_gain_seg_f32(clips, 3, max(lens), g_dev.data_ptr(), st()), "fh_row_gain_seg_f32")
    got = buf.cpu()
    mask = torch.ones(got.numel(), dtype=torch.bool)
    for o, n, x, g in zip(offs, lens, xs, gains):
        assert torch.equal(got[o:o + n], x * g)
        mask[o:o + n] = False
    assert bool((got.view(torch.int32)[mask] == SENTINEL).all())


def test_channel_peaks_gives_the_gains_and_floors_a_silent_row():
    L = hip.lib()
    peaks = np.array([0.0, 1e-40, 0.5, 1.0, 0.0, 3.25], dtype=np.float32)          # zero, denormal, ordinary
    assert peaks[1] != 0
    want_gains, want_div = ref_level.channel_peaks(peaks)
    buf, slots = framed(torch.from_numpy(peaks), 61)
    gbuf, gains = framed(torch.zeros(len(peaks)), 63)
    hip.check(L.fh_channel_peaks_f32(slots.data_ptr(), gains.data_ptr(), len(peaks), st()), "fh_channel_peaks_f32")
    assert np.array_equal(gains.cpu().numpy().view(np.uint32), want_gains.view(np.uint32))
    assert np.array_equal(slots.cpu().numpy().view(np.uint32), want_div.view(np.uint32))
    assert sentinels_intact(buf, 61, len(peaks)) and sentinels_intact(gbuf, 63, len(peaks))


def test_group_peak_is_the_joint_peak_of_a_group_s_live_rows():
    L = hip.lib()
    f = np.float32
    # groups of 1, 2 and 3 rows: the pair has a silent row with a NaN q behind its zero gain, the triple is all silent; then
    # 300 groups of 1 .. 3 rows over three blocks of the launch, some across a block's edge, every fifth row silent
    q = [0.8, 0.5, np.nan, 3.0, np.nan, 7.0]
    g = [0.5, 0.25, 0.0, 0.0, 0.0, 0.0]
    group = [0, 1, 1, 2, 2, 2]
    rng = np.random.default_rng(5)
    for k in range(300):
        c = 1 + k % 3
        group += [3 + k] * c
        q += list(rng.uniform(0.1, 2.0, c))
        g += list(rng.uniform(0.01, 1.0, c))
    q, g, group = np.array(q, dtype=f), np.array(g, dtype=f), np.array(group, dtype=np.int32)
    g[10::5] = 0
    want = ref_level.group_peak(q, g, group)
    assert want[:6].tolist() == [float(f(0.8) * f(0.5)), 0.125, 0.125, 1.0, 1.0, 1.0] and len(q) > 512
    buf, slots = framed(torch.from_numpy(q), 62)
    g_dev, group_dev = torch.from_numpy(g).cuda(), torch.from_numpy(group).cuda()
    hip.check(L.fh_group_peak_f32(slots.data_ptr(), g_dev.data_ptr(), group_dev.data_ptr(), len(q), st()), "fh_group_peak_f32")
    assert np.array_equal(slots.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert sentinels_intact(buf, 62, len(q))


# ---- the model ---------------------------------------------------------------------------------------------------------------
def flownet():
    if "fh" not in _STATE:
        _STATE["sd"] = synth.make_state_dict(synth.TINY_CFG, 0)
        _STATE["fh"] = FLowHigh(_STATE["sd"], synth.TINY_CFG, "cuda")
    return _STATE["fh"]


def model(method="scipy", prior="reference"):
    key = (method, prior)
    if key not in _STATE:
        _STATE[key] = FlowHighSR(flownet(), torchdiffeq_ode_method="euler", upsampling_method=method, prior=prior)
    return _STATE[key]


def clip(name):
    """'A': 3 channels of 3000 samples at three levels; 'B': 2 channels of 3960; 'M': a mono clip of 3960."""
    chans, n, seed, scale = dict(A=(3, 3000, 500, (1.0, 0.4, 2.5)), B=(2, 3960, 510, (0.3, 1.7)), M=(1, 3960, 520, (1.0,)))[name]
    x = np.stack([synth.lowres_clip(seed + c, n / SR, SR)[:n] * np.float32(scale[c]) for c in range(chans)])
    assert x.shape == (chans, n) and np.abs(x).max() <= 1
    return x[0] if name == "M" else x


def noise(name):
    return synth.prior_noise(dict(A=30, B=31, M=32)[name], dict(A=25, B=33, M=33)[name])


def oracle_row(name, c):
    """(w, p, cr) of channel c of a clip through the oracle, once per session: scipy's resample_poly and the host's peak, the
    sampler with the CLIP's noise, the cutoff and splice of ref_cpu.post_processing, the inverse STFT in float64."""
    key = ("oracle", name, c)
    if key not in _STATE:
        flownet()
        x = np.atleast_2d(clip(name))[c]
        cond = scipy.signal.resample_poly(x, 48000, SR)
        p = ref_level.peak(cond)
        cond48 = torch.tensor(ref_level.normalise(cond, np.max(np.abs(cond)))).unsqueeze(0).float()
        wav = ref_cpu.sample(_STATE["sd"], synth.TINY_CFG, cond48, noise(name), 1, "euler").squeeze(1)
        sp, ss = ref_cpu.stft_center(wav), ref_cpu.stft_center(cond48)
        cr = ref_cpu.cutoff_index(ss)
        n = min(sp.size(-1), ss.size(-1))
        res = torch.cat([ss[0, :cr, :n], sp[0, cr:, :n]], 0)                           # [1025, frames]
        w, _ = ref_frontend.istft_ola(ref_frontend.irfft(res.transpose(0, 1)), torch.hann_window(2048), cond48.shape[1], 2048, 480)
        _STATE[key] = (w.numpy().astype(np.float32), p, cr)
    return _STATE[key]


def oracle_clip(name, level, live=None):
    """The clip's rows by the six rules; live: the channels that are not silenced (the others' peaks are 0)."""
    chans = np.atleast_2d(clip(name)).shape[0]
    rows = [oracle_row(name, c) for c in range(chans)]
    ps = [p if live is None or c in live else np.float32(0) for c, (_, p, _) in enumerate(rows)]
    return ref_level.finish([w for w, _, _ in rows], ps, level), [cr for _, _, cr in rows]


def test_one_channel_given_as_a_layout_is_the_mono_clip():
    """(a) [1, T] with channels='first', [T, 1] with channels='last' and the 1-D clip: one result, [1, T48]."""
    m, x, z = model(), clip("M"), noise("M")
    ref = m.generate(x, SR, noise=z).clone()
    assert ref.shape == (1, 15840)
    assert torch.equal(m.generate(x[None], SR, noise=z, channels="first"), ref)
    assert torch.equal(m.generate(x[:, None], SR, noise=z, channels="last"), ref)
    assert torch.equal(model("hip").generate(x[None], SR, noise=z, channels="first"), model("hip").generate(x, SR, noise=z))


@pytest.mark.parametrize("level", ["peak", "input"])
def test_swapping_the_channels_swaps_the_rows(level):
    """(b) ... bit for bit: the rows are independent up to the joint peak, and a maximum does not depend on the order."""
    m, x, z = model("hip"), clip("B"), noise("B")
    out = m.generate(x, SR, noise=z, channels="first", level=level)
    swapped = m.generate(np.ascontiguousarray(x[::-1].T), SR, noise=z, channels="last", level=level)
    assert out.shape == swapped.shape == (2, 15840) and torch.isfinite(out).all()
    assert torch.equal(swapped, out.flip(0)) and not torch.equal(out[0], out[1])


@pytest.mark.parametrize("prior,method", [("reference", "scipy"), ("device", "hip")])
@pytest.mark.parametrize("level", ["peak", "input"])
def test_a_clip_gives_the_same_bits_alone_in_a_batch_and_in_a_ragged_group(prior, method, level):
    """(c) the stereo clip B alone = beside a second clip of its length in generate_batch = beside clips of another length in
    generate_many, for ends='per_clip', ends='ragged' and ragged=False.  The mono clip beside it keeps the bits of the default
    path at level='peak' (its gain is 1 there)."""
    m, kw = model(method, prior), dict(channels="first", level=level)
    A, B, M = clip("A"), clip("B"), clip("M")
    B2 = B[::-1] * np.float32(0.5)
    if prior == "reference":
        pr = lambda *names: dict(noise=[noise(n) for n in names])                       # noqa: E731
        alone = m.generate(B, SR, noise=noise("B"), **kw).clone()
        mono = m.generate(M, SR, noise=noise("M"), level=level).clone()
    else:
        pr = lambda *names: dict(seed=77)                                               # noqa: E731  (clip i of a list: key (77, i))
        alone = m.generate(B, SR, seed=[(77, 0)], **kw).clone()
        mono = m.generate(M, SR, seed=[(77, 1)], level=level).clone()
    assert alone.shape == (2, 15840) and torch.isfinite(alone).all()
    batch = m.generate_batch([B, B2], SR, **pr("B", "B"), **kw)
    assert torch.equal(batch[0], alone) and batch[1].shape == (2, 15840)
    for how in (dict(ends="per_clip"), dict(ends="ragged"), dict(ragged=False)):
        outs = m.generate_many([B, M[None], A], SR, **pr("B", "M", "A"), **how, **kw)
        assert [tuple(o.shape) for o in outs] == [(2, 15840), (1, 15840), (3, 12000)], how
        assert torch.equal(outs[0], alone), how
        assert torch.equal(outs[1], mono), how
    if prior == "device":                                           # one key for the clip: equal channels are equal rows
        twin = m.generate(np.stack([M, M]), SR, seed=5, **kw)
        assert torch.equal(twin[0], twin[1]) and torch.isfinite(twin).all()


@pytest.mark.parametrize("method", ["scipy", "hip"])
@pytest.mark.parametrize("level", ["peak", "input"])
def test_multichannel_run_against_the_oracle(method, level):
    """(d) clips A (3 channels, 25 frames) and B (2 channels, 33 frames): every row within 1e-4 of the oracle's row finished by
    ref_level (|out| <= 0.99 at 'peak', <= p_c q_c at 'input'), the cutoff bin of every channel exact."""
    m = model(method)
    for name in ("A", "B"):
        x = clip(name)
        (out,), stages = m.generate_batch([x], SR, noise=noise(name), channels="first", level=level, return_stages=True)
        want, crs = oracle_clip(name, level)
        assert stages["cr"].tolist() == crs, (name, stages["cr"].tolist(), crs)
        p_err = max(abs(float(g) - float(oracle_row(name, c)[1])) for c, g in enumerate(stages["gains"].cpu()))
        errs = [float(np.abs(out[c].cpu().numpy() - want[c]).max()) for c in range(x.shape[0])]
        peaks = [float(np.abs(w).max()) for w in want]
        print(f"level: oracle {method:5s} {level:5s} clip {name}: max-abs per channel {['%.2e' % e for e in errs]}, "
              f"|want| <= {['%.3f' % p for p in peaks]}, |p - p_oracle| <= {p_err:.1e}, cr {crs}")
        # (p is the magnitude of a sample of the resampled waveform: scipy's on the host, the bar of a waveform on the device)
        assert max(errs) <= TOL_WAVEFORM and p_err <= (0 if method == "scipy" else TOL_WAVEFORM)
        if level == "peak":
            assert abs(max(peaks) - 0.99) < 1e-6 and float(out.abs().max()) == float(np.float32(0.99))


@pytest.mark.parametrize("method", ["scipy", "hip"])
@pytest.mark.parametrize("level", ["peak", "input"])
def test_silent_channels_come_back_as_zeros(method, level):
    """(e) [x, 0, 0]: the silent rows are exact zeros, everything is finite, and the live row is what rules 3-6 make of the
    oracle's row when the others do not count.  [0, 0]: zeros."""
    m, x, z = model(method), clip("A").copy(), noise("A")
    x[1:] = 0
    out = m.generate(x, SR, noise=z, channels="first", level=level)
    assert out.shape == (3, 12000) and torch.isfinite(out).all()
    assert not out[1:].any() and out[0].any()
    want, _ = oracle_clip("A", level, live=(0,))
    err = float(np.abs(out[0].cpu().numpy() - want[0]).max())
    print(f"level: silent {method:5s} {level:5s}: live row max-abs {err:.2e}")
    assert err <= TOL_WAVEFORM and not want[1].any()
    if level == "peak":
        assert float(out.abs().max()) == float(np.float32(0.99))
    out = m.generate(np.zeros((2, 3000), dtype=np.float32), SR, noise=z, channels="first", level=level)
    assert out.shape == (2, 12000) and not out.any()


@pytest.mark.parametrize("method", ["scipy", "hip"])
def test_level_input_on_a_mono_clip_differs_from_the_default_by_its_last_scaling(method):
    """(f) With w the inverse STFT's output, q = max |w| and p the input's peak, the default run returns d = fl(fl(w / q) * 0.99f)
    and level='input' returns u = fl(w * p), whose peak is max |u| = fl(q * p) (rounding is monotone).  Hence in exact arithmetic
    u * 0.99f = d * max |u|: the two runs differ only in their last scaling steps.  In float32 u carries one rounding and
    d * max |u| three (the division, the product with 0.99f, fl(q * p)), each at most 2^-24 relative, so
        |u - d * max |u| / 0.99f|  <=  4 * 2^-24 * |w p|  <=  4 ulp(max |u|),
    evaluated here in float64.  (p itself is pinned against the oracle by the parity test above; here it is also compared with
    the host's scipy peak.)  The relation is the one that holds for these definitions: u = d * p would need q = 0.99."""
    m, x, z = model(method), clip("M"), noise("M")
    d = m.generate(x, SR, noise=z).cpu().numpy().astype(np.float64)
    u32, stages = m.generate_batch([x], SR, noise=z, level="input", return_stages=True)
    assert u32.shape == (1, 15840) and torch.equal(u32, m.generate(x, SR, noise=z, level="input"))
    u = u32.cpu().numpy().astype(np.float64)
    peak = np.float32(np.abs(u32.cpu().numpy()).max())
    dist = float(np.abs(u - d * float(peak) / float(np.float32(0.99))).max())
    ulp = float(np.spacing(peak))
    p_host = ref_level.peak(scipy.signal.resample_poly(x, 48000, SR))
    p_err = abs(float(stages["gains"][0]) - float(p_host))
    print(f"level: input-vs-default {method:5s}: {dist:.3e} = {dist / ulp:.2f} ulp of the peak {float(peak):.4f}; |p - p_host| {p_err:.1e}")
    assert dist <= 4 * ulp
    assert p_err <= (0 if method == "scipy" else TOL_WAVEFORM)
