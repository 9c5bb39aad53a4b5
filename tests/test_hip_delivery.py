"""GPU: delivery on the device -- fh_pcm_i16_f32 / fh_pcm_i16_seg_f32 against flowhigh_amd/pcm.py bit for bit, the resampler's
kernels with the plans of the output rates against float64, and generate*(output_rate=, pcm=, dither=, interleaved=) and the
batching server on TINY_CFG: clips of 0.33 to 0.4 s at 12 and 16 kHz.

The encoder does exact or correctly rounded float32 operations, so its tests are equalities and its outputs are framed by
sentinels that must keep their bits.  The model tests are bitwise where two runs of this project are compared, and against a
float64 resampling of the same model's own 48 kHz result at the bar derived in each test."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_frontend                                                        # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, delivery, hip, pcm, synth, tables    # noqa: E402
from flowhigh_amd import frontend as FE                                    # noqa: E402

U = 2.0 ** -24
GUARD = 64
SENT16 = 0x5A17                # an int16 no test value encodes to by accident: an element that was written loses it
SENT32 = 0x7fc12345
LSB = np.float32(2.0 ** -15)
DOWN_RATES = [44100, 32000, 24000, 22050, 16000, 11025, 8000, 96000]
_STATE = {}


def st():
    return hip.stream()


def planted(n_clips, C, T, seed):
    """N(0, 0.3) [n_clips, C, T] with the values that decide an encoder planted over it: ties, +-1, beyond +-1, NaN, +-inf,
    denormals, the last steps below full scale."""
    x = (torch.randn(n_clips, C, T, generator=torch.Generator().manual_seed(seed)) * 0.3).numpy()
    f = np.float32
    special = f([0.5 * LSB, 1.5 * LSB, 2.5 * LSB, -0.5 * LSB, -1.5 * LSB, 1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 1e-40,
                 -1e-40, 32766.5 * LSB, 32767.5 * LSB, -32767.5 * LSB, 0.0])
    flat = x.reshape(-1)
    pos = np.random.default_rng(seed).permutation(flat.size)[:len(special)]
    flat[pos] = np.roll(special, seed)[:len(pos)]
    return x


def frame16(n, lead):
    buf = torch.full((lead + n + GUARD,), SENT16, dtype=torch.int16, device="cuda")
    return buf, buf[lead:lead + n]


def intact16(buf, lead, n):
    return bool((buf[:lead] == SENT16).all()) and bool((buf[lead + n:] == SENT16).all())


def dev_keys(keys):
    return torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)).cuda()


def want_clip(x, key, interleaved):
    return torch.from_numpy(pcm.encode(x, key, interleaved).reshape(-1))


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_clips", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 8])
def test_pcm_kernel_gives_pcm_py_s_bits(C, n_clips):
    """Every length either side of a run of 8 and of a block of 2048 samples, planar and interleaved, with and without dither,
    the output on a 16-byte boundary and one int16 past it (the later rows and clips move with C * len), the input on the
    16-byte grid and one float past it.  Interleaved with C = 2, 4, 8: the aligned output is written as whole frames, the one
    an int16 further on sample by sample -- the same values."""
    L = hip.lib()
    keys = [(77 + 2 ** 33, 5), (2 ** 64 - 1, 0), (3, 2 ** 40)][:n_clips]
    kd = dev_keys(keys)
    for T in (1, 2, 3, 7, 8, 9, 255, 256, 257, 2049):
        x = planted(n_clips, C, T, seed=T + 10 * C + n_clips)
        n = x.size
        xbuf = torch.full((GUARD + 1 + n,), SENT32, dtype=torch.int32).view(torch.float32).cuda()
        wants = {(i, d): torch.cat([want_clip(x[b], keys[b] if d else None, i) for b in range(n_clips)])
                 for i in (0, 1) for d in (False, True)}
        for lead, xlead in ((GUARD, GUARD), (GUARD + 1, GUARD), (GUARD, GUARD + 1)):
            xd = xbuf[xlead:xlead + n]
            xd.copy_(torch.from_numpy(x.reshape(-1)))
            for interleaved in (0, 1):
                for dither in (False, True):
                    buf, y = frame16(n, lead)
                    hip.check(L.fh_pcm_i16_f32(xd.data_ptr(), y.data_ptr(), kd.data_ptr() if dither else 0, n_clips, C, T,
                                               interleaved, st()), "fh_pcm_i16_f32")
                    case = (T, lead, xlead, interleaved, dither)
                    assert torch.equal(y.cpu(), wants[interleaved, dither]), case
                    assert intact16(buf, lead, n), case


@pytest.mark.parametrize("C", [1, 3])
def test_pcm_planar_rows_at_every_lead(C):
    """A planar row starts 0 .. 7 int16 past a 16-byte boundary, so its first run holds 8 .. 1 of its samples: every one of the 8
    offsets (the later rows move with T), lengths below, at and above a run and two runs, the input on the 16-byte grid and one
    float past it, with and without dither."""
    L = hip.lib()
    key = (77 + 2 ** 33, 5)
    kd = dev_keys([key])
    for T in (1, 7, 8, 9, 17, 23):
        x = planted(1, C, T, seed=T + 10 * C)
        n = x.size
        xbuf = torch.full((GUARD + 1 + n,), SENT32, dtype=torch.int32).view(torch.float32).cuda()
        wants = {d: want_clip(x[0], key if d else None, 0) for d in (False, True)}
        for xlead in (GUARD, GUARD + 1):
            xd = xbuf[xlead:xlead + n]
            xd.copy_(torch.from_numpy(x.reshape(-1)))
            assert xd.data_ptr() % 16 == 4 * (xlead - GUARD)
            for lead in range(GUARD, GUARD + 8):
                for dither in (False, True):
                    buf, y = frame16(n, lead)
                    assert y.data_ptr() % 16 == 2 * (lead - GUARD)
                    hip.check(L.fh_pcm_i16_f32(xd.data_ptr(), y.data_ptr(), kd.data_ptr() if dither else 0, 1, C, T, 0, st()),
                              "fh_pcm_i16_f32")
                    case = (T, lead, xlead, dither)
                    assert torch.equal(y.cpu(), wants[dither]), case
                    assert intact16(buf, lead, n), case


def test_pcm_kernel_dither_does_not_depend_on_layout_batch_or_channel_count():
    """Channel 1 of clip 2 of a batch of 4-channel clips = channel 1 of a 2-channel clip alone under the same key, planar or
    interleaved; channel 0 is not channel 1."""
    L = hip.lib()
    T, key = 777, (123456789, 42)
    x = planted(3, 4, T, seed=5) * LSB * 3                          # a few LSB: the dither decides most samples
    x = np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)
    kd = dev_keys([(1, 1), (2, 2), key])
    y = torch.empty(3 * 4 * T, dtype=torch.int16, device="cuda")
    xd = torch.from_numpy(x).cuda()
    hip.check(L.fh_pcm_i16_f32(xd.data_ptr(), y.data_ptr(), kd.data_ptr(), 3, 4, T, 0, st()), "fh_pcm_i16_f32")
    big = y.view(3, 4, T)[2].cpu()
    pair = torch.from_numpy(np.ascontiguousarray(x[2, :2])).cuda()
    y2, k1 = torch.empty(2 * T, dtype=torch.int16, device="cuda"), dev_keys([key])
    hip.check(L.fh_pcm_i16_f32(pair.data_ptr(), y2.data_ptr(), k1.data_ptr(), 1, 2, T, 1, st()), "fh_pcm_i16_f32")
    assert torch.equal(y2.view(T, 2).t().cpu(), big[:2])
    same = torch.from_numpy(np.stack([x[2, 0], x[2, 0]])).cuda()
    hip.check(L.fh_pcm_i16_f32(same.data_ptr(), y2.data_ptr(), k1.data_ptr(), 1, 2, T, 0, st()), "fh_pcm_i16_f32")
    assert not torch.equal(y2.view(2, T)[0], y2.view(2, T)[1])


@pytest.mark.parametrize("interleaved", [0, 1])
@pytest.mark.parametrize("dither", [False, True])
def test_pcm_seg_gives_every_clip_the_bits_of_the_batched_entry(dither, interleaved):
    """Clips of (len, C) = (1, 1), (9, 3), (257, 2) in one launch, the second with its rows 13 floats apart in a wider buffer,
    the outputs back to back (so at odd int16 offsets): each torch.equal to fh_pcm_i16_f32 on that clip alone."""
    L = hip.lib()
    shapes, pitches = [(1, 1), (9, 3), (257, 2)], [1, 13, 257]
    keys = [(9, 0), (9, 1), (2 ** 63, 7)]
    xs = [planted(1, c, t, seed=40 + t)[0] for t, c in shapes]
    srcs, alone = [], []
    for x, (t, c), pitch, key in zip(xs, shapes, pitches, keys):
        wide = torch.full((c, pitch), float("nan"))
        wide[:, :t] = torch.from_numpy(x)
        srcs.append(wide.cuda())
        y = torch.empty(c * t, dtype=torch.int16, device="cuda")
        xd, k1 = torch.from_numpy(x).cuda(), dev_keys([key])
        hip.check(L.fh_pcm_i16_f32(xd.data_ptr(), y.data_ptr(), k1.data_ptr() if dither else 0, 1, c, t,
                                   interleaved, st()), "fh_pcm_i16_f32")
        alone.append(y.cpu())
        assert torch.equal(alone[-1], want_clip(x, key if dither else None, interleaved))
    total = sum(t * c for t, c in shapes)
    buf, y = frame16(total, GUARD + 1)
    off = [0, 1, 1 + 27]
    table = (hip.PcmClip * 3)(*[hip.PcmClip(s.data_ptr(), y.data_ptr() + 2 * o, p, c, t)
                               for s, o, p, (t, c) in zip(srcs, off, pitches, shapes)])
    keep, (clips,) = FE.upload_tables([table], torch.device("cuda"))
    kd = dev_keys(keys)
    hip.check(L.fh_pcm_i16_seg_f32(clips, 3, 3, 257, kd.data_ptr() if dither else 0, interleaved, st()),
              "fh_pcm_i16_seg_f32")
    got = y.cpu()
    for o, (t, c), a in zip(off, shapes, alone):
        assert torch.equal(got[o:o + t * c], a), (t, c)
    assert intact16(buf, GUARD + 1, total)


def test_pcm_entries_check_their_arguments():
    """The checks run on the host before anything is launched: the device pointers are fake addresses, never read."""
    L = hip.lib()
    assert L.fh_sizeof_pcm_clip() == 32
    A, B, K = 256, 512, 1024
    bad = [("fh_pcm_i16_f32", a) for a in ((0, B, K, 1, 1, 8, 0), (A, 0, K, 1, 1, 8, 0), (A, B, K, 0, 1, 8, 0),
                                           (A, B, K, 65536, 1, 8, 0), (A, B, K, 1, 0, 8, 0), (A, B, K, 1, 9, 8, 0),
                                           (A, B, K, 1, 1, 0, 0), (A, B, K, 1, 1, -3, 0), (A + 2, B, K, 1, 1, 8, 0),
                                           (A, B + 1, K, 1, 1, 8, 0))]
    bad += [("fh_pcm_i16_seg_f32", a) for a in ((0, 1, 1, 8, K, 0), (A, 0, 1, 8, K, 0), (A, 65536, 1, 8, K, 0), (A, 1, 0, 8, K, 0),
                                               (A, 1, 9, 8, K, 0), (A, 1, 1, 0, K, 0))]
    for name, args in bad:
        assert getattr(L, name)(*args, 0) == -1, (name, args)
        assert name.encode() in L.fh_last_error(), (name, args)


# ---- the resampler with the plans of the output rates ---------------------------------------------------------------------------
def resample_ref(x, taps, up, down, pre, n_out):
    """tests/ref_frontend.resample in output chunks (its matrix for a 0.33 s clip would be 2 GB): chunk a starts at output
    up * a * c, whose inputs start at down * a * c; the window opens `back` inputs earlier, back = down * s with back * up >=
    n_taps, which is the same sum with pre + up * s in place of pre."""
    n_in = x.shape[1]
    s = math.ceil(taps.numel() / (up * down))
    c = max(1, 1024 // up)
    outs, As = [], []
    for i0 in range(0, n_out, up * c):
        i1 = min(n_out, i0 + up * c)
        j0 = i0 // up * down
        back = min(j0 // down, s)
        lo = j0 - back * down
        hi = min(n_in, ((i1 + pre) * down) // up + 1)
        r, A = ref_frontend.resample(x[:, lo:hi], taps, up, down, pre + up * back, i1 - i0)
        outs.append(r)
        As.append(A)
    return torch.cat(outs, 1), torch.cat(As, 1)


def test_resample_ref_in_chunks_is_the_whole_matrix():
    for rate in (44100, 16000, 96000):
        taps, pre, up, down = tables.resample_poly_plan(rate, 48000)
        x = torch.randn(2, 3001, generator=torch.Generator().manual_seed(rate))
        n_out = tables.resample_out_len(3001, rate, 48000)
        whole, chunked = ref_frontend.resample(x, taps, up, down, pre, n_out), resample_ref(x, taps, up, down, pre, n_out)
        # (the same terms in float64 sums of another length: equal up to the order of a few hundred additions)
        assert float((whole[0] - chunked[0]).abs().max()) <= 1e-12 and float((whole[1] - chunked[1]).abs().max()) <= 1e-12


@pytest.mark.parametrize("rate", DOWN_RATES)
def test_resample_poly_kernel_with_the_down_plans(rate):
    """fh_resample_poly_f32 with resample_poly_plan(R, 48000), batch 2: |got - ref| <= (ceil(n_taps / up) + 1) u A, A = sum |x h|:
    a chain of at most ceil(n_taps / up) fused terms, each adding at most u of the running sum of |x h|, and one to spare --
    the existing resampler test's bar with this plan's chain length."""
    L = hip.lib()
    taps, pre, up, down = tables.resample_poly_plan(rate, 48000)
    terms = math.ceil(taps.numel() / up) + 1
    tdev = taps.cuda()
    for n_in in (1, 2, 19, 601, 4801):
        n_out = tables.resample_out_len(n_in, rate, 48000)
        x = torch.randn(2, n_in, generator=torch.Generator().manual_seed(rate + n_in)) * 0.3
        y = torch.full((2 * n_out + GUARD,), float("nan"), device="cuda")
        hip.check(L.fh_resample_poly_f32(x.cuda().data_ptr(), tdev.data_ptr(), y.data_ptr(), 2, n_in, n_out, up, down,
                                         taps.numel(), pre, st()), "fh_resample_poly_f32")
        assert torch.isnan(y[2 * n_out:]).all()
        ref, A = resample_ref(x, taps, up, down, pre, n_out)
        err = (y[:2 * n_out].cpu().view(2, n_out).double() - ref).abs()
        assert float(ref.abs().max()) > 0.0 and bool((err <= terms * U * A).all()), (rate, n_in, float((err - terms * U * A).max()))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def model(method="hip", prior="reference"):
    if "fh" not in _STATE:
        _STATE["fh"] = FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda")
    if (method, prior) not in _STATE:
        _STATE[(method, prior)] = FlowHighSR(_STATE["fh"], torchdiffeq_ode_method="euler", upsampling_method=method, prior=prior)
    return _STATE[(method, prior)]


CLIPS = dict(M=(1, 3960, 12000, 33), S=(2, 3960, 12000, 33), L=(1, 4800, 12000, 40), W=(1, 5400, 16000, 33))


def clip(name):
    """'M': mono, 3960 samples at 12 kHz (0.33 s, 33 frames); 'S': stereo of that length; 'L': mono, 4800 samples (0.4 s);
    'W': mono, 5400 samples at 16 kHz (0.34 s).  -> (array, its rate)"""
    chans, n, sr, _ = CLIPS[name]
    scale = (1.0, 0.45)
    x = np.stack([synth.lowres_clip(600 + ord(name) + c, n / sr, sr)[:n] * np.float32(scale[c]) for c in range(chans)])
    assert x.shape == (chans, n) and np.abs(x).max() <= 1
    return (x[0] if chans == 1 else x), sr


def noise(name):
    return synth.prior_noise(700 + ord(name), CLIPS[name][3])


def run48(name, level="peak"):
    """The model's own 48 kHz result of the call without a delivery keyword, once per session: [C, T48] float32 on the host."""
    key = ("y48", name, level)
    if key not in _STATE:
        x, sr = clip(name)
        kw = dict(channels="first") if x.ndim == 2 else {}
        if level != "peak":
            kw["level"] = level
        _STATE[key] = model().generate(x, sr, noise=noise(name), **kw).cpu().clone()
    return _STATE[key]


def resampled48(name, level, rate):
    """(float64 resample_poly of run48 by the plan, A = sum |x h|, K = ceil(n_taps / up)), once per session."""
    key = ("ref", name, level, rate)
    if key not in _STATE:
        taps, pre, up, down = tables.resample_poly_plan(rate, 48000)
        y48 = run48(name, level)
        _STATE[key] = resample_ref(y48, taps, up, down, pre, tables.resample_out_len(y48.shape[1], rate, 48000)) + \
            (math.ceil(taps.numel() / up),)
    return _STATE[key]


@pytest.mark.parametrize("name", ["M", "S"])
@pytest.mark.parametrize("rate", [44100, 16000])
def test_output_rate_is_resample_poly_of_the_48k_result_at_099_of_its_peak(rate, name):
    """generate(output_rate=R) against r = float64 resample_poly of the same model's 48 kHz result, put at 0.99 of max |r| (over
    the clip's channels).  The kernel's sum is within (K + 1) u A of r (K = ceil(n_taps / up) fused terms and one to spare); the
    scaling (the peak's own rounding, a division, a product) adds at most 4 u |r|; both are scaled by 0.99 / peak."""
    x, sr = clip(name)
    kw = dict(channels="first") if x.ndim == 2 else {}
    got = model().generate(x, sr, noise=noise(name), output_rate=rate, **kw)
    r, A, K = resampled48(name, "peak", rate)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(r.shape) == (run48(name).shape[0], delivery.delivered_len(15840, rate))
    peak = float(r.abs().max())
    bar = ((K + 1) * U * A + 4 * U * r.abs()) * 0.99 / peak
    err = (got.cpu().double() - r * 0.99 / peak).abs()
    print(f"delivery: output_rate {rate} clip {name}: worst error / bar {float((err / bar).max()):.3f}, max-abs {float(err.max()):.2e}")
    assert bool((err <= bar).all())
    assert abs(float(got.abs().max()) - 0.99) <= 2 * U


@pytest.mark.parametrize("rate", [44100, 16000])
def test_output_rate_at_level_input_is_not_rescaled(rate):
    """level='input': the resampling of that call's own 48 kHz result and nothing else: within (K + 1) u A."""
    x, sr = clip("S")
    got = model().generate(x, sr, noise=noise("S"), output_rate=rate, channels="first", level="input")
    r, A, K = resampled48("S", "input", rate)
    err = (got.cpu().double() - r).abs()
    print(f"delivery: output_rate {rate} level=input: worst error / bar {float((err / ((K + 1) * U * A)).max()):.3f}")
    assert tuple(got.shape) == tuple(r.shape) and bool((err <= (K + 1) * U * A).all())


def test_a_silent_clip_stays_zeros():
    got = model().generate(np.zeros((2, 3960), dtype=np.float32), 12000, noise=noise("S"), channels="first", output_rate=44100,
                           pcm="int16", dither=None)
    assert got.dtype == torch.int16 and got.shape == (2, 14553) and not got.any()
    got = model().generate(np.zeros((2, 3960), dtype=np.float32), 12000, noise=noise("S"), channels="first", output_rate=44100)
    assert got.dtype == torch.float32 and not got.any()


@pytest.mark.parametrize("rate", [None, 44100])
def test_pcm_is_pcm_py_s_encoding_of_the_float_result(rate):
    """pcm='int16' = pcm.encode of what the same call returns without it, with and without dither; interleaved=True is its
    transpose, exactly."""
    m = model()
    for name in ("M", "S"):
        x, sr = clip(name)
        kw = dict(noise=noise(name), output_rate=rate, **(dict(channels="first") if x.ndim == 2 else {}))
        y = m.generate(x, sr, **kw).cpu().numpy()
        plain = m.generate(x, sr, pcm="int16", **kw)
        assert plain.dtype == torch.int16 and plain.is_cuda and tuple(plain.shape) == y.shape
        assert np.array_equal(plain.cpu().numpy(), pcm.encode(y))
        dith = m.generate(x, sr, pcm="int16", dither="tpdf", dither_seed=31, **kw)
        assert np.array_equal(dith.cpu().numpy(), pcm.encode(y, key=(31, 0)))
        assert not np.array_equal(dith.cpu().numpy(), plain.cpu().numpy())
        inter = m.generate(x, sr, pcm="int16", dither="tpdf", dither_seed=[(31, 0)], interleaved=True, **kw)
        assert tuple(inter.shape) == y.shape[::-1] and inter.is_contiguous() and torch.equal(inter.t(), dith)


@pytest.mark.parametrize("prior", ["reference", "device"])
@pytest.mark.parametrize("deliver", [dict(output_rate=44100), dict(output_rate=16000, level="input"),
                                     dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=5),
                                     dict(pcm="int16", interleaved=True)])
def test_a_clip_is_delivered_the_same_alone_in_a_batch_and_in_a_ragged_group(deliver, prior):
    """The stereo clip S alone = beside a second clip of its length in generate_batch = beside clips of other lengths and another
    input rate in generate_many, under both `ends` and without the ragged sequence.  Clip i of a call dithers with (seed, i):
    the run alone is given that pair."""
    m = model("hip", prior)
    (S, _), (M, _), (L_, _), (W, _) = clip("S"), clip("M"), clip("L"), clip("W")
    S2 = S[::-1] * np.float32(0.5)
    kw = dict(channels="first", **deliver)

    def at(i):             # the keywords of a run alone of clip i of a list
        return dict(kw, dither_seed=[(5, i)]) if "dither_seed" in kw else kw
    if prior == "reference":
        pr = lambda *names: dict(noise=[noise(n) for n in names])                       # noqa: E731
        one = lambda name, i: dict(noise=noise(name))                                   # noqa: E731
    else:
        pr = lambda *names: dict(seed=77)                                               # noqa: E731
        one = lambda name, i: dict(seed=[(77, i)])                                      # noqa: E731
    alone = m.generate(S, 12000, **one("S", 0), **at(0))
    batch = m.generate_batch([S, S2], 12000, **pr("S", "S"), **kw)
    assert torch.equal(batch[0], alone) and batch[1].shape == alone.shape and batch[1].dtype == alone.dtype
    mono = m.generate(M[None], 12000, **one("M", 2), **at(2))
    wide = m.generate(W[None], 16000, **one("W", 3), **at(3))
    for how in (dict(ends="per_clip"), dict(ends="ragged"), dict(ragged=False)):
        outs = m.generate_many([S, L_[None], M[None], W[None]], [12000, 12000, 12000, 16000], **pr("S", "L", "M", "W"), **how, **kw)
        assert torch.equal(outs[0], alone), how
        assert torch.equal(outs[2], mono), how
        assert torch.equal(outs[3], wide), how
        t = delivery.delivered_len(19200, deliver.get("output_rate"))
        assert tuple(outs[1].shape) == ((t, 1) if deliver.get("interleaved") else (1, t)), how
    assert alone.any() and mono.any() and wide.any()


def test_a_ragged_group_of_mono_clips_without_channels():
    """The default path's clips (no channels=): generate_many over two lengths, both ends, = generate per clip."""
    m = model()
    (M, _), (L_, _) = clip("M"), clip("L")
    kw = dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=9)
    a = m.generate(M, 12000, noise=noise("M"), **dict(kw, dither_seed=[(9, 0)]))
    b = m.generate(L_, 12000, noise=noise("L"), **dict(kw, dither_seed=[(9, 1)]))
    assert a.shape == (1, 14553) and b.shape == (1, 17640) and a.dtype == torch.int16
    for ends in ("per_clip", "ragged"):
        outs = m.generate_many([M, L_], 12000, noise=[noise("M"), noise("L")], ends=ends, **kw)
        assert torch.equal(outs[0], a) and torch.equal(outs[1], b), ends
    two = m.generate_batch([M, M * np.float32(0.5)], 12000, noise=torch.cat([noise("M"), noise("M")]), **kw)
    assert two.shape == (2, 14553) and torch.equal(two[:1], a)
    two = m.generate_batch([M, M], 12000, noise=torch.cat([noise("M"), noise("M")]), pcm="int16", interleaved=True)
    assert two.shape == (2, 15840, 1) and torch.equal(two[0], m.generate(M, 12000, noise=noise("M"), pcm="int16", interleaved=True))


def test_every_keyword_at_its_default_is_the_call_without_them():
    m = model()
    (M, _), (S, _), (L_, _) = clip("M"), clip("S"), clip("L")
    dflt = dict(output_rate=None, pcm=None, dither=None, dither_seed=0, interleaved=False)
    assert torch.equal(m.generate(M, 12000, noise=noise("M"), **dflt), m.generate(M, 12000, noise=noise("M")))
    assert torch.equal(m.generate(M, 12000, noise=noise("M"), **dict(dflt, output_rate=48000)), run48("M").cuda())
    assert torch.equal(m.generate(S, 12000, noise=noise("S"), channels="first", **dflt), run48("S").cuda())
    a = m.generate_many([M, L_], 12000, noise=[noise("M"), noise("L")], ends="ragged", **dflt)
    b = m.generate_many([M, L_], 12000, noise=[noise("M"), noise("L")], ends="ragged")
    assert all(torch.equal(p, q) and p.dtype == torch.float32 for p, q in zip(a, b))


def test_batching_server_delivers_what_the_model_does():
    from flowhigh_amd.serve import BatchingServer
    m = model()
    (M, _), (S, _) = clip("M"), clip("S")
    srv = BatchingServer(m, max_batch=4, max_wait_ms=5)
    try:
        torch.manual_seed(11)
        sr, y = srv.generate((12000, M), 44100, 1, pcm="int16")
        torch.manual_seed(11)
        want = m.generate_many([M], 12000, output_rate=44100, pcm="int16")[0]
        assert sr == 44100 and y.dtype == np.int16 and y.shape == (14553,) and np.array_equal(y, want[0].cpu().numpy())
        torch.manual_seed(12)
        sr, y = srv.generate((12000, np.ascontiguousarray(S.T)), 16000, 1, pcm="int16", dither="tpdf")
        torch.manual_seed(12)
        want = m.generate(S, 12000, channels="first", output_rate=16000, pcm="int16", dither="tpdf", interleaved=True)
        assert sr == 16000 and y.shape == (5280, 2) and np.array_equal(y, want.cpu().numpy())
    finally:
        srv.close()
