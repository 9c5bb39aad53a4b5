"""GPU: streaming delivery -- fh_stream_resample_f32, fh_stream_limit_f32 and fh_stream_pcm_i16_f32 (csrc/stream_delivery.hip)
through DeliveryStream against the one-shot entries on the whole stream, stage by stage and as a chain; streams pushed together
against themselves alone; what a launch may write; the C entries' argument checks; and FlowHighSR.stream(delivery=) /
generate_long(delivery=) on TINY_CFG at 12 kHz (window 200 ms, overlap 60 ms, guard 10 ms, a 0.75 s clip).

Everything compares this project with itself, or a kernel with its numpy definition: bitwise."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, pcm, synth, tables, truepeak       # noqa: E402
from flowhigh_amd import delivery_stream as DS                                          # noqa: E402
from flowhigh_amd import stream as S                                                    # noqa: E402
from flowhigh_amd import stream_delivery as SD                                          # noqa: E402
from flowhigh_amd.delivery import Delivery, delivered_len, resolve_delivery             # noqa: E402
from flowhigh_amd.frontend import Resampler, upload_tables                              # noqa: E402

T48 = 5000
CUTS = {"one": [T48], "odd": [1, 7, 300, 301, 1500, 2222, 4999, 5000], "every37": list(range(37, T48, 37)) + [T48]}
FULL = dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=9, true_peak=-1.0, limiter="lookahead")
SENTINEL = 0x7fc12345          # a NaN with a payload: an element that was written, by anything, loses these bits
SR = 12000
PLAN = dict(window_ms=200, overlap_ms=60, guard_ms=10)
SEED = 41 + (3 << 32)
E2E = dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=9, true_peak=-3.0, limiter="lookahead")
_STATE = {}


def delivery():
    if "delivery" not in _STATE:
        _STATE["delivery"] = Delivery("cuda", Resampler("cuda"))
    return _STATE["delivery"]


def noise(n=T48, seed=1, cuts=None):
    """Seeded noise at 0.9; cuts: one sample of 1.5 at the first and the last index and on each side of a cut."""
    x = (0.9 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)).astype(np.float32)
    if cuts is not None:
        c = cuts[len(cuts) // 2] if len(cuts) > 1 else n // 2
        for i in (0, n - 1, c - 1, c):
            x[i] = 1.5
    return torch.from_numpy(x).cuda()


def stream_of(**kw):
    return DS.DeliveryStream(DS.resolve(kw))


def pushed(ds, x, cuts):
    """x [T] pushed in the blocks the cuts make, then flushed -> the blocks' concatenation [1, n]."""
    outs, prev = [], 0
    for c in cuts:
        outs.append(DS.push(delivery(), [ds], [x[None, prev:c]])[0])
        prev = c
    outs.append(DS.push(delivery(), [ds], [None], final=True)[0])
    assert ds.closed and all(o.ndim == 2 and o.shape[0] == 1 and o.is_cuda for o in outs)
    return torch.cat(outs, 1)


def one_shot(x, **kw):
    """Delivery.batch of the whole stream at level='input': [1, n]."""
    return delivery().batch(x[None], [1], "input", resolve_delivery(1, level="input", **kw), [0])[0]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---- the stages ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", sorted(CUTS))
@pytest.mark.parametrize("rate", [44100, 16000, 96000])
def test_resampler_alone(rate, cuts):
    x = noise()
    taps, n_taps, pre, up, down = delivery().resampler._filter(rate, 48000)
    n = tables.resample_out_len(T48, rate, 48000)
    want = torch.empty(1, n, dtype=torch.float32, device="cuda")
    hip.check(hip.lib().fh_resample_poly_f32(x.data_ptr(), taps, want.data_ptr(), 1, T48, n, up, down, n_taps, pre, hip.stream()), "resample")
    ds = stream_of(output_rate=rate)
    got = pushed(ds, x, CUTS[cuts])
    assert got.dtype == torch.float32 and got.shape == (1, delivered_len(T48, rate)) and same_bits(got, want)
    with pytest.raises(RuntimeError):
        DS.push(delivery(), [ds], [x[None, :10]])


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_limiter_alone_at_48000(cuts):
    x = noise(seed=2, cuts=CUTS[cuts])
    D, L = delivery(), hip.lib()
    H, c32 = truepeak.half_window(48000), float(np.float32(truepeak.ceiling(-6.0)))
    m, want = torch.empty(1, T48, dtype=torch.float32, device="cuda"), torch.empty(1, T48, dtype=torch.float32, device="cuda")
    hip.check(L.fh_tp_envelope_f32(x.data_ptr(), D._tp_taps(), m.data_ptr(), 1, 1, T48, hip.stream()), "envelope")
    hip.check(L.fh_limit_f32(x.data_ptr(), want.data_ptr(), m.data_ptr(), D._window(H), 0, 1, 1, T48, H, c32, hip.stream()), "limit")
    got = pushed(stream_of(true_peak=-6.0, limiter="lookahead"), x, CUTS[cuts])
    assert same_bits(got, want)
    assert float(m.max()) > 1.4 and float(want.abs().max()) <= c32 and not same_bits(want, x[None])      # the limiter works
    assert same_bits(got, one_shot(x, true_peak=-6.0, limiter="lookahead"))


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_limiter_at_8000_through_the_chain(cuts):
    x = noise(seed=3, cuts=CUTS[cuts])
    kw = dict(output_rate=8000, true_peak=-6.0, limiter="lookahead")
    got = pushed(stream_of(**kw), x, CUTS[cuts])
    assert got.shape == (1, delivered_len(T48, 8000)) and same_bits(got, one_shot(x, **kw))


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_encoder_with_dither(cuts):
    x = noise(seed=4)
    key = torch.from_numpy(np.array([[77, 0]], dtype=np.uint64).view(np.int64)).cuda()
    want = torch.empty(1, T48, dtype=torch.int16, device="cuda")
    hip.check(hip.lib().fh_pcm_i16_f32(x.data_ptr(), want.data_ptr(), key.data_ptr(), 1, 1, T48, 0, hip.stream()), "pcm")
    got = pushed(stream_of(pcm="int16", dither="tpdf", dither_seed=77), x, CUTS[cuts])
    assert got.dtype == torch.int16 and torch.equal(got, want)
    assert np.array_equal(got[0].cpu().numpy(), pcm.encode(x.cpu().numpy(), (77, 0))[0])
    plain = pushed(stream_of(pcm="int16"), x, CUTS[cuts])                # keys NULL: no dither
    assert np.array_equal(plain[0].cpu().numpy(), pcm.encode(x.cpu().numpy())[0]) and not torch.equal(plain, got)


def test_dither_at_indices_past_32_bits():
    first = 2 ** 33 + 5
    x = noise(1000, seed=5)
    ds = stream_of(pcm="int16", dither="tpdf", dither_seed=77)
    ds.stages["encode"].counters = SD.EncodeStage(first)                 # the stream has been running for a while
    got = pushed(ds, x, [1, 7, 300, 301, 1000])
    d = pcm.tpdf_dither(77, 0, 0, 1000, first=first)
    assert np.array_equal(got[0].cpu().numpy(), pcm.quantize(x.cpu().numpy(), d))
    low = pcm.quantize(x.cpu().numpy(), pcm.tpdf_dither(77, 0, 0, 1000, first=5))
    assert not np.array_equal(got[0].cpu().numpy(), low)                 # (the high word counts)


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_full_chain(cuts):
    x = noise(seed=6, cuts=CUTS[cuts])
    got = pushed(stream_of(**FULL), x, CUTS[cuts])
    want = one_shot(x, **FULL)
    assert got.dtype == torch.int16 and got.shape == (1, delivered_len(T48, 44100)) and torch.equal(got, want)


def test_streams_pushed_together_are_the_streams_alone():
    """Three streams of one plan with other lengths and cuts, and one of another plan, in the same pushes; a stream whose blocks
    have run out gets zero-length blocks (or None) until all end."""
    specs = [(5000, [1, 7, 300, 301, 1500, 2222, 4999, 5000], FULL), (3333, [1200, 1200, 3333], FULL),
             (4100, list(range(500, 4100, 500)) + [4100], FULL), (2000, [2000], dict(output_rate=16000))]
    xs = [noise(n, seed=10 + i, cuts=c) for i, (n, c, _) in enumerate(specs)]
    alone = [pushed(stream_of(**kw), x, c) for x, (_, c, kw) in zip(xs, specs)]
    streams = [stream_of(**kw) for _, _, kw in specs]
    outs = [[] for _ in specs]
    for r in range(max(len(c) for _, c, _ in specs)):
        blocks = []
        for x, (_, c, _) in zip(xs, specs):
            a, b = (c[r - 1] if r else 0, c[r]) if r < len(c) else (0, 0)
            blocks.append(x[None, a:b] if r < len(c) or r % 2 else None)
        for o, y in zip(outs, DS.push(delivery(), streams, blocks)):
            o.append(y)
    for o, y in zip(outs, DS.push(delivery(), streams, [None] * len(streams), final=True)):
        o.append(y)
    for o, want in zip(outs, alone):
        assert same_bits(torch.cat(o, 1), want)
    assert specs[1][1][0] == specs[1][1][1]                               # (the second stream's second block is empty)
    with pytest.raises(ValueError):
        DS.push(delivery(), [stream_of(**FULL)] * 2, [None, None])


# ---- what a launch may write -----------------------------------------------------------------------------------------------
PAD = 64


def sentinel_buffer(n, dtype=torch.float32):
    """n elements holding the sentinel's bits (an int16 buffer: its two halves in turn)."""
    per = 4 // torch.empty(0, dtype=dtype).element_size()
    return torch.full((-(-n // per),), SENTINEL, dtype=torch.int32).cuda().view(dtype)[:n]


def untouched(buf, a=0, b=0):
    """Every element of a sentinel buffer outside [a, b) still has its bits."""
    ints = torch.int32 if buf.dtype == torch.float32 else buf.dtype
    same = buf.view(ints) == sentinel_buffer(buf.numel(), buf.dtype).view(ints)
    same[a:b] = True
    return bool(same.all())


def launch(entry, jobs, max_out):
    D, L = delivery(), hip.lib()
    keep, (jp,) = upload_tables([(hip.StreamJob * len(jobs))(*jobs)], torch.device("cuda"))
    if entry == "resample":
        taps, n_taps, pre, up, down = D.resampler._filter(44100, 48000)
        rc = L.fh_stream_resample_f32(jp, len(jobs), max_out, taps, up, down, n_taps, pre, hip.stream())
    elif entry == "limit":
        rc = L.fh_stream_limit_f32(jp, len(jobs), max_out, D._tp_taps(), D._window(240), 240, 0.5, hip.stream())
    else:
        rc = L.fh_stream_pcm_i16_f32(jp, len(jobs), max_out, 0, hip.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("entry", ["resample", "limit", "encode"])
def test_nothing_past_the_end_is_written(entry):
    """One consistent job and three that are not, in one launch: dst and carry_out are over-allocated sentinel buffers; the good
    job writes dst[0 .. n_out) and carry_out[0 .. n_keep) only, the others at the most their own dst[0 .. n_out).  Every pointer and
    every count of every job stays inside a live allocation, so a guard that is missing shows as a lost sentinel, not as a fault."""
    n_carry, n_fresh, n_out, n_keep = 700, 1500, 1200, 600
    carry, fresh = noise(n_carry, seed=20), noise(n_fresh, seed=21)
    odt = torch.int16 if entry == "encode" else torch.float32
    esz = 2 if entry == "encode" else 4
    base = 40000
    # the first output whose inputs the spans hold
    first = {"resample": SD.ResampleFilter(44100).n_final(base + 300), "limit": base + 2 * 240 + 10, "encode": base}[entry]
    too_many = n_carry + n_fresh + 1                                     # more than the source holds
    dsts = [sentinel_buffer(PAD + n_out + PAD + 3, odt) for _ in range(4)]
    keeps = [sentinel_buffer(PAD + too_many + PAD) for _ in range(4)]    # (room for what the refused job asks for)

    def job(k, **kw):
        f = dict(carry=carry.data_ptr(), fresh=fresh.data_ptr(), dst=dsts[k].data_ptr() + esz * (PAD + 1), carry_out=keeps[k].data_ptr() + 4 * PAD,
                 base=base, first=first, n_carry=n_carry, n_fresh=n_fresh, n_out=n_out, n_keep=n_keep, ended=0, pad_=0)
        f.update(kw)
        return hip.StreamJob(**f)
    jobs = [job(0),
            job(1, first=0),                                             # outputs whose inputs lie far below `base`
            job(2, n_out=-5), job(3, n_keep=too_many)]                   # a negative count; more to keep than there is
    assert launch(entry, jobs, n_out) == 0
    a, b = PAD + 1, PAD + 1 + n_out
    assert untouched(dsts[0], a, b) and not untouched(dsts[0])           # the good job wrote, and only there
    assert untouched(dsts[1], a, b)                                      # the inconsistent one: at the most its own outputs
    assert untouched(dsts[2]) and untouched(dsts[3])
    if entry == "encode":                                                # (the encoder keeps nothing)
        assert all(untouched(k) for k in keeps)
        return
    src = torch.cat([carry, fresh])
    assert untouched(keeps[0], PAD, PAD + n_keep) and untouched(keeps[1], PAD, PAD + n_keep)
    assert same_bits(keeps[0][PAD:PAD + n_keep], src[-n_keep:]) and same_bits(keeps[1][PAD:PAD + n_keep], src[-n_keep:])
    assert untouched(keeps[2]) and untouched(keeps[3])


def test_argument_errors_write_nothing():
    D, L, st = delivery(), hip.lib(), hip.stream()
    dst = sentinel_buffer(4096)
    src = noise(2048, seed=22)
    jobs = [hip.StreamJob(0, src.data_ptr(), dst.data_ptr(), 0, 0, 0, 0, 2048, 1024, 0, 0, 0)]
    keep, (jp,) = upload_tables([(hip.StreamJob * 1)(*jobs)], torch.device("cuda"))
    taps, n_taps, pre, up, down = D.resampler._filter(44100, 48000)
    t4, w = D._tp_taps(), D._window(240)
    bad = {"fh_stream_resample_f32": [(0, 1, 1024, taps, up, down, n_taps, pre, st), (jp, 0, 1024, taps, up, down, n_taps, pre, st),
                                      (jp, 1, 1024, 0, up, down, n_taps, pre, st), (jp, 1, 1024, taps, 0, down, n_taps, pre, st),
                                      (jp, 1, 1024, taps, up, 0, n_taps, pre, st), (jp, 1, 1024, taps, up, down, 0, pre, st),
                                      (jp, 65536, 1024, taps, up, down, n_taps, pre, st), (jp, 1, -1, taps, up, down, n_taps, pre, st)],
           "fh_stream_limit_f32": [(0, 1, 1024, t4, w, 240, 0.5, st), (jp, 0, 1024, t4, w, 240, 0.5, st), (jp, 1, 1024, 0, w, 240, 0.5, st),
                                   (jp, 1, 1024, t4, 0, 240, 0.5, st), (jp, 1, 1024, t4, w, 513, 0.5, st), (jp, 1, 1024, t4, w, 0, 0.5, st),
                                   (jp, 1, 1024, t4, w, 240, 0.0, st), (jp, 1, 1024, t4, w, 240, 1.5, st)],
           "fh_stream_pcm_i16_f32": [(0, 1, 1024, 0, st), (jp, 0, 1024, 0, st), (jp, 1, -1, 0, st)]}
    for name, calls in bad.items():
        for args in calls:
            assert getattr(L, name)(*args) == -1, (name, args)
            assert name.encode() in L.fh_last_error()
    torch.cuda.synchronize()
    assert untouched(dst)
    assert L.fh_sizeof_stream_job() == ctypes.sizeof(hip.StreamJob) == 72


# ---- sessions --------------------------------------------------------------------------------------------------------------
def model():
    if "model" not in _STATE:
        fh = FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda")
        _STATE["model"] = FlowHighSR(fh, prior="device", torchdiffeq_ode_method="euler")
    return _STATE["model"]


def clip(seconds=0.75, i=0):
    return synth.lowres_clip(400 + i, seconds, SR)


def long_float(i=0, seconds=0.75):
    """generate_long without delivery, once per session: float32 [1, T48]."""
    if ("long", i) not in _STATE:
        _STATE["long", i] = model().generate_long(clip(seconds, i), SR, seed=SEED + i, **PLAN).clone()
    return _STATE["long", i]


def delivered(i=0, seconds=0.75):
    """The one-shot delivery of long_float at level='input'."""
    if ("delivered", i) not in _STATE:
        m = model()
        opt = resolve_delivery(1, level="input", **E2E)
        _STATE["delivered", i] = m.delivery.batch(long_float(i, seconds), [1], "input", opt, [0])[0].clone()
    return _STATE["delivered", i]


def test_generate_long_with_delivery_is_the_delivery_of_generate_long():
    m, x = model(), clip()
    got = m.generate_long(x, SR, seed=SEED, delivery=E2E, **PLAN)
    want = delivered()
    T48 = long_float().shape[1]
    assert T48 == S.StreamPlan(SR, **PLAN).out_len(len(x))
    assert got.dtype == torch.int16 and got.is_cuda and got.shape == (1, delivered_len(T48, 44100)) and torch.equal(got, want)


def test_a_session_pushed_in_blocks_delivers_the_same():
    m, x = model(), clip()
    s = m.stream(SR, seed=SEED, delivery=E2E, **PLAN)
    outs = [s.push(x[a:a + 2400]) for a in range(0, len(x), 2400)] + [s.flush()]
    assert all(o.dtype == torch.int16 and o.shape[0] == 1 and o.is_cuda for o in outs)
    assert torch.equal(torch.cat(outs, 1), delivered())
    with pytest.raises(RuntimeError):
        s.push(x[:10])
    # the float delivery too: 44.1 kHz under the ceiling, no encoder
    kw = dict(output_rate=44100, true_peak=-3.0, limiter="lookahead")
    got = m.generate_long(x, SR, seed=SEED, delivery=kw, **PLAN)
    want = m.delivery.batch(long_float(), [1], "input", resolve_delivery(1, level="input", **kw), [0])[0]
    assert got.dtype == torch.float32 and same_bits(got, want)


def test_two_sessions_in_one_push_deliver_their_own():
    m = model()
    xs = [clip(), clip(0.6, 1)]
    sessions = [m.stream(SR, seed=SEED + i, delivery=E2E, **PLAN) for i in range(2)]
    outs = [[], []]
    for a in range(0, max(len(x) for x in xs), 4200):
        for o, y in zip(outs, m.stream_push(sessions, [x[a:a + 4200] for x in xs])):
            o.append(y)
    for o, s in zip(outs, sessions):
        o.append(s.flush())
    assert torch.equal(torch.cat(outs[0], 1), delivered()) and torch.equal(torch.cat(outs[1], 1), delivered(1, 0.6))


def test_a_session_without_delivery_is_todays():
    """stream.stitch of the windows through generate(level='input') with the session's prior at the window's first frame."""
    m, p, x = model(), S.StreamPlan(SR, **PLAN), clip()
    wins = []
    for i, (a, b) in enumerate(p.spans(len(x))):
        z = m.draw_prior(S.resample_out_len(b - a, 48000, SR) // 480, SEED, stream=0, first_frame=p.first_frame(i))
        wins.append(m.generate(x[a:b], SR, level="input", noise=z)[0].cpu().numpy().copy())
    want = S.stitch(wins, p)
    assert np.array_equal(long_float()[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    s = m.stream(SR, seed=SEED, delivery=dict(output_rate=48000, pcm=None), **PLAN)          # every value a default
    assert s.delivery is None
    got = torch.cat([s.push(x[a:a + 2400]) for a in range(0, len(x), 2400)] + [s.flush()], 1)
    assert same_bits(got, long_float())
