"""GPU: streams of channels -- fh_stream_limit_linked_f32 and fh_stream_pcm_i16_rows_f32 (csrc/stream_delivery.hip) through
DeliveryStream(n_channels=) against the one-shot entries on the whole [C, T] stream, stage by stage and as a chain; streams of
different channel counts pushed together against themselves alone; what a launch may write and which groups it refuses; the C
entries' argument checks; and FlowHighSR.stream(n_channels=) / generate_long(n_channels=) on TINY_CFG at 12 kHz (window 200 ms,
overlap 60 ms, guard 10 ms, a 0.75 s clip).

Everything compares this project with itself, or a kernel with its numpy definition: bitwise."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, pcm, synth, truepeak                # noqa: E402
from flowhigh_amd import delivery_stream as DS                                          # noqa: E402
from flowhigh_amd import stream as S                                                    # noqa: E402
from flowhigh_amd import stream_delivery as SD                                          # noqa: E402
from flowhigh_amd.delivery import Delivery, delivered_len, resolve_delivery             # noqa: E402
from flowhigh_amd.frontend import Resampler, upload_tables                              # noqa: E402

T48 = 5000
CUTS = {"one": [T48], "odd": [1, 7, 300, 301, 1500, 2222, 4999, 5000], "every37": list(range(37, T48, 37)) + [T48]}
CHANNELS = [1, 2, 3, 8]
LIMIT = dict(true_peak=-1.0, limiter="lookahead")       # 0.89: over the quiet rows' true peak, far under the spikes of 1.5
FULL = dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=9, true_peak=-1.0, limiter="lookahead")
SENTINEL = 0x7fc12345          # a NaN with a payload: an element that was written, by anything, loses these bits
SR = 12000
PLAN = dict(window_ms=200, overlap_ms=60, guard_ms=10)
SEED = 41 + (3 << 32)
E2E = dict(output_rate=44100, pcm="int16", dither="tpdf", dither_seed=9, true_peak=-3.0, limiter="lookahead", interleaved=True)
_STATE = {}


def delivery():
    if "delivery" not in _STATE:
        _STATE["delivery"] = Delivery("cuda", Resampler("cuda"))
    return _STATE["delivery"]


def linked_clip(C, cuts, n=T48, seed=1):
    """[C, n] on the device: channel 0 is 0.3 noise with one sample of 1.5 at the first and the last index and on each side of
    a cut; the other channels are 0.3 noise."""
    x = (0.3 * np.random.default_rng(seed).uniform(-1.0, 1.0, (C, n))).astype(np.float32)
    c = cuts[len(cuts) // 2] if len(cuts) > 1 else n // 2
    for i in (0, n - 1, c - 1, c):
        x[0, i] = 1.5
    return torch.from_numpy(x).cuda()


def stream_of(n_channels=None, **kw):
    return DS.DeliveryStream(DS.resolve(kw, None, n_channels))


def pushed(ds, x, cuts):
    """x [C, T] pushed in the blocks the cuts make, then flushed -> the blocks' concatenation, [C, n] or frames [n, C]."""
    outs, prev = [], 0
    for c in cuts:
        outs.append(DS.push(delivery(), [ds], [x[:, prev:c]])[0])
        prev = c
    outs.append(DS.push(delivery(), [ds], [None], final=True)[0])
    rows = ds.rows
    if ds.interleaved:
        assert ds.closed and all(o.ndim == 2 and o.shape[1] == rows and o.is_cuda and o.is_contiguous() for o in outs)
        return torch.cat(outs, 0)
    assert ds.closed and all(o.ndim == 2 and o.shape[0] == rows and o.is_cuda and o.is_contiguous() for o in outs)
    return torch.cat(outs, 1)


def one_shot(x, **kw):
    """Delivery.batch of the whole stream [C, T] as one clip at level='input': [C, n], or [n, C] interleaved."""
    return delivery().batch(x, [x.shape[0]], "input", resolve_delivery(1, level="input", **kw), [0])[0]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---- the stages ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", sorted(CUTS))
@pytest.mark.parametrize("C", CHANNELS)
def test_linked_limiter_alone_at_48000(C, cuts):
    """H = 240: five 1024-tiles in 5000 samples, blocks shorter than 2 H + 10."""
    x = linked_clip(C, CUTS[cuts])
    D, L = delivery(), hip.lib()
    H, c32 = truepeak.half_window(48000), float(np.float32(truepeak.ceiling(LIMIT["true_peak"])))
    m, want = torch.empty(1, T48, dtype=torch.float32, device="cuda"), torch.empty(C, T48, dtype=torch.float32, device="cuda")
    hip.check(L.fh_tp_envelope_f32(x.data_ptr(), D._tp_taps(), m.data_ptr(), 1, C, T48, hip.stream()), "envelope")
    hip.check(L.fh_limit_f32(x.data_ptr(), want.data_ptr(), m.data_ptr(), D._window(H), 0, 1, C, T48, H, c32, hip.stream()), "limit")
    got = pushed(stream_of(C, **LIMIT), x, CUTS[cuts])
    assert same_bits(got, want) and same_bits(got, one_shot(x, **LIMIT))
    assert float(m.max()) > 1.4 and float(want.abs().max()) <= c32 and not same_bits(want[0], x[0])      # the limiter works
    if C == 1:
        mono = pushed(stream_of(**LIMIT), x, CUTS[cuts])                  # the stream opened without n_channels: fh_stream_limit_f32
        assert same_bits(got, mono)
        return
    # the quiet channels move with channel 0 (every one near every spike); limited without it they come back as they went in
    c = CUTS[cuts][len(CUTS[cuts]) // 2] if len(CUTS[cuts]) > 1 else T48 // 2
    for i in (0, T48 - 1, c - 1, c):
        near = slice(max(0, i - 100), i + 100)
        assert all(not same_bits(got[r, near], x[r, near]) for r in range(1, C))
    assert same_bits(one_shot(x[1:], **LIMIT), x[1:])


@pytest.mark.parametrize("C", [1, 2])
def test_non_finite_samples_give_the_same_bits_in_every_limiter(C):
    """A NaN at 700 and a +Inf at 2300 of the last channel of [C, 3000] (three tiles; H = 240, so they are further apart than
    4 H + 20 and do not interact).  A NaN peak folds to m = 0 in the envelope (fmaxf(0, NaN)), which the limiter of a stream of
    channels does too; both give r = 1 there, as a compare of the NaN itself with the ceiling does.  The stream without
    n_channels, the stream with n_channels=C and fh_tp_envelope_f32 + fh_limit_f32 on the whole rows: the same bits."""
    n, cuts = 3000, [1, 7, 300, 301, 1500, 2222, 2999, 3000]
    host = (0.3 * np.random.default_rng(30).uniform(-1.0, 1.0, (C, n))).astype(np.float32)
    host[C - 1, 700], host[C - 1, 2300] = np.nan, np.inf
    x = torch.from_numpy(host).cuda()
    D, L = delivery(), hip.lib()
    H, c32 = truepeak.half_window(48000), float(np.float32(truepeak.ceiling(LIMIT["true_peak"])))
    assert H == 240
    m, want = torch.empty(1, n, dtype=torch.float32, device="cuda"), torch.empty(C, n, dtype=torch.float32, device="cuda")
    hip.check(L.fh_tp_envelope_f32(x.data_ptr(), D._tp_taps(), m.data_ptr(), 1, C, n, hip.stream()), "envelope")
    hip.check(L.fh_limit_f32(x.data_ptr(), want.data_ptr(), m.data_ptr(), D._window(H), 0, 1, C, n, H, c32, hip.stream()), "limit")
    # the NaN does not reach m (what is left at 700 is the other channel's peak, 0 where there is none); the Inf does
    assert bool(torch.isfinite(m[0, 700])) and (C > 1 or float(m[0, 700]) == 0.0) and float(m[0, 2300]) == float("inf")
    assert not same_bits(want[0, 2100:2290], x[0, 2100:2290])            # the gain comes down before the Inf, in every channel
    assert same_bits(pushed(stream_of(C, **LIMIT), x, cuts), want)
    if C == 1:
        assert same_bits(pushed(stream_of(**LIMIT), x, cuts), want)


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_linked_limiter_at_8000_through_the_chain(cuts):
    x = linked_clip(2, CUTS[cuts], seed=3)
    kw = dict(output_rate=8000, true_peak=-6.0, limiter="lookahead")
    got = pushed(stream_of(2, **kw), x, CUTS[cuts])
    assert got.shape == (2, delivered_len(T48, 8000)) and same_bits(got, one_shot(x, **kw))


@pytest.mark.parametrize("C", CHANNELS)
def test_encoder_of_rows(C):
    x = linked_clip(C, CUTS["odd"], seed=4)
    key = torch.from_numpy(np.array([[77, 0]], dtype=np.uint64).view(np.int64)).cuda()
    host = x.cpu().numpy()
    for frames in (False, True):
        for dither in (True, False):
            want = torch.empty((T48, C) if frames else (C, T48), dtype=torch.int16, device="cuda")
            hip.check(hip.lib().fh_pcm_i16_f32(x.data_ptr(), want.data_ptr(), key.data_ptr() if dither else 0, 1, C, T48, int(frames),
                                               hip.stream()), "pcm")
            kw = dict(pcm="int16", interleaved=frames, **(dict(dither="tpdf", dither_seed=77) if dither else {}))
            for cuts in sorted(CUTS):
                got = pushed(stream_of(C, **kw), x, CUTS[cuts])
                assert got.dtype == torch.int16 and got.shape == want.shape and torch.equal(got, want), (frames, dither, cuts)
            assert np.array_equal(got.cpu().numpy(), pcm.encode(host, (77, 0) if dither else None, frames))
    if C == 1:                                                            # planar, one row: the mono stream's bits
        kw = dict(pcm="int16", dither="tpdf", dither_seed=77)
        assert torch.equal(pushed(stream_of(1, **kw), x, CUTS["odd"]), pushed(stream_of(**kw), x, CUTS["odd"]))


def rows_jobs(src, dsts, n_out, first=0):
    """One job per row of src [C, n]: nothing carried, the row fresh, dsts[c] its destination."""
    return [hip.StreamJob(0, src[c].data_ptr(), dsts[c], 0, first, first, 0, src.shape[1], n_out, 0, 0, 0) for c in range(src.shape[0])]


def launch_rows(jobs, groups, max_out, keys=0, frames=0):
    keep, (jp, gp) = upload_tables([(hip.StreamJob * len(jobs))(*jobs), np.asarray(groups, dtype=np.int32)], torch.device("cuda"))
    rc = hip.lib().fh_stream_pcm_i16_rows_f32(jp, len(jobs), gp, len(groups) - 1, max_out, keys, frames, hip.stream())
    torch.cuda.synchronize()
    return rc


def test_frames_at_an_address_that_is_no_multiple_of_a_frame():
    """C = 2 interleaved into a dst that is 2 mod 4: 2-byte stores, the values of the 4-byte ones."""
    n = 1003
    x = linked_clip(2, [n], n, seed=5)
    key = torch.from_numpy(np.array([[77, 0]], dtype=np.uint64).view(np.int64)).cuda()
    want = torch.empty(n, 2, dtype=torch.int16, device="cuda")
    hip.check(hip.lib().fh_pcm_i16_f32(x.data_ptr(), want.data_ptr(), key.data_ptr(), 1, 2, n, 1, hip.stream()), "pcm")
    for shift in (0, 1):                                                  # elements: dst 0 mod 4 (whole frames), then 2 mod 4
        buf = sentinel_buffer(2 * n + 8, torch.int16)
        dst = buf.data_ptr() + 2 * (2 + shift)
        assert dst % 4 == 2 * shift
        assert launch_rows(rows_jobs(x, [dst, dst], n), [0, 2], n, key.data_ptr(), 1) == 0
        assert torch.equal(buf[2 + shift:2 + shift + 2 * n].view(n, 2), want) and untouched(buf, 2 + shift, 2 + shift + 2 * n)


def test_dither_at_indices_past_32_bits():
    first = 2 ** 33 + 5
    x = linked_clip(2, [1000], 1000, seed=5)
    host = x.cpu().numpy()
    d = np.stack([pcm.tpdf_dither(77, 0, c, 1000, first=first) for c in range(2)])
    for frames in (False, True):
        ds = stream_of(2, pcm="int16", dither="tpdf", dither_seed=77, interleaved=frames)
        ds.stages["encode"].counters = SD.EncodeStage(first)             # the stream has been running for a while
        got = pushed(ds, x, [1, 7, 300, 301, 1000]).cpu().numpy()
        got = got.T if frames else got
        assert np.array_equal(got, pcm.quantize(host, d))
        low = np.stack([pcm.tpdf_dither(77, 0, c, 1000, first=5) for c in range(2)])
        assert not np.array_equal(got[1], pcm.quantize(host[1], low[1]))  # (the high word counts)


BLOCK_CUTS = (0, 1, 9, 24, 41)


@pytest.mark.parametrize("first", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("C", CHANNELS)
def test_int16_blocks_add_up_to_the_batched_entry(C, first):
    """A clip [C, 41] encoded in the blocks the cuts 0, 1, 9, 24, 41 make, each a launch of the rows entry (planar, and in frames)
    or, for C = 1, of the mono entry, `first` running on from 0 and from past 2^32: the blocks side by side are pcm.py's
    encoding under the dither from `first` on, and from 0 fh_pcm_i16_f32's of the whole clip.  Nothing else is written."""
    L, T, key, lo = hip.lib(), BLOCK_CUTS[-1], (77, 5), 8
    host = np.random.default_rng(70 + C).uniform(-1.05, 1.05, (C, T)).astype(np.float32)
    host[:, ::3] *= np.float32(2.0 ** -13)                               # a few LSB: the dither decides
    x = torch.from_numpy(host).cuda()
    kd = torch.from_numpy(np.array([key], dtype=np.uint64).view(np.int64)).cuda()
    want = pcm.quantize(host, np.stack([pcm.tpdf_dither(key[0], key[1], c, T, first=first) for c in range(C)]))
    for entry, frames in [("rows", 0), ("rows", 1)] + ([("mono", 0)] if C == 1 else []):
        buf = sentinel_buffer(C * T + 2 * lo, torch.int16)
        y0 = buf.data_ptr() + 2 * lo
        for a, b in zip(BLOCK_CUTS, BLOCK_CUTS[1:]):
            n = b - a
            dsts = [y0 + 2 * a * C] * C if frames else [y0 + 2 * (c * T + a) for c in range(C)]
            jobs = [hip.StreamJob(0, x[c, a:].data_ptr(), dsts[c], 0, first + a, first + a, 0, n, n, 0, 0, 0) for c in range(C)]
            if entry == "rows":
                assert launch_rows(jobs, [0, C], n, kd.data_ptr(), frames) == 0
            else:
                keep, (jp,) = upload_tables([(hip.StreamJob * 1)(*jobs)], torch.device("cuda"))
                hip.check(L.fh_stream_pcm_i16_f32(jp, 1, n, kd.data_ptr(), hip.stream()), "fh_stream_pcm_i16_f32")
                torch.cuda.synchronize()
        got = buf[lo:lo + C * T]
        blocks = got.cpu().numpy()
        assert np.array_equal(blocks.reshape(T, C).T if frames else blocks.reshape(C, T), want), (entry, frames)
        assert untouched(buf, lo, lo + C * T), (entry, frames)
        if first == 0:
            whole = torch.empty(C * T, dtype=torch.int16, device="cuda")
            hip.check(L.fh_pcm_i16_f32(x.data_ptr(), whole.data_ptr(), kd.data_ptr(), 1, C, T, frames, hip.stream()), "fh_pcm_i16_f32")
            assert torch.equal(whole, got), (entry, frames)


@pytest.mark.parametrize("C", [2, 4, 8])
def test_whole_frames_and_scattered_frames_agree(C):
    """Interleaved C = 2, 4, 8 from the segment entry and from the rows entry, the destination on a frame boundary (whole-frame
    stores) and one int16 past it (2-byte stores): both pcm.py's frames, dithered, the neighbours intact."""
    L, key, lo = hip.lib(), (77, 0), 16
    kd = torch.from_numpy(np.array([key], dtype=np.uint64).view(np.int64)).cuda()
    for T in (7, 9, 257):
        host = np.random.default_rng(80 + C + T).uniform(-1.05, 1.05, (C, T)).astype(np.float32)
        host[:, ::3] *= np.float32(2.0 ** -13)
        x = torch.from_numpy(host).cuda()
        want = torch.from_numpy(np.ascontiguousarray(pcm.encode(host, key, True)).reshape(-1))
        for entry in ("seg", "rows"):
            for shift in (0, 1):
                buf = sentinel_buffer(C * T + 2 * lo, torch.int16)
                at = lo + shift
                dst = buf.data_ptr() + 2 * at
                assert dst % (2 * C) == 2 * shift
                if entry == "seg":
                    keep, (clips,) = upload_tables([(hip.PcmClip * 1)(hip.PcmClip(x.data_ptr(), dst, T, C, T))], torch.device("cuda"))
                    hip.check(L.fh_pcm_i16_seg_f32(clips, 1, C, T, kd.data_ptr(), 1, hip.stream()), "fh_pcm_i16_seg_f32")
                    torch.cuda.synchronize()
                else:
                    assert launch_rows(rows_jobs(x, [dst] * C, T), [0, C], T, kd.data_ptr(), 1) == 0
                assert torch.equal(buf[at:at + C * T].cpu(), want), (T, entry, shift)
                assert untouched(buf, at, at + C * T), (T, entry, shift)


@pytest.mark.parametrize("cuts", sorted(CUTS))
def test_full_chain_in_frames(cuts):
    x = linked_clip(2, CUTS[cuts], seed=6)
    got = pushed(stream_of(2, interleaved=True, **FULL), x, CUTS[cuts])
    want = one_shot(x, interleaved=True, **FULL)
    assert got.dtype == torch.int16 and got.shape == (delivered_len(T48, 44100), 2) and torch.equal(got, want)


def test_streams_pushed_together_are_the_streams_alone():
    """Streams of 1, 2 and 3 channels of one plan, with other lengths and cuts, a stereo stream in frames and a stereo stream of
    another plan, in the same pushes; a stream whose blocks have run out gets zero-length blocks (or None) until all end."""
    frames = dict(FULL, interleaved=True)
    specs = [(1, 5000, [1, 7, 300, 301, 1500, 2222, 4999, 5000], FULL), (2, 3333, [1200, 1200, 3333], FULL),
             (3, 4100, list(range(500, 4100, 500)) + [4100], FULL), (2, 2500, [100, 1300, 2500], frames), (2, 2000, [2000], dict(output_rate=16000))]
    xs = [linked_clip(C, c, n, seed=10 + i) for i, (C, n, c, _) in enumerate(specs)]
    alone = [pushed(stream_of(C, **kw), x, c) for x, (C, _, c, kw) in zip(xs, specs)]
    streams = [stream_of(C, **kw) for C, _, _, kw in specs]
    assert streams[0].key == streams[1].key == streams[2].key and len({s.key for s in streams}) == 3
    outs = [[] for _ in specs]
    for r in range(max(len(c) for _, _, c, _ in specs)):
        blocks = []
        for x, (_, _, c, _) in zip(xs, specs):
            a, b = (c[r - 1] if r else 0, c[r]) if r < len(c) else (0, 0)
            blocks.append(x[:, a:b] if r < len(c) or r % 2 else None)
        for o, y in zip(outs, DS.push(delivery(), streams, blocks)):
            o.append(y)
    for o, y in zip(outs, DS.push(delivery(), streams, [None] * len(streams), final=True)):
        o.append(y)
    for o, want, s in zip(outs, alone, streams):
        assert same_bits(torch.cat(o, 0 if s.interleaved else 1), want)
    # a block of another row count is refused before any stream moves
    a, b = stream_of(2, **FULL), stream_of(3, **FULL)
    with pytest.raises(ValueError, match=r"\[3, n\]"):
        DS.push(delivery(), [a, b], [xs[1][:, :10], xs[1][:, :10]])
    assert a.stages["resample"].counters.arrived == 0 and not a.closed


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


@pytest.mark.parametrize("entry", ["limit", "encode", "frames"])
def test_nothing_past_the_end_is_written_and_bad_groups_are_left_alone(entry):
    """One consistent stereo group, and an empty group, a group of 9, a group whose second job has another n_out and a group
    whose job has a negative count, in one launch.  Every job has sentinel buffers of its own, over-allocated, and every pointer
    and count of every job stays inside a live allocation: a guard that is missing shows as a lost sentinel, not as a fault."""
    n_carry, n_fresh, n_out, n_keep = 700, 1500, 1200, 600
    sizes = [2, 0, 9, 2, 1]
    groups = np.cumsum([0] + sizes)
    n_jobs = int(groups[-1])
    rng = np.random.default_rng(20)
    carry = torch.from_numpy(rng.uniform(-0.9, 0.9, (n_jobs, n_carry)).astype(np.float32)).cuda()
    fresh = torch.from_numpy(rng.uniform(-0.9, 0.9, (n_jobs, n_fresh)).astype(np.float32)).cuda()
    odt, esz = (torch.float32, 4) if entry == "limit" else (torch.int16, 2)
    base = 40000
    first = base + 2 * 240 + 10 if entry == "limit" else base
    room = n_out * (9 if entry == "frames" else 1)                        # (frames: the first job's dst holds the group's)
    dsts = [sentinel_buffer(PAD + room + PAD + 3, odt) for _ in range(n_jobs)]
    keeps = [sentinel_buffer(PAD + n_keep + PAD) for _ in range(n_jobs)]
    jobs = []
    for g, size in enumerate(sizes):
        for c in range(size):
            k = int(groups[g]) + c
            own = int(groups[g]) if entry == "frames" else k
            f = dict(carry=carry[k].data_ptr(), fresh=fresh[k].data_ptr(), dst=dsts[own].data_ptr() + esz * PAD,
                     carry_out=keeps[k].data_ptr() + 4 * PAD, base=base, first=first, n_carry=n_carry, n_fresh=n_fresh, n_out=n_out,
                     n_keep=n_keep, ended=0, pad_=0)
            if g == 3 and c == 1:
                f["n_out"] = n_out - 1                                    # the counters differ inside the group
            if g == 4:
                f["n_out"] = -5
            jobs.append(hip.StreamJob(**f))
    D, L = delivery(), hip.lib()
    keep, (jp, gp) = upload_tables([(hip.StreamJob * n_jobs)(*jobs), groups.astype(np.int32)], torch.device("cuda"))
    if entry == "limit":
        rc = L.fh_stream_limit_linked_f32(jp, n_jobs, gp, len(sizes), n_out, D._tp_taps(), D._window(240), 240, 0.5, hip.stream())
    else:
        rc = L.fh_stream_pcm_i16_rows_f32(jp, n_jobs, gp, len(sizes), n_out, 0, int(entry == "frames"), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    if entry == "frames":
        assert untouched(dsts[0], PAD, PAD + 2 * n_out) and not untouched(dsts[0]) and untouched(dsts[1])
        src = torch.cat([carry[:2], fresh[:2]], 1)[:, first - base:first - base + n_out]
        assert np.array_equal(dsts[0][PAD:PAD + 2 * n_out].view(n_out, 2).cpu().numpy(), pcm.encode(src.cpu().numpy(), None, True))
    else:
        for k in (0, 1):                                                 # the good group wrote, and only there
            assert untouched(dsts[k], PAD, PAD + n_out) and not untouched(dsts[k])
    assert all(untouched(d) for d in dsts[2:])                           # the refused groups: nothing
    if entry != "limit":                                                 # (the encoder keeps nothing)
        assert all(untouched(k) for k in keeps)
        return
    src = torch.cat([carry, fresh], 1)
    for k in (0, 1):
        assert untouched(keeps[k], PAD, PAD + n_keep) and same_bits(keeps[k][PAD:PAD + n_keep], src[k, -n_keep:])
    assert all(untouched(k) for k in keeps[2:])


@pytest.mark.parametrize("entry", ["limit", "encode"])
def test_jobs_of_one_mono_launch_are_groups_of_one(entry):
    """Three jobs of other sizes, bases and dither keys in ONE launch of a mono entry, each with a carry and a fresh span and a
    dst at an odd element offset of a sentinel buffer, against the entry of streams of channels on the groups [0, 1, 2, 3] of the
    same jobs, planar, with the same key table: the same bits, nothing written outside dst[0 .. n_out) and carry_out[0 .. n_keep)."""
    n_outs, n_carry, n_keep, H = [1, 1025, 2500], 700, 600, 240
    rng = np.random.default_rng(31)
    carry = [torch.from_numpy(rng.uniform(-0.9, 0.9, n_carry).astype(np.float32)).cuda() for _ in n_outs]
    fresh = [torch.from_numpy(rng.uniform(-0.9, 0.9, n + 300).astype(np.float32)).cuda() for n in n_outs]
    bases = [40000, 2 ** 33 + 7, 123457]
    lead = 2 * H + 10 if entry == "limit" else 3                         # (the limiter's outputs trail its source by 2 H + 10)
    odt, esz = (torch.float32, 4) if entry == "limit" else (torch.int16, 2)
    keys = np.array([[77, 0], [78, 5], [2 ** 40 + 3, 1]], dtype=np.uint64)
    kp = torch.from_numpy(keys.view(np.int64)).cuda()
    D, L = delivery(), hip.lib()

    def launch(linked):
        dsts = [sentinel_buffer(PAD + 1 + n + PAD, odt) for n in n_outs]
        keeps = [sentinel_buffer(PAD + 1 + n_keep + PAD) for _ in n_outs]
        jobs = [hip.StreamJob(carry[j].data_ptr(), fresh[j].data_ptr(), dsts[j].data_ptr() + esz * (PAD + 1),
                              keeps[j].data_ptr() + 4 * (PAD + 1), bases[j], bases[j] + lead, n_carry, fresh[j].numel(), n,
                              n_keep if entry == "limit" else 0, 0, 0) for j, n in enumerate(n_outs)]
        keep, (jp, gp) = upload_tables([(hip.StreamJob * 3)(*jobs), np.arange(4, dtype=np.int32)], torch.device("cuda"))
        tables = (jp, 3, gp, 3) if linked else (jp, 3)
        if entry == "limit":
            rc = getattr(L, "fh_stream_limit_linked_f32" if linked else "fh_stream_limit_f32")(
                *tables, max(n_outs), D._tp_taps(), D._window(H), H, 0.5, hip.stream())
        else:
            rc = getattr(L, "fh_stream_pcm_i16_rows_f32" if linked else "fh_stream_pcm_i16_f32")(
                *tables, max(n_outs), kp.data_ptr(), *((0,) if linked else ()), hip.stream())
        torch.cuda.synchronize()
        assert rc == 0
        return dsts, keeps

    (dm, km), (dl, kl) = launch(False), launch(True)
    ints = torch.int32 if entry == "limit" else torch.int16
    for j, n in enumerate(n_outs):
        assert torch.equal(dm[j].view(ints), dl[j].view(ints)) and same_bits(km[j], kl[j])
        assert untouched(dm[j], PAD + 1, PAD + 1 + n) and not untouched(dm[j])
        src = torch.cat([carry[j], fresh[j]])
        if entry == "limit":
            assert untouched(km[j], PAD + 1, PAD + 1 + n_keep) and same_bits(km[j][PAD + 1:PAD + 1 + n_keep], src[-n_keep:])
            assert float(dm[j][PAD + 1:PAD + 1 + n].abs().max()) <= 0.5
        else:                                                             # job j under its own key, at its absolute indices
            assert untouched(km[j])
            d = pcm.tpdf_dither(int(keys[j, 0]), int(keys[j, 1]), 0, n, first=bases[j] + lead)
            assert np.array_equal(dm[j][PAD + 1:PAD + 1 + n].cpu().numpy(), pcm.quantize(src[lead:lead + n].cpu().numpy(), d))


def test_a_group_with_an_odd_dst_is_left_unwritten():
    x = linked_clip(2, [500], 500, seed=7)
    for frames in (0, 1):
        bufs = [sentinel_buffer(1200, torch.int16) for _ in range(2)]
        dsts = [bufs[0].data_ptr() + 2 * PAD, bufs[1].data_ptr() + 2 * PAD + 1]
        if frames:
            dsts = [dsts[1], dsts[0]]                                     # (frames: the first job's dst is the one written)
        assert launch_rows(rows_jobs(x, dsts, 500), [0, 2], 500, 0, frames) == 0
        assert untouched(bufs[0]) and untouched(bufs[1])


def test_argument_errors_write_nothing():
    D, L, st = delivery(), hip.lib(), hip.stream()
    dst = sentinel_buffer(4096)
    x = linked_clip(2, [2048], 2048, seed=22)
    jobs = rows_jobs(x, [dst.data_ptr(), dst.data_ptr() + 4 * 2048], 1024)
    keep, (jp, gp) = upload_tables([(hip.StreamJob * 2)(*jobs), np.array([0, 2], dtype=np.int32)], torch.device("cuda"))
    t4, w = D._tp_taps(), D._window(240)
    bad = {"fh_stream_limit_linked_f32": [(0, 2, gp, 1, 1024, t4, w, 240, 0.5, st), (jp, 0, gp, 1, 1024, t4, w, 240, 0.5, st),
                                          (jp, 65536, gp, 1, 1024, t4, w, 240, 0.5, st), (jp, 2, 0, 1, 1024, t4, w, 240, 0.5, st),
                                          (jp, 2, gp, 0, 1024, t4, w, 240, 0.5, st), (jp, 2, gp, 65536, 1024, t4, w, 240, 0.5, st),
                                          (jp, 2, gp + 2, 1, 1024, t4, w, 240, 0.5, st), (jp, 2, gp, 1, -1, t4, w, 240, 0.5, st),
                                          (jp, 2, gp, 1, 1024, 0, w, 240, 0.5, st), (jp, 2, gp, 1, 1024, t4, 0, 240, 0.5, st),
                                          (jp, 2, gp, 1, 1024, t4, w, 513, 0.5, st), (jp, 2, gp, 1, 1024, t4, w, 0, 0.5, st),
                                          (jp, 2, gp, 1, 1024, t4, w, 240, 0.0, st), (jp, 2, gp, 1, 1024, t4, w, 240, 1.5, st),
                                          (jp, 2, gp, 1, 1024, t4 + 2, w, 240, 0.5, st), (jp, 2, gp, 1, 1024, t4, w + 4, 240, 0.5, st)],
           "fh_stream_pcm_i16_rows_f32": [(0, 2, gp, 1, 1024, 0, 0, st), (jp, 0, gp, 1, 1024, 0, 0, st), (jp, 65536, gp, 1, 1024, 0, 1, st),
                                          (jp, 2, 0, 1, 1024, 0, 0, st), (jp, 2, gp, 0, 1024, 0, 1, st), (jp, 2, gp, 65536, 1024, 0, 0, st),
                                          (jp, 2, gp + 2, 1, 1024, 0, 0, st), (jp, 2, gp, 1, -1, 0, 0, st)]}
    for name, calls in bad.items():
        for args in calls:
            assert getattr(L, name)(*args) == -1, (name, args)
            assert name.encode() in L.fh_last_error()
    torch.cuda.synchronize()
    assert untouched(dst)
    assert L.fh_sizeof_stream_job() == ctypes.sizeof(hip.StreamJob) == 72 and L.fh_abi_version() == 6


# ---- sessions --------------------------------------------------------------------------------------------------------------
def model():
    if "model" not in _STATE:
        fh = FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda")
        _STATE["model"] = FlowHighSR(fh, prior="device", torchdiffeq_ode_method="euler")
    return _STATE["model"]


def clip(C, seconds=0.75):
    """[C, T] at 12 kHz: C different clips."""
    return np.stack([synth.lowres_clip(400 + i, seconds, SR) for i in range(C)])


def long_float(C):
    """generate_long(n_channels=C) without delivery, once per session: float32 [C, T48]."""
    if ("long", C) not in _STATE:
        _STATE["long", C] = model().generate_long(clip(C), SR, seed=SEED, n_channels=C, **PLAN).clone()
    return _STATE["long", C]


@pytest.mark.parametrize("C", [2, 3])
def test_a_session_of_channels_is_generate_long_and_the_stitch_of_its_windows(C):
    m, p, x = model(), S.StreamPlan(SR, **PLAN), clip(C)
    want = long_float(C)
    assert want.shape == (C, p.out_len(x.shape[1])) and want.dtype == torch.float32 and want.is_cuda
    s = m.stream(SR, seed=SEED, n_channels=C, **PLAN)
    outs = [s.push(x[:, a:a + 1111]) for a in range(0, x.shape[1], 1111)]
    with pytest.raises(ValueError, match=rf"\[{C}, n\]"):
        s.push(x[:1, :10])                                                # another row count: refused, the session as it was
    outs.append(s.flush())
    assert all(o.shape[0] == C and o.dtype == torch.float32 and o.is_cuda for o in outs) and same_bits(torch.cat(outs, 1), want)
    with pytest.raises(RuntimeError):
        s.push(x[:, :10])
    # window i: generate(window_i [C, n], channels='first', level='input') with the session's prior at the window's first frame
    wins = []
    for i, (a, b) in enumerate(p.spans(x.shape[1])):
        z = m.draw_prior(S.resample_out_len(b - a, 48000, SR) // 480, SEED, stream=0, first_frame=p.first_frame(i))
        wins.append(m.generate(x[:, a:b], SR, channels="first", level="input", noise=z).cpu().numpy().copy())
    assert len(wins) == 5 and wins[0].shape == (C, p.W48)
    stitched = S.stitch(wins, p, channels=C)
    assert np.array_equal(want.cpu().numpy().view(np.uint32), stitched.view(np.uint32))
    assert not same_bits(want[0], want[1])
    # the session's own encoder: C channels, planar
    enc = m.generate_long(x, SR, seed=SEED, n_channels=C, pcm="int16", **PLAN)
    assert enc.dtype == torch.int16 and np.array_equal(enc.cpu().numpy(), pcm.encode(want.cpu().numpy()))


def test_identical_channels_give_identical_rows():
    m, x = model(), clip(1)
    got = m.generate_long(np.concatenate([x, x]), SR, seed=SEED, n_channels=2, **PLAN)
    assert got.shape[0] == 2 and same_bits(got[0], got[1]) and bool(got[0].any())


@pytest.mark.parametrize("C", [2, 3])
def test_a_session_of_channels_with_delivery_is_the_delivery_of_generate_long(C):
    m, x = model(), clip(C)
    opt = resolve_delivery(1, level="input", **E2E)
    want = m.delivery.batch(long_float(C), [C], "input", opt, [0])[0]
    T = delivered_len(long_float(C).shape[1], 44100)
    s = m.stream(SR, seed=SEED, n_channels=C, delivery=E2E, **PLAN)
    outs = [s.push(x[:, a:a + 2400]) for a in range(0, x.shape[1], 2400)] + [s.flush()]
    assert all(o.dtype == torch.int16 and o.ndim == 2 and o.shape[1] == C and o.is_cuda for o in outs)
    got = torch.cat(outs, 0)
    assert got.shape == want.shape == (T, C) and torch.equal(got, want)
    assert torch.equal(m.generate_long(x, SR, seed=SEED, n_channels=C, delivery=E2E, **PLAN), want)


def test_one_channel_is_the_mono_session_and_the_mono_session_is_todays():
    m, p, x = model(), S.StreamPlan(SR, **PLAN), clip(1)
    mono = m.generate_long(x[0], SR, seed=SEED, **PLAN)
    one = m.generate_long(x, SR, seed=SEED, n_channels=1, **PLAN)
    assert one.shape == mono.shape == (1, p.out_len(x.shape[1])) and same_bits(one, mono)
    # today's bits: the stitch of the windows through generate(level='input') on the mono clip
    wins = []
    for i, (a, b) in enumerate(p.spans(x.shape[1])):
        z = m.draw_prior(S.resample_out_len(b - a, 48000, SR) // 480, SEED, stream=0, first_frame=p.first_frame(i))
        wins.append(m.generate(x[0, a:b], SR, level="input", noise=z)[0].cpu().numpy().copy())
    assert np.array_equal(mono[0].cpu().numpy().view(np.uint32), S.stitch(wins, p).view(np.uint32))
    kw = {k: v for k, v in E2E.items() if k != "interleaved"}
    a = m.generate_long(x[0], SR, seed=SEED, delivery=kw, **PLAN)
    b = m.generate_long(x, SR, seed=SEED, n_channels=1, delivery=kw, **PLAN)
    assert a.dtype == torch.int16 and a.shape == b.shape and a.shape[0] == 1 and torch.equal(a, b)
    opt = resolve_delivery(1, level="input", **kw)
    assert torch.equal(a, m.delivery.batch(mono, [1], "input", opt, [0])[0])
