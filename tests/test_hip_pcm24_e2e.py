"""GPU: pcm='s24' / 's24in32' through the public entries on TINY_CFG (clips of 0.33 to 0.4 s at 12 kHz): generate against pcm.py's
encode24 of the same call's float result, generate_many under both `ends` against generate per clip, a delivery stream pushed in
uneven blocks against the one-shot delivery of the whole clip in bytes, the session's own pcm=, and the batching server.  Every
comparison is an equality: two runs of this project, or the definition on this project's own float result."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, pcm, synth                               # noqa: E402
from flowhigh_amd import delivery_stream as DS                                          # noqa: E402
from flowhigh_amd.delivery import resolve_delivery                                      # noqa: E402

SR = 12000
PLAN = dict(window_ms=200, overlap_ms=60, guard_ms=10)
FORMATS = {"s24": torch.uint8, "s24in32": torch.int32}
_STATE = {}


def model(prior="reference"):
    if "fh" not in _STATE:
        _STATE["fh"] = FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda")
    if prior not in _STATE:
        _STATE[prior] = FlowHighSR(_STATE["fh"], torchdiffeq_ode_method="euler", upsampling_method="hip", prior=prior)
    return _STATE[prior]


def clip(chans, n, seed):
    """[chans, n] at 12 kHz, the second channel quieter; mono: [n]."""
    x = np.stack([synth.lowres_clip(seed + c, n / SR, SR)[:n] * np.float32((1.0, 0.45)[c]) for c in range(chans)])
    return x[0] if chans == 1 else x


def noise(seed, frames):
    return synth.prior_noise(seed, frames)


def shape_of(fmt, *shape):
    return tuple(shape) + ((3,) if fmt == "s24" else ())


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_generate_is_encode24_of_the_float_result(fmt):
    m, S = model(), clip(2, 3960, 600)
    kw = dict(noise=noise(700, 33), channels="first")
    y = m.generate(S, SR, **kw).cpu().numpy()
    got = m.generate(S, SR, pcm=fmt, dither="tpdf", dither_seed=5, interleaved=True, **kw)
    assert got.dtype == FORMATS[fmt] and got.is_cuda and got.is_contiguous() and tuple(got.shape) == shape_of(fmt, y.shape[1], 2)
    assert np.array_equal(got.cpu().numpy(), pcm.encode24(y, (5, 0), True, packed=fmt == "s24"))
    planar = m.generate(S, SR, pcm=fmt, **kw)
    assert tuple(planar.shape) == shape_of(fmt, 2, y.shape[1])
    assert np.array_equal(planar.cpu().numpy(), pcm.encode24(y, None, False, packed=fmt == "s24"))
    # a mono clip without channels=: [1, T] as the float result is, [T, 1] interleaved
    M = clip(1, 3960, 610)
    y = m.generate(M, SR, noise=noise(710, 33)).cpu().numpy()
    mono = m.generate(M, SR, noise=noise(710, 33), pcm=fmt, dither="tpdf", dither_seed=5)
    assert tuple(mono.shape) == shape_of(fmt, 1, y.shape[1])
    assert np.array_equal(mono.cpu().numpy(), pcm.encode24(y, (5, 0), False, packed=fmt == "s24"))
    inter = m.generate(M, SR, noise=noise(710, 33), pcm=fmt, dither="tpdf", dither_seed=5, interleaved=True)
    assert tuple(inter.shape) == shape_of(fmt, y.shape[1], 1) and torch.equal(inter.reshape(-1), mono.reshape(-1))
    if fmt == "s24":                                     # the bytes behind a 24-bit WAV header: 3 little-endian bytes a sample
        q = pcm.quantize24(y[0], pcm.tpdf_dither(5, 0, 0, y.shape[1]))
        assert inter.reshape(-1).cpu().numpy().tobytes() == b"".join(int(v).to_bytes(3, "little", signed=True) for v in q)


@pytest.mark.parametrize("ends", ["ragged", "per_clip"])
def test_generate_many_is_generate_per_clip(ends):
    """Two clips of different lengths and channel counts behind the resampler and the limiter: each the bits of its own generate."""
    m = model()
    S, L_ = clip(2, 3960, 600), clip(1, 4800, 620)
    deliver = dict(output_rate=44100, true_peak=-1.0, limiter="lookahead", pcm="s24", dither="tpdf", channels="first")
    a = m.generate(S, SR, noise=noise(700, 33), dither_seed=[(9, 0)], **deliver)
    b = m.generate(L_[None], SR, noise=noise(720, 40), dither_seed=[(9, 1)], **deliver)
    assert a.dtype == b.dtype == torch.uint8 and tuple(a.shape) == (2, 14553, 3) and tuple(b.shape) == (1, 17640, 3)
    outs = m.generate_many([S, L_[None]], SR, noise=[noise(700, 33), noise(720, 40)], ends=ends, dither_seed=9, **deliver)
    assert torch.equal(outs[0], a) and torch.equal(outs[1], b)
    wide = m.generate_many([S, L_[None]], SR, noise=[noise(700, 33), noise(720, 40)], ends=ends, dither_seed=9,
                           **dict(deliver, pcm="s24in32", interleaved=True))
    assert wide[0].dtype == torch.int32 and tuple(wide[0].shape) == (14553, 2) and tuple(wide[1].shape) == (17640, 1)
    for w, p in zip(wide, (a, b)):
        assert np.array_equal(pcm.pack24(w.t().cpu().numpy()), p.cpu().numpy())


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_a_delivery_stream_adds_up_to_the_one_shot_delivery(fmt):
    m = model()
    kw = dict(output_rate=44100, pcm=fmt, dither="tpdf", dither_seed=9, true_peak=-3.0, limiter="lookahead")
    x = torch.from_numpy(clip(2, 14400, 630) * np.float32(0.9)).cuda()          # 0.3 s at 48 kHz
    for interleaved in (False, True):
        want = m.delivery.batch(x, [2], "input", resolve_delivery(1, level="input", interleaved=interleaved, **kw), [0])[0]
        ds = m.delivery_stream(n_channels=2, interleaved=interleaved, **kw)
        outs, prev = [], 0
        for c in (1, 8, 17, 2048, 2048, 5000, 5007, 9999, 14400):
            outs.append(ds.push(x[:, prev:c]))
            prev = c
        outs.append(ds.flush())
        assert all(o.dtype == FORMATS[fmt] and o.is_contiguous() for o in outs)
        empty = shape_of(fmt, *((0, 2) if interleaved else (2, 0)))
        assert tuple(outs[0].shape) == empty and tuple(outs[4].shape) == empty        # nothing final yet; an empty push
        got = torch.cat(outs, 0 if interleaved else 1)
        assert got.shape == want.shape and torch.equal(got.reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8))
    # a mono stream is a group of one job: the bits of the one-channel stream and of the one-shot [1, T] clip
    want = m.delivery.batch(x[:1], [1], "input", resolve_delivery(1, level="input", **kw), [0])[0]
    ds = m.delivery_stream(**kw)
    got = torch.cat([ds.push(x[:1, :7]), ds.push(x[:1, 7:9000]), ds.push(x[:1, 9000:]), ds.flush()], 1)
    assert torch.equal(got, want) and tuple(got.shape[:1]) == (1,)


def test_the_session_s_own_pcm():
    m = model("device")
    x = synth.lowres_clip(400, 0.75, SR)
    whole = m.generate_long(x, SR, seed=41, stream=2, **PLAN).cpu().numpy()
    for fmt in sorted(FORMATS):
        s = m.stream(SR, seed=41, stream=2, pcm=fmt, **PLAN)
        blocks = [s.push(x[a:a + 2400]) for a in range(0, 9000, 2400)] + [s.flush()]
        assert all(b.dtype == FORMATS[fmt] and b.shape[0] == 1 and b.ndim == (3 if fmt == "s24" else 2) for b in blocks)
        q = pcm.quantize24(whole)
        assert np.array_equal(torch.cat(blocks, 1).cpu().numpy(), pcm.pack24(q) if fmt == "s24" else q)
        s = m.stream(SR, seed=1, pcm=fmt, **PLAN)
        assert tuple(s.push(np.zeros(0, dtype=np.float32)).shape) == shape_of(fmt, 1, 0) and s.flush().dtype == FORMATS[fmt]


def test_batching_server_hands_out_the_bytes():
    from flowhigh_amd.serve import BatchingServer
    m, S, M = model(), clip(2, 3960, 600), clip(1, 3960, 610)
    srv = BatchingServer(m, max_batch=4, max_wait_ms=5)
    try:
        torch.manual_seed(12)
        sr, y = srv.generate((SR, np.ascontiguousarray(S.T)), 16000, 1, pcm="s24", dither="tpdf")
        torch.manual_seed(12)
        want = m.generate(S, SR, channels="first", output_rate=16000, pcm="s24", dither="tpdf", interleaved=True)
        assert sr == 16000 and y.dtype == np.uint8 and y.shape == (5280, 2, 3) and np.array_equal(y, want.cpu().numpy())
        torch.manual_seed(11)
        sr, y = srv.generate((SR, M), 44100, 1, pcm="s24")
        torch.manual_seed(11)
        want = m.generate_many([M], SR, output_rate=44100, pcm="s24")[0]
        assert y.dtype == np.uint8 and y.shape == (1, 14553, 3) and np.array_equal(y, want.cpu().numpy())
        torch.manual_seed(11)
        sr, y = srv.generate((SR, M), 44100, 1, pcm="s24in32")
        assert y.dtype == np.int32 and y.shape == (14553,) and np.array_equal(pcm.pack24(y)[None], want.cpu().numpy())
    finally:
        srv.close()
