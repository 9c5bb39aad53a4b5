"""CPU: the host side of multichannel clips and level-true output (channels=, level=): layouts and their errors, the noise of a
clip's channels, the int16 rule on a whole clip, the four entries of csrc/level.hip in header / EXPORTS / _SIGS, their argument
checks, the rules' restatement (tests/ref_level.py) on worked numbers, and the batching server with a stub model."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import ref_level
from flowhigh_amd import hip
from flowhigh_amd.flowhighsr import FlowHighSR, channel_noise, clip_noises, resolve_channels, resolve_clips

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"fh_channel_peaks_f32": 4, "fh_group_peak_f32": 5, "fh_row_gain_f32": 5, "fh_row_gain_seg_f32": 5}


def stereo(T=50, dtype=np.float32):
    x = (np.arange(2 * T).reshape(2, T) % 7 - 3).astype(dtype)
    return x / dtype(8) if np.issubdtype(dtype, np.floating) else x


# ---- layouts -------------------------------------------------------------------------------------------------------------
def test_resolve_channels_accepts_every_layout_as_planar():
    x = stereo()
    for channels in (None, "first", "last"):                       # a 1-D clip is one channel whatever the keyword
        got = resolve_channels(x[0], channels)
        assert got.shape == (1, 50) and np.array_equal(got[0], x[0])
    assert np.array_equal(resolve_channels(x[:1]), x[:1])          # [1, T] without the keyword: as always
    assert np.array_equal(resolve_channels(x, "first"), x)
    assert np.array_equal(resolve_channels(np.ascontiguousarray(x.T), "last"), x)
    assert np.array_equal(resolve_channels(torch.from_numpy(x).T, "last"), x)          # tensors too
    assert resolve_channels(np.zeros((8, 9)), "first").shape == (8, 9)                  # C = 8 is the most
    assert resolve_channels(np.zeros((9, 8)), "last").shape == (8, 9)
    assert resolve_channels(np.zeros((1, 8)), "last").shape == (8, 1)                   # eight channels of one sample: a layout
    i16 = stereo(dtype=np.int16)
    assert resolve_channels(i16, "first").dtype == np.int16        # values and dtype untouched: scaling is resolve_clips'


@pytest.mark.parametrize("audio,channels,say", [
    (np.zeros((2, 50)), None, "channels"),                          # 2-D without the keyword
    (np.zeros((50, 2)), None, "channels"),
    (np.zeros((50, 1)), None, "channels"),                          # [T, 1]: a layout that needs naming as well
    (np.zeros((9, 50)), "first", "9 channels"),                     # C above 8
    (np.zeros((50, 9)), "last", "9 channels"),
    (np.zeros((50, 2)), "first", "50 channels"),                    # the other layout's keyword
    (np.zeros((1, 2, 50)), "first", "shape"),                       # 3-D
    (np.zeros((1, 2, 50)), None, "shape"),
    (np.float32(0.5), None, "shape"),                               # 0-D
    (np.zeros((2, 0)), "first", "empty"),
    (np.zeros(0), None, "empty"),
    (np.zeros((2, 50)), "planar", "channels must be"),
])
def test_resolve_channels_refuses(audio, channels, say):
    with pytest.raises(ValueError, match=say):
        resolve_channels(audio, channels)


def test_a_noise_tensor_is_shared_or_one_per_channel():
    z1, z3 = torch.randn(1, 25, 8), torch.randn(3, 25, 8)
    assert channel_noise(z1, 3).shape == (3, 25, 8) and all(torch.equal(r, z1[0]) for r in channel_noise(z1, 3))
    assert channel_noise(z3, 3) .shape == (3, 25, 8) and torch.equal(channel_noise(z3, 3), z3)
    for bad, c in ((torch.randn(2, 25, 8), 3), (z3, 2), (torch.randn(25, 8), 1), (z3, 1)):          # a wrong leading dimension
        with pytest.raises(ValueError, match="noise of shape"):
            channel_noise(bad, c)
    assert [tuple(z.shape) for z in clip_noises([z1, z3], [2, 3])] == [(2, 25, 8), (3, 25, 8)]
    assert [tuple(z.shape) for z in clip_noises(z3, [3])] == [(3, 25, 8)]                    # one clip: the tensor is its noise
    assert [tuple(z.shape) for z in clip_noises(z3, [2, 1, 2])] == [(2, 25, 8), (1, 25, 8), (2, 25, 8)]          # [B, ...]: per clip
    assert clip_noises(None, [2]) is None
    with pytest.raises(ValueError, match="one noise tensor per clip"):
        clip_noises([z1], [2, 2])
    with pytest.raises(ValueError, match="noise of shape"):
        clip_noises([z1, z3], [2, 2])


def test_resolve_clips_picks_the_path_and_scales_a_whole_clip_once():
    x = stereo()
    same, planar = resolve_clips([x[0], x[:1]])
    assert planar is None and same[0] is not None and same[0].shape == (50,)            # mono, 'peak': the clips as they came
    same, planar = resolve_clips([x[:1]], "first")
    assert planar is None and same[0].shape == (1, 50)                                  # ... or as [1, T]
    assert resolve_clips([x[0]], None, "input")[0] is None                              # level='input' leaves the default path
    assert resolve_clips([x], "first")[0] is None
    loud = np.stack([np.full(50, 20000, np.int16), np.full(50, 1, np.int16)])           # the second channel alone would NOT scale
    (got,) = resolve_clips([loud], "first")[1]
    assert np.array_equal(got, loud / 32768.0)
    (got,) = resolve_clips([loud.T], "last", "input")[1]
    assert np.array_equal(got, loud / 32768.0)
    (got,) = resolve_clips([x], "first")[1]
    assert np.array_equal(got, x)                                                       # |x| <= 1: untouched
    with pytest.raises(ValueError, match="level must be"):
        resolve_clips([x[0]], None, "rms")
    with pytest.raises(ValueError, match="channels"):
        resolve_clips([x[0], x])


def test_the_public_entries_have_the_keywords_and_refuse_before_any_gpu_work():
    from flowhigh_amd.serve import BatchingServer
    for fn in (FlowHighSR.generate, FlowHighSR.generate_batch, FlowHighSR.generate_many, BatchingServer.submit):
        p = inspect.signature(fn).parameters
        assert p["channels"].kind is p["level"].kind is inspect.Parameter.KEYWORD_ONLY, fn
        assert p["channels"].default is None and p["level"].default == "peak", fn
    for fn in (FlowHighSR.generate_from_device, FlowHighSR.capture):
        assert "channels" not in inspect.signature(fn).parameters and "mono" in fn.__doc__.lower(), fn
    m = FlowHighSR.__new__(FlowHighSR)                               # no device, no library: anything past the checks would raise
    m.flowhigh = type("F", (), {"device": torch.device("cpu")})()
    m.prior = "reference"
    x = stereo()
    with pytest.raises(ValueError, match="channels="):
        m.generate(x, 12000)
    with pytest.raises(ValueError, match="channels="):
        m.generate_many([x[0], x], 12000)
    with pytest.raises(ValueError, match="9 channels"):
        m.generate_batch([np.zeros((9, 50))], 12000, channels="first")
    with pytest.raises(ValueError, match="level must be"):
        m.generate(x[0], 12000, level="lufs")
    with pytest.raises(ValueError, match="noise of shape"):
        m.generate(x, 12000, channels="first", noise=torch.zeros(3, 1, 8))
    with pytest.raises(ValueError, match="noise of shape"):
        m.generate_many([x, x[:1]], 12000, channels="first", noise=[torch.zeros(2, 1, 8), torch.zeros(2, 1, 8)])


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_header_exports_and_abi_are_consistent():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    for name, n_params in ENTRIES.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/flowhigh_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert name in hip.EXPORTS and len(hip._SIGS[name]) == len(params) == n_params, name
        for p, ctype in zip(params, hip._SIGS[name]):
            assert ctype is (hip._P if "*" in p else hip._I), (name, p)
    assert "level.hip" in __import__("flowhigh_amd.build", fromlist=["SOURCES"]).SOURCES


def test_library_exports_the_entries_and_checks_their_arguments():
    """The argument checks run on the host before anything is launched: the device pointers are fake addresses, never read."""
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    A, B, G = 256, 512, 768
    bad = [("fh_channel_peaks_f32", a) for a in ((0, B, 3), (A, 0, 3), (A, B, 0), (A, B, -1))]
    bad += [("fh_group_peak_f32", a) for a in ((0, B, G, 3), (A, 0, G, 3), (A, B, 0, 3), (A, B, G, 0))]
    bad += [("fh_row_gain_f32", a) for a in ((0, B, 2, 100), (A, 0, 2, 100), (A, B, 0, 100), (A, B, 65536, 100), (A, B, 2, 0),
                                             (A + 2, B, 2, 100))]
    bad += [("fh_row_gain_seg_f32", a) for a in ((0, 2, 100, B), (A, 0, 100, B), (A, 65536, 100, B), (A, 2, 0, B), (A, 2, 100, 0))]
    for name, args in bad:
        assert getattr(L, name)(*args, 0) == -1, (name, args)
        assert name.encode() in L.fh_last_error(), (name, args)


# ---- the rules, on numbers worked by hand ------------------------------------------------------------------------------------
def test_ref_level_on_worked_numbers():
    f = np.float32
    gains, div = ref_level.channel_peaks([0.5, 0.0, 1e-40])
    assert gains.tolist() == [0.5, 0.0, float(f(1e-40))] and div.tolist() == [0.5, 1.0, float(f(1e-40))]
    # groups of 1, 2, 3 rows; the pair has a silent row whose q is a NaN, the triple is all silent
    q = f([0.8, 0.5, np.nan, 3.0, np.nan, 7.0])
    g = f([0.5, 0.25, 0.0, 0.0, 0.0, 0.0])
    G = ref_level.group_peak(q, g, [0, 1, 1, 2, 2, 2])
    assert G.tolist() == [float(f(0.8) * f(0.5)), 0.125, 0.125, 1.0, 1.0, 1.0]
    w = [f([0.5, -1.0]), f([0.25, 0.5])]
    out = ref_level.finish(w, f([0.5, 1.0]), "input")
    assert [o.tolist() for o in out] == [[0.25, -0.5], [0.25, 0.5]]
    out = ref_level.finish(w, f([0.5, 1.0]), "peak")                  # u = [.25, -.5], [.25, .5]; G = 0.5
    assert [o.tolist() for o in out] == [[float(f(0.5) * f(0.99)), -float(f(0.99))], [float(f(0.5) * f(0.99)), float(f(0.99))]]
    out = ref_level.finish(w, f([0.0, 0.0]), "peak")
    assert all(not o.any() for o in out)
    # a mono clip: G = fl(q p), so the result is (w p / (q p)) * 0.99 -- the default's (w / q) * 0.99 up to two roundings
    assert ref_level.finish([f([0.3, -0.6])], f([1.0]), "peak")[0].tolist() == ref_level.peak_scale(f([0.3, -0.6]), f(0.6)).tolist()


# ---- the serving front -----------------------------------------------------------------------------------------------------
class _StubModel:
    """tests/test_parallel_cpu.py's stand-in with the keywords: records the calls, returns [C, 4 T] per clip."""

    def __init__(self):
        self.calls = []

    def _draw_noise(self, batch, n_frames, generator):
        return torch.randn(batch, n_frames, 4, generator=generator)

    def generate_many(self, clips, sr, target, steps, noise=None, max_batch=64, channels=None, level="peak"):
        planar = [resolve_channels(c, channels) for c in clips]
        self.calls.append(dict(shapes=[p.shape for p in planar], sr=sr, channels=channels, level=level,
                               noise=None if noise is None else [tuple(n.shape) for n in noise]))
        return [torch.from_numpy(np.repeat(p.astype(np.float32), 4, axis=1)) * (2 if level == "peak" else 3) for p in planar]


def test_batching_server_takes_multichannel_clips_and_levels():
    from flowhigh_amd.serve import BatchingServer
    m = _StubModel()
    srv = BatchingServer(m, max_batch=8, max_wait_ms=20)
    try:
        up = (np.arange(240).reshape(120, 2) % 11 - 5).astype(np.int16)                  # gradio: int16 [T, 2]
        sr, y = srv.generate((12000, up), 48000, 1)
        assert sr == 48000 and y.dtype == np.float32 and y.shape == (480, 2)              # [T48, C]: the caller's layout
        assert np.array_equal(y, 2 * np.repeat(up.astype(np.float32), 4, axis=0))
        assert m.calls[-1]["channels"] == "first" and m.calls[-1]["shapes"] == [(2, 120)] and m.calls[-1]["level"] == "peak"
        mono = np.linspace(-1, 1, 100, dtype=np.float32)
        sr, y = srv.generate((12000, mono), 48000, 1)                                     # a mono clip: the call it always was
        assert y.shape == (400,) and m.calls[-1]["channels"] is None and m.calls[-1]["level"] == "peak"
        y = srv.submit(mono, 12000, level="input").result(timeout=30)
        assert y.shape == (400,) and np.array_equal(y, 3 * np.repeat(mono, 4)) and m.calls[-1]["level"] == "input"
        y = srv.submit(up.T, 12000, seed=3, channels="first", level="input").result(timeout=30)
        assert y.shape == (2, 480) and m.calls[-1]["level"] == "input" and m.calls[-1]["noise"] == [(1, 1, 4)]          # one draw per CLIP
        # a mono request beside a stereo one in one window: one channels='first' call, the mono clip as [1, T], back as [T48]
        pair = BatchingServer(m, max_batch=2, max_wait_ms=30000)                          # (its window ends with the second request)
        futs = [pair.submit(mono, 12000), pair.submit(up, 12000, channels="last")]
        a, b = [f.result(timeout=30) for f in futs]
        pair.close()
        assert a.shape == (400,) and b.shape == (2, 480)
        assert m.calls[-1]["shapes"] == [(1, 100), (2, 120)] and m.calls[-1]["channels"] == "first"
        # malformed shapes raise in submit, in the caller's thread
        for bad, kw in ((np.zeros((2, 120)), {}), (np.zeros((120, 9)), dict(channels="last")), (np.zeros((1, 2, 120)), dict(channels="first")),
                        (mono, dict(level="rms")), (mono, dict(channels="interleaved"))):
            with pytest.raises(ValueError):
                srv.submit(bad, 12000, **kw)
        with pytest.raises(ValueError):
            srv.generate((12000, np.zeros((3, 3))), 48000, 1)                             # 2-D, not gradio's [T, C <= 8 < T]
        with pytest.raises(NotImplementedError):
            srv.generate((12000, up), 44100, 1)
    finally:
        srv.close()
    with pytest.raises(RuntimeError):
        srv.submit(up, 12000, channels="last")
