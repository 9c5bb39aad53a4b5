"""CPU: the device prior's host side -- the numpy restatement of its stream (flowhigh_amd/prior.py: Philox4x32-10 known answers,
moments, layout), the prior= / seed= keywords of FlowHighSR and the C entry's binding."""
import types

import numpy as np
import pytest
import torch

from flowhigh_amd import FlowHighSR, hip
from flowhigh_amd import flowhighsr as M
from flowhigh_amd.prior import expand_seed, philox4x32_10, prior_normal_host

# Random123's known-answer vectors for philox4x32 with 10 rounds (kat_vectors of the Random123 distribution)
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def fake_model(**kw):
    """A FlowHighSR over a CPU-device stand-in: the keyword checks run before anything touches a GPU."""
    return FlowHighSR(types.SimpleNamespace(device=torch.device("cpu"), n_mels=256), **kw)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox4x32_10_reproduces_the_random123_known_answers(counter, key, want):
    got = philox4x32_10(np.array(counter), key)
    assert got.dtype == np.uint32 and " ".join(f"{int(v):08x}" for v in got) == want


def test_philox_is_vectorised_over_counters():
    ctr = np.array([k[0] for k in KAT[:1]] * 3 + [(1, 0, 0, 0)], dtype=np.uint64)
    out = philox4x32_10(ctr, (0, 0))
    assert out.shape == (4, 4) and (out[0] == out[1]).all() and (out[0] == out[2]).all() and (out[3] != out[0]).any()
    assert (out[3] == philox4x32_10(np.array((1, 0, 0, 0)), (0, 0))).all()


def test_moments_of_two_million_draws():
    """Four-sigma bounds of the sample mean, variance and fourth moment of n = 2^21 standard normals, and the largest value the
    formulas can give: u1 >= 2^-24, so |z| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.7682."""
    z = prior_normal_host(seed=12345 + (678 << 32), stream=3, n_frames=8192, n_mels=256)
    n = z.size
    assert z.shape == (8192, 256) and z.dtype == np.float64 and n == 1 << 21
    mean, var, m4, top = abs(z.mean()), abs(z.var() - 1.0), abs((z ** 4).mean() - 3.0), np.abs(z).max()
    print(f"|mean| {mean:.2e}  |var - 1| {var:.2e}  |E z^4 - 3| {m4:.2e}  max |z| {top:.4f}")
    assert mean < 4.0 / np.sqrt(n)
    assert var < 4.0 * np.sqrt(2.0 / n)
    assert m4 < 4.0 * np.sqrt(96.0 / n)
    assert top <= 5.7682


def test_layout_rows_do_not_depend_on_the_clip_length_and_every_key_word_counts():
    seed, stream = 12345 + (678 << 32), 3
    a = prior_normal_host(seed, stream, 9, 256)
    b = prior_normal_host(seed, stream, 4, 256)
    assert np.array_equal(a[:4], b)                                      # row f of a clip: the same in a longer clip
    assert prior_normal_host(seed, stream, 0, 256).shape == (0, 256)
    assert prior_normal_host(seed, stream, 3, 8, dtype=np.float32).dtype == np.float32
    # a row is d / 4 consecutive quads of the flat index: another row width is another layout of the same values
    assert np.array_equal(prior_normal_host(seed, stream, 4, 8).reshape(-1), prior_normal_host(seed, stream, 2, 16).reshape(-1))
    for other in ((seed, stream + 1), (seed, stream + (1 << 32)),        # either word of the stream
                  (seed + 1, stream), (seed + (1 << 32), stream)):       # either 32-bit half of the seed
        c = prior_normal_host(other[0], other[1], 4, 256)
        assert not np.array_equal(c, b) and np.abs(c - b).max() > 1.0
    with pytest.raises(ValueError):
        prior_normal_host(seed, stream, 4, 6)
    # a negative int64 is its two's complement, as the device reads it
    assert np.array_equal(prior_normal_host(-1, 0, 2, 8), prior_normal_host(2 ** 64 - 1, 0, 2, 8))


def test_seed_keyword_forms():
    assert expand_seed(7, 3) == [(7, 0), (7, 1), (7, 2)]                               # an int: clip i gets (s, i)
    assert expand_seed([5, (6, 9), np.int64(8)], 3) == [(5, 0), (6, 9), (8, 0)]          # one int or pair per clip
    assert expand_seed((1 << 40, 2), 2) == [(1 << 40, 0), (2, 0)]
    assert expand_seed([(3, 1 << 33)], 1) == [(3, 1 << 33)]
    with pytest.raises(ValueError):
        expand_seed([1, 2], 3)
    with pytest.raises(ValueError):
        expand_seed([(1, 2, 3)], 1)
    with pytest.raises(TypeError):
        expand_seed(1.5, 1)


def test_prior_keyword_is_validated_and_defaults_to_reference():
    assert fake_model().prior == "reference" and fake_model(prior="device").prior == "device"
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="prior"):
            fake_model(prior=bad)
    # from_local / from_pretrained hand it to the constructor through **kwargs: a wrong value fails there, after the load
    import inspect
    assert "prior" in inspect.signature(FlowHighSR.__init__).parameters
    for fn in (FlowHighSR.from_local.__func__, FlowHighSR.from_pretrained.__func__):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(fn).parameters.values())


def test_seed_under_the_reference_prior_is_refused_before_any_work():
    m = fake_model()
    clip = np.zeros(1200, dtype=np.float32)
    for call in (lambda: m.generate(clip, 12000, seed=1),
                 lambda: m.generate_batch([clip], 12000, seed=[1]),
                 lambda: m.generate_many([clip, clip[:600]], 12000, seed=1),
                 lambda: m.sample(cond=torch.zeros(1, 4800), seed=1),
                 lambda: m.sample_many([torch.zeros(4800)], seed=[(1, 2)]),
                 lambda: m.generate_from_device(torch.zeros(1, 1200), 12000, seed=1)):
        with pytest.raises(ValueError, match="prior='device'"):
            call()
    with pytest.raises(ValueError, match="noise="):                       # no device-side draw on a reference model
        m.generate_from_device(torch.zeros(1, 1200), 12000)


def test_keys_of_a_device_prior_call():
    m = fake_model(prior="device")
    assert m._prior_keys(9, 2) == [(9, 0), (9, 1)]
    assert m._prior_keys([4, (5, 6)], 2) == [(4, 0), (5, 6)]
    assert m._prior_keys(9, 2, noise=torch.zeros(2, 3, 256)) is None            # an explicit noise= wins
    # no seed=: one torch.randint(0, 2^63 - 1) per clip from the generator, in clip order, stream 0
    g = torch.Generator().manual_seed(7)
    want = [(int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g)), 0) for _ in range(3)]
    got = m._prior_keys(None, 3, torch.Generator().manual_seed(7))
    assert got == want and len({k[0] for k in got}) == 3
    g2 = torch.Generator().manual_seed(7)                                        # a list = a loop over its clips
    assert [m._prior_keys(None, 1, g2)[0] for _ in range(3)] == want
    torch.manual_seed(11)
    a = m._prior_keys(None, 2)
    torch.manual_seed(11)
    assert m._prior_keys(None, 2) == a                                          # torch.manual_seed reproduces a run
    assert fake_model()._prior_keys(None, 2) is None                            # the reference prior has no keys


def test_reference_prior_is_not_drawn_under_the_device_prior(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("host draw")
    monkeypatch.setattr(M, "reference_prior_draw", boom)
    m = fake_model(prior="device")
    assert m._prior_keys(3, 1) == [(3, 0)]
    with pytest.raises(AssertionError, match="host draw"):
        fake_model()._draw_noise(1, 4, None)


def test_entry_is_bound_and_declared():
    from pathlib import Path
    assert "fh_prior_normal_f32" in hip.EXPORTS and hip.ABI_VERSION == 6
    assert hip._SIGS["fh_prior_normal_f32"] == [hip._P, hip._P, hip._P, hip._I, hip._I, hip._I, hip._P]
    header = (Path(__file__).resolve().parents[1] / "include" / "flowhigh_hip.h").read_text()
    assert "int fh_prior_normal_f32(float* out, const uint64_t* keys, const int32_t* seg, int n_seg, int n, int d, void* stream);" in header
    from flowhigh_amd import build
    assert "prior.hip" in build.SOURCES
