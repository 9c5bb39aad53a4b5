"""GPU: the prior drawn on the device -- fh_prior_normal_f32 (csrc/prior.hip) against its float64 host restatement
(flowhigh_amd/prior.py), its bitwise invariants (alone / batched / ragged), its argument errors, and the prior='device' / seed=
surface of FlowHighSR: equal to the noise= path bit for bit, no host draw, graph capture with replaceable keys, the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth                 # noqa: E402
from flowhigh_amd import flowhighsr as M                                   # noqa: E402
from flowhigh_amd.prior import prior_normal_host                           # noqa: E402
from oracle import ref_cpu                                                 # noqa: E402

# |z| <= 5.77; log and sin / cos at 2 ulp or better and a correctly rounded sqrt give ~3e-6; the bound is 3 x that
TOL_KERNEL = 1e-5
TOL_WAVEFORM = 1e-4
# (seed, stream): a seed >= 2^32, a stream >= 2^32 (both word mappings), and all 64 bits set
KEYS = [(12345 + (678 << 32), 3), (7, 5 + (9 << 32)), (2 ** 64 - 1, 1)]
SR = 12000
_STATE = {}


def flownet():
    if "fh" not in _STATE:
        _STATE["sd"] = synth.make_state_dict(synth.TINY_CFG, 0)
        _STATE["fh"] = FLowHigh(_STATE["sd"], synth.TINY_CFG, "cuda")
    return _STATE["fh"]


def model(prior="device", **kw):
    kw.setdefault("torchdiffeq_ode_method", "euler")
    return FlowHighSR(flownet(), prior=prior, **kw)


def clip(i, seconds):
    return synth.lowres_clip(300 + i, seconds, SR)


def frames_of(audio):
    return (len(audio) * 4) // 480


def keys_tensor(keys):
    return torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64).reshape(-1, 2)).cuda()


def launch(keys, n, d, seg=None):
    """(rc, out): out is NaN wherever the kernel did not write."""
    segt = torch.tensor(seg, dtype=torch.int32).cuda() if seg is not None else None
    rows = sum(r for _, r in seg) if seg is not None else len(keys) * n
    out = torch.full((rows, d), float("nan"), dtype=torch.float32, device="cuda")
    rc = hip.lib().fh_prior_normal_f32(out.data_ptr(), keys_tensor(keys).data_ptr(), hip.ptr(segt), len(keys), n, d, hip.stream())
    return rc, out


@pytest.fixture
def no_host_draw(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reference_prior_draw called on a prior='device' path")
    monkeypatch.setattr(M, "reference_prior_draw", boom)


# ---- the kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(7, 8), (33, 256), (1, 256)])       # 14 quads: less than a block; 2112: several, last one partial
def test_uniform_launch_matches_the_host_restatement_and_a_clip_alone(n, d):
    rc, out = launch(KEYS, n, d)
    assert rc == 0
    out = out.view(len(KEYS), n, d)
    worst = 0.0
    for i, (seed, stream) in enumerate(KEYS):
        want = prior_normal_host(seed, stream, n, d)
        err = np.abs(out[i].cpu().numpy().astype(np.float64) - want).max()
        worst = max(worst, err)
        rc1, alone = launch([KEYS[i]], n, d)
        assert rc1 == 0 and torch.equal(alone, out[i])                 # same bits in a batch as alone
    print(f"n {n} d {d}: max |kernel - float64 definition| {worst:.2e}")
    assert worst <= TOL_KERNEL


def test_ragged_launch_matches_the_host_restatement_and_a_clip_alone():
    seg, d = [(0, 5), (5, 1), (6, 33)], 256
    rc, out = launch(KEYS, 33, d, seg=seg)
    assert rc == 0 and not torch.isnan(out).any()
    worst = 0.0
    for (seed, stream), (r0, rows) in zip(KEYS, seg):
        got = out[r0:r0 + rows]
        worst = max(worst, np.abs(got.cpu().numpy().astype(np.float64) - prior_normal_host(seed, stream, rows, d)).max())
        rc1, alone = launch([(seed, stream)], rows, d)
        assert rc1 == 0 and torch.equal(alone, got)
        rc2, longer = launch([(seed, stream)], 40, d)                  # a row does not depend on the clip's length
        assert rc2 == 0 and torch.equal(longer[:rows], got)
    print(f"ragged: max |kernel - float64 definition| {worst:.2e}")
    assert worst <= TOL_KERNEL


def test_argument_errors_launch_nothing():
    L = hip.lib()
    keys = keys_tensor(KEYS)
    out = torch.full((3 * 8, 8), 7.0, dtype=torch.float32, device="cuda")
    st = hip.stream()
    for args in ((out.data_ptr(), keys.data_ptr(), 0, 3, 4, 6, st),            # d % 4
                 (out.data_ptr(), 0, 0, 3, 8, 8, st),                          # null keys
                 (0, keys.data_ptr(), 0, 3, 8, 8, st),                         # null out
                 (out.data_ptr(), keys.data_ptr(), 0, 0, 8, 8, st),            # n_seg = 0
                 (out.data_ptr() + 4, keys.data_ptr(), 0, 2, 8, 8, st)):       # out not 16-byte aligned
        assert L.fh_prior_normal_f32(*args) == -1
        assert b"fh_prior_normal_f32" in L.fh_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the model ----------------------------------------------------------------------------------------------------------
def test_generate_with_a_seed_is_generate_with_that_key_s_noise(no_host_draw):
    m = model()
    a = clip(0, 0.5)
    n, s = frames_of(a), 41 + (3 << 32)
    z = m.draw_prior(n, s)
    assert z.shape == (1, n, 256) and z.is_cuda
    assert np.abs(z[0].cpu().numpy().astype(np.float64) - prior_normal_host(s, 0, n)).max() <= TOL_KERNEL
    got = m.generate(a, SR, seed=s).clone()
    assert torch.equal(got, m.generate(a, SR, noise=z))
    assert torch.equal(got, m.generate(a, SR, seed=s))                         # a second identical call: same bits
    assert torch.equal(got, m.generate(a, SR, seed=[(s, 0)]))                  # the pair form of the same key
    assert torch.equal(got, m.generate(a, SR, seed=s, noise=z))
    other = m.generate(a, SR, seed=s + 1)
    assert not torch.equal(got, other) and (got - other).abs().max().item() > 1e-3
    assert not torch.equal(got, m.generate(a, SR, seed=[(s, 1)]))              # another stream of the same seed
    # an explicit noise= wins under the device prior too
    zr = torch.randn(1, n, 256, generator=torch.Generator().manual_seed(3))      # (any host tensor: nothing is drawn for it)
    assert torch.equal(m.generate(a, SR, noise=zr), model("reference").generate(a, SR, noise=zr))


def test_batch_keys_and_torch_generators(no_host_draw):
    m = model()
    a, b = clip(1, 0.3), clip(2, 0.3)
    n, s = frames_of(a), 99
    both = m.generate_batch([a, b], SR, seed=s).clone()                        # an int: clip i gets (s, i)
    assert torch.equal(both[0:1], m.generate(a, SR, seed=[(s, 0)])) and torch.equal(both[1:2], m.generate(b, SR, seed=[(s, 1)]))
    assert torch.equal(both, m.generate_batch([a, b], SR, noise=m.draw_prior(n, [(s, 0), (s, 1)])))
    # no seed=: keys come from the generator, one torch.randint per clip
    g = torch.Generator().manual_seed(5)
    k = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g))
    one = m.generate(a, SR, generator=torch.Generator().manual_seed(5)).clone()
    assert torch.equal(one, m.generate(a, SR, seed=k))
    torch.manual_seed(1234)
    first = m.generate(a, SR).clone()
    second = m.generate(a, SR).clone()
    torch.manual_seed(1234)
    assert torch.equal(first, m.generate(a, SR)) and not torch.equal(first, second)


def test_sample_mix_method_with_a_seed(no_host_draw):
    m = model(sigma=0.5, cfm_method="independent_cfm_mix")
    x = np.stack([synth.lowres_clip(310 + i, 0.3, 48000) for i in range(2)])
    cond = torch.from_numpy(x / np.abs(x).max(axis=1, keepdims=True)).cuda()
    n, s = cond.shape[1] // 480, 2 ** 40 + 17
    z = m.draw_prior(n, [(s, 0), (s, 1)])
    for kw in (dict(), dict(decode_to_audio=False, mel_pp=True, cond_scale=1.5)):
        got = m.sample(cond=cond, time_steps=1, cfm_method="independent_cfm_mix", seed=s, **kw)
        assert torch.equal(got, m.sample(cond=cond, time_steps=1, cfm_method="independent_cfm_mix", noise=z, **kw))
        assert not torch.equal(got, m.sample(cond=cond, time_steps=1, cfm_method="independent_cfm_mix", seed=s + 1, **kw))
    many = m.sample_many([cond[0], cond[1, :9600]], time_steps=1, seed=[(s, 0), 23])
    assert torch.equal(many[0], m.sample(cond=cond[0:1], time_steps=1, seed=[(s, 0)]))
    assert torch.equal(many[1], m.sample(cond=cond[1:2, :9600], time_steps=1, seed=[23]))


def test_generate_many_ragged_with_seeds_and_with_a_generator(no_host_draw):
    m = model()
    clips = [clip(3, 0.5), clip(4, 0.23), clip(5, 0.37)]
    seeds = [11, (12 + (1 << 35), 4), 13]
    many = m.generate_many(clips, SR, seed=seeds, ragged=True)
    alone = [m.generate(c, SR, seed=[s]).clone() for c, s in zip(clips, seeds)]
    assert all(torch.equal(x, y) for x, y in zip(many, alone))
    per_length = m.generate_many(clips, SR, seed=seeds, ragged=False)           # one batch per length: the same keys
    assert all(torch.equal(x, y) for x, y in zip(per_length, alone))
    zs = m.draw_prior([frames_of(c) for c in clips], seeds)                     # the ragged form of draw_prior
    assert all(torch.equal(m.generate(c, SR, noise=z), y) for c, z, y in zip(clips, zs, alone))
    # a list consumes the generator as a loop over generate() does
    many = m.generate_many(clips, SR, generator=torch.Generator().manual_seed(7))
    g = torch.Generator().manual_seed(7)
    loop = [m.generate(c, SR, generator=g).clone() for c in clips]
    assert all(torch.equal(x, y) for x, y in zip(many, loop))
    # an int seed over a list: clip i gets (s, i)
    many = m.generate_many(clips[:2], SR, seed=77)
    assert torch.equal(many[0], m.generate(clips[0], SR, seed=[(77, 0)])) and torch.equal(many[1], m.generate(clips[1], SR, seed=[(77, 1)]))


def test_batching_server_takes_a_request_seed_as_its_key(no_host_draw):
    from flowhigh_amd.serve import BatchingServer
    m = model()
    clips = [clip(6, 0.3), clip(7, 0.23)]
    srv = BatchingServer(m, max_batch=4, max_wait_ms=20.0)
    try:
        futs = [srv.submit(c, SR, 1, seed=50 + i) for i, c in enumerate(clips)]
        got = [f.result(timeout=120) for f in futs]
    finally:
        srv.close()
    for i, (c, y) in enumerate(zip(clips, got)):
        assert np.array_equal(y, m.generate(c, SR, seed=50 + i).cpu().numpy()[0])


def test_captured_graph_draws_from_the_keys_it_finds(no_host_draw):
    m = model(upsampling_method="hip")
    a = clip(8, 0.23)
    x = torch.from_numpy(a[None]).cuda()
    g = m.capture(1, len(a), SR, 1)
    assert not hasattr(g, "noise") and g.keys.shape == (1, 2) and g.keys.dtype == torch.int64 and g.keys.is_cuda
    g.x.copy_(x)
    for key in ((31, 0), (5 + (7 << 33), 9)):
        g.keys.copy_(torch.tensor([key], dtype=torch.int64))
        got = g.replay().clone()
        assert torch.equal(got, m.generate_from_device(x, SR, 1, seed=[key]))
    assert torch.equal(got, m.generate_from_device(x, SR, 1, noise=m.draw_prior(frames_of(a), 5 + (7 << 33), stream=9)))
    # a reference-prior model keeps its noise buffer, and has no device-side draw
    gr = model("reference", upsampling_method="hip").capture(1, len(a), SR, 1)
    assert hasattr(gr, "noise") and not hasattr(gr, "keys")
    with pytest.raises(ValueError):
        model("reference", upsampling_method="hip").generate_from_device(x, SR, 1)


def test_device_prior_run_against_the_oracle(no_host_draw):
    """TINY_CFG, euler x 1, a 0.23 s clip at 12 kHz: the device run with seed=s against the CPU oracle fed the noise of that key."""
    m = model()
    a = clip(9, 0.23)
    s = 2024 + (5 << 32)
    out, st = m.generate_batch([a], SR, 48000, 1, seed=s, return_stages=True)
    z = m.draw_prior(frames_of(a), s).cpu()
    ref, rs = ref_cpu.generate(_STATE["sd"], synth.TINY_CFG, a, SR, z, 1, "euler", return_stages=True)
    assert int(st["cr"][0].item()) == rs["cr"]
    e_wav = (st["wav"].cpu() - rs["wav"]).abs().max().item()
    e_out = (out.cpu() - ref).abs().max().item()
    print(f"device prior vs oracle: wav {e_wav:.2e}, out {e_out:.2e}")
    assert e_wav <= TOL_WAVEFORM and e_out <= TOL_WAVEFORM


def test_default_model_still_draws_the_reference_stream():
    m = FlowHighSR(flownet(), torchdiffeq_ode_method="euler")
    assert m.prior == "reference"
    a = clip(10, 0.3)
    got = m.generate(a, SR, generator=torch.Generator().manual_seed(4242)).clone()
    z = M.reference_prior_draw(frames_of(a), 256, torch.Generator().manual_seed(4242))
    assert torch.equal(got, m.generate(a, SR, noise=z))
    with pytest.raises(ValueError):
        m.generate(a, SR, seed=1)
