"""GPU: the ODE methods heun2 / heun3 / rk4 -- fh_rk_combine_f32 (csrc/ode.hip) at its edges against a float64 evaluation, and the
tableau stepper of integrate.solve through sample / generate_batch / generate_many / sample_many / capture on both backbones,
against the textbook stepper (tests/ref_odeint.py) over the oracle's vector field.

Bars.  Kernel: per element 2^-21 (|y| + |h| sum |w_j k_j|) -- at most 5 roundings of half an ulp (2^-24 relative each, of partial
results that |y| + |h| sum |w_j k_j| bounds), with slack.  Mel: the project's 2e-4 for up to 8 chained passes at |mel| <= 10
(test_hip_e2e.py); on these inputs the oracle in float32 is 6e-7 .. 9e-7 from itself in float64 (2.2e-5 .. 2.8e-5 with guidance)
and the methods are >= 4e-2 apart, so the bar separates a wrong coefficient from rounding.  Waveform: 1e-4, `cr` exact.  Every
measured distance is printed (pytest -s); profiles/ode_methods.md records them."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_convnext as rc                                          # noqa: E402
import ref_odeint                                                   # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, hip, ode, synth      # noqa: E402
from oracle import ref_cpu                                          # noqa: E402

DEV = "cuda"
TOL_MEL = 2e-4
TOL_WAVEFORM = 1e-4
SENTINEL = 12345.678
PAD = 8                    # sentinel floats either side of an output (keeps it 16-byte aligned)
_CACHE = {}


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def kernel_inputs(n, seed=0):
    """y and four k's of n floats (host), magnitudes of a mel and of a field."""
    return rnd(n, seed=10 * n + seed, scale=3.0), [rnd(n, seed=10 * n + seed + 1 + j, scale=2.0 + j) for j in range(4)]


def combine(y, ks, h, wa, wb=None, alias_a=None, alias_b=None):
    """One launch of fh_rk_combine_f32 on host tensors -> (out_a, out_b or None) on the host.  alias_a / alias_b: 'y' or the
    index of a k the output is written onto.  Outputs of their own are framed by sentinels, which must keep their bits."""
    n, n_k = y.numel(), len(ks)
    yd, kd = y.to(DEV), [k.to(DEV) for k in ks]

    def dest(alias):
        if alias is None:
            buf = torch.full((n + 2 * PAD,), SENTINEL, device=DEV)
            return buf, buf[PAD:PAD + n]
        t = yd if alias == "y" else kd[alias]
        return None, t
    frame_a, out_a = dest(alias_a)
    frame_b, out_b = dest(alias_b) if wb is not None else (None, None)
    kp = (ctypes.c_void_p * n_k)(*[k.data_ptr() for k in kd])
    fa = (ctypes.c_float * n_k)(*wa)
    fb = None if wb is None else (ctypes.c_float * n_k)(*wb)
    hip.check(hip.lib().fh_rk_combine_f32(yd.data_ptr(), kp, n_k, float(h), fa, out_a.data_ptr(), fb, hip.ptr(out_b), n, hip.stream()),
              "fh_rk_combine_f32")
    torch.cuda.synchronize()
    for frame in (frame_a, frame_b):
        if frame is not None:
            f = frame.cpu()
            assert (f[:PAD] == SENTINEL).all() and (f[PAD + n:] == SENTINEL).all(), "an element outside the output was written"
    return out_a.cpu().clone(), None if out_b is None else out_b.cpu().clone()


def exact(y, ks, h, w):
    """(float64 value, error bar) of y + h sum w_j k_j with the weights and h as the kernel gets them (rounded to float32)."""
    w32 = [float(torch.tensor(v, dtype=torch.float32)) for v in w]
    h32 = float(torch.tensor(h, dtype=torch.float32))
    s = sum(wj * k.double() for wj, k in zip(w32, ks) if wj != 0.)
    mag = sum((wj * k.double()).abs() for wj, k in zip(w32, ks) if wj != 0.)
    return y.double() + h32 * s, 2.0 ** -21 * (y.double().abs() + abs(h32) * mag)


# (wa, wb) per n_k: a zero weight first, in the middle and last, negative weights, weights that are no float32
WEIGHTS = {
    1: [((0.75,), (-1 / 3,))],
    2: [((0., 2 / 3), (0.25, 0.)), ((-1 / 3, 1.), (1.7, -0.9))],
    3: [((1., -1., 1.), (1 / 8, 0., 3 / 8)), ((0., 0., -2.5), (0.3, 0.1, 0.))],
    4: [((-0.5, 0., 0.3, 0.), (0., 0., 0., 1.7)), ((0.1, -0.2, 0.3, 0.4), (1 / 8, 3 / 8, 3 / 8, 1 / 8))],
}
NS = [4, 1020, 1024, 1028, 4 * (3 * 256 + 1)]


@pytest.mark.parametrize("n", NS)
def test_combine_against_float64(n):
    y, ks = kernel_inputs(n)
    worst = 0.0
    for n_k, rows in WEIGHTS.items():
        for wa, wb in rows:
            for h in (0.5, -1 / 3):
                one, none = combine(y, ks[:n_k], h, wa)
                two_a, two_b = combine(y, ks[:n_k], h, wa, wb)
                assert none is None and torch.equal(two_a, one), "out_a of the two-output launch differs from the one-output launch"
                only_b, _ = combine(y, ks[:n_k], h, wb)
                assert torch.equal(two_b, only_b)
                for got, w in ((one, wa), (two_b, wb)):
                    ref, bar = exact(y, ks[:n_k], h, w)
                    err = (got.double() - ref).abs()
                    worst = max(worst, (err / bar).max().item())
                    assert (err <= bar).all(), f"n {n}, n_k {n_k}, weights {w}, h {h}: {(err / bar).max().item():.3f} x the bar"
    print(f"fh_rk_combine_f32 n = {n}: worst error / bar {worst:.3f} (bar = 2^-21 (|y| + |h| sum |w k|))")


def test_combine_prefix_aliasing_and_zero_weights():
    y, ks = kernel_inputs(1028)
    wa, wb, h = (1., -1., 1.), (1 / 8, 3 / 8, 3 / 8), 0.5
    # an element depends on its own index alone: the first 1020 of the n = 1028 launch are the n = 1020 launch
    long_a, long_b = combine(y, ks[:3], h, wa, wb)
    short_a, short_b = combine(y[:1020].clone(), [k[:1020].clone() for k in ks[:3]], h, wa, wb)
    assert torch.equal(long_a[:1020], short_a) and torch.equal(long_b[:1020], short_b)
    # outputs onto y and onto a k
    assert torch.equal(combine(y, ks[:3], h, wa, alias_a="y")[0], long_a)
    al_a, al_b = combine(y, ks[:3], h, wa, wb, alias_a="y", alias_b=0)
    assert torch.equal(al_a, long_a) and torch.equal(al_b, long_b)
    al_a, al_b = combine(y, ks[:3], h, wa, wb, alias_a=2, alias_b="y")
    assert torch.equal(al_a, long_a) and torch.equal(al_b, long_b)
    # a term of weight 0 is skipped, not multiplied: what its k holds does not reach the output
    for pos in (0, 1, 2):
        w, v = [0.7, -1.2, 0.4], [-0.3, 0.9, 1.1]
        w[pos] = 0.
        bad = [k.clone() for k in ks[:3]]
        bad[pos][::3] = float("inf")
        bad[pos][1::3] = float("nan")
        clean_a, clean_b = combine(y, ks[:3], h, w, v)
        got_a, got_b = combine(y, bad, h, w, v)          # the k is read for out_b alone
        assert torch.isfinite(got_a).all() and torch.equal(got_a, clean_a) and not torch.isfinite(got_b).all(), f"zero weight at {pos}"
        v[pos] = 0.                                      # and for neither
        clean_a, clean_b = combine(y, ks[:3], h, w, v)
        got_a, got_b = combine(y, bad, h, w, v)
        assert torch.isfinite(got_a).all() and torch.equal(got_a, clean_a), f"zero weight at {pos}"
        assert torch.isfinite(got_b).all() and torch.equal(got_b, clean_b), f"zero weight at {pos}"
        assert torch.equal(combine(y, bad, h, w)[0], clean_a)
    # the argument checks on real device pointers
    L, yd = hip.lib(), y.to(DEV)
    kp, w1 = (ctypes.c_void_p * 1)(yd.data_ptr()), (ctypes.c_float * 1)(1.)
    out = torch.empty_like(yd)
    assert L.fh_rk_combine_f32(yd.data_ptr(), kp, 1, 0.5, w1, out.data_ptr(), w1, out.data_ptr(), 1028, hip.stream()) == -1
    assert b"same buffer" in L.fh_last_error()
    assert L.fh_rk_combine_f32(yd.data_ptr(), kp, 1, 0.5, w1, out.data_ptr() + 4, None, 0, 1024, hip.stream()) == -1
    assert L.fh_rk_combine_f32(yd.data_ptr(), kp, 1, 0.5, (ctypes.c_float * 1)(0.), out.data_ptr(), None, 0, 1028, hip.stream()) == -1
    torch.cuda.synchronize()


# ---- the transformer model -------------------------------------------------------------------------------------------------
CFG, SR_IN, C_SEED = synth.TINY_CFG, 12000, 7
CLIPS = {33: 0.33, 70: 0.7}          # frames: seconds of lowres_clip(7, secs, 12000)
MEL_CASES = [("heun2", 3, 1.), ("heun3", 2, 1.), ("rk4", 1, 1.), ("rk4", 2, 1.), ("rk4", 2, 1.3)]


def model_for(method, **kw):
    if "fh" not in _CACHE:
        _CACHE["sd"] = synth.make_state_dict(CFG, 0)
        _CACHE["fh"] = FLowHigh(_CACHE["sd"], CFG, "cuda")
    return FlowHighSR(_CACHE["fh"], **{**dict(torchdiffeq_ode_method=method), **kw}), _CACHE["sd"]


def clip_case(frames):
    """The clip, its 48 kHz conditioning, log-mel and prior noise: computed once and shared."""
    key = ("clip", frames)
    if key not in _CACHE:
        audio = synth.lowres_clip(C_SEED, CLIPS[frames], SR_IN)
        cond = ref_cpu.preprocess(audio, SR_IN)
        cond_mel = ref_cpu.logmel(cond)
        assert cond_mel.shape[1] == frames
        _CACHE[key] = (audio, cond, cond_mel, synth.prior_noise(C_SEED, frames))
    return _CACHE[key]


def ref_mel(frames, method, steps, cond_scale=1.):
    key = ("mel", frames, method, steps, cond_scale)
    if key not in _CACHE:
        model_for(method)
        sd = _CACHE["sd"]
        _, _, cond_mel, noise = clip_case(frames)
        _CACHE[key] = ref_odeint.sample_mel(lambda y, c, t: ref_cpu.vector_field(sd, y, c, t, cond_scale=cond_scale),
                                            cond_mel, noise, steps, method)
    return _CACHE[key]


@pytest.mark.parametrize("frames", sorted(CLIPS))
@pytest.mark.parametrize("method,steps,cond_scale", MEL_CASES)
def test_mel_against_the_oracle(method, steps, cond_scale, frames):
    m, _ = model_for(method)
    _, cond, _, noise = clip_case(frames)
    ref = ref_mel(frames, method, steps, cond_scale)
    got = m.sample(cond=cond, time_steps=steps, cond_scale=cond_scale, decode_to_audio=False, noise=noise)
    err = (got.cpu() - ref).abs().max().item()
    euler = ref_mel(frames, "euler", steps, cond_scale)
    print(f"mel {method} x {steps}, cond_scale {cond_scale}, {frames} frames: {err:.3e} from the oracle "
          f"(|mel| <= {ref.abs().max().item():.2f}; the oracle's euler x {steps} is {(euler - ref).abs().max().item():.2e} away)")
    assert tuple(got.shape) == tuple(ref.shape) == (1, frames, 256) and err <= TOL_MEL


def test_waveform_against_the_oracle():
    m, sd = model_for("rk4")
    audio, cond, _, noise = clip_case(33)
    with torch.no_grad():
        wav = ref_cpu.bigvgan_forward(sd, CFG, ref_mel(33, "rk4", 1).transpose(1, 2)).squeeze(1)
        ref, cr = ref_cpu.post_processing(wav, cond, cond.size(-1), return_cr=True)
    out, got = m.generate_batch([audio], SR_IN, 48000, 1, noise=noise, return_stages=True)
    e_wav, e_out = (got["wav"].cpu() - wav).abs().max().item(), (out.cpu() - ref).abs().max().item()
    print(f"generate_batch rk4 x 1, 33 frames: vocoder {e_wav:.3e}, final {e_out:.3e} from the oracle, cr {int(got['cr'][0].item())} / {cr}")
    assert int(got["cr"][0].item()) == cr
    assert tuple(out.shape) == tuple(ref.shape) and e_wav <= TOL_WAVEFORM and e_out <= TOL_WAVEFORM


@pytest.mark.parametrize("method", ["rk4", "heun3"])
def test_batch_rows_equal_single_clip_runs(method):
    m, _ = model_for(method)
    clips = [synth.lowres_clip(20 + i, 0.33, SR_IN) for i in range(3)]
    noise = torch.cat([synth.prior_noise(20 + i, 33) for i in range(3)], 0)
    both = m.generate_batch(clips, SR_IN, 48000, 2, noise=noise)
    for i in range(3):
        assert torch.equal(both[i:i + 1], m.generate(clips[i], SR_IN, 48000, 2, noise=noise[i:i + 1])), f"clip {i}"
    other, _ = model_for("midpoint")
    assert not torch.equal(other.generate(clips[0], SR_IN, 48000, 2, noise=noise[:1]), both[:1])          # the method is used


@pytest.mark.parametrize("ends", ["per_clip", "ragged"])
@pytest.mark.parametrize("method", ["rk4", "heun3"])
def test_generate_many_equals_generate_per_clip(method, ends):
    m, _ = model_for(method)
    secs = [0.33, 0.7, 0.5]
    clips = [synth.lowres_clip(140 + i, s_, SR_IN) for i, s_ in enumerate(secs)]
    noise = [synth.prior_noise(140 + i, (len(c) * 4) // 480) for i, c in enumerate(clips)]
    assert [z.shape[1] for z in noise] == [33, 70, 50]
    many = m.generate_many(clips, SR_IN, 48000, 2, noise=noise, ragged=True, ends=ends)
    for i, c in enumerate(clips):
        one = m.generate(c, SR_IN, 48000, 2, noise=noise[i])
        assert tuple(many[i].shape) == tuple(one.shape) == (1, len(c) * 4)
        assert torch.equal(many[i], one), f"clip {i} ({secs[i]} s) differs from generate() alone"


@pytest.mark.parametrize("method", ["rk4", "heun3"])
def test_sample_many_with_guidance_and_mel_pp_equals_sample_per_clip(method):
    m, _ = model_for(method)
    secs = [0.33, 0.7, 0.5]
    conds = [ref_cpu.preprocess(synth.lowres_clip(60 + i, s_, SR_IN), SR_IN)[0] for i, s_ in enumerate(secs)]
    noise = [synth.prior_noise(60 + i, c.shape[0] // 480) for i, c in enumerate(conds)]
    many = m.sample_many(conds, time_steps=2, cond_scale=1.3, mel_pp=True, noise=noise, decode_to_audio=False)
    for c, z, got in zip(conds, noise, many):
        one = m.sample(cond=c[None], time_steps=2, cond_scale=1.3, mel_pp=True, noise=z, decode_to_audio=False)
        assert got.shape == one.shape and torch.equal(got, one)


def test_graph_capture_replays_bit_identical():
    m, _ = model_for("rk4", upsampling_method="hip")
    n_in = 3960
    g = m.capture(2, n_in, SR_IN, 1)
    x = torch.from_numpy(np.stack([synth.lowres_clip(50 + i, n_in / SR_IN, SR_IN) for i in range(2)])).cuda()
    noise = torch.cat([synth.prior_noise(50 + i, 33) for i in range(2)], 0).cuda().reshape(66, -1).contiguous()
    g.x.copy_(x)
    g.noise.copy_(noise)
    got = g.replay().clone()
    assert torch.equal(got, m.generate_from_device(x, SR_IN, 1, noise=noise))


def test_unknown_method_raises_at_the_first_call():
    m, _ = model_for("dopri5")
    _, cond, _, noise = clip_case(33)
    with pytest.raises(NotImplementedError, match=r"euler, midpoint, heun2, heun3, rk4.*adaptive"):
        m.sample(cond=cond, time_steps=1, decode_to_audio=False, noise=noise)


# ---- the ConvNeXt model ----------------------------------------------------------------------------------------------------
def test_convnext_rk4_against_the_restated_field():
    """sample() with rk4 x 1 on the ConvNeXt backbone: ConvNextNet has FlowNet's forward, the stepper is the same."""
    w_seed = 5
    flow = synth.make_convnext_state_dict(w_seed)
    sd = dict(flow, **synth.make_vocoder_state_dict(CFG, w_seed))
    fh = FLowHigh(sd, CFG, "cuda")
    assert fh.architecture == "convnext"
    m = FlowHighSR(fh, torchdiffeq_ode_method="rk4")
    cond = ref_cpu.preprocess(synth.lowres_clip(C_SEED, 0.25, SR_IN), SR_IN)
    noise = synth.prior_noise(C_SEED, 25)
    with torch.no_grad():
        mel = ref_odeint.sample_mel(lambda y, c, t: rc.vector_field(sd, y, c, t), ref_cpu.logmel(cond), noise, 1, "rk4")
        euler = ref_odeint.sample_mel(lambda y, c, t: rc.vector_field(sd, y, c, t), ref_cpu.logmel(cond), noise, 1, "euler")
        ref = ref_cpu.bigvgan_forward(sd, CFG, mel.transpose(1, 2))
    got_mel = m.sample(cond=cond, time_steps=1, noise=noise, decode_to_audio=False)
    got = m.sample(cond=cond, time_steps=1, noise=noise)
    e_mel, e_wav = (got_mel.cpu() - mel).abs().max().item(), (got.cpu() - ref).abs().max().item()
    print(f"convnext rk4 x 1, 25 frames: mel {e_mel:.3e}, waveform {e_wav:.3e} from the CPU path "
          f"(its euler x 1 mel is {(euler - mel).abs().max().item():.2e} away)")
    assert tuple(got.shape) == tuple(ref.shape) and e_wav <= TOL_WAVEFORM          # the bar of test_hip_convnext.py's sample()
