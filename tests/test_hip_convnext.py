"""GPU: the ConvNeXt vector field (FLowHigh(architecture='convnext')) -- the two kernels of csrc/convnext.hip against the float64
restatement (tests/ref_convnext.py), their bit contract (a row's bits depend on its own 7 input rows alone), ConvNextNet against
the restated field, and the model through generate / generate_many / capture / sample.

Bars.  Kernel and net: 4 x the distance of the SAME restatement run in float32 on the CPU to its float64 run on the same inputs
(the kernel sums a row's channels in another order than torch does; both orders carry the same bound), the kernel's never above
5e-6 (the bar of fh_dwconv_gelu_res_f32 and fh_rmsnorm_f32).  Model: the project's 1e-4 on the waveform, `cr` equal.  Every
measured pair is printed (pytest -s); profiles/convnext.md records them.

Model seeds: weights 5, clip / noise 7 -- for them the CPU path in float32 is 2.4e-6 (euler x 1) and 2.4e-6 (midpoint x 2) from
itself in float64 on the final waveform (bar for picking a seed: 2.5e-5), `cr` = 271 in both (checked on the CPU,
profiles/convnext.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ref_convnext as rc                                           # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, convnext, hip, synth  # noqa: E402

DEV = "cuda"
R = convnext.DWLN_ROWS
NS = [1, 2, 3, 4, 6, 7, 8, R - 1, R, R + 1, 2 * R + 3]
KERNEL_CAP = 5e-6
TOL_WAVEFORM = 1e-4
SENTINEL = 12345.678
W_SEED, C_SEED = 5, 7
_CACHE = {}


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def kernel_inputs(dim, n, batch=2, seed=0):
    """x [batch, n, dim] with the rows a LayerNorm can get wrong: |mean| = 50 x std twice, and one all-equal row."""
    x = rnd(batch, n, dim, seed=1000 * dim + 10 * n + seed)
    x[0, 0] = x[0, 0] + 50.0                                  # mean +50, std 1
    x[0, n // 2] = 0.25 * x[0, n // 2] - 12.5 if n > 1 else x[0, n // 2]      # mean -12.5, std 0.25
    x[batch - 1, n - 1] = 3.7                                 # all equal
    w = (torch.rand(dim, 1, 7, generator=torch.Generator().manual_seed(dim + 1)) * 2 - 1) / 7 ** 0.5
    b = rnd(dim, seed=dim + 2, scale=0.3)
    scale, shift = 1.0 + rnd(dim, seed=dim + 3, scale=0.3), rnd(dim, seed=dim + 4, scale=0.3)
    return x, w, b, scale, shift


def run_kernel(x, w, b, scale, shift, seg=None, eps=1e-6):
    """x [batch, n, dim] (or [rows, dim] with seg = list of lengths) through fh_dwconv_ln(_seg)_f32; the output buffer is
    framed by one sentinel row either side, which must keep its bits."""
    dim = x.shape[-1]
    rows = x.numel() // dim
    xd = x.to(DEV).contiguous()
    wd = None if w is None else w.reshape(dim, -1).t().contiguous().to(DEV)          # tap-major [ksz, dim]
    bd = None if w is None else b.to(DEV)
    ksz = 1 if w is None else w.shape[-1]
    sd_, hd = scale.to(DEV), shift.to(DEV)
    buf = torch.full((rows + 2, dim), SENTINEL, device=DEV)
    y = buf[1:rows + 1]
    L, st = hip.lib(), hip.stream()
    if seg is None:
        hip.check(L.fh_dwconv_ln_f32(xd.data_ptr(), hip.ptr(wd), hip.ptr(bd), sd_.data_ptr(), hd.data_ptr(), y.data_ptr(),
                                     x.shape[0], x.shape[1], dim, ksz, eps, st), "fh_dwconv_ln_f32")
    else:
        starts = np.concatenate([[0], np.cumsum(seg)[:-1]])
        table = torch.tensor([[int(s_), int(n)] for s_, n in zip(starts, seg)], dtype=torch.int32).to(DEV)
        hip.check(L.fh_dwconv_ln_seg_f32(xd.data_ptr(), hip.ptr(wd), hip.ptr(bd), sd_.data_ptr(), hd.data_ptr(), y.data_ptr(),
                                         table.data_ptr(), len(seg), max(seg), dim, ksz, eps, st), "fh_dwconv_ln_seg_f32")
    torch.cuda.synchronize()
    out = buf.cpu()
    assert torch.equal(out[0], torch.full((dim,), SENTINEL)) and torch.equal(out[-1], torch.full((dim,), SENTINEL)), \
        "a row outside the output was written"
    return out[1:-1].reshape(x.shape)


@pytest.mark.parametrize("conv", [True, False], ids=["dwconv7", "no_conv"])
@pytest.mark.parametrize("dim", [256, 1024])
def test_dwconv_ln_against_float64(dim, conv):
    e32, ek = 0.0, 0.0
    for n in NS:
        x, w, b, scale, shift = kernel_inputs(dim, n)
        if not conv:
            w = b = None
        d = lambda t: None if t is None else t.double()
        ref64 = rc.dwconv_ln(x.double(), d(w), d(b), scale.double(), shift.double())
        ref32 = rc.dwconv_ln(x, w, b, scale, shift)
        got = run_kernel(x, w, b, scale, shift)
        assert torch.isfinite(got).all()
        e32 = max(e32, (ref32.double() - ref64).abs().max().item())
        ek = max(ek, (got.double() - ref64).abs().max().item())
    bar = min(4.0 * e32, KERNEL_CAP)
    print(f"fh_dwconv_ln_f32 dim {dim} {'k=7' if conv else 'no conv'}: fp32 CPU restatement {e32:.3e} from float64, kernel {ek:.3e}, bar {bar:.3e}")
    assert ek <= bar


@pytest.mark.parametrize("conv", [True, False], ids=["dwconv7", "no_conv"])
@pytest.mark.parametrize("dim", [256, 1024])
def test_a_rows_bits_depend_on_its_own_input_rows_alone(dim, conv):
    """Clip alone == the same clip inside B = 3 == the same clip in a segment launch of lengths (1, 3, n, 7); other
    neighbours leave its bits unchanged."""
    for n in NS:
        x, w, b, scale, shift = kernel_inputs(dim, n, batch=1)
        if not conv:
            w = b = None
        alone = run_kernel(x, w, b, scale, shift)
        for seed in (1, 2):                                    # two sets of neighbours
            nb = rnd(2, n, dim, seed=77 * n + seed, scale=3.0)
            in_batch = run_kernel(torch.cat([nb[:1], x, nb[1:]], 0), w, b, scale, shift)
            assert torch.equal(in_batch[1:2], alone), f"n = {n}: the clip inside B = 3 differs from the clip alone"
            others = [rnd(m, dim, seed=13 * m + seed, scale=3.0) for m in (1, 3, 7)]
            packed = torch.cat([others[0], others[1], x[0], others[2]], 0)
            in_seg = run_kernel(packed, w, b, scale, shift, seg=[1, 3, n, 7])
            assert torch.equal(in_seg[4:4 + n], alone[0]), f"n = {n}: the clip in a segment launch differs from the clip alone"


def test_dwconv_ln_shorter_kernels_and_argument_errors():
    dim, n = 256, 9
    x, w, b, scale, shift = kernel_inputs(dim, n)
    for k in (1, 3, 5):                                        # odd ksz <= 7: centred, same arithmetic
        wk = w[..., :k].contiguous()
        ref = rc.dwconv_ln(x.double(), wk.double(), b.double(), scale.double(), shift.double())
        assert (run_kernel(x, wk, b, scale, shift).double() - ref).abs().max().item() <= KERNEL_CAP
    L, st = hip.lib(), hip.stream()
    xd, yd = x.to(DEV), torch.empty_like(x, device=DEV)
    wd, v = torch.zeros(9, dim, device=DEV), torch.zeros(dim + 4, device=DEV)
    seg = torch.tensor([[0, n], [n, n]], dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    call = lambda x_=p(xd), dim_=dim, k_=7, n_=n, y_=p(yd): L.fh_dwconv_ln_f32(x_, p(wd), p(v), p(v), p(v), y_, 2, n_, dim_, k_, 1e-6, st)
    assert call() == 0
    assert call(dim_=200) == -1 and b"dim 200" in L.fh_last_error()
    assert call(k_=4) == -1 and call(k_=9) == -1 and b"ksz 9" in L.fh_last_error()
    assert call(n_=0) == -1
    assert call(x_=p(xd) + 4) == -1 and b"aligned" in L.fh_last_error()
    assert call(y_=p(yd) + 8) == -1
    assert L.fh_dwconv_ln_f32(p(xd), p(wd), p(v), p(v) + 4, p(v), p(yd), 2, n, dim, 7, 1e-6, st) == -1
    for bad in (dict(dim=200), dict(k=4), dict(k=9), dict(max_n=0), dict(n_seg=0)):
        a = dict(dim=dim, k=7, max_n=n, n_seg=2, **{}) | bad
        assert L.fh_dwconv_ln_seg_f32(p(xd), p(wd), p(v), p(v), p(v), p(yd), p(seg), a["n_seg"], a["max_n"], a["dim"], a["k"], 1e-6, st) == -1
    assert L.fh_dwconv_ln_seg_f32(p(xd) + 4, p(wd), p(v), p(v), p(v), p(yd), p(seg), 2, n, dim, 7, 1e-6, st) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_gelu(n):
    x = rnd(n, seed=n, scale=2.5)
    x[0] = -7.0 if n > 1 else x[0]
    ref = F.gelu(x)
    L, st = hip.lib(), hip.stream()
    xd = x.to(DEV)
    buf = torch.full((n + 8,), SENTINEL, device=DEV)
    y = buf[4:4 + n]                                           # 16-byte aligned, framed by sentinels
    hip.check(L.fh_gelu_f32(xd.data_ptr(), y.data_ptr(), n, st), "fh_gelu_f32")
    odd = torch.full((n + 2,), SENTINEL, device=DEV)           # a destination that is not 16-byte aligned: same bits
    hip.check(L.fh_gelu_f32(xd.data_ptr(), odd[1:1 + n].data_ptr(), n, st), "fh_gelu_f32")
    inplace = xd.clone()
    hip.check(L.fh_gelu_f32(inplace.data_ptr(), inplace.data_ptr(), n, st), "fh_gelu_f32")
    torch.cuda.synchronize()
    out = buf.cpu()
    assert (out[:4] == SENTINEL).all() and (out[4 + n:] == SENTINEL).all()
    assert (out[4:4 + n] - ref).abs().max().item() <= 5e-5      # the bar of test_gemm_geglu_packed
    assert torch.equal(inplace.cpu(), out[4:4 + n]) and torch.equal(odd.cpu()[1:1 + n], out[4:4 + n])
    assert float(odd[0]) == float(odd[-1]) == pytest.approx(SENTINEL)
    assert L.fh_gelu_f32(xd.data_ptr(), y.data_ptr(), 0, st) == -1 and L.fh_gelu_f32(0, y.data_ptr(), n, st) == -1


# ---- the net ---------------------------------------------------------------------------------------------------------------
def flow_sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = synth.make_convnext_state_dict(W_SEED)
        _CACHE["sd64"] = rc.cast(_CACHE["sd"], torch.float64)
    return _CACHE["sd"]


def net_for(bf):
    if ("net", bf) not in _CACHE:
        _CACHE[("net", bf)] = convnext.ConvNextNet(flow_sd(), DEV, bf=bf)
    return _CACHE[("net", bf)]


def net_case(batch, n, t):
    """Inputs and the two CPU runs of the restated field, computed once and shared by the bf = False / True cases."""
    key = ("case", batch, n, t)
    if key not in _CACHE:
        sd = flow_sd()
        x, cond = rnd(batch, n, 256, seed=n), rnd(batch, n, 256, seed=n + 1) * 2.0 - 3.0
        res = rnd(batch, n, 256, seed=n + 2)
        with torch.no_grad():
            v64 = rc.convnext_forward(_CACHE["sd64"], x.double(), cond.double(), t)
            v32 = rc.convnext_forward(sd, x, cond, t)
            null = sd[rc.FH + "null_cond"].expand_as(cond)
            n64 = rc.convnext_forward(_CACHE["sd64"], x.double(), null.double(), t)
            n32 = rc.convnext_forward(sd, x, null, t)
        _CACHE[key] = (x, cond, res, v64, v32, n64, n32)
    return _CACHE[key]


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16x6"])
@pytest.mark.parametrize("batch,n,t", [(1, 5, 0.0), (2, 40, 0.3), (1, 300, 0.5)])
def test_net_forward_against_the_restated_field(batch, n, t, bf):
    x, cond, res, v64, v32, n64, n32 = net_case(batch, n, t)
    net = net_for(bf)
    M = batch * n
    xd, cd, rd = (a.reshape(M, 256).contiguous().to(DEV) for a in (x, cond, res))
    net.set_cond(cd, batch, n)
    out = torch.empty(M, 256, device=DEV)
    v = net.forward(xd, t, out, batch, n).cpu().view(batch, n, 256).clone()
    axpy = net.forward(xd, t, out, batch, n, alpha=0.5, res=rd).cpu().view(batch, n, 256).clone()
    null = net.forward(xd, t, out, batch, n, null_cond=True).cpu().view(batch, n, 256).clone()
    e32 = max((v32.double() - v64).abs().max().item(), (n32.double() - n64).abs().max().item())
    bar = 4.0 * e32
    ev, ea, en = ((a.double() - b).abs().max().item() for a, b in ((v, v64), (axpy, 0.5 * v64 + res.double()), (null, n64)))
    print(f"ConvNextNet (B, n, t) = ({batch}, {n}, {t}) {'bf16x6' if bf else 'f32'}: fp32 CPU restatement {e32:.3e} from float64; "
          f"net {ev:.3e}, alpha / res {ea:.3e}, null_cond {en:.3e}; bar {bar:.3e}")
    assert max(ev, ea, en) <= bar


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16x6"])
def test_net_ragged_rows_equal_each_clip_alone(bf):
    net = net_for(bf)
    frames = (5, 40, 17)
    xs = [rnd(n, 256, seed=300 + n).to(DEV) for n in frames]
    cs = [(rnd(n, 256, seed=400 + n) * 2.0 - 3.0).to(DEV) for n in frames]
    alone = []
    for x, c, n in zip(xs, cs, frames):
        net.set_cond(c, 1, n)
        alone.append(net.forward(x, 0.3, torch.empty(n, 256, device=DEV), 1, n, alpha=0.7, res=x).clone())
    ws = net.ragged_workspace(frames)
    net.set_cond(torch.cat(cs, 0), len(frames), max(frames), ragged=ws)
    xp = torch.cat(xs, 0)
    got = net.forward(xp, 0.3, torch.empty_like(xp), len(frames), max(frames), alpha=0.7, res=xp, ragged=ws)
    r = 0
    for i, n in enumerate(frames):
        assert torch.equal(got[r:r + n], alone[i]), f"clip {i} ({n} frames) in the ragged rows differs from the clip alone"
        r += n


# ---- the model -------------------------------------------------------------------------------------------------------------
def model_for(method="euler", **kw):
    if "fh" not in _CACHE:
        cfg = synth.TINY_CFG
        sd = dict(flow_sd(), **synth.make_vocoder_state_dict(cfg, W_SEED))
        _CACHE["full_sd"] = sd
        _CACHE["fh"] = FLowHigh(sd, cfg, "cuda")                 # architecture detected from the keys
        assert _CACHE["fh"].architecture == "convnext" and isinstance(_CACHE["fh"].net, convnext.ConvNextNet)
        assert _CACHE["fh"].attn_window is None and _CACHE["fh"].attn_form is None
    return FlowHighSR(_CACHE["fh"], **{**dict(torchdiffeq_ode_method=method), **kw}), _CACHE["full_sd"]


@pytest.mark.parametrize("method,steps", [("euler", 1), ("midpoint", 2)])
def test_generate_vs_cpu_path(method, steps):
    """generate() against the CPU path: the oracle's front end, vocoder and post-processing around the restated field."""
    cfg, sr_in = synth.TINY_CFG, 12000
    m, sd = model_for(method)
    audio, noise = synth.lowres_clip(C_SEED, 0.25, sr_in), synth.prior_noise(C_SEED, 25)
    ref, cr = rc.generate(sd, cfg, audio, sr_in, noise, steps, method)
    out, got = m.generate_batch([audio], sr_in, 48000, steps, noise=noise, return_stages=True)
    err = (out.cpu() - ref).abs().max().item()
    print(f"generate {method} x {steps}: {err:.3e} from the CPU path, cr {int(got['cr'][0].item())} / {cr}")
    assert int(got["cr"][0].item()) == cr
    assert tuple(out.shape) == tuple(ref.shape) and err <= TOL_WAVEFORM


def test_named_architecture_and_keyword_errors_on_the_device():
    m, sd = model_for()
    with pytest.raises(RuntimeError, match="loading state_dict"):
        FLowHigh(sd, synth.TINY_CFG, "cuda", architecture="transformer")
    with pytest.raises(ValueError, match="convnext"):
        FLowHigh(sd, synth.TINY_CFG, "cuda", attn_window=500)
    with pytest.raises(ValueError, match="convnext"):
        FLowHigh(sd, synth.TINY_CFG, "cuda", architecture="convnext", attn_form="bf16x6")


@pytest.mark.parametrize("ends", ["per_clip", "ragged"])
def test_generate_many_equals_generate_per_clip(ends):
    m, _ = model_for()
    secs = [0.25, 0.61, 0.2]
    clips = [synth.lowres_clip(140 + i, s_, 12000) for i, s_ in enumerate(secs)]
    noise = [synth.prior_noise(140 + i, (len(c) * 4) // 480) for i, c in enumerate(clips)]
    many = m.generate_many(clips, 12000, 48000, 1, noise=noise, ragged=True, ends=ends)
    for i, c in enumerate(clips):
        one = m.generate(c, 12000, 48000, 1, noise=noise[i])
        assert tuple(many[i].shape) == tuple(one.shape) == (1, len(c) * 4)
        assert torch.equal(many[i], one), f"clip {i} ({secs[i]} s) differs from generate() alone"


def test_graph_capture_replays_bit_identical():
    m, _ = model_for(upsampling_method="hip")
    n_in = 3000
    g = m.capture(2, n_in, 12000, 1)
    x = torch.from_numpy(np.stack([synth.lowres_clip(50 + i, n_in / 12000, 12000) for i in range(2)])).cuda()
    noise = torch.cat([synth.prior_noise(50 + i, 25) for i in range(2)], 0).cuda().reshape(50, -1).contiguous()
    g.x.copy_(x)
    g.noise.copy_(noise)
    got = g.replay().clone()
    assert torch.equal(got, m.generate_from_device(x, 12000, 1, noise=noise))


def test_sample_with_classifier_free_guidance():
    """cond_scale = 1.3 through sample(): two evaluations per step, the second against null_cond, chained in the GEMM epilogues."""
    cfg = synth.TINY_CFG
    m, sd = model_for()
    cond = rc.ref_cpu.preprocess(synth.lowres_clip(C_SEED, 0.25, 12000), 12000)
    noise = synth.prior_noise(C_SEED, 25)
    ref = rc.sample(sd, cfg, cond, noise, 1, "euler", cond_scale=1.3)
    got = m.sample(cond=cond, time_steps=1, cond_scale=1.3, noise=noise)
    assert tuple(got.shape) == tuple(ref.shape)
    assert (got.cpu() - ref).abs().max().item() <= TOL_WAVEFORM
    plain = m.sample(cond=cond, time_steps=1, noise=noise)
    assert not torch.equal(plain, got)
