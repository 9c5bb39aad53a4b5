"""GPU: clips of different STEP COUNTS in one ragged sequence -- the grouped entries of csrc/steps.hip against their one-time twins,
FlowNet's grouped forward, generate_many(timestep=[s_0, ...]) / sample_many(time_steps=[...]) against generate() / sample() per
clip, and BatchingServer(mix_steps=True).

The contract is bitwise: a row of group g gets what the twin entry gives with that group's scalar, clip i of a mixed call gets
what generate(clip_i, sr_i, timestep=steps[i]) gives.  Every comparison is torch.equal unless it says otherwise; outputs are
NaN-filled first and followed by a NaN guard that must survive."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, ode, synth             # noqa: E402
from flowhigh_amd import tables                                            # noqa: E402
from flowhigh_amd.packing import pack_gemm_bf_weight                       # noqa: E402
from flowhigh_amd.serve import BatchingServer                              # noqa: E402

GUARD = 64
_STATE = {}
TIMES = {1: [1.0], 3: [0.0, float(np.float32(1 / 3)), 1.0],
         8: [0.0, float(np.float32(0.1)), 0.25, float(np.float32(1 / 3)), 0.5, float(np.float32(2 / 3)), float(np.float32(0.9)), 1.0]}
EIGHT_ENDS = (1, 2, 3, 5, 6, 8, 9, 11)


def rnd(shape, seed, scale=1.0):
    shape = (shape,) if isinstance(shape, int) else shape
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def st():
    return hip.stream()


def ranges(ends):
    return list(zip((0,) + tuple(ends[:-1]), ends))


def refused(rc, name):
    assert rc == -1 and name.encode() in hip.lib().fh_last_error(), (rc, hip.lib().fh_last_error())


BAD_GROUPS = [hip.RowGroups(0, (ctypes.c_int32 * 8)()), hip.row_groups([1, 2, 3, 4, 5, 6, 7, 8, 9]), hip.row_groups([4, 4, 9]),
              hip.row_groups([5, 3, 9]), hip.row_groups([0, 9])]


# ------------------------------------------------------------------------------------------
# the entries
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [5, 512])
@pytest.mark.parametrize("G", [1, 3, 8])
def test_time_fourier_groups_equals_the_entry_per_time(half, G):
    L, name = hip.lib(), "fh_time_fourier_groups_f32"
    w = rnd(half, 3)
    out = nan(G * 2 * half + GUARD)
    hip.check(L.fh_time_fourier_groups_f32(w.data_ptr(), hip.group_floats(TIMES[G]), out.data_ptr(), half, G, st()), name)
    for g, t in enumerate(TIMES[G]):
        ref = nan(2 * half)
        hip.check(L.fh_time_fourier_f32(w.data_ptr(), t, ref.data_ptr(), half, st()), "fh_time_fourier_f32")
        assert torch.isfinite(ref).all() and torch.equal(out[g * 2 * half:(g + 1) * 2 * half], ref), (g, t)
    assert torch.isnan(out[-GUARD:]).all()
    bad = nan(2 * half)
    for n in (0, 9):
        refused(L.fh_time_fourier_groups_f32(w.data_ptr(), hip.group_floats(TIMES[8]), bad.data_ptr(), half, n, st()), name)
    refused(L.fh_time_fourier_groups_f32(0, hip.group_floats([0.5]), bad.data_ptr(), half, 1, st()), name)
    refused(L.fh_time_fourier_groups_f32(w.data_ptr(), None, bad.data_ptr(), half, 1, st()), name)
    refused(L.fh_time_fourier_groups_f32(w.data_ptr(), hip.group_floats([0.5]), 0, half, 1, st()), name)
    assert torch.isnan(bad).all()


@pytest.mark.parametrize("N,K", [(6, 256), (1027, 1024), (8, 260)])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_gemv_rows_equals_the_gemv_per_vector(N, K, T):
    L, name = hip.lib(), "fh_gemv_rows_f32"
    ldx, ldy = K + 8, N + 3
    W, X, b = rnd((N, K), 5, K ** -0.5), rnd((T, ldx), 6), rnd(N, 7)
    for act in (0, 1):
        for bias in (b, None):
            Y = nan(T * ldy + GUARD)
            hip.check(L.fh_gemv_rows_f32(W.data_ptr(), X.data_ptr(), ldx, hip.ptr(bias), Y.data_ptr(), ldy, N, K, T, act, st()), name)
            for j in range(T):
                ref = nan(N)
                hip.check(L.fh_gemv_f32(W.data_ptr(), X[j].data_ptr(), hip.ptr(bias), ref.data_ptr(), N, K, act, st()), "fh_gemv_f32")
                assert torch.isfinite(ref).all() and torch.equal(Y[j * ldy:j * ldy + N], ref), (act, bias is None, j)
                assert torch.isnan(Y[j * ldy + N:(j + 1) * ldy]).all()
            assert torch.isnan(Y[-GUARD:]).all()
    bad = nan(T * ldy)
    for t_bad in (0, 9):
        refused(L.fh_gemv_rows_f32(W.data_ptr(), X.data_ptr(), ldx, 0, bad.data_ptr(), ldy, N, K, t_bad, 0, st()), name)
    refused(L.fh_gemv_rows_f32(0, X.data_ptr(), ldx, 0, bad.data_ptr(), ldy, N, K, T, 0, st()), name)
    refused(L.fh_gemv_rows_f32(W.data_ptr(), 0, ldx, 0, bad.data_ptr(), ldy, N, K, T, 0, st()), name)
    refused(L.fh_gemv_rows_f32(W.data_ptr(), X.data_ptr(), ldx, 0, 0, ldy, N, K, T, 0, st()), name)
    refused(L.fh_gemv_rows_f32(W.data_ptr(), X.data_ptr(), K - 4, 0, bad.data_ptr(), ldy, N, K, T, 0, st()), name)
    refused(L.fh_gemv_rows_f32(W.data_ptr(), X.data_ptr(), ldx, 0, bad.data_ptr(), N - 1, N, K, T, 0, st()), name)
    assert torch.isnan(bad).all()


@pytest.mark.parametrize("dim", [256, 1024])
@pytest.mark.parametrize("ends", [(1, 5, 9), (4, 8), EIGHT_ENDS, (9,)])
def test_rmsnorm_groups_equals_the_rmsnorm_per_group(dim, ends):
    L, name = hip.lib(), "fh_rmsnorm_groups_f32"
    rows, G, stride = ends[-1], len(ends), 3 * dim + 4
    x, gb = rnd((rows, dim), 11), rnd((G, stride), 12)               # group g: gamma at gb[g, :dim], beta at gb[g, dim:2 dim]
    for with_beta in (True, False):
        y = nan(rows * dim + GUARD)
        beta0 = gb[0, dim:].data_ptr() if with_beta else 0
        hip.check(L.fh_rmsnorm_groups_f32(x.data_ptr(), gb.data_ptr(), beta0, stride, y.data_ptr(), rows, dim,
                                          ctypes.byref(hip.row_groups(ends)), st()), name)
        for g, (r0, r1) in enumerate(ranges(ends)):
            ref = nan((r1 - r0) * dim)
            hip.check(L.fh_rmsnorm_f32(x[r0:r1].data_ptr(), gb[g].data_ptr(), gb[g, dim:].data_ptr() if with_beta else 0,
                                       ref.data_ptr(), r1 - r0, dim, st()), "fh_rmsnorm_f32")
            assert torch.isfinite(ref).all() and torch.equal(y[r0 * dim:r1 * dim], ref), (with_beta, g)
        assert torch.isnan(y[-GUARD:]).all()
    bad = nan(rows * dim)
    for grp in BAD_GROUPS + [hip.row_groups(ends[:-1] + (rows + 1,))]:
        refused(L.fh_rmsnorm_groups_f32(x.data_ptr(), gb.data_ptr(), 0, stride, bad.data_ptr(), rows, dim, ctypes.byref(grp), st()), name)
    good = ctypes.byref(hip.row_groups(ends))
    refused(L.fh_rmsnorm_groups_f32(0, gb.data_ptr(), 0, stride, bad.data_ptr(), rows, dim, good, st()), name)
    refused(L.fh_rmsnorm_groups_f32(x.data_ptr(), 0, 0, stride, bad.data_ptr(), rows, dim, good, st()), name)
    refused(L.fh_rmsnorm_groups_f32(x.data_ptr(), gb.data_ptr(), 0, stride, 0, rows, dim, good, st()), name)
    refused(L.fh_rmsnorm_groups_f32(x.data_ptr(), gb.data_ptr(), 0, stride, bad.data_ptr(), rows, dim, None, st()), name)
    refused(L.fh_rmsnorm_groups_f32(x.data_ptr(), gb.data_ptr(), 0, stride, bad.data_ptr(), rows, 384, good, st()), name)
    assert torch.isnan(bad).all()


ALPHAS = [float(np.float32(a)) for a in (0.25, 1 / 3, -0.7, 1.0, 0.125, 1e-3, 2 / 3, 0.9)]


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("ends", [(1, 5, 9), (4, 9), (1, 2, 3, 4, 5, 6, 7, 9)])
def test_axpy_groups_equals_the_gemm_epilogue(bf, ends):
    """hip.gemm(alpha=a_g, R=res) on every group's rows against hip.gemm(alpha=1, R=None) on all rows followed by the grouped update."""
    L, name = hip.lib(), "fh_axpy_groups_f32"
    M, N, K = 9, 256, 256
    A, W, res = rnd((M, K), 21), rnd((N, K), 22, K ** -0.5), rnd((M, N), 23)
    Wd = pack_gemm_bf_weight(W.cpu()).cuda() if bf else W
    alphas = ALPHAS[:len(ends)]
    raw = nan(M, N)
    hip.gemm(A, Wd, raw, M, N, K, bf=bf)
    assert torch.isfinite(raw).all()
    grp = hip.row_groups(ends)
    for R in (res, None):
        ref = nan(M, N)
        for (r0, r1), a in zip(ranges(ends), alphas):
            hip.gemm(A[r0:r1], Wd, ref[r0:r1], r1 - r0, N, K, alpha=a, R=None if R is None else R[r0:r1], bf=bf)
        out = nan(M * N + GUARD)
        hip.check(L.fh_axpy_groups_f32(raw.data_ptr(), hip.group_floats(alphas), hip.ptr(R), out.data_ptr(), M, N, ctypes.byref(grp), st()),
                  name)
        got = out[:M * N].view(M, N)
        assert torch.isfinite(ref).all() and torch.equal(got, ref), f"with res: {R is not None}"
        assert torch.isnan(out[-GUARD:]).all()
        # beside the bits: within 2^-22 (|alpha v| + |res|) of the float64 update of the raw field
        a_rows = torch.tensor(np.repeat(alphas, [r1 - r0 for r0, r1 in ranges(ends)]), dtype=torch.float64, device="cuda")[:, None]
        av = a_rows * raw.double()
        want = av + (0 if R is None else R.double())
        bound = 2.0 ** -22 * (av.abs() + (0 if R is None else R.double().abs()))
        assert bool(((got.double() - want).abs() <= bound).all())
    # in place (out = v): what went into a fresh buffer (the last pass above: no res)
    v = raw.clone()
    hip.check(L.fh_axpy_groups_f32(v.data_ptr(), hip.group_floats(alphas), 0, v.data_ptr(), M, N, ctypes.byref(grp), st()), name)
    assert torch.equal(v, ref)
    bad = nan(M * N)
    for g in BAD_GROUPS:
        refused(L.fh_axpy_groups_f32(raw.data_ptr(), hip.group_floats(ALPHAS), 0, bad.data_ptr(), M, N, ctypes.byref(g), st()), name)
    refused(L.fh_axpy_groups_f32(0, hip.group_floats(alphas), 0, bad.data_ptr(), M, N, ctypes.byref(grp), st()), name)
    refused(L.fh_axpy_groups_f32(raw.data_ptr(), None, 0, bad.data_ptr(), M, N, ctypes.byref(grp), st()), name)
    refused(L.fh_axpy_groups_f32(raw.data_ptr(), hip.group_floats(alphas), 0, 0, M, N, ctypes.byref(grp), st()), name)
    refused(L.fh_axpy_groups_f32(raw.data_ptr(), hip.group_floats(alphas), 0, bad.data_ptr(), M, N, None, st()), name)
    refused(L.fh_axpy_groups_f32(raw.data_ptr(), hip.group_floats(alphas), 0, bad.data_ptr(), M, 254, ctypes.byref(grp), st()), name)
    assert torch.isnan(bad).all()


def combine(entry_args, groups=None):
    """One launch of fh_rk_combine_f32 / fh_rk_combine_groups_f32 over device tensors."""
    y, ks, h, wa, out_a, wb, out_b, shape = entry_args
    L = hip.lib()
    kp = (ctypes.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
    fa = (ctypes.c_float * len(ks))(*wa)
    fb = None if wb is None else (ctypes.c_float * len(ks))(*wb)
    if groups is None:
        return L.fh_rk_combine_f32(y.data_ptr(), kp, len(ks), float(h), fa, out_a.data_ptr(), fb, hip.ptr(out_b), shape[0] * shape[1], st())
    return L.fh_rk_combine_groups_f32(y.data_ptr(), kp, len(ks), hip.group_floats(h), fa, out_a.data_ptr(), fb, hip.ptr(out_b),
                                      shape[0], shape[1], ctypes.byref(groups), st())


@pytest.mark.parametrize("ends", [(1, 5, 9), (4, 9), EIGHT_ENDS])
@pytest.mark.parametrize("dim", [256, 260])
def test_rk_combine_groups_equals_the_combine_per_group(ends, dim):
    name = "fh_rk_combine_groups_f32"
    rows, G = ends[-1], len(ends)
    hs = ALPHAS[:G]
    y = rnd((rows, dim), 31)
    ks = [rnd((rows, dim), 32 + j) for j in range(4)]
    ks[1][:] = float("nan")                                          # a NaN k behind a zero weight must not reach the result
    grp = hip.row_groups(ends)
    cases = [((0.5, 0.0, 0.25, -1.0), None), ((1 / 3, 0.0, 0.0, 1.0), (0.125, 0.0, 0.375, 0.0)), ((0.0, 0.0, 1.0, 0.0), (0.5, 0.0, 0.0, 0.5))]
    for wa, wb in cases:
        out_a, out_b = nan(rows * dim + GUARD), (None if wb is None else nan(rows * dim + GUARD))
        hip.check(combine((y, ks, hs, wa, out_a, wb, out_b, (rows, dim)), grp), name)
        for (r0, r1), h in zip(ranges(ends), hs):
            ref_a, ref_b = nan((r1 - r0) * dim), (None if wb is None else nan((r1 - r0) * dim))
            hip.check(combine((y[r0:r1], [k[r0:r1] for k in ks], h, wa, ref_a, wb, ref_b, (r1 - r0, dim))), "fh_rk_combine_f32")
            assert torch.isfinite(ref_a).all() and torch.equal(out_a[r0 * dim:r1 * dim], ref_a), (wa, r0)
            if wb is not None:
                assert torch.isfinite(ref_b).all() and torch.equal(out_b[r0 * dim:r1 * dim], ref_b), (wb, r0)
        assert torch.isnan(out_a[-GUARD:]).all() and (out_b is None or torch.isnan(out_b[-GUARD:]).all())
    # an output aliasing y: the same values as into a fresh buffer
    wa, wb = cases[1]
    fresh_a, fresh_b = nan(rows, dim), nan(rows, dim)
    hip.check(combine((y, ks, hs, wa, fresh_a, wb, fresh_b, (rows, dim)), grp), name)
    y2 = y.clone()
    hip.check(combine((y2, ks, hs, wa, y2, wb, fresh_b.clone().fill_(float("nan")), (rows, dim)), grp), name)
    assert torch.equal(y2, fresh_a)
    bad = nan(rows, dim)
    for g in BAD_GROUPS + [hip.row_groups(ends[:-1] + (rows + 1,))]:
        refused(combine((y, ks, ALPHAS, cases[0][0], bad, None, None, (rows, dim)), g), name)
    refused(combine((y, ks, hs, (0.0, 0.0, 0.0, 0.0), bad, None, None, (rows, dim)), grp), name)
    L = hip.lib()
    kp = (ctypes.c_void_p * 1)(ks[0].data_ptr())
    w1 = (ctypes.c_float * 1)(1.0)
    refused(L.fh_rk_combine_groups_f32(0, kp, 1, hip.group_floats(hs), w1, bad.data_ptr(), None, 0, rows, dim, ctypes.byref(grp), st()), name)
    refused(L.fh_rk_combine_groups_f32(y.data_ptr(), kp, 1, None, w1, bad.data_ptr(), None, 0, rows, dim, ctypes.byref(grp), st()), name)
    refused(L.fh_rk_combine_groups_f32(y.data_ptr(), kp, 1, hip.group_floats(hs), w1, 0, None, 0, rows, dim, ctypes.byref(grp), st()), name)
    refused(L.fh_rk_combine_groups_f32(y.data_ptr(), kp, 1, hip.group_floats(hs), w1, bad.data_ptr(), None, 0, rows, dim, None, st()), name)
    refused(L.fh_rk_combine_groups_f32(y.data_ptr(), kp, 1, hip.group_floats(hs), w1, bad.data_ptr(), w1, bad.data_ptr(), rows, dim,
                                       ctypes.byref(grp), st()), name)
    assert torch.isnan(bad).all()


# ------------------------------------------------------------------------------------------
# FlowNet: the grouped raw forward against the ragged forward of each group's clips alone
# ------------------------------------------------------------------------------------------
def flowhigh(**kw):
    key = ("fh",) + tuple(sorted(kw.items()))
    if key not in _STATE:
        cfg = synth.TINY_CFG
        if "sd" not in _STATE:
            _STATE["sd"] = synth.make_state_dict(cfg, 0)
        _STATE[key] = FLowHigh(_STATE["sd"], cfg, "cuda", **kw)
    return _STATE[key]


@pytest.mark.parametrize("null_cond", [False, True])
def test_flownet_grouped_forward_equals_the_ragged_forward_per_group(null_cond):
    net = flowhigh().net
    frames, d = (12, 7, 20), net.dim_in
    t_a, t_b = float(np.float32(1 / 3)), 0.75
    x, cond = rnd((39, d), 41), rnd((39, d), 42)
    refs = []
    for sl, fr, t in ((slice(0, 19), (12, 7), t_a), (slice(19, 39), (20,), t_b)):
        ws = net.ragged_workspace(fr)
        net.set_cond(cond[sl].contiguous(), len(fr), max(fr), ragged=ws)
        refs.append(net.forward(x[sl].contiguous(), t, nan(sl.stop - sl.start, d), len(fr), max(fr), null_cond=null_cond, ragged=ws).clone())
    ws = net.ragged_workspace(frames)
    net.set_cond(cond, 3, 20, ragged=ws)
    out = nan(39 + 1, d)
    net.forward(x, None, out, 0, 0, null_cond=null_cond, ragged=ws, groups=((19, 39), (t_a, t_b)), n_seg=3)
    assert torch.isfinite(out[:39]).all() and torch.equal(out[:19], refs[0]) and torch.equal(out[19:39], refs[1])
    assert torch.isnan(out[39:]).all()
    assert not torch.equal(refs[0][:12], refs[1][:12])
    # the prefix: two of the three segments, one group; the rows behind it are not written
    out2 = nan(39, d)
    net.forward(x, None, out2, 0, 0, null_cond=null_cond, ragged=ws, groups=((19,), (t_a,)), n_seg=2)
    assert torch.equal(out2[:19], refs[0]) and torch.isnan(out2[19:]).all()
    with pytest.raises(ValueError):
        net.forward(x, None, out2, 0, 0, ragged=ws, groups=((19, 38), (t_a, t_b)), n_seg=3)
    with pytest.raises(ValueError):
        net.forward(x, None, out2, 0, 0, groups=((19, 39), (t_a, t_b)))


# ------------------------------------------------------------------------------------------
# end to end: generate_many(timestep=[...]) against generate() per clip
# ------------------------------------------------------------------------------------------
MIX = [(0.1, 12000), (0.3, 16000), (0.2, 12000), (0.15, 16000)]
RATES = [sr for _, sr in MIX]
STEPS = [1, 4, 2, 4]


def model_for(method="euler", cfm="basic_cfm", prior="reference", **net_kw):
    return FlowHighSR(flowhigh(**net_kw), sigma=1e-4 if cfm != "basic_cfm" else 0.0, cfm_method=cfm, torchdiffeq_ode_method=method,
                      upsampling_method="hip", prior=prior)


def clip_list():
    if "clips" not in _STATE:
        clips = [synth.lowres_clip(400 + i, s_, sr) for i, (s_, sr) in enumerate(MIX)]
        t48 = [tables.resample_out_len(len(c), 48000, sr) for c, sr in zip(clips, RATES)]
        assert [t // 480 for t in t48] == [10, 30, 20, 15]
        _STATE["clips"] = clips, [synth.prior_noise(400 + i, t // 480) for i, t in enumerate(t48)], t48
    return _STATE["clips"]


def alone(tag, m, steps, prior_of, **kw):
    """generate() per clip at its own rate and step count, computed once per configuration."""
    if tag not in _STATE:
        clips = clip_list()[0]
        _STATE[tag] = [m.generate(c, sr, 48000, s, **prior_of(i), **kw).clone() for i, (c, sr, s) in enumerate(zip(clips, RATES, steps))]
    return _STATE[tag]


def same(many, ones):
    assert len(many) == len(ones)
    for i, (a, b) in enumerate(zip(many, ones)):
        assert tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype
        assert torch.equal(a, b), f"clip {i} differs from generate() alone"


def count_calls(monkeypatch, fn):
    """Names of the library calls `fn` makes (every call goes through hip.check)."""
    names, real = [], hip.check

    def check(rc, what=""):
        names.append(what)
        return real(rc, what)
    monkeypatch.setattr(hip, "check", check)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(hip, "check", real)
    return out, names


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_generate_many_mixed_steps_equals_generate_per_clip(method, monkeypatch):
    m = model_for(method)
    clips, noise, _ = clip_list()
    ones = alone(method, m, STEPS, lambda i: dict(noise=noise[i]))
    assert not torch.equal(ones[1][:, :4800], m.generate(clips[1], RATES[1], 48000, 1, noise=noise[1])[:, :4800])     # (the count matters)
    many, names = count_calls(monkeypatch, lambda: m.generate_many(clips, RATES, 48000, STEPS, noise=noise, ends="ragged"))
    same(many, ones)
    # one sequence: max(steps) passes of the field's stages over a shrinking prefix, no one-time entry of the time path
    assert names.count("fh_time_fourier_groups_f32") == 4 * ode.stages(method) and names.count("fh_time_fourier_f32") == 0
    assert names.count("fh_gemv_rows_f32") == 2 * names.count("fh_time_fourier_groups_f32") and names.count("fh_gemv_f32") == 0
    assert names.count("fh_axpy_groups_f32") >= 4 and names.count("fh_rmsnorm_f32") == 0
    same(m.generate_many(clips, RATES, 48000, tuple(STEPS), noise=noise, ends="per_clip"), ones)


def test_generate_many_equal_counts_as_a_list_are_the_int(monkeypatch):
    m = model_for("midpoint")
    clips, noise, _ = clip_list()
    m.generate_many(clips, RATES, 48000, 2, noise=noise, ends="ragged")          # (plans and workspaces of the mix)
    by_int, names_int = count_calls(monkeypatch, lambda: m.generate_many(clips, RATES, 48000, 2, noise=noise, ends="ragged"))
    by_list, names_list = count_calls(monkeypatch, lambda: m.generate_many(clips, RATES, 48000, [2, 2, 2, 2], noise=noise, ends="ragged"))
    assert names_int == names_list and "fh_axpy_groups_f32" not in names_int
    same(by_list, by_int)


def test_generate_many_mixed_steps_refuses_bad_counts_before_any_work(monkeypatch):
    m = model_for()
    clips, noise, _ = clip_list()
    for bad in ([1, 2, 3], [1, 0, 2, 4], [1, True, 2, 4], [1, 2.0, 2, 4]):
        _, names = count_calls(monkeypatch, lambda: pytest.raises(ValueError, m.generate_many, clips, RATES, 48000, bad, noise=noise))
        assert names == []
    with pytest.raises(ValueError):
        m.sample_many([torch.zeros(4800)] * 2, time_steps=[1, 2, 3])


def test_generate_many_mixed_steps_with_the_device_prior():
    m = model_for("midpoint", prior="device")
    clips = clip_list()[0]
    ones = alone("device", m, STEPS, lambda i: dict(seed=[(31, i)]))
    same(m.generate_many(clips, RATES, 48000, STEPS, seed=31, ends="ragged"), ones)
    same(m.generate_many(clips, RATES, 48000, STEPS, seed=31, ends="per_clip"), ones)


def test_generate_many_mixed_steps_independent_cfm_mix():
    m = model_for("euler", cfm="independent_cfm_mix")
    clips, noise, _ = clip_list()
    ones = alone("mix", m, STEPS, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, RATES, 48000, STEPS, noise=noise, ends="ragged"), ones)


def test_generate_many_mixed_steps_with_attention_keywords():
    m = model_for("euler", attn_form="bf16x6", attn_window=6)
    clips, noise, _ = clip_list()
    ones = alone("attn", m, STEPS, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, RATES, 48000, STEPS, noise=noise, ends="ragged"), ones)


def test_sample_many_mixed_steps_with_guidance_and_mel_pp():
    m = model_for("midpoint")
    steps = [2, 1, 2, 1]
    conds = [rnd(480 * n, 50 + i, 0.1) for i, n in enumerate((10, 30, 20, 15))]
    conds = [c / c.abs().max() for c in conds]
    noise = [synth.prior_noise(60 + i, n) for i, n in enumerate((10, 30, 20, 15))]
    ones = [m.sample(cond=c[None], time_steps=s, cond_scale=1.5, mel_pp=True, noise=z) for c, s, z in zip(conds, steps, noise)]
    many = m.sample_many(conds, time_steps=steps, cond_scale=1.5, mel_pp=True, noise=noise)
    same(many, ones)
    mels = m.sample_many(conds, time_steps=steps, cond_scale=1.5, noise=noise, decode_to_audio=False)
    for mel, c, s, z in zip(mels, conds, steps, noise):
        assert torch.equal(mel, m.sample(cond=c[None], time_steps=s, cond_scale=1.5, noise=z, decode_to_audio=False))


def test_generate_many_mixed_steps_with_a_stereo_clip_among_mono_ones():
    m = model_for("euler")
    clips, noise, _ = clip_list()
    stereo = np.stack([clips[1], synth.lowres_clip(450, 0.3, 16000)])
    mixed = [clips[0], stereo, clips[2], clips[3]]
    ones = [m.generate(c, sr, 48000, s, noise=z, channels="first").clone() for c, sr, s, z in zip(mixed, RATES, STEPS, noise)]
    for ends in ("ragged", "per_clip"):
        many = m.generate_many(mixed, RATES, 48000, STEPS, noise=noise, channels="first", ends=ends)
        assert tuple(many[1].shape) == (2, ones[1].shape[1])
        same(many, ones)


def test_generate_many_mixed_steps_delivered_as_dithered_int16():
    m = model_for("euler")
    clips, noise, _ = clip_list()
    kw = dict(pcm="int16", dither="tpdf")
    ones = [m.generate(c, sr, 48000, s, noise=z, dither_seed=[(9, i)], **kw).clone()
            for i, (c, sr, s, z) in enumerate(zip(clips, RATES, STEPS, noise))]
    many = m.generate_many(clips, RATES, 48000, STEPS, noise=noise, dither_seed=9, ends="ragged", **kw)
    assert many[0].dtype == torch.int16
    same(many, ones)


def test_generate_many_nine_distinct_counts_in_one_call(monkeypatch):
    m = model_for("euler")
    steps = [3, 9, 1, 5, 7, 2, 8, 4, 6]
    clips = [synth.lowres_clip(500 + i, 0.05 + 0.01 * (i % 3), 12000) for i in range(9)]
    noise = [synth.prior_noise(500 + i, tables.resample_out_len(len(c), 48000, 12000) // 480) for i, c in enumerate(clips)]
    ones = [m.generate(c, 12000, 48000, s, noise=z).clone() for c, s, z in zip(clips, steps, noise)]
    many, names = count_calls(monkeypatch, lambda: m.generate_many(clips, 12000, 48000, steps, noise=noise, ends="ragged"))
    same(many, ones)
    # two sequences: counts 9 .. 2 in one (9 passes), the clip of one step alone
    assert names.count("fh_time_fourier_groups_f32") == 9 and names.count("fh_time_fourier_f32") == 1


def test_generate_many_mixed_steps_without_the_ragged_path_runs_buckets(monkeypatch):
    m = model_for("euler")
    clips, noise, _ = clip_list()
    ones = alone("euler", m, STEPS, lambda i: dict(noise=noise[i]))
    many, names = count_calls(monkeypatch, lambda: m.generate_many(clips, RATES, 48000, STEPS, noise=noise, ragged=False))
    same(many, ones)
    assert "fh_axpy_groups_f32" not in names
    # generate_batch: clips of one shape, one batch per count
    pair = [clips[0], clips[0] * 0.5, clips[0] * 0.25]
    zs = [noise[0], noise[0] * 0.5, noise[0]]
    got = m.generate_batch(pair, 12000, 48000, [2, 1, 2], noise=torch.cat(zs, 0))
    for i, (c, z, s) in enumerate(zip(pair, zs, [2, 1, 2])):
        assert torch.equal(got[i:i + 1], m.generate(c, 12000, 48000, s, noise=z))


def test_generate_many_mixed_steps_on_the_convnext_backbone_runs_buckets(monkeypatch):
    cfg = synth.TINY_CFG
    sd = dict(synth.make_convnext_state_dict(3), **synth.make_vocoder_state_dict(cfg, 3))
    m = FlowHighSR(FLowHigh(sd, cfg, "cuda"), torchdiffeq_ode_method="euler", upsampling_method="hip")
    assert m.flowhigh.architecture == "convnext"
    clips, noise, _ = clip_list()
    ones = [m.generate(c, sr, 48000, s, noise=z).clone() for c, sr, s, z in zip(clips, RATES, STEPS, noise)]
    many, names = count_calls(monkeypatch, lambda: m.generate_many(clips, RATES, 48000, STEPS, noise=noise, ends="ragged"))
    same(many, ones)
    assert "fh_axpy_groups_f32" not in names


# ------------------------------------------------------------------------------------------
# the server
# ------------------------------------------------------------------------------------------
def test_batching_server_with_mixed_steps_makes_one_call(monkeypatch):
    m = model_for("midpoint")
    calls, real = [], m.generate_many

    def generate_many(clips, sr, target, steps, **kw):
        calls.append((len(clips), steps))
        return real(clips, sr, target, steps, **kw)
    monkeypatch.setattr(m, "generate_many", generate_many)
    srv = BatchingServer(m, max_batch=3, max_wait_ms=2000, ends="ragged", mix_steps=True)
    assert srv.mix_steps is True
    reqs = [(0.1, 1), (0.21, 2), (0.15, 4)]
    clips = [synth.lowres_clip(460 + i, s_, 12000) for i, (s_, _) in enumerate(reqs)]
    futs = [srv.submit(c, 12000, steps, seed=100 + i) for i, (c, (_, steps)) in enumerate(zip(clips, reqs))]
    outs = [f.result(timeout=120) for f in futs]
    srv.close()
    assert calls == [(3, [1, 2, 4])]
    for i, (c, (_, steps), y) in enumerate(zip(clips, reqs, outs)):
        one = m.generate(c, 12000, 48000, steps, generator=torch.Generator().manual_seed(100 + i))
        assert y.shape == (tables.resample_out_len(len(c), 48000, 12000),) and np.array_equal(y, one.cpu().numpy()[0])
