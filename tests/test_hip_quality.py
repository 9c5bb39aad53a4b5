"""GPU: the spectral quality report -- fh_quality_frames_f32, fh_quality_frames_seg_f32 and fh_quality_report_f32 on raw buffers,
and FlowHighSR.measure_quality end to end, against flowhigh_amd/quality.py (numpy float64).

Shapes: T in {1, 479, 480, 481, 2047, 2048, 4807} (where the frame count F = 1 + T // 480, the zero pad and the ownership of the
last partial hop change), R in {1, 3} rows, C in {1, 2, 8} channels, kc in {-1, 0, 1, 341, 1024, 1025}.  Inputs
(quality_inputs.py): noise of amplitude 0.1 against another, a scaled copy, a brick-wall pair, a pair whose high band lies 100 dB
under the reference's, and a pair with a stretch of exact zeros on both sides.  Every input is asserted, from the definition
alone, to have each bin power exactly 0 or at least 1e-6 (100 times the floor), so no bin sits at the clamp's corner.

Bars.  The double arithmetic error is negligible and the one-transform separation costs at most about
11 * 2^-52 * sqrt(P_ref / P_est) in a bin's d, under 3e-8 even at the floor; what remains is the float32 output:
  LSD figures (below 8): 5e-7 absolute -- one float32 half-spacing there, 2.4e-7, plus margin;
  snr_db (below 128 in magnitude): 1e-5 dB, the bar of test_hip_loudness.py for the same reason;
  infinities and NaN exactly; identical rows lsd <= 1e-12 and snr +inf; all-zero pairs lsd exactly 0.
Where two runs of this project are compared the test is bitwise.  Every output buffer stands between guard words."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quality_inputs as qi                                                     # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, delivery, hip, quality, synth, tables      # noqa: E402

GUARD = 16
SENT32 = 0x7fc12345
SENT64 = 0x7ff8123456789abc
LSD_BAR, SNR_BAR = 5e-7, 1e-5
_STATE = {}


def st():
    return hip.stream()


def fft_tables():
    if "fft" not in _STATE:
        _STATE["fft"] = (tables.hann_window().cuda(), tables.fft_twiddles().cuda())
    return _STATE["fft"][0].data_ptr(), _STATE["fft"][1].data_ptr()


def model():
    if "model" not in _STATE:
        fh = FLowHigh(synth.make_state_dict(synth.TINY_CFG, 0), synth.TINY_CFG, "cuda")
        _STATE["model"] = FlowHighSR(fh, prior="device", torchdiffeq_ode_method="euler")
    return _STATE["model"]


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def guarded(n, dtype):
    """A buffer of n elements between guard words -> (the whole int tensor, the address of its payload, check())."""
    whole = torch.full((GUARD + n + GUARD,), SENT64 if dtype == torch.int64 else SENT32, dtype=dtype, device="cuda")

    def check():
        sent = SENT64 if dtype == torch.int64 else SENT32
        assert bool((whole[:GUARD] == sent).all()) and bool((whole[GUARD + n:] == sent).all()), "a guard word was written"
    return whole, whole[GUARD:].data_ptr(), check


def frames_batched(est, ref, kc):
    """est, ref numpy [R, T] -> the frames [R, F, 5] float64 on the device (guards checked), and which of them were written."""
    R, T = est.shape
    F = quality.n_frames(T)
    e, r = torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda()
    whole, p, check = guarded(R * F * 5, torch.int64)
    w, tw = fft_tables()
    hip.check(hip.lib().fh_quality_frames_f32(e.data_ptr(), r.data_ptr(), w, tw, p, R, T, kc, st()), "fh_quality_frames_f32")
    check()
    assert not bool((whole[GUARD:GUARD + R * F * 5] == SENT64).any()), "a frame was left unwritten"
    return whole[GUARD:GUARD + R * F * 5].view(torch.float64).view(R, F, 5)


def frames_seg(clips):
    """clips: [(est [C, T], ref [C, T], kc)] numpy -> (frames [rows, F_max, 5], F_max, lens, group, the device tensors kept)."""
    n, chans, lens = len(clips), [c[0].shape[0] for c in clips], [c[0].shape[1] for c in clips]
    R, max_len = sum(chans), max(lens)
    F = quality.n_frames(max_len)
    dev = [(torch.from_numpy(e).cuda(), torch.from_numpy(r).cuda()) for e, r, _ in clips]
    table = (hip.QualityClip * n)(*[hip.QualityClip(e.data_ptr(), r.data_ptr(), e.stride(0), r.stride(0), c, t, k, 0)
                                    for (e, r), c, t, (_, _, k) in zip(dev, chans, lens, clips)])
    d_table = hip.to_device_struct_array(list(table), "cuda")
    row_len = np.repeat(np.asarray(lens, dtype=np.int32), chans)
    group = np.repeat(np.arange(n, dtype=np.int32), chans)
    d_group = torch.from_numpy(group).cuda()
    whole, p, check = guarded(R * F * 5, torch.int64)
    w, tw = fft_tables()
    hip.check(hip.lib().fh_quality_frames_seg_f32(d_table.data_ptr(), ctypes.addressof(table), d_group.data_ptr(), n, R, max_len, w, tw,
                                                  p, st()), "fh_quality_frames_seg_f32")
    torch.cuda.synchronize()
    check()
    frames = whole[GUARD:GUARD + R * F * 5].view(R, F, 5)
    for row, t in enumerate(row_len):                     # a row is written up to its own frames and no further
        f = quality.n_frames(int(t))
        assert not bool((frames[row, :f] == SENT64).any()) and bool((frames[row, f:] == SENT64).all())
    return frames.view(torch.float64), F, row_len, group


def report_of(frames, F, row_len, group, n):
    """fh_quality_report_f32 -> float32 [n, 4] on the device (guards checked)."""
    lens, grp = torch.from_numpy(np.asarray(row_len, dtype=np.int32)).cuda(), torch.from_numpy(np.asarray(group, dtype=np.int32)).cuda()
    whole, p, check = guarded(4 * n, torch.int32)
    hip.check(hip.lib().fh_quality_report_f32(frames.data_ptr(), F, lens.data_ptr(), grp.data_ptr(), len(row_len), n, p, st()),
              "fh_quality_report_f32")
    check()
    return whole[GUARD:GUARD + 4 * n].view(torch.float32).view(n, 4).clone()


def batched_report(est, ref, kc, chans=None):
    R, T = est.shape
    chans = [1] * R if chans is None else chans
    frames = frames_batched(est, ref, kc)
    return report_of(frames, quality.n_frames(T), [T] * R, np.repeat(np.arange(len(chans)), chans), len(chans))


def seg_report(clips):
    frames, F, row_len, group = frames_seg(clips)
    return report_of(frames, F, row_len, group, len(clips))


def close(got, want, what):
    """One report row against the definition's four floats -> the worst error over its bar."""
    worst = 0.0
    for name, g, w, bar in zip(quality.FIELDS, (float(v) for v in got), want, (LSD_BAR, LSD_BAR, LSD_BAR, SNR_BAR)):
        if math.isnan(w):
            assert math.isnan(g), (what, name, g, w)
        elif math.isinf(w):
            assert g == w, (what, name, g, w)
        else:
            assert abs(w) < (128.0 if name == "snr_db" else 8.0), (what, name, w)       # (the range the bar is made for)
            worst = max(worst, abs(g - w) / bar)
            assert abs(g - w) <= bar, (what, name, g, w, abs(g - w))
    return worst


def assert_clear(*arrays):
    for a in arrays:
        assert qi.clear_of_the_floor(a)


# ---- 1. the raw entries against the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", qi.T_CASES)
@pytest.mark.parametrize("name", list(qi.MAKERS))
def test_rows_against_the_definition(name, T):
    """R = 1 and R = 3 rows, every row a clip, at every kc; the frames' SNR sums as well."""
    worst = 0.0
    for R in (1, 3):
        est, ref = qi.MAKERS[name](R, T, seed=R)
        assert_clear(est, ref)
        d = [quality.log_power_difference(e, r) for e, r in zip(est, ref)]
        for kc in qi.KC_CASES:
            frames = frames_batched(est, ref, kc)
            got = report_of(frames, quality.n_frames(T), [T] * R, list(range(R)), R).cpu().numpy()
            f = frames.cpu().numpy()
            for row in range(R):
                l = quality.frame_lsd(d[row], None if kc < 0 else kc)
                want = (l[:, 0].mean(), l[:, 1].mean(), l[:, 2].mean(), quality.snr_db(est[row:row + 1], ref[row:row + 1]))
                worst = max(worst, close(got[row], want, (name, T, R, kc, row)))
                assert np.array_equal(np.isnan(f[row, :, :3]), np.isnan(l))
                assert np.nanmax(np.abs(f[row, :, :3] - l), initial=0.0) < 1e-7
                # the frames' two sums: the samples each frame owns, in double
                r64, e64 = ref[row].astype(np.float64), est[row].astype(np.float64)
                for t in range(quality.n_frames(T)):
                    own = slice(480 * t, min(480 * t + 480, T))
                    assert abs(f[row, t, 3] - (r64[own] ** 2).sum()) <= 1e-13 * max(1.0, (r64[own] ** 2).sum())
                    assert abs(f[row, t, 4] - ((r64[own] - e64[own]) ** 2).sum()) <= 1e-13 * max(1.0, ((r64[own] - e64[own]) ** 2).sum())
    print(f"{name} T={T}: worst error {worst:.3f} of its bar")


@pytest.mark.parametrize("C", [1, 2, 8])
def test_channels_against_the_definition(C):
    """Clips of C channels through both frame entries: the mean over all C F frames and the pooled SNR."""
    worst = 0.0
    for T in (481, 4807):
        pairs = [qi.MAKERS[name](C, T, seed=3) for name in ("noise", "brick wall", "zero stretch")]
        for e, r in pairs:
            assert_clear(e, r)
        est, ref = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
        b = batched_report(est, ref, 341, [C] * len(pairs))
        s = seg_report([(e, r, 341) for e, r in pairs])
        assert same_bits(b, s)
        for i, (e, r) in enumerate(pairs):
            worst = max(worst, close(b[i].cpu().numpy(), qi.define(e, r, 341), (C, T, i)))
    print(f"C={C}: worst error {worst:.3f} of its bar")


def test_identical_silent_and_empty():
    for T in qi.T_CASES:
        r = qi.noise(3, T, seed=T)
        z = np.zeros_like(r)
        same = batched_report(r.copy(), r, 341).cpu().numpy()
        assert (np.abs(same[:, :3]) <= 1e-12).all() and (same[:, 3] == math.inf).all(), (T, same)
        zero = batched_report(z, z, 341).cpu().numpy()
        assert (zero[:, :3] == 0.0).all() and np.isnan(zero[:, 3]).all(), (T, zero)
        quiet = qi.noise(3, T, 0.01, seed=T)             # (an estimate whose bins lie under 1: the distance from the floor stays below 8)
        silent_ref = batched_report(quiet, z, 341).cpu().numpy()
        assert (silent_ref[:, 3] == -math.inf).all()
        for i in range(3):
            close(silent_ref[i], qi.define(quiet[i:i + 1], z[i:i + 1], 341), ("silent reference", T, i))
    # the bands' ends: an empty band is NaN, no cutoff makes both NaN
    e, r = qi.noise_pair(1, 2048)
    for kc, nan in ((-1, (1, 2)), (0, (1,)), (1025, (2,)), (1, ()), (1024, ())):
        got = batched_report(e, r, kc).cpu().numpy()[0]
        assert [k for k in range(4) if math.isnan(got[k])] == list(nan), (kc, got)


# ---- 2. two runs of this project: bitwise ------------------------------------------------------------------------------------------
def ragged_clips():
    """Clips of mixed T and C, each with its own kc."""
    shapes = [(1, 4807, 341), (2, 481, -1), (8, 2048, 1025), (1, 1, 0), (3, 479, 1), (2, 4807, 1024), (1, 2047, 171)]
    names = list(qi.MAKERS)
    return [(*qi.MAKERS[names[i % len(names)]](C, T, seed=10 + i), kc) for i, (C, T, kc) in enumerate(shapes)]


def test_a_clip_alone_and_inside_a_ragged_list_bitwise():
    clips = ragged_clips()
    packed = seg_report(clips)
    again = seg_report(clips)
    assert same_bits(packed, again)                      # two consecutive runs
    worst = 0.0
    for i, (e, r, kc) in enumerate(clips):
        alone = seg_report([(e, r, kc)])
        assert same_bits(alone[0], packed[i]), (i, alone, packed[i])
        batched = batched_report(e, r, kc, [e.shape[0]])
        assert same_bits(batched[0], packed[i]), (i, batched, packed[i])
        worst = max(worst, close(packed[i].cpu().numpy(), qi.define(e, r, kc), ("ragged", i)))
    print(f"ragged list: worst error {worst:.3f} of its bar")


def test_frames_batched_and_segment_bitwise():
    e, r = qi.noise_pair(3, 4807, seed=4)
    b = frames_batched(e, r, 341)
    s, F, _, _ = frames_seg([(e[:1], r[:1], 341), (e[1:], r[1:], 341)])
    assert same_bits(b, s) and same_bits(b, frames_batched(e, r, 341))
    # rows read where they are: a pitch that is not the length
    wide_e, wide_r = np.zeros((3, 5000), np.float32), np.full((3, 6000), 7.0, np.float32)
    wide_e[:, :4807], wide_r[:, :4807] = e, r
    s2, _, _, _ = frames_seg([(wide_e[:, :4807], wide_r[:, :4807], 341)])
    assert same_bits(b, s2)


def test_bad_arguments_are_refused():
    L = hip.lib()
    x = torch.zeros(1, 480, device="cuda")
    f = torch.zeros(2 * 5, dtype=torch.float64, device="cuda")
    w, tw = fft_tables()
    for args, what in (((x.data_ptr(), x.data_ptr(), w, tw, f.data_ptr(), 1, 0, 341), b"len 0"),
                       ((x.data_ptr(), x.data_ptr(), w, tw, f.data_ptr(), 1, 480, 1026), b"kc 1026"),
                       ((x.data_ptr(), x.data_ptr(), w, tw, f.data_ptr(), 1, 480, -2), b"kc -2"),
                       ((x.data_ptr(), 0, w, tw, f.data_ptr(), 1, 480, 341), b"null pointer"),
                       ((x.data_ptr(), x.data_ptr(), w, tw, 0, 1, 480, 341), b"null pointer")):
        assert L.fh_quality_frames_f32(*args, st()) == -1 and what in L.fh_last_error(), L.fh_last_error()
    torch.cuda.synchronize()
    assert bool((f == 0).all())


# ---- 3. FlowHighSR.measure_quality --------------------------------------------------------------------------------------------------
def test_measure_quality_forms():
    m = model()
    clips = ragged_clips()
    est = [torch.from_numpy(e).cuda() for e, _, _ in clips]
    ref = [torch.from_numpy(r).cuda() for _, r, _ in clips]
    # cutoffs in Hz that give the clips' bins (None: no cutoff)
    hz = {341: 8000.0, -1: None, 1025: 30000.0, 0: 1.0, 1: 23.4375, 1024: 24000.0, 171: 4000.0}
    assert all(quality.cutoff_bin(v) == k for k, v in hz.items() if v is not None)
    packed = seg_report(clips)
    # a list with one cutoff for all of it, and clip by clip with its own
    for i, (e, r, kc) in enumerate(clips):
        got = m.measure_quality([est[i]], [ref[i]], cutoff_hz=hz[kc])
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 4) and got.is_cuda
        assert same_bits(got[0], packed[i])
        got = m.measure_quality(est[i], ref[i], chans=[e.shape[0]], cutoff_hz=hz[kc])          # the batched entry
        assert same_bits(got[0], packed[i])
    with_cut = [i for i, c in enumerate(clips) if c[2] >= 0]
    got = m.measure_quality([est[i] for i in with_cut], [ref[i] for i in with_cut], cutoff_hz=[hz[clips[i][2]] for i in with_cut])
    assert same_bits(got, packed[with_cut])
    # rows of one length with a cutoff per clip: the segment form over views of the two tensors
    e, r = qi.noise_pair(3, 4807, seed=4)
    te, tr = torch.from_numpy(e).cuda(), torch.from_numpy(r).cuda()
    per_clip = m.measure_quality(te, tr, chans=[1, 2], cutoff_hz=[8000.0, 4000.0])
    assert same_bits(per_clip[0], m.measure_quality(te[:1], tr[:1], cutoff_hz=8000.0)[0])
    assert same_bits(per_clip[1], m.measure_quality(te[1:], tr[1:], chans=[2], cutoff_hz=4000.0)[0])
    # a rate other than 48000 only moves the bin
    assert same_bits(m.measure_quality(te, tr, rate=16000, cutoff_hz=4000.0), m.measure_quality(te, tr, cutoff_hz=12000.0))
    # itself
    same = m.measure_quality(te, te.clone(), cutoff_hz=8000.0).cpu().numpy()
    assert (np.abs(same[:, :3]) <= 1e-12).all() and (same[:, 3] == math.inf).all()


def test_measure_quality_of_a_generated_clip_against_its_input():
    m = model()
    sr = 16000
    audio = (np.random.default_rng(5).uniform(-1.0, 1.0, 8000) * 0.3).astype(np.float32)
    out, stages = m.generate_batch([audio], sr, 48000, 1, seed=1, return_stages=True)
    y, cond = out.clone(), stages["cond"].reshape(out.shape).clone()
    same = m.measure_quality(y, y, cutoff_hz=sr / 2).cpu().numpy()
    assert (np.abs(same[:, :3]) <= 1e-12).all() and (same[:, 3] == math.inf).all()
    got = m.measure_quality(y, cond, cutoff_hz=sr / 2)
    assert tuple(got.shape) == (1, 4)
    ye, yr = y.cpu().numpy(), cond.cpu().numpy()
    want = quality.report(ye, yr, cutoff_hz=sr / 2)
    print("generated against its 48 kHz input:", dict(zip(quality.FIELDS, want)))
    close(got[0].cpu().numpy(), want, "generated")


def test_measure_quality_refuses_before_any_gpu_work(monkeypatch):
    m = model()
    x = torch.zeros(2, 960, device="cuda")
    torch.cuda.synchronize()

    def no_launch(*a, **k):
        raise AssertionError("a launch before the arguments were checked")
    monkeypatch.setattr(delivery, "_launch", no_launch)
    monkeypatch.setattr(delivery, "upload_tables", no_launch)
    bad = [
        dict(rows=x, ref_rows=x[:, :959]),                                   # unequal shapes
        dict(rows=x, ref_rows=x[:1]),
        dict(rows=x, ref_rows=x.double()),                                   # a wrong dtype
        dict(rows=x.half(), ref_rows=x.half()),
        dict(rows=x, ref_rows=x.cpu()),                                      # a wrong device
        dict(rows=x[:, :0], ref_rows=x[:, :0]),                              # empty clips
        dict(rows=[], ref_rows=[]),
        dict(rows=[x], ref_rows=[x, x]),
        dict(rows=[x, x[:0]], ref_rows=[x, x[:0]]),
        dict(rows=x, ref_rows=[x]),
        dict(rows=x, ref_rows=x, chans=[1]),                                 # chans that do not sum to the rows
        dict(rows=x, ref_rows=x, chans=[2, 0]),
        dict(rows=[x], ref_rows=[x], chans=[2]),                             # chans with lists
        dict(rows=x[0], ref_rows=x[0]),                                      # not [R, T]
        dict(rows=x, ref_rows=x, cutoff_hz=0.0),                             # a cutoff that is not finite and positive
        dict(rows=x, ref_rows=x, cutoff_hz=-8000.0),
        dict(rows=x, ref_rows=x, cutoff_hz=math.nan),
        dict(rows=x, ref_rows=x, cutoff_hz=math.inf),
        dict(rows=x, ref_rows=x, cutoff_hz="8000"),
        dict(rows=x, ref_rows=x, cutoff_hz=[8000.0]),                        # a cutoff list of the wrong length
        dict(rows=x, ref_rows=x, cutoff_hz=[8000.0, 8000.0, 8000.0]),
        dict(rows=x, ref_rows=x, cutoff_hz=[8000.0, math.nan]),
        dict(rows=x, ref_rows=x, cutoff_hz=8000.0, rate=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            m.measure_quality(**kw)
