"""GPU: the segment forms of the front / back end entries (fh_*_seg_f32, csrc/frontend.hip) and generate_many(ends='ragged').

The contract is bitwise: every clip of a ragged launch gets what the batched entry gives for that clip alone, so every
comparison is torch.equal.  Entry tests run five clips of 600 / 1500 / 2401 / 2401 / 3000 samples at 12 kHz (48 kHz lengths
2400 / 6000 / 9604 / 9604 / 12000: 5 frames, a length that is no multiple of 480, two equal clips); outputs are NaN-filled first
and followed by a guard, so that an element the kernel did not write, or one it wrote past a clip's end, shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_frontend                                                        # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth                 # noqa: E402
from flowhigh_amd import frontend as FE                                    # noqa: E402
from flowhigh_amd import tables                                            # noqa: E402
from flowhigh_amd.serve import BatchingServer                              # noqa: E402
from flowhigh_amd.tables import HOP, N_FFT, P_WIDTH                        # noqa: E402

LENS = [600, 1500, 2401, 2401, 3000]
GUARD = 64
_STATE = {}


def rnd(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def st():
    return hip.stream()


def tables_dev(*parts):
    buf, addrs = FE.upload_tables(list(parts), torch.device("cuda"))
    _STATE.setdefault("keep", []).append(buf)
    return addrs


def clips48(seed=0):
    """The five clips at 48 kHz (random samples) and their table."""
    tab = FE.ragged_clip_tables(LENS, 12000)
    return [rnd(T, seed + i, 0.3) for i, T in enumerate(tab["len_out"])], tab


def hann():
    return FE._Const.get("cuda")["hann"]


# ------------------------------------------------------------------------------------------
# one test per entry: the seg form on the five clips against the batched entry on each clip alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [12000, 22050, 48000])
def test_resample_poly_seg_equals_the_entry_per_clip(sr):
    L = hip.lib()
    tab = FE.ragged_clip_tables(LENS, sr, check_mel=False)
    xs = [rnd(n, 10 + i, 0.2) for i, n in enumerate(LENS)]
    x = torch.cat(xs)
    y = nan(sum(tab["len_out"]) + GUARD)
    plan = tables.resample_poly_plan(48000, sr)
    (clips,) = tables_dev(FE.clip_array(src=[x.data_ptr() + 4 * o for o in tab["in_off"]], len_in=tab["len_in"],
                                        dst=[y.data_ptr() + 4 * o for o in tab["out_off"]], len_out=tab["len_out"]))
    if plan is None:
        hip.check(L.fh_resample_poly_seg_f32(clips, 5, max(tab["len_out"]), 0, 1, 1, 0, 0, st()), "seg")
        refs = [v.clone() for v in xs]
    else:
        taps, pre, up, down = plan
        taps = taps.cuda()
        assert (down > 1) == (sr == 22050)
        hip.check(L.fh_resample_poly_seg_f32(clips, 5, max(tab["len_out"]), taps.data_ptr(), up, down, taps.numel(), pre, st()), "seg")
        refs = []
        for v, n_out in zip(xs, tab["len_out"]):
            r = nan(n_out)
            hip.check(L.fh_resample_poly_f32(v.data_ptr(), taps.data_ptr(), r.data_ptr(), 1, v.numel(), n_out, up, down,
                                             taps.numel(), pre, st()), "fh_resample_poly_f32")
            refs.append(r)
    for o, n, r in zip(tab["out_off"], tab["len_out"], refs):
        assert torch.isfinite(r).all() and torch.equal(y[o:o + n], r)
    assert torch.isnan(y[-GUARD:]).all()
    # taps left out at unequal rates: an argument error, nothing launched
    assert L.fh_resample_poly_seg_f32(clips, 5, 100, 0, 4, 1, 0, 0, st()) == -1 and b"fh_resample_poly_seg_f32" in L.fh_last_error()
    assert L.fh_resample_poly_seg_f32(0, 5, 100, 0, 1, 1, 0, 0, st()) == -1
    assert L.fh_resample_poly_seg_f32(clips, 65536, 100, 0, 1, 1, 0, 0, st()) == -1


def test_peak_abs_and_peak_scale_seg_equal_the_entries_per_clip():
    L = hip.lib()
    xs, tab = clips48(20)
    y = torch.cat(xs + [nan(GUARD)])
    (clips,) = tables_dev(FE.clip_array(dst=[y.data_ptr() + 4 * o for o in tab["out_off"]], len_out=tab["len_out"]))
    peak = torch.zeros(5, dtype=torch.int32, device="cuda")
    hip.check(L.fh_peak_abs_seg_f32(clips, 5, max(tab["len_out"]), peak.data_ptr(), st()), "fh_peak_abs_seg_f32")
    ref_peak = torch.zeros(5, dtype=torch.int32, device="cuda")
    refs = []
    for i, v in enumerate(xs):
        r = v.clone()
        hip.check(L.fh_peak_abs_f32(r.data_ptr(), ref_peak[i:].data_ptr(), 1, r.numel(), st()), "fh_peak_abs_f32")
        hip.check(L.fh_peak_scale_f32(r.data_ptr(), ref_peak[i:].data_ptr(), 1, r.numel(), 0.99, st()), "fh_peak_scale_f32")
        refs.append(r)
    assert torch.equal(peak, ref_peak)
    assert torch.equal(peak.view(torch.float32), torch.stack([v.abs().max() for v in xs]))
    hip.check(L.fh_peak_scale_seg_f32(clips, 5, max(tab["len_out"]), peak.data_ptr(), 0.99, st()), "fh_peak_scale_seg_f32")
    for o, n, r in zip(tab["out_off"], tab["len_out"], refs):
        assert torch.equal(y[o:o + n], r)
    assert torch.isnan(y[-GUARD:]).all()
    assert L.fh_peak_abs_seg_f32(clips, 5, 100, 0, st()) == -1 and L.fh_peak_scale_seg_f32(clips, 0, 100, peak.data_ptr(), 1.0, st()) == -1


@pytest.mark.parametrize("mode", ["reflect", "zero"])
def test_frame_seg_equals_the_entry_per_clip(mode):
    """reflect 784 with N_i = T_i // 480 rows (the mel front end), zero 1024 with F_i = 1 + T_i // 480 rows (post-processing); the
    clips lie at per-clip pointers with gaps between them."""
    L = hip.lib()
    xs, tab = clips48(30)
    pad, pm, rows, row0 = ((N_FFT - HOP) // 2, 0, tab["mel_rows"], tab["mel_row0"]) if mode == "reflect" else \
        (N_FFT // 2, 1, tab["pp_rows"], tab["pp_row0"])
    frames = nan(sum(rows) + 1, N_FFT)
    (clips,) = tables_dev(FE.clip_array(src=[v.data_ptr() for v in xs], len_in=tab["len_out"], row0=row0, rows=rows))
    hip.check(L.fh_frame_seg_f32(clips, 5, max(rows), min(tab["len_out"]), hann().data_ptr(), frames.data_ptr(), N_FFT, HOP, pad,
                                 pm, st()), "fh_frame_seg_f32")
    for v, r0, n in zip(xs, row0, rows):
        ref = nan(n, N_FFT)
        hip.check(L.fh_frame_f32(v.data_ptr(), hann().data_ptr(), ref.data_ptr(), 1, v.numel(), n, N_FFT, HOP, pad, pm, st()),
                  "fh_frame_f32")
        assert torch.isfinite(ref).all() and torch.equal(frames[r0:r0 + n], ref)
    assert torch.isnan(frames[-1]).all()
    # the reflect pad needs pad < len for every clip: the shortest length is an argument
    assert L.fh_frame_seg_f32(clips, 5, max(rows), 784, hann().data_ptr(), frames.data_ptr(), N_FFT, HOP, 784, 0, st()) == -1
    assert b"reflect pad" in L.fh_last_error()


def test_spec_energy_seg_equals_the_entry_per_clip():
    """The clips' F_i = 6 / 13 / 21 / 21 / 26 rows and one segment of 150 rows (more than the 64 frames one pass of the 32 frame
    lanes takes: both chains of every lane and the loop run)."""
    L = hip.lib()
    tab = FE.ragged_clip_tables(LENS, 12000)
    rows = tab["pp_rows"] + [150]
    assert rows[:5] == [6, 13, 21, 21, 26]
    row0 = [sum(rows[:i]) for i in range(6)]
    spec = rnd(sum(rows) * P_WIDTH, 40).view(-1, P_WIDTH)
    energy = nan(7, 1025)
    (seg,) = tables_dev(FE.seg_table(row0, rows))
    hip.check(L.fh_spec_energy_seg_f32(spec.data_ptr(), energy.data_ptr(), seg, 6, st()), "fh_spec_energy_seg_f32")
    for i, (r0, n) in enumerate(zip(row0, rows)):
        ref = nan(1025)
        hip.check(L.fh_spec_energy_f32(spec[r0:r0 + n].data_ptr(), ref.data_ptr(), 1, n, st()), "fh_spec_energy_f32")
        assert torch.isfinite(ref).all() and torch.equal(energy[i], ref)
    assert torch.isnan(energy[6]).all()
    # fh_cutoff_index_f32 takes the [n, 1025] result as it is
    cr = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    hip.check(L.fh_cutoff_index_f32(energy.data_ptr(), cr.data_ptr(), 6, 1025, 0.99, st()), "fh_cutoff_index_f32")
    assert cr.tolist() == [ref_frontend.cutoff_index(energy[i], 0.99) for i in range(6)]
    assert L.fh_spec_energy_seg_f32(spec.data_ptr(), energy.data_ptr(), 0, 6, st()) == -1


def test_spec_splice_seg_equals_the_entry_per_clip():
    L = hip.lib()
    tab = FE.ragged_clip_tables(LENS, 12000)
    rows, row0 = tab["pp_rows"], tab["pp_row0"]
    R = sum(rows)
    pred, src = rnd(R * P_WIDTH, 50).view(R, P_WIDTH), rnd(R * P_WIDTH, 51).view(R, P_WIDTH)
    cr = torch.tensor([0, 1025, 300, 31, 777], dtype=torch.int32, device="cuda")        # per clip: none, all, and in between
    out = nan(R + 1, P_WIDTH)
    (seg,) = tables_dev(FE.seg_table(row0, rows))
    hip.check(L.fh_spec_splice_seg_f32(pred.data_ptr(), src.data_ptr(), cr.data_ptr(), out.data_ptr(), seg, 5, max(rows), st()),
              "fh_spec_splice_seg_f32")
    for i, (r0, n) in enumerate(zip(row0, rows)):
        ref = nan(n, P_WIDTH)
        hip.check(L.fh_spec_splice_f32(pred[r0:r0 + n].data_ptr(), src[r0:r0 + n].data_ptr(), cr[i:].data_ptr(), ref.data_ptr(),
                                       1, n, st()), "fh_spec_splice_f32")
        assert torch.equal(out[r0:r0 + n], ref)
    assert torch.equal(out[:rows[0]], pred[:rows[0]]) and torch.isnan(out[-1]).all()
    assert not torch.equal(out[row0[2]:row0[2] + rows[2]], out[row0[3]:row0[3] + rows[3]])    # (equal lengths, different cr and data)
    assert L.fh_spec_splice_seg_f32(pred.data_ptr(), src.data_ptr(), cr.data_ptr(), out.data_ptr(), seg, 5, 0, st()) == -1


def test_istft_ola_seg_equals_the_entry_per_clip():
    """Output lengths T_i, except clip 1: 7000 > 480 (13 - 1) + 1024 = 6784, so its tail is the zero fill past the OLA signal's end."""
    L = hip.lib()
    tab = FE.ragged_clip_tables(LENS, 12000)
    rows, row0 = tab["pp_rows"], tab["pp_row0"]
    lengths = list(tab["len_out"])
    lengths[1] = 7000
    assert lengths[1] > HOP * (rows[1] - 1) + N_FFT // 2
    off = [sum(lengths[:i]) for i in range(5)]
    frames = rnd(sum(rows) * N_FFT, 60).view(-1, N_FFT)
    y = nan(sum(lengths) + GUARD)
    peak = torch.zeros(5, dtype=torch.int32, device="cuda")
    (clips,) = tables_dev(FE.clip_array(dst=[y.data_ptr() + 4 * o for o in off], len_out=lengths, row0=row0, rows=rows))
    hip.check(L.fh_istft_ola_seg_f32(frames.data_ptr(), hann().data_ptr(), clips, 5, max(lengths), peak.data_ptr(), N_FFT, HOP, st()),
              "fh_istft_ola_seg_f32")
    ref_peak = torch.zeros(5, dtype=torch.int32, device="cuda")
    for i, (o, n, r0, f) in enumerate(zip(off, lengths, row0, rows)):
        ref = nan(n)
        hip.check(L.fh_istft_ola_f32(frames[r0:r0 + f].data_ptr(), hann().data_ptr(), ref.data_ptr(), ref_peak[i:].data_ptr(), 1, f, n,
                                     N_FFT, HOP, st()), "fh_istft_ola_f32")
        assert torch.isfinite(ref).all() and torch.equal(y[o:o + n], ref)
    assert torch.equal(peak, ref_peak)
    tail = y[off[1] + 6784:off[1] + 7000]
    assert float(tail.abs().max()) == 0.0 and float(y[off[1] + 6783].abs()) > 0.0
    assert torch.isnan(y[-GUARD:]).all()
    assert L.fh_istft_ola_seg_f32(frames.data_ptr(), hann().data_ptr(), clips, 5, 0, peak.data_ptr(), N_FFT, HOP, st()) == -1


@pytest.mark.parametrize("d", [256, 40])
def test_rows_to_channels_seg_is_the_transposing_copy_per_clip(d):
    """[N_i, d] rows of the packed batch -> every clip's own [d, N_i] buffer, as forward_ragged's copy_ of the transposed view
    (d = 40 and the clips' N_i = 5 / 12 / 20 / 20 / 25: no multiple of the 32 x 32 tile either way)."""
    L = hip.lib()
    tab = FE.ragged_clip_tables(LENS, 12000)
    rows, row0 = tab["mel_rows"], tab["mel_row0"]
    mel = rnd(sum(rows) * d, 70).view(-1, d)
    outs = [nan(d + 1, n) for n in rows]                                     # (one more channel row: the guard)
    (clips,) = tables_dev(FE.clip_array(dst=[o.data_ptr() for o in outs], row0=row0, rows=rows, len_out=[d * n for n in rows]))
    hip.check(L.fh_rows_to_channels_seg_f32(mel.data_ptr(), clips, 5, max(rows), d, st()), "fh_rows_to_channels_seg_f32")
    for o, r0, n in zip(outs, row0, rows):
        ref = torch.empty(1, d, n, device="cuda")
        ref.copy_(mel[r0:r0 + n].view(1, n, -1).transpose(1, 2))
        assert torch.equal(o[:d], ref[0]) and torch.isnan(o[d]).all()
    assert L.fh_rows_to_channels_seg_f32(mel.data_ptr(), clips, 5, max(rows), 0, st()) == -1


# ------------------------------------------------------------------------------------------
# the ragged methods of Resampler / LogMel / PostProcessor against their per-clip calls
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [12000, 22050, 48000])
@pytest.mark.parametrize("where", ["host", "device"])
def test_resampler_ragged_equals_per_clip_calls(sr, where):
    rs = FE.Resampler("cuda")
    host = [(0.1 * np.random.default_rng(80 + i).standard_normal(n)).astype(np.float32) for i, n in enumerate(LENS)]
    xs = host if where == "host" else [torch.from_numpy(h).cuda() for h in host]
    packed, views = rs.ragged(xs, sr)
    refs = [rs(torch.from_numpy(h).cuda()[None], sr)[0] for h in host]
    assert packed.numel() == sum(r.numel() for r in refs)
    for v, r in zip(views, refs):
        assert torch.equal(v, r) and float(r.abs().max()) == 1.0
    # a mix seen before: same buffers, same descriptors, same result
    ptr, desc = packed.data_ptr(), rs._ws[(sr, 48000, tuple(LENS))]["desc"]
    packed2, views2 = rs.ragged(xs, sr)
    assert packed2.data_ptr() == ptr and rs._ws[(sr, 48000, tuple(LENS))]["desc"] is desc
    assert all(torch.equal(v, r) for v, r in zip(views2, refs))


def test_resampler_upload_packed_is_one_buffer_of_the_host_clips():
    rs = FE.Resampler("cuda")
    host = [np.random.default_rng(90 + i).standard_normal(n) for i, n in enumerate([2400, 6000, 9604])]     # float64, as scipy returns
    packed, views = rs.upload_packed(host)
    for v, h in zip(views, host):
        assert torch.equal(v.cpu(), torch.tensor(h).float())
    assert packed.numel() == 18004 and views[1].data_ptr() == packed.data_ptr() + 4 * 2400


def test_logmel_ragged_equals_per_clip_calls():
    lm = FE.LogMel("cuda")
    xs, tab = clips48(100)
    refs = [lm(v[None]).clone() for v in xs]
    mel, views = lm.ragged(xs)
    assert tuple(mel.shape) == (sum(tab["mel_rows"]), 256)
    for v, r in zip(views, refs):
        assert torch.equal(v, r)
    # the same lengths at other addresses: the descriptors follow the clips
    moved = [v.clone() * 0.5 for v in xs]
    refs2 = [lm(v[None]).clone() for v in moved]
    _, views2 = lm.ragged(moved)
    assert all(torch.equal(v, r) for v, r in zip(views2, refs2)) and not torch.equal(refs2[0], refs[0])
    with pytest.raises(ValueError, match="clip of 784 samples is too short for the mel front end"):
        lm.ragged([xs[0], xs[1][:784]])


@pytest.mark.parametrize("extra", [0, 98])
def test_postprocessor_ragged_equals_per_clip_calls(extra):
    """pred of 480 N_i (+ 98: a vocoder with an odd k - u) samples, src of T_i, length T_i; cr included."""
    pp = FE.PostProcessor("cuda")
    srcs, tab = clips48(110)
    preds = [rnd(HOP * n + extra, 120 + i, 0.3) for i, n in enumerate(tab["mel_rows"])]
    # (src: noise low-passed by a moving average of another width per clip, so that every clip has a cutoff of its own)
    srcs = [torch.nn.functional.avg_pool1d(v[None, None], k, 1, k // 2)[0, 0].contiguous() for v, k in zip(srcs, (3, 5, 9, 13, 17))]
    assert [v.numel() for v in srcs] == tab["len_out"]
    refs, crs = [], []
    for p, s_, T in zip(preds, srcs, tab["len_out"]):
        o, cr = pp(p[None], s_[None], T, return_cr=True)
        refs.append(o.clone())
        crs.append(cr.clone())
    packed, views, cr = pp.ragged([p[None] for p in preds], srcs, tab["len_out"], return_cr=True)
    assert packed.numel() == sum(tab["len_out"])
    assert torch.equal(cr, torch.cat(crs)) and len(set(cr.tolist())) > 1
    for v, r in zip(views, refs):
        assert torch.equal(v, r[0])
    assert torch.allclose(torch.stack([v.abs().max() for v in views]), torch.full((5,), 0.99, device="cuda"), atol=1e-6)
    again = pp.ragged(preds, srcs, tab["len_out"])
    assert len(again) == 2 and all(torch.equal(v, r[0]) for v, r in zip(again[1], refs))


# ------------------------------------------------------------------------------------------
# model level: generate_many(ends='ragged') against generate() per clip
# ------------------------------------------------------------------------------------------
SECS = [0.5, 1.31, 0.2, 0.5, 2.2, 0.7713, 0.05]


def net_for(cfgname):
    if cfgname not in _STATE:
        cfg = getattr(synth, cfgname)
        _STATE[cfgname] = FLowHigh(synth.make_state_dict(cfg, 0), cfg, "cuda")
    return _STATE[cfgname]


def model_for(cfgname="TINY_CFG", cfm="basic_cfm", upsampling="hip", prior="reference"):
    return FlowHighSR(net_for(cfgname), sigma=1e-4 if cfm != "basic_cfm" else 0.0, cfm_method=cfm, torchdiffeq_ode_method="euler",
                      upsampling_method=upsampling, prior=prior)


def clip_list():
    """0.05 - 2.2 s at 12 kHz: odd sample counts, an int16 clip, two of equal length, a 5-frame clip."""
    clips = [synth.lowres_clip(140 + i, s_, 12000) for i, s_ in enumerate(SECS)]
    clips[2] = (clips[2] * 20000).astype(np.int16)
    noise = [synth.prior_noise(140 + i, (len(c) * 4) // 480) for i, c in enumerate(clips)]
    return clips, noise


def alone(tag, m, clips, steps, prior_of):
    """generate() per clip, computed once per configuration and shared by the tests that compare against it."""
    if tag not in _STATE:
        _STATE[tag] = [m.generate(c, 12000, 48000, steps, **prior_of(i)).clone() for i, c in enumerate(clips)]
    return _STATE[tag]


def same(many, ones, clips):
    assert len(many) == len(ones)
    for i, (a, b) in enumerate(zip(many, ones)):
        assert tuple(a.shape) == tuple(b.shape) == (1, len(clips[i]) * 4)
        assert torch.equal(a, b), f"clip {i} ({SECS[i]} s) differs from generate() alone"


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


PER_CLIP_ENTRIES = {"fh_frame_f32", "fh_resample_poly_f32", "fh_peak_abs_f32", "fh_peak_scale_f32", "fh_spec_energy_f32",
                    "fh_spec_splice_f32", "fh_istft_ola_f32"}
SEG_ENTRIES = {"fh_frame_seg_f32": 3, "fh_resample_poly_seg_f32": 1, "fh_peak_abs_seg_f32": 1, "fh_peak_scale_seg_f32": 2,
               "fh_spec_energy_seg_f32": 1, "fh_spec_splice_seg_f32": 1, "fh_istft_ola_seg_f32": 1, "fh_rows_to_channels_seg_f32": 1}


@pytest.mark.parametrize("cfgname", ["TINY_CFG", "ODD_CFG"])
def test_generate_many_ragged_ends_equal_generate_per_clip(cfgname, monkeypatch):
    """upsampling_method='hip', prior='reference' with noise=.  ODD_CFG: the vocoder returns 480 N + 98 samples.  A second call of
    the same mix runs out of the cached workspaces: equal again, and the first call's tensors (the caller's own) are untouched.
    The front and back end are one launch per step for the whole list: no per-clip entry is called."""
    m = model_for(cfgname)
    clips, noise = clip_list()
    ones = alone(("hip", cfgname), m, clips, 1, lambda i: dict(noise=noise[i]))
    if cfgname == "ODD_CFG":
        assert m.flowhigh.vocoder.out_len(50) == 480 * 50 + 98
    first, names = count_calls(monkeypatch, lambda: m.generate_many(clips, 12000, 48000, 1, noise=noise, ends="ragged"))
    same(first, ones, clips)
    assert not PER_CLIP_ENTRIES & set(names)
    assert {k: names.count(k) for k in SEG_ENTRIES} == SEG_ENTRIES
    kept = [t.clone() for t in first]
    second = m.generate_many(clips[::-1], 12000, 48000, 1, noise=noise[::-1], ends="ragged")      # another mix in between
    same(second[::-1], ones, clips)
    third = m.generate_many(clips, 12000, 48000, 1, noise=noise, ends="ragged")
    same(third, ones, clips)
    assert all(torch.equal(a, b) for a, b in zip(first, kept))
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(first, third))
    # the default is the per-clip path
    monkeypatch.delenv("FH_RAGGED_ENDS", raising=False)
    _, names = count_calls(monkeypatch, lambda: m.generate_many(clips, 12000, 48000, 1, noise=noise))
    assert not set(SEG_ENTRIES) & set(names) and names.count("fh_istft_ola_f32") == len(clips)
    monkeypatch.setenv("FH_RAGGED_ENDS", "ragged")
    out, names = count_calls(monkeypatch, lambda: m.generate_many(clips, 12000, 48000, 1, noise=noise))
    assert names.count("fh_istft_ola_seg_f32") == 1
    same(out, ones, clips)


def test_generate_many_ragged_ends_in_several_groups():
    """max_frames=200 cuts the list (50 131 20 50 220 77 5 frames) into two ragged groups and a clip that runs alone."""
    m = model_for()
    clips, noise = clip_list()
    ones = alone(("hip", "TINY_CFG"), m, clips, 1, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, 12000, 48000, 1, noise=noise, ends="ragged", max_frames=200), ones, clips)
    # max_frames = 131: [50] alone as a group of one, [131], [20 50], 220 too long, [77 5]
    same(m.generate_many(clips, 12000, 48000, 1, noise=noise, ends="ragged", max_frames=131), ones, clips)


def test_generate_many_ragged_ends_with_host_resampling():
    """upsampling_method='scipy': resampled and normalised on the host per clip, uploaded as one buffer."""
    m = model_for(upsampling="scipy")
    clips, noise = clip_list()
    ones = alone(("scipy", "TINY_CFG"), m, clips, 1, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, 12000, 48000, 1, noise=noise, ends="ragged"), ones, clips)
    same(m.generate_many(clips, 12000, 48000, 1, noise=noise, ends="ragged"), ones, clips)


def test_generate_many_ragged_ends_with_the_device_prior():
    m = model_for(prior="device")
    clips, _ = clip_list()
    ones = alone(("device", "TINY_CFG"), m, clips, 1, lambda i: dict(seed=[(31, i)]))
    same(m.generate_many(clips, 12000, 48000, 1, seed=31, ends="ragged"), ones, clips)
    same(m.generate_many(clips, 12000, 48000, 1, seed=31, ends="ragged", max_frames=200), ones, clips)


def test_generate_many_ragged_ends_independent_cfm_mix_two_steps():
    m = model_for(cfm="independent_cfm_mix")
    clips, noise = clip_list()
    ones = alone(("mix", "TINY_CFG"), m, clips, 2, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, 12000, 48000, 2, noise=noise, ends="ragged"), ones, clips)


def test_batching_server_with_ragged_ends():
    m = model_for()
    srv = BatchingServer(m, max_batch=4, max_wait_ms=200, ends="ragged")
    assert srv.ends == "ragged"
    clips = [synth.lowres_clip(160 + i, s_, 12000) for i, s_ in enumerate([0.2, 0.31, 0.45])]
    futs = [srv.submit(c, 12000, 1, seed=100 + i) for i, c in enumerate(clips)]
    outs = [f.result(timeout=120) for f in futs]
    srv.close()
    for i, (c, y) in enumerate(zip(clips, outs)):
        g = torch.Generator().manual_seed(100 + i)
        one = m.generate(c, 12000, 48000, 1, generator=g)
        assert y.shape == (len(c) * 4,) and np.array_equal(y, one.cpu().numpy()[0])
