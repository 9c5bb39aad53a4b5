"""The batched and the segment form of every front / back end entry are instantiations of one kernel body (csrc/frontend.hip)
that differ in how a block finds its clip.  The seg-vs-batched tests of test_hip_ragged_ends.py therefore compare two
instantiations of one body; this file pins the batched locator's own arithmetic (clip b at b * len, rows from b * rows):

  GPU  for every batched entry, ONE call on a batch of 3 == three calls on batches of 1 == the segment entry on a table that
       describes the same three equal-length clips, torch.equal.  2401 samples at 48 kHz (5 mel frames, 6 post-processing
       frames, no multiple of 256 or 480); the resampler on 601 samples at 12 kHz and at 22 050 Hz (down > 1); 70 rows for
       spec_energy (more than the 64 of one pass: both chains run); 5 mel rows at d = 256 and d = 40.  Outputs are NaN-filled
       and followed by a guard; cr / cut and the data differ per clip, so a wrong b shows.
  GPU  the capped grid of the two peak_abs entries: a clip just past 1024 blocks, whose maximum only the grid-stride loop reaches.
  CPU  Resampler.ragged builds the same clip descriptors whether the list has one input rate or one per clip."""
import numpy as np
import pytest
import torch

from flowhigh_amd import frontend as FE                                    # noqa: E402
from flowhigh_amd import hip, tables                                       # noqa: E402
from flowhigh_amd.tables import HOP, N_FFT, P_WIDTH                        # noqa: E402

gpu = pytest.mark.gpu
B, T, GUARD = 3, 2401, 64
N_MEL, N_PP = T // HOP, 1 + T // HOP                                       # 5, 6
_KEEP = []


def rnd(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def call(name, *args):
    hip.check(getattr(hip.lib(), name)(*args, hip.stream()), name)


def dev(part):
    buf, (addr,) = FE.upload_tables([part], torch.device("cuda"))
    _KEEP.append(buf)
    return addr


def p(t, first=0):
    """Address of element `first` of the contiguous float32 / int32 tensor t."""
    return t.data_ptr() + 4 * first


def check_forms(make_out, per_clip, launch):
    """launch(form, out) fills `out` (a tuple of fresh tensors from make_out(): out[0] NaN-filled, B * per_clip elements and a
    guard) by form 'b3' (one batched call), 'b1' (three batched calls of one clip) or 'seg' (the segment entry).  All three
    must give the same bits: out[0] finite over the clips and NaN behind them, every other output equal as it is."""
    outs = {}
    for form in ("b3", "b1", "seg"):
        outs[form] = make_out()
        launch(form, outs[form])
    ref = outs["b3"]
    body = ref[0].reshape(-1)[:B * per_clip]
    assert torch.isfinite(body).all()
    assert not torch.equal(body[:per_clip], body[per_clip:2 * per_clip])          # (the clips differ: a wrong b would show)
    for form, out in outs.items():
        flat = out[0].reshape(-1)
        assert flat.numel() > B * per_clip and torch.isnan(flat[B * per_clip:]).all(), form
        assert torch.equal(flat[:B * per_clip], body), form
        assert all(torch.equal(a, r) for a, r in zip(out[1:], ref[1:])), form
    return ref


@gpu
@pytest.mark.parametrize("mode", ["reflect", "zero"])
def test_frame_forms(mode):
    pad, pm, rows = ((N_FFT - HOP) // 2, 0, N_MEL) if mode == "reflect" else (N_FFT // 2, 1, N_PP)
    x, hann = rnd(B * T, 1, 0.3).view(B, T), FE._Const.get("cuda")["hann"]
    clips = dev(FE.clip_array(src=[p(x, b * T) for b in range(B)], len_in=[T] * B, row0=[b * rows for b in range(B)], rows=[rows] * B))

    def launch(form, out):
        (f,) = out
        if form == "b3":
            call("fh_frame_f32", p(x), p(hann), p(f), B, T, rows, N_FFT, HOP, pad, pm)
        elif form == "b1":
            for b in range(B):
                call("fh_frame_f32", p(x, b * T), p(hann), p(f, b * rows * N_FFT), 1, T, rows, N_FFT, HOP, pad, pm)
        else:
            call("fh_frame_seg_f32", clips, B, rows, T, p(hann), p(f), N_FFT, HOP, pad, pm)
    check_forms(lambda: (nan(B * rows + 1, N_FFT),), rows * N_FFT, launch)


@gpu
def test_spec_energy_forms():
    rows = 70
    spec = rnd(B * rows * P_WIDTH, 2).view(-1, P_WIDTH)
    seg = dev(FE.seg_table([b * rows for b in range(B)], [rows] * B))

    def launch(form, out):
        (e,) = out
        if form == "b3":
            call("fh_spec_energy_f32", p(spec), p(e), B, rows)
        elif form == "b1":
            for b in range(B):
                call("fh_spec_energy_f32", p(spec, b * rows * P_WIDTH), p(e, b * 1025), 1, rows)
        else:
            call("fh_spec_energy_seg_f32", p(spec), p(e), seg, B)
    check_forms(lambda: (nan(B + 1, 1025),), 1025, launch)


@gpu
def test_spec_splice_forms():
    R = B * N_PP
    pred, src = rnd(R * P_WIDTH, 3).view(R, P_WIDTH), rnd(R * P_WIDTH, 4).view(R, P_WIDTH)
    cr = torch.tensor([31, 300, 777], dtype=torch.int32, device="cuda")
    seg = dev(FE.seg_table([b * N_PP for b in range(B)], [N_PP] * B))

    def launch(form, out):
        (o,) = out
        if form == "b3":
            call("fh_spec_splice_f32", p(pred), p(src), p(cr), p(o), B, N_PP)
        elif form == "b1":
            for b in range(B):
                k = b * N_PP * P_WIDTH
                call("fh_spec_splice_f32", p(pred, k), p(src, k), p(cr, b), p(o, k), 1, N_PP)
        else:
            call("fh_spec_splice_seg_f32", p(pred), p(src), p(cr), p(o), seg, B, N_PP)
    (o,) = check_forms(lambda: (nan(R + 1, P_WIDTH),), N_PP * P_WIDTH, launch)
    # bin = 32 q + i of column 64 q + i (re) and 64 q + 32 + i (im): below cr[b] from src, else from pred
    col = torch.arange(P_WIDTH, device="cuda")
    binn = (col >> 6) * 32 + (col & 31)
    for b in range(B):
        rows = slice(b * N_PP, (b + 1) * N_PP)
        assert torch.equal(o[rows], torch.where(binn[None] < cr[b], src[rows], pred[rows]))


@gpu
def test_istft_ola_forms():
    frames, hann = rnd(B * N_PP * N_FFT, 5).view(-1, N_FFT), FE._Const.get("cuda")["hann"]

    def make():
        return nan(B * T + GUARD), torch.zeros(B, dtype=torch.int32, device="cuda")

    def launch(form, out):
        y, peak = out
        if form == "b3":
            call("fh_istft_ola_f32", p(frames), p(hann), p(y), p(peak), B, N_PP, T, N_FFT, HOP)
        elif form == "b1":
            for b in range(B):
                call("fh_istft_ola_f32", p(frames, b * N_PP * N_FFT), p(hann), p(y, b * T), p(peak, b), 1, N_PP, T, N_FFT, HOP)
        else:
            clips = dev(FE.clip_array(dst=[p(y, b * T) for b in range(B)], len_out=[T] * B, row0=[b * N_PP for b in range(B)],
                                      rows=[N_PP] * B))
            call("fh_istft_ola_seg_f32", p(frames), p(hann), clips, B, T, p(peak), N_FFT, HOP)
    y, peak = check_forms(make, T, launch)
    assert torch.equal(peak.view(torch.float32), y[:B * T].view(B, T).abs().max(dim=1).values)


@gpu
def test_peak_abs_and_peak_scale_forms():
    x = rnd(B * T, 6, 0.3).view(B, T) * torch.tensor([1.0, 0.5, 2.0], device="cuda")[:, None]

    def make():
        return torch.cat([x.reshape(-1), nan(GUARD)]), torch.zeros(B, dtype=torch.int32, device="cuda")

    def launch(form, out):
        y, peak = out
        if form == "b3":
            call("fh_peak_abs_f32", p(y), p(peak), B, T)
            call("fh_peak_scale_f32", p(y), p(peak), B, T, 0.99)
        elif form == "b1":
            for b in range(B):
                call("fh_peak_abs_f32", p(y, b * T), p(peak, b), 1, T)
                call("fh_peak_scale_f32", p(y, b * T), p(peak, b), 1, T, 0.99)
        else:
            clips = dev(FE.clip_array(dst=[p(y, b * T) for b in range(B)], len_out=[T] * B))
            call("fh_peak_abs_seg_f32", clips, B, T, p(peak))
            call("fh_peak_scale_seg_f32", clips, B, T, p(peak), 0.99)
    y, peak = check_forms(make, T, launch)
    assert torch.equal(peak.view(torch.float32), x.abs().max(dim=1).values)
    assert torch.allclose(y[:B * T].view(B, T).abs().max(dim=1).values, torch.full((B,), 0.99, device="cuda"), atol=1e-6)


@gpu
@pytest.mark.parametrize("sr", [12000, 22050])
def test_resample_poly_forms(sr):
    n_in = 601
    n_out = tables.resample_out_len(n_in, 48000, sr)
    taps, pre, up, down = tables.resample_poly_plan(48000, sr)
    taps = taps.cuda()
    assert (down > 1) == (sr == 22050) and n_out % 256 != 0
    x = rnd(B * n_in, 7, 0.2).view(B, n_in)

    def launch(form, out):
        (y,) = out
        if form == "b3":
            call("fh_resample_poly_f32", p(x), p(taps), p(y), B, n_in, n_out, up, down, taps.numel(), pre)
        elif form == "b1":
            for b in range(B):
                call("fh_resample_poly_f32", p(x, b * n_in), p(taps), p(y, b * n_out), 1, n_in, n_out, up, down, taps.numel(), pre)
        else:
            clips = dev(FE.clip_array(src=[p(x, b * n_in) for b in range(B)], len_in=[n_in] * B,
                                      dst=[p(y, b * n_out) for b in range(B)], len_out=[n_out] * B))
            call("fh_resample_poly_seg_f32", clips, B, n_out, p(taps), up, down, taps.numel(), pre)
    check_forms(lambda: (nan(B * n_out + GUARD),), n_out, launch)


@gpu
@pytest.mark.parametrize("d", [256, 40])
def test_mel_energy_and_mel_splice_forms(d):
    n = N_MEL
    low, high = rnd(B * n * d, 8).view(-1, d), rnd(B * n * d, 9).view(-1, d)
    cut = torch.tensor([3, 17, 39], dtype=torch.int32, device="cuda")
    seg = dev(FE.seg_table([b * n for b in range(B)], [n] * B))

    def energy(form, out):
        (e,) = out
        if form == "b3":
            call("fh_mel_energy_f32", p(low), p(e), B, n, d)
        elif form == "b1":
            for b in range(B):
                call("fh_mel_energy_f32", p(low, b * n * d), p(e, b * d), 1, n, d)
        else:
            call("fh_mel_energy_seg_f32", p(low), p(e), seg, B, d)
    check_forms(lambda: (nan(B + 1, d),), d, energy)

    def splice(form, out):
        (o,) = out
        if form == "b3":
            call("fh_mel_splice_f32", p(low), p(high), p(cut), p(o), B, n, d)
        elif form == "b1":
            for b in range(B):
                k = b * n * d
                call("fh_mel_splice_f32", p(low, k), p(high, k), p(cut, b), p(o, k), 1, n, d)
        else:
            call("fh_mel_splice_seg_f32", p(low), p(high), p(cut), p(o), seg, B, n, d)
    (o,) = check_forms(lambda: (nan(B * n + 1, d),), n * d, splice)
    col = torch.arange(d, device="cuda")
    for b in range(B):
        rows = slice(b * n, (b + 1) * n)
        assert torch.equal(o[rows], torch.where(col[None] < cut[b], low[rows], high[rows]))


@gpu
def test_peak_abs_capped_grid():
    """262 144 + 300 samples are 1026 blocks of 256, two more than the cap of 1024, so blocks 0 and 1 take a second pass of the
    grid-stride loop; the clip's maximum lies there.  Beside it a clip of 300 samples, most of whose blocks return at once."""
    lens = [1024 * 256 + 300, 300]
    xs = [rnd(n, 10 + i, 0.3) for i, n in enumerate(lens)]
    xs[0][-7] = -5.0
    clips = dev(FE.clip_array(dst=[p(v) for v in xs], len_out=lens))
    peak = torch.zeros(2, dtype=torch.int32, device="cuda")
    call("fh_peak_abs_seg_f32", clips, 2, max(lens), p(peak))
    ref = torch.zeros(2, dtype=torch.int32, device="cuda")
    for i, v in enumerate(xs):
        call("fh_peak_abs_f32", p(v), p(ref, i), 1, v.numel())
    assert torch.equal(peak, ref)
    assert torch.equal(peak.view(torch.float32), torch.stack([v.abs().max() for v in xs]))
    assert float(peak.view(torch.float32)[0]) == 5.0


def test_resampler_descriptors_do_not_depend_on_the_rate_form():
    """Resampler.ragged builds its fh_clip array from ragged_clip_tables and resample_clip_array whether sr_in is one rate or
    one per clip: the same lengths and rates give the same bytes, and in a mixed list a clip's lengths are those of its rate."""
    lens, X, Y = [600, 1500, 2401, 2401, 3000], 0x7f0000001000, 0x7f0000800000
    for sr in (12000, 22050, 48000):
        one = FE.ragged_clip_tables(lens, sr, check_mel=False)
        per = FE.ragged_clip_tables(lens, [sr] * len(lens), check_mel=False)
        assert one == per
        assert bytes(FE.resample_clip_array(one, X, Y)) == bytes(FE.resample_clip_array(per, X, Y))
    a = FE.resample_clip_array(one, X, Y)
    assert [(c.src, c.dst, c.len_in, c.len_out, c.row0, c.rows) for c in a][:2] == \
        [(X, Y, 600, 600, 0, 0), (X + 4 * 600, Y + 4 * 600, 1500, 1500, 0, 0)]
    rates = [12000, 22050, 12000, 48000, 22050]
    mixed = FE.resample_clip_array(FE.ragged_clip_tables(lens, rates, check_mel=False), X, Y)
    assert [c.len_in for c in mixed] == lens
    assert [c.len_out for c in mixed] == [tables.resample_out_len(n, 48000, r) for n, r in zip(lens, rates)]
    assert [c.src for c in mixed] == [X + 4 * sum(lens[:i]) for i in range(5)]
    assert [c.dst for c in mixed] == [Y + 4 * sum(c.len_out for c in list(mixed)[:i]) for i in range(5)]
    distinct, rate_of = FE.rate_index(rates)
    assert distinct == [12000, 22050, 48000] and rate_of.tolist() == [0, 1, 0, 2, 1] and rate_of.dtype == np.int32
    assert FE.rate_tables(rates)[2].tolist() == rate_of.tolist()
