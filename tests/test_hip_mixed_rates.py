"""GPU: clips of different INPUT RATES in one ragged sequence -- fh_resample_poly_rates_seg_f32 (csrc/frontend.hip),
Resampler.ragged with a rate per clip, generate_many(clips, [sr_0, sr_1, ...]) and the BatchingServer on top of it.

The contract is bitwise: every clip gets what the one-rate entry / generate() gives for that clip alone at its own rate, so
every comparison is torch.equal.  Entry tests run five clips of 600 / 1500 / 2401 / 2401 / 3000 samples at 12 / 22.05 / 48 / 8 /
44.1 kHz (48 kHz lengths 2400 / 3266 / 2401 / 14406 / 3266: up = 4, 320, 1 (the copy), 6, 160; two clips of one input length
at different rates, two of one output length at different rates); outputs are NaN-filled first and followed by a guard."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth                 # noqa: E402
from flowhigh_amd import frontend as FE                                    # noqa: E402
from flowhigh_amd import tables                                            # noqa: E402
from flowhigh_amd.serve import BatchingServer                              # noqa: E402

LENS = [600, 1500, 2401, 2401, 3000]
RATES = [12000, 22050, 48000, 8000, 44100]
GUARD = 64
ENTRY = "fh_resample_poly_rates_seg_f32"
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


def entry_refs(xs, rates):
    """fh_resample_poly_f32 on every clip alone with the plan of its own rate (equal rates: a clone)."""
    L, refs = hip.lib(), []
    for v, sr in zip(xs, rates):
        plan = tables.resample_poly_plan(48000, sr)
        if plan is None:
            refs.append(v.clone())
            continue
        taps, pre, up, down = plan
        taps = taps.cuda()
        r = nan(tables.resample_out_len(v.numel(), 48000, sr))
        hip.check(L.fh_resample_poly_f32(v.data_ptr(), taps.data_ptr(), r.data_ptr(), 1, v.numel(), r.numel(), up, down,
                                         taps.numel(), pre, st()), "fh_resample_poly_f32")
        refs.append(r)
    return refs


# ------------------------------------------------------------------------------------------
# the entry
# ------------------------------------------------------------------------------------------
def test_resample_poly_rates_seg_equals_the_entry_per_clip():
    L = hip.lib()
    tab = FE.ragged_clip_tables(LENS, RATES, check_mel=False)
    assert tab["len_out"] == [2400, 3266, 2401, 14406, 3266]
    xs = [rnd(n, 10 + i, 0.2) for i, n in enumerate(LENS)]
    x = torch.cat(xs)
    y = nan(sum(tab["len_out"]) + GUARD)
    bank, rows, rate_of = FE.rate_tables(RATES)
    bank_dev = torch.from_numpy(bank).cuda()
    clips, rows_dev, rate_of_dev = tables_dev(
        FE.clip_array(src=[x.data_ptr() + 4 * o for o in tab["in_off"]], len_in=tab["len_in"],
                      dst=[y.data_ptr() + 4 * o for o in tab["out_off"]], len_out=tab["len_out"]), rows, rate_of)
    hip.check(L.fh_resample_poly_rates_seg_f32(clips, rate_of_dev, 5, max(tab["len_out"]), rows_dev, len(rows), bank_dev.data_ptr(),
                                               bank_dev.numel(), st()), ENTRY)
    refs = entry_refs(xs, RATES)
    for o, n, r in zip(tab["out_off"], tab["len_out"], refs):
        assert r.numel() == n and torch.isfinite(r).all() and torch.equal(y[o:o + n], r)
    assert torch.equal(y[tab["out_off"][2]:tab["out_off"][2] + 2401], xs[2])                 # 48 kHz in: the copy
    assert not torch.equal(y[tab["out_off"][1]:tab["out_off"][1] + 3266], y[tab["out_off"][4]:tab["out_off"][4] + 3266])
    assert torch.isnan(y[-GUARD:]).all()
    # argument errors: nothing launched
    assert L.fh_resample_poly_rates_seg_f32(clips, 0, 5, 100, rows_dev, 5, bank_dev.data_ptr(), bank_dev.numel(), st()) == -1
    assert ENTRY.encode() in L.fh_last_error()
    assert L.fh_resample_poly_rates_seg_f32(clips, rate_of_dev, 5, 100, rows_dev, 0, bank_dev.data_ptr(), bank_dev.numel(), st()) == -1
    assert L.fh_resample_poly_rates_seg_f32(clips, rate_of_dev, 5, 100, rows_dev, 5, 0, 8, st()) == -1


def test_resample_poly_rates_seg_leaves_a_clip_with_a_bad_row_unwritten():
    """The tables are device memory the entry cannot read, so the kernel checks a clip's row before it uses it.  Seven clips: the
    five above and two more of 600 samples.  Clip 5 has rate_of == n_rates, where a VALID spare row lies behind the table; clip 6
    has a row of the table whose taps end 100 floats past the bank_len handed over, inside spare finite floats behind the bank.
    A kernel without the guards would compute finite numbers for them from allocated memory; with them both stay NaN."""
    L = hip.lib()
    lens, rates = LENS + [600, 600], RATES + [12000, 12000]
    tab = FE.ragged_clip_tables(lens, rates, check_mel=False)
    xs = [rnd(n, 30 + i, 0.2) for i, n in enumerate(lens)]
    x = torch.cat(xs)
    y = nan(sum(tab["len_out"]) + GUARD)
    bank, rows, rate_of = FE.rate_tables(RATES)
    spare = 256
    bank_dev = torch.cat([torch.from_numpy(bank), torch.full((spare,), 0.01)]).cuda()
    good = rows[0]                                                                # the 12 kHz row
    n_rates = 6
    over = hip.Rate(bank.size - 100, 200, good.up, good.down, 25)                 # ends at bank_len + 100 <= bank_len + spare
    table = (hip.Rate * (n_rates + 1))(*rows, over, hip.Rate(good.taps_off, good.n_taps, good.up, good.down, good.n_pre_remove))
    rate_of = np.concatenate([rate_of, np.array([n_rates, 5], dtype=np.int32)])
    clips, rows_dev, rate_of_dev = tables_dev(
        FE.clip_array(src=[x.data_ptr() + 4 * o for o in tab["in_off"]], len_in=tab["len_in"],
                      dst=[y.data_ptr() + 4 * o for o in tab["out_off"]], len_out=tab["len_out"]), table, rate_of)
    hip.check(L.fh_resample_poly_rates_seg_f32(clips, rate_of_dev, 7, max(tab["len_out"]), rows_dev, n_rates, bank_dev.data_ptr(),
                                               bank.size, st()), ENTRY)
    refs = entry_refs(xs[:5], RATES)
    for o, n, r in zip(tab["out_off"], tab["len_out"], refs):
        assert torch.equal(y[o:o + n], r)
    for i in (5, 6):
        o, n = tab["out_off"][i], tab["len_out"][i]
        assert n == 2400 and torch.isnan(y[o:o + n]).all(), f"clip {i}: a bad rate row was used"
    assert torch.isnan(y[-GUARD:]).all()
    # a negative field or a non-positive up / down is refused the same way (the bank handed over starts 8 floats into the
    # allocation, so that taps_off = -1 stays inside it too)
    for bad in (hip.Rate(-1, 10, 4, 1, 0), hip.Rate(0, -1, 4, 1, 0), hip.Rate(0, 10, 0, 1, 0), hip.Rate(0, 10, 4, 0, 0),
                hip.Rate(0, 10, -4, 1, 0)):
        y2 = nan(2400 + GUARD)
        c2, r2, ro2 = tables_dev(FE.clip_array(src=[xs[5].data_ptr()], len_in=[600], dst=[y2.data_ptr()], len_out=[2400]),
                                 (hip.Rate * 1)(bad), np.zeros(1, np.int32))
        hip.check(L.fh_resample_poly_rates_seg_f32(c2, ro2, 1, 2400, r2, 1, bank_dev.data_ptr() + 32, bank.size - 8, st()), ENTRY)
        assert torch.isnan(y2).all(), (bad.taps_off, bad.n_taps, bad.up, bad.down)


# ------------------------------------------------------------------------------------------
# Resampler.ragged with a rate per clip
# ------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("where", ["host", "device"])
def test_resampler_ragged_with_a_rate_per_clip_equals_per_clip_calls(where, monkeypatch):
    rs = FE.Resampler("cuda")
    host = [(0.1 * np.random.default_rng(80 + i).standard_normal(n)).astype(np.float32) for i, n in enumerate(LENS)]
    xs = host if where == "host" else [torch.from_numpy(h).cuda() for h in host]

    def alone(rates):
        return [rs(torch.from_numpy(h).cuda()[None], sr)[0] for h, sr in zip(host, rates)]
    refs = alone(RATES)
    (packed, views), names = count_calls(monkeypatch, lambda: rs.ragged(xs, RATES))
    assert names.count(ENTRY) == 1 and names.count("fh_resample_poly_seg_f32") == 0
    assert names.count("fh_peak_abs_seg_f32") == 1 and names.count("fh_peak_scale_seg_f32") == 1 and len(names) == 3
    assert packed.numel() == sum(r.numel() for r in refs)
    for v, r in zip(views, refs):
        assert torch.equal(v, r) and float(r.abs().max()) == 1.0
    kept = [v.clone() for v in views]
    # the same lengths at permuted rates: another mix with buffers and descriptors of its own
    perm = RATES[::-1]
    refs_p = alone(perm)
    packed_p, views_p = rs.ragged(xs, perm)
    assert packed_p.data_ptr() != packed.data_ptr()
    assert [v.numel() for v in views_p] != [v.numel() for v in views]
    for v, r in zip(views_p, refs_p):
        assert torch.equal(v, r)
    assert all(torch.equal(v, k) for v, k in zip(views, kept))
    # the first mix again: its workspace, its descriptors, the same result
    n_ws = len(rs._ws)
    packed2, views2 = rs.ragged(xs, RATES)
    assert packed2.data_ptr() == packed.data_ptr() and len(rs._ws) == n_ws
    assert all(torch.equal(v, r) for v, r in zip(views2, refs))
    # one rate for every clip, as an int or as a list: the one-rate entry, as before
    for sr in (12000, [12000] * 5):
        (_, views1), names = count_calls(monkeypatch, lambda: rs.ragged(xs, sr))
        assert names.count("fh_resample_poly_seg_f32") == 1 and names.count(ENTRY) == 0 and len(names) == 3
        assert all(torch.equal(v, r) for v, r in zip(views1, alone([12000] * 5)))
    assert (12000, 48000, tuple(LENS)) in rs._ws


# ------------------------------------------------------------------------------------------
# model level: generate_many(clips, rates) against generate(clip_i, sr_i) per clip
# ------------------------------------------------------------------------------------------
MIX = [(0.5, 12000), (1.31, 8000), (0.2, 22050), (0.5, 12000), (0.5, 24000), (0.7713, 44100), (0.05, 16000), (0.3, 48000)]
T48 = [24000, 62880, 9600, 24000, 24000, 37023, 2400, 14400]
MIX_RATES = [sr for _, sr in MIX]


def net():
    if "net" not in _STATE:
        cfg = synth.TINY_CFG
        _STATE["net"] = FLowHigh(synth.make_state_dict(cfg, 0), cfg, "cuda")
    return _STATE["net"]


def model_for(cfm="basic_cfm", upsampling="hip", prior="reference"):
    return FlowHighSR(net(), sigma=1e-4 if cfm != "basic_cfm" else 0.0, cfm_method=cfm, torchdiffeq_ode_method="euler",
                      upsampling_method=upsampling, prior=prior)


def clip_list():
    """Two clips equal in length and rate, one of the same 48 kHz length at another rate, a 48 kHz length that is no multiple
    of 480, an int16 clip, a 5-frame clip and one that is 48 kHz already."""
    clips = [synth.lowres_clip(240 + i, s_, sr) for i, (s_, sr) in enumerate(MIX)]
    clips[2] = (clips[2] * 20000).astype(np.int16)
    assert [tables.resample_out_len(len(c), 48000, sr) for c, sr in zip(clips, MIX_RATES)] == T48
    assert [t // 480 for t in T48] == [50, 131, 20, 50, 50, 77, 5, 30]
    assert len(clips[0]) == len(clips[3]) and len(clips[0]) != len(clips[4])
    noise = [synth.prior_noise(240 + i, t // 480) for i, t in enumerate(T48)]
    return clips, noise


def alone(tag, m, clips, steps, prior_of):
    """generate() per clip at its own rate, computed once per configuration and shared by the tests that compare against it."""
    if tag not in _STATE:
        _STATE[tag] = [m.generate(c, sr, 48000, steps, **prior_of(i)).clone() for i, (c, sr) in enumerate(zip(clips, MIX_RATES))]
    return _STATE[tag]


def same(many, ones, t48=T48, what=MIX):
    assert len(many) == len(ones)
    for i, (a, b) in enumerate(zip(many, ones)):
        assert tuple(a.shape) == tuple(b.shape) == (1, t48[i])
        assert torch.equal(a, b), f"clip {i} {what[i]} differs from generate() alone"


PER_CLIP_ENTRIES = {"fh_frame_f32", "fh_resample_poly_f32", "fh_peak_abs_f32", "fh_peak_scale_f32", "fh_spec_energy_f32",
                    "fh_spec_splice_f32", "fh_istft_ola_f32"}
SEG_ENTRIES = {"fh_frame_seg_f32": 3, "fh_resample_poly_seg_f32": 0, ENTRY: 1, "fh_peak_abs_seg_f32": 1, "fh_peak_scale_seg_f32": 2,
               "fh_spec_energy_seg_f32": 1, "fh_spec_splice_seg_f32": 1, "fh_istft_ola_seg_f32": 1, "fh_rows_to_channels_seg_f32": 1}


def test_generate_many_mixed_rates_ragged_ends(monkeypatch):
    """One launch sequence for the eight clips, its front end one launch per step: one resampling launch with a filter per clip,
    no per-clip entry.  The second call of the mix runs out of the cached workspaces; the first call's tensors are the caller's."""
    m = model_for()
    clips, noise = clip_list()
    ones = alone("hip", m, clips, 1, lambda i: dict(noise=noise[i]))
    first, names = count_calls(monkeypatch, lambda: m.generate_many(clips, MIX_RATES, 48000, 1, noise=noise, ends="ragged"))
    same(first, ones)
    assert not PER_CLIP_ENTRIES & set(names)
    assert {k: names.count(k) for k in SEG_ENTRIES} == SEG_ENTRIES
    kept = [t.clone() for t in first]
    second = m.generate_many(clips, tuple(MIX_RATES), 48000, 1, noise=noise, ends="ragged")
    same(second, ones)
    assert all(torch.equal(a, b) for a, b in zip(first, kept))
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(first, second))
    # equal lengths at different rates are different shapes: two clips of 6000 samples, at 12 and at 24 kHz, are a ragged pair
    pair, names = count_calls(monkeypatch, lambda: m.generate_many([clips[0], clips[0]], [12000, 24000], 48000, 1,
                                                                   noise=[noise[0], synth.prior_noise(1, 25)], ends="ragged"))
    assert names.count(ENTRY) == 1 and tuple(pair[1].shape) == (1, 12000) and torch.equal(pair[0], ones[0])


def test_generate_many_mixed_rates_per_clip_ends_and_buckets():
    m = model_for()
    clips, noise = clip_list()
    ones = alone("hip", m, clips, 1, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, MIX_RATES, 48000, 1, noise=noise, ends="per_clip"), ones)
    same(m.generate_many(clips, MIX_RATES, 48000, 1, noise=noise, ragged=False), ones)


@pytest.mark.parametrize("ends", ["ragged", "per_clip"])
def test_generate_many_mixed_rates_in_several_groups(ends):
    """max_frames=200 cuts 50 131 20 50 50 77 5 30 frames into [50 131] [20 50 50 77] [5 30]; max_frames=131 into [50] and [131]
    alone, [20 50 50] and [77 5 30]: the clips that run alone take their own rate."""
    m = model_for()
    clips, noise = clip_list()
    ones = alone("hip", m, clips, 1, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, MIX_RATES, 48000, 1, noise=noise, ends=ends, max_frames=200), ones)
    same(m.generate_many(clips, MIX_RATES, 48000, 1, noise=noise, ends=ends, max_frames=131), ones)


def test_generate_many_mixed_rates_with_host_resampling():
    m = model_for(upsampling="scipy")
    clips, noise = clip_list()
    ones = alone("scipy", m, clips, 1, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, MIX_RATES, 48000, 1, noise=noise, ends="ragged"), ones)
    same(m.generate_many(clips, MIX_RATES, 48000, 1, noise=noise, ends="ragged"), ones)


def test_generate_many_mixed_rates_with_the_device_prior():
    m = model_for(prior="device")
    clips, _ = clip_list()
    ones = alone("device", m, clips, 1, lambda i: dict(seed=[(31, i)]))
    same(m.generate_many(clips, MIX_RATES, 48000, 1, seed=31, ends="ragged"), ones)
    same(m.generate_many(clips, MIX_RATES, 48000, 1, seed=31, ends="ragged", max_frames=200), ones)


def test_generate_many_mixed_rates_independent_cfm_mix_two_steps():
    m = model_for(cfm="independent_cfm_mix")
    clips, noise = clip_list()
    ones = alone("mix", m, clips, 2, lambda i: dict(noise=noise[i]))
    same(m.generate_many(clips, MIX_RATES, 48000, 2, noise=noise, ends="ragged"), ones)


def test_generate_many_draws_the_host_prior_per_clip_rate():
    """No noise=: the frame count of every clip's draw comes from its own rate, in list order from one generator."""
    m = model_for()
    clips, _ = clip_list()
    g = torch.Generator().manual_seed(5)
    ones = [m.generate(c, sr, 48000, 1, generator=g).clone() for c, sr in zip(clips[:4], MIX_RATES[:4])]
    same(m.generate_many(clips[:4], MIX_RATES[:4], 48000, 1, generator=torch.Generator().manual_seed(5), ends="ragged"), ones)


def test_generate_many_refuses_a_bad_rate_list_before_any_work():
    m = model_for()
    clips, noise = clip_list()
    with pytest.raises(ValueError, match="7 rates for 8 clips"):
        m.generate_many(clips, MIX_RATES[:7], 48000, 1, noise=noise)
    with pytest.raises(ValueError):
        m.generate_many(clips[:2], [12000, 0], 48000, 1, noise=noise[:2])


def test_generate_many_nine_rates_in_one_call(monkeypatch):
    """0.1 s at every rate of a serving mix.  11025 Hz: up = 640, a filter of 12 801 taps (+ padding) in the middle of a bank of
    nine filters."""
    m = model_for()
    rates = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
    clips = [synth.lowres_clip(300 + i, 0.1, sr) for i, sr in enumerate(rates)]
    t48 = [tables.resample_out_len(len(c), 48000, sr) for c, sr in zip(clips, rates)]
    assert t48[1] == 4798 and set(t48) == {4798, 4800}
    plan = tables.resample_poly_plan(48000, 11025)
    assert plan[2:] == (640, 147) and plan[0].numel() > 12801
    noise = [synth.prior_noise(300 + i, t // 480) for i, t in enumerate(t48)]
    ones = [m.generate(c, sr, 48000, 1, noise=z).clone() for c, sr, z in zip(clips, rates, noise)]
    many, names = count_calls(monkeypatch, lambda: m.generate_many(clips, rates, 48000, 1, noise=noise, ends="ragged"))
    assert names.count(ENTRY) == 1 and not PER_CLIP_ENTRIES & set(names)
    same(many, ones, t48, rates)


def test_batching_server_with_three_rates():
    m = model_for()
    srv = BatchingServer(m, max_batch=4, max_wait_ms=200, ends="ragged", mix_rates=True)
    assert srv.mix_rates is True
    reqs = [(0.2, 8000), (0.31, 12000), (0.45, 16000)]
    clips = [synth.lowres_clip(260 + i, s_, sr) for i, (s_, sr) in enumerate(reqs)]
    futs = [srv.submit(c, sr, 1, seed=100 + i) for i, (c, (_, sr)) in enumerate(zip(clips, reqs))]
    outs = [f.result(timeout=120) for f in futs]
    srv.close()
    for i, (c, (_, sr), y) in enumerate(zip(clips, reqs, outs)):
        g = torch.Generator().manual_seed(100 + i)
        one = m.generate(c, sr, 48000, 1, generator=g)
        assert y.shape == (tables.resample_out_len(len(c), 48000, sr),) and np.array_equal(y, one.cpu().numpy()[0])
