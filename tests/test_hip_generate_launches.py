"""GPU: the library entries every form of generate / generate_batch / generate_many / generate_long calls, in order.

Bit equality against generate() per clip (the other test_hip_* files) does not see a mono clip at level='peak' -- a *plain* call --
that takes the multichannel kernels: fh_channel_peaks_f32, fh_row_gain_f32 and fh_group_peak_f32 give the same bits at gain 1,
cost three launches and turn the silent clip's 0 / 0 into zeros.  So the names of every form's library calls (every call goes
through hip.check: count_calls) are compared, as an ordered list, with tests/golden/generate_launch_names.json.  Each form is
called once to warm the per-shape workspaces and plans; the names of the second call are the ones compared.

The fixture is written by `python tests/test_hip_generate_launches.py --record [form ...]` on a GPU (no form: all).  It pins the sequences of the commit it
was recorded at: a change that is meant to leave the launches alone does not record it again.

Models are TINY_CFG at 12 kHz, euler x 1, upsampling_method='hip'; clips are those of test_hip_ragged_ends.clip_list (50, 131, 20,
50, 77 and 5 frames; the 220-frame one is left out), a stereo clip is two of the 50-frame ones."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if __name__ == "__main__":                                                # (--record: no conftest has put the package on the path)
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowhigh_amd import FlowHighSR                                       # noqa: E402
from oracle import ref_cpu                                                # noqa: E402
from test_hip_ragged_ends import clip_list, count_calls, model_for, net_for       # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "generate_launch_names.json"
SR = 12000
LEVEL_ENTRIES = ("fh_channel_peaks_f32", "fh_row_gain_f32", "fh_row_gain_seg_f32", "fh_group_peak_f32")
DELIVERED = dict(pcm="int16", output_rate=16000)
PLAN = dict(window_ms=200, overlap_ms=60, guard_ms=10)          # a 0.3 s clip is two windows: 200 ms, then 160 ms at 140 ms
_STATE = {}


def models():
    if "models" not in _STATE:
        _STATE["models"] = model_for(), model_for(prior="device")
    return _STATE["models"]


def method_model(method):
    """model_for() with another ODE method (the forms that pin the steppers beyond euler x 1)."""
    if method not in _STATE:
        _STATE[method] = FlowHighSR(net_for("TINY_CFG"), sigma=0.0, cfm_method="basic_cfm", torchdiffeq_ode_method=method,
                                    upsampling_method="hip", prior="reference")
    return _STATE[method]


def inputs():
    """(clips, noises): 0 / 1 / 2 / 3 / 5 / 6 of clip_list (0 and 3 are 6000 samples both, 2 is int16), 'st' = the stereo clip."""
    if "inputs" not in _STATE:
        clips, noise = clip_list()
        c, z = {i: clips[i] for i in (0, 1, 2, 3, 5, 6)}, {i: noise[i] for i in (0, 1, 2, 3, 5, 6)}
        c["st"], z["st"] = np.stack([clips[0], clips[3]]), noise[3]
        _STATE["inputs"] = c, z
    return _STATE["inputs"]


def forms():
    """form name -> (plain, the call)."""
    m, md = models()
    c, z = inputs()

    def pick(*ids):
        return [c[i] for i in ids], [z[i] for i in ids]

    def batch(ids, **kw):
        xs, zs = pick(*ids)
        return lambda: m.generate_batch(xs, SR, 48000, 1, noise=torch.cat(zs, 0) if "channels" not in kw else zs, **kw)

    def many(ids, model=m, **kw):
        xs, zs = pick(*ids)
        prior = dict(noise=zs) if model is m else dict(seed=31)
        return lambda: model.generate_many(xs, SR, 48000, 1, **prior, **kw)

    mono, mixed, buckets = (0, 1, 2), (0, "st", 2), (0, 2, 3, 0)
    long_clip = c[1][:3600]
    # the steppers beyond euler x 1: the clips' 48 kHz conditionings for sample / sample_many, the other methods' models
    conds, (xs, zs) = [ref_cpu.preprocess(c[i], SR)[0] for i in mono], pick(*mono)
    rk4, heun3 = method_model("rk4"), method_model("heun3")
    return {
        "sample_rk4_guided": (True, lambda: rk4.sample(cond=conds[0][None], time_steps=2, cond_scale=1.3, noise=zs[0])),
        "many_heun3_ragged": (True, lambda: heun3.generate_many(xs, SR, 48000, 2, noise=zs, ends="ragged")),
        "many_rk4_mixed_steps": (True, lambda: rk4.generate_many(xs, SR, 48000, [1, 3, 2], noise=zs, ends="ragged")),
        "sample_many_mixed_guided": (True, lambda: m.sample_many(conds, time_steps=[1, 3, 2], cond_scale=1.3, mel_pp=True, noise=zs)),
        "generate": (True, lambda: m.generate(c[0], SR, 48000, 1, noise=z[0])),
        "generate_level_input": (False, lambda: m.generate(c[0], SR, 48000, 1, noise=z[0], level="input")),
        "generate_stereo": (False, lambda: m.generate(c["st"], SR, 48000, 1, noise=z["st"], channels="first")),
        "generate_device_prior": (True, lambda: md.generate(c[0], SR, 48000, 1, seed=31)),
        "batch": (True, batch((0, 3))),
        "batch_channels": (False, batch((0, "st"), channels="first")),
        # two lengths, the bucket of three 6000-sample clips splits into 2 + 1
        "buckets": (True, many(buckets, ragged=False, max_batch=2)),
        "buckets_channels": (False, many(mixed, ragged=False, max_batch=2, channels="first")),
        "buckets_channels_split": (False, many(mixed, ragged=False, max_batch=1, channels="first")),
        "buckets_device_prior": (True, many(buckets, md, ragged=False, max_batch=2)),
        "ragged_per_clip": (True, many(mono, ends="per_clip")),
        "ragged_per_clip_channels": (False, many(mixed, ends="per_clip", channels="first")),
        "ragged_ends": (True, many(mono, ends="ragged")),
        "ragged_ends_channels": (False, many(mixed, ends="ragged", channels="first")),
        "ragged_ends_device_prior": (True, many(mono, md, ends="ragged")),
        # max_frames=60 over 50 131 20 5 frames: a group of one (50 + 20 > 60), a clip too long for a sequence, a group of two
        "ragged_ends_small_groups": (True, many((0, 1, 2, 6), ends="ragged", max_frames=60)),
        "ragged_ends_delivered": (True, many(mono, ends="ragged", **DELIVERED)),
        "ragged_per_clip_delivered": (True, many(mono, ends="per_clip", **DELIVERED)),
        "buckets_delivered": (True, many(buckets, ragged=False, max_batch=2, **DELIVERED)),
        "generate_long": (False, lambda: md.generate_long(long_clip, SR, seed=31, **PLAN)),
    }


def names_of(monkeypatch, fn):
    fn()                                        # (workspaces, plans and descriptors of the form's shapes)
    _, names = count_calls(monkeypatch, fn)
    torch.cuda.synchronize()
    return names


def recorded():
    return json.loads(FIXTURE.read_text())


def test_the_fixture_holds_every_form_and_only_entry_names():
    rec = recorded()
    assert sorted(rec) == sorted(forms())
    assert all(n.startswith("fh_") and n.isidentifier() for v in rec.values() for n in v)


@pytest.mark.parametrize("form", sorted(recorded()) if FIXTURE.exists() else ["(no fixture)"])
def test_a_form_calls_the_recorded_entries_in_order(form, monkeypatch):
    plain, fn = forms()[form]
    names = names_of(monkeypatch, fn)
    if plain:
        # (a delivered form rescales at the output rate with fh_group_peak_f32, Delivery's own launch; the post-processor's
        # comes only behind a fh_row_gain*, so their absence covers it)
        level = set(LEVEL_ENTRIES) - ({"fh_group_peak_f32"} if form.endswith("_delivered") else set())
        assert not level & set(names), sorted(level & set(names))
    else:
        assert "fh_channel_peaks_f32" in names
    want = recorded()[form]
    first = next((i for i, (a, b) in enumerate(zip(names, want)) if a != b), min(len(names), len(want)))
    assert names == want, f"{len(names)} calls against {len(want)} recorded; first difference at {first}: " \
                          f"{names[first:first + 3]} against {want[first:first + 3]}"


def test_a_silent_mono_clip_tells_the_two_front_ends_apart():
    """The plain front end divides by the peak as it is: the conditioning signal of a silent clip is 0 / 0, every sample NaN
    (DESIGN.md "Channels and level" rule 6), and the call has no gains.  level='input' goes through fh_channel_peaks_f32, which
    divides a silent row by 1 and gives it gain 0: exact zeros in, exact zeros out.
    The NaN shows in the `cond` stage and not in the waveform: the log-mel's clamp (fmaxf against 1e-5) and the cutoff search
    (no bin's sum is below a NaN limit: bin 0, nothing spliced in) both drop it, so the plain call returns the vocoder's answer
    to the floor mel at 0.99 peak -- finite, and the same bits a zero condition gives."""
    m, _ = models()
    _, z = inputs()
    silent = np.zeros(6000, dtype=np.float32)
    out, stages = m.generate_batch([silent], SR, 48000, 1, noise=z[0], return_stages=True)
    assert "gains" not in stages and not torch.isfinite(stages["cond"]).any()
    assert torch.equal(out, m.generate(silent, SR, 48000, 1, noise=z[0])) and torch.isfinite(out).all() and out.any()
    out, stages = m.generate_batch([silent], SR, 48000, 1, noise=z[0], level="input", return_stages=True)
    assert tuple(out.shape) == (1, 24000) and not out.any()
    assert not stages["cond"].any() and stages["gains"].tolist() == [0.0]
    assert not m.generate(silent, SR, 48000, 1, noise=z[0], level="input").any()


@pytest.mark.parametrize("channels", [None, "first"])
def test_generate_batch_moves_the_generator_as_generate_per_clip_does(channels):
    """One [1, N, n_mels] draw per clip, in clip order, whatever the clips' channel counts (C = 2, 1, 2 with channels=)."""
    m, _ = models()
    c, _ = inputs()
    clips = [c[0], c[3], c[0]] if channels is None else [c["st"], c[3], np.ascontiguousarray(c["st"][::-1])]
    g_batch, g_loop = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    batch = m.generate_batch(clips, SR, 48000, 1, generator=g_batch, channels=channels)
    loop = [m.generate(x, SR, 48000, 1, generator=g_loop, channels=channels) for x in clips]
    assert torch.equal(g_batch.get_state(), g_loop.get_state())
    assert not torch.equal(g_batch.get_state(), torch.Generator().manual_seed(5).get_state())
    for got, want in zip(batch, loop):
        assert torch.equal(got.reshape(want.shape), want)


def record(only):
    mp = pytest.MonkeyPatch()
    out = recorded() if only else {}
    out.update({name: names_of(mp, fn) for name, (_, fn) in forms().items() if not only or name in only})
    FIXTURE.write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
    for name, names in out.items():
        print(f"{name}: {len(names)} calls")


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_hip_generate_launches.py --record [form ...]   (writes tests/golden/generate_launch_names.json)")
    record(sys.argv[2:])
