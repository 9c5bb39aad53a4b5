"""GPU: whole models in conv_form='direct_bf16x3' -- the launch plan of 'direct_bf16x6' with its bf16 convs on the two-piece entries
(fh_conv_grouped_bf16x3_f32, fh_narrow_conv_bf16x3_f32): the reference-generated goldens and the full-width vocoder against the CPU
oracle at the project's 1e-4 bar on the waveform (not loosened for this form; tests/tools/bf16x3_estimate.py predicts 2-3e-5), the
bitwise invariants (alone / ragged / batched / chunked / captured) and the weight blob."""
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import E2E_CASES, load_golden          # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, synth  # noqa: E402
from oracle import ref_cpu                            # noqa: E402

FORM = "direct_bf16x3"
FAMILIES = {"direct_bf16x3", "narrow_bf16x3", "direct"}
TOL_WAVEFORM = 1e-4
_MODELS = {}


def model_for(cfg, seed, method="euler", cfm_method="basic_cfm", sigma=0.0, upsampling="scipy", form=FORM):
    key = (repr(sorted(cfg.items())), seed, form)
    if key not in _MODELS:
        sd = synth.make_state_dict(cfg, seed)
        _MODELS[key] = (FLowHigh(sd, cfg, "cuda", conv_form=form), sd)
    fh, sd = _MODELS[key]
    return FlowHighSR(fh, sigma=sigma, cfm_method=cfm_method, torchdiffeq_ode_method=method, upsampling_method=upsampling), sd


@pytest.mark.parametrize("name", E2E_CASES)
def test_generate_matches_reference_golden(name):
    g = load_golden(name)
    m, _ = model_for(g["cfg"], g["seed"], g["method"], g["cfm_method"], g["sigma"])
    voc = m.flowhigh.vocoder
    assert voc.form == FORM and m.flowhigh.conv_form == FORM and m.flowhigh.net.bf is True and not voc.bf and voc.direct_bf == 2
    fams = {f for f, _, _ in voc.plan(1, 20)["conv_launches"]}
    assert "direct_bf16x3" in fams and fams <= FAMILIES
    out, st = m.generate_batch([g["audio"]], g["sr_in"], 48000, g["steps"], noise=torch.from_numpy(g["noise"]), return_stages=True)
    assert int(st["cr"][0].item()) == g["cr"]                               # integer: exact
    e_wav, e_out = np.abs(st["wav"].cpu().numpy() - g["wav"]).max(), np.abs(out.cpu().numpy() - g["out"]).max()
    print(f"{name}: wav {e_wav:.2e}, out {e_out:.2e} from the reference's golden (bar {TOL_WAVEFORM:.0e})")
    assert e_wav <= TOL_WAVEFORM
    assert e_out <= TOL_WAVEFORM


def test_full_width_vs_oracle_and_the_other_direct_forms():
    """SYNTH_CFG (1536 .. 24 channels) on a 0.3 s clip, 16 -> 48 kHz, midpoint x 1: against the CPU oracle at the 1e-4 bar; the
    distances to 'direct' and 'direct_bf16x6' are printed, and the bits differ from 'direct_bf16x6': the two-piece entries ran."""
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    cfg = synth.SYNTH_CFG
    mn, sd = model_for(cfg, 0, "midpoint")
    assert {f for f, _, _ in mn.flowhigh.vocoder.plan(1, 30)["conv_launches"]} == FAMILIES
    audio = synth.lowres_clip(0, 0.3, 16000)
    noise = synth.prior_noise(0, (len(audio) * 3) // 480)
    on, sn = mn.generate_batch([audio], 16000, 48000, 1, noise=noise, return_stages=True)
    others = {}
    for form in ("direct", "direct_bf16x6"):
        mo, _ = model_for(cfg, 0, "midpoint", form=form)
        others[form] = mo.generate_batch([audio], 16000, 48000, 1, noise=noise, return_stages=True)[1]["wav"]
    ref, rs = ref_cpu.generate(sd, cfg, audio, 16000, noise, 1, "midpoint", return_stages=True)
    assert int(sn["cr"][0].item()) == rs["cr"]
    e_new = (sn["wav"].cpu() - rs["wav"]).abs().max().item()
    e_out = (on.cpu() - ref).abs().max().item()
    dist = {f: (sn["wav"] - w).abs().max().item() for f, w in others.items()}
    e_oth = {f: (w.cpu() - rs["wav"]).abs().max().item() for f, w in others.items()}
    print(f"vocoder output vs oracle: direct_bf16x3 {e_new:.2e} (out {e_out:.2e}), direct {e_oth['direct']:.2e}, direct_bf16x6 "
          f"{e_oth['direct_bf16x6']:.2e}; direct_bf16x3 to direct {dist['direct']:.2e}, to direct_bf16x6 {dist['direct_bf16x6']:.2e}")
    assert e_new <= TOL_WAVEFORM and e_out <= TOL_WAVEFORM
    assert not torch.equal(sn["wav"], others["direct_bf16x6"])


def test_alone_ragged_batched_chunked_and_captured_runs_give_the_same_bits():
    cfg = synth.SYNTH_CFG
    m, _ = model_for(cfg, 0, "euler")
    secs = [0.5, 1.31, 0.5, 2.2]
    clips = [synth.lowres_clip(240 + i, s_, 12000) for i, s_ in enumerate(secs)]
    noise = [synth.prior_noise(240 + i, (len(c) * 4) // 480) for i, c in enumerate(clips)]
    alone = [m.generate(c, 12000, 48000, 1, noise=z).clone() for c, z in zip(clips, noise)]
    many = m.generate_many(clips, 12000, 48000, 1, noise=noise, ragged=True)
    assert all(torch.equal(a, b) for a, b in zip(alone, many))
    both = m.generate_batch([clips[0], clips[2]], 12000, 48000, 1, noise=torch.cat([noise[0], noise[2]], 0))
    assert torch.equal(both[0:1], alone[0]) and torch.equal(both[1:2], alone[2])
    voc = m.flowhigh.vocoder
    mel = (torch.randn(1, 150, 256, generator=torch.Generator().manual_seed(5)) * 2.0 - 3.0).cuda()
    assert torch.equal(voc.forward_chunked(mel, 48), voc.forward(mel))
    # the whole device path as one captured graph
    mh, _ = model_for(cfg, 0, "euler", upsampling="hip")
    n_in = 6000
    g = mh.capture(1, n_in, 12000, 1)
    x = torch.from_numpy(synth.lowres_clip(50, n_in / 12000, 12000)[None]).cuda()
    z = synth.prior_noise(50, 50).cuda().reshape(50, -1).contiguous()
    g.x.copy_(x)
    g.noise.copy_(z)
    got = g.replay().clone()
    assert torch.equal(got, mh.generate_from_device(x, 12000, 1, noise=z))


def test_weight_blob_round_trip_and_refusal_for_another_form(tmp_path, monkeypatch, caplog):
    from flowhigh_amd import convert, weights
    cfg = synth.TINY_CFG
    synth.write_checkpoint_dir(tmp_path, cfg, seed=5)
    monkeypatch.setenv("FH_BLOB", "0")
    ref_model = FlowHighSR.from_local(tmp_path, "cuda", conv_form=FORM, torchdiffeq_ode_method="euler")
    assert ref_model.flowhigh.conv_form == FORM
    clip, noise = synth.lowres_clip(3, 1.0, 12000), synth.prior_noise(3, 100)
    ref = ref_model.generate(clip, 12000, 48000, 1, noise=noise)
    r = convert.convert(tmp_path, conv_form=FORM)
    assert r["form"] == FORM
    monkeypatch.delenv("FH_BLOB")
    calls = []
    import flowhigh_amd.flowhighsr as M
    real = M._load_checkpoint
    monkeypatch.setattr(M, "_load_checkpoint", lambda p: calls.append(p) or real(p))
    m = FlowHighSR.from_local(tmp_path, "cuda", conv_form=FORM, torchdiffeq_ode_method="euler")
    assert not calls and m.flowhigh.conv_form == FORM and m.flowhigh.net.bf is True and m.flowhigh.vocoder.direct_bf == 2
    assert torch.equal(m.generate(clip, 12000, 48000, 1, noise=noise), ref)
    # the same blob asked for conv_form='direct_bf16x6': declined with a log line, the checkpoints are read instead
    with caplog.at_level(logging.WARNING, logger="flowhigh_amd"):
        md = FlowHighSR.from_local(tmp_path, "cuda", conv_form="direct_bf16x6", torchdiffeq_ode_method="euler")
    assert calls and md.flowhigh.conv_form == "direct_bf16x6"
    assert any("not used" in rec.getMessage() for rec in caplog.records)
    assert weights.WeightStore.why
    assert (md.generate(clip, 12000, 48000, 1, noise=noise) - ref).abs().max().item() <= TOL_WAVEFORM
