"""GPU: attention in the bf16 x 6 form (attention_bf.hip; fh_attention_bf16x6_f32 / _seg_f32; attn_form='bf16x6').

  * the project's tolerances, mirrored from tests/test_hip_ops.py and tests/test_hip_e2e.py with the new entry / keyword;
  * the bitwise invariants the fp32 kernel has (batch, ragged, generate_many, graph replay, run to run);
  * accuracy with the fp32 kernel as yardstick: RMS error to a float64 attention of the very tensor the kernels read, bf16 x 6
    <= 1.25 x fp32 (measured ratios: profiles/attention_bf16x6.md);
  * every one of the twelve piece-pair MFMAs pinned by an exact construction (tests/tools/attn_pins.py, checked on the host by
    tests/test_attn_form_cpu.py; the mutant table: profiles/attention_bf16x6.md)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import attn_pins as AP                                       # noqa: E402
from conftest import E2E_CASES, load_golden                  # noqa: E402
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth, tables      # noqa: E402
from oracle import ref_cpu                                   # noqa: E402
from test_hip_bf16x6_pairs import assert_same, designed_values         # noqa: E402

DEV = "cuda"
H, D = 16, 1024
TOL_WAVEFORM = 1e-4
RMS_RATIO_MAX = 1.25
_MODELS = {}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def maxdiff(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def attn(qkv, B, n, form="bf16x6", scale=AP.SCALE):
    name = "fh_attention_bf16x6_f32" if form == "bf16x6" else "fh_attention_f32"
    out = torch.full((B * n, D), float("nan"), device=DEV)
    hip.check(getattr(hip.lib(), name)(qkv.data_ptr(), out.data_ptr(), B, n, H, scale, hip.stream()), name)
    return out


def model_for(cfg, seed, method="euler", cfm_method="basic_cfm", sigma=0.0, upsampling="scipy", conv_form=None, attn_form="bf16x6"):
    key = (repr(sorted(cfg.items())), seed, conv_form, attn_form)
    if key not in _MODELS:
        sd = synth.make_state_dict(cfg, seed)
        _MODELS[key] = (FLowHigh(sd, cfg, "cuda", conv_form=conv_form, attn_form=attn_form), sd)
    fh, sd = _MODELS[key]
    assert fh.attn_form == attn_form and fh.net.attn_form == attn_form
    return FlowHighSR(fh, sigma=sigma, cfm_method=cfm_method, torchdiffeq_ode_method=method, upsampling_method=upsampling), sd


def post_rope_qkv(n, B):
    """The qkv tensor of tests/test_hip_ops.py::test_attention_block after fh_qknorm_rope_f32, and what is needed to finish the block."""
    sd = synth.make_flow_state_dict(seed=3)
    p = "flowhigh.transformer.layers.0.3."
    x = rnd(B, n, D, seed=150)
    M = B * n
    L = hip.lib()
    qkv = torch.empty(M, 3 * D, device=DEV)
    hip.gemm(x.view(M, D).to(DEV), sd[p + "to_qkv.weight"].to(DEV), qkv, M, 3 * D, D)
    cos_t, sin_t = tables.rotary_tables(sd["flowhigh.transformer.rotary_emb.inv_freq"], n)
    gq = sd[p + "q_norm.gamma"].reshape(H, 64).contiguous().to(DEV)
    gk = sd[p + "k_norm.gamma"].reshape(H, 64).contiguous().to(DEV)
    cd, sn = cos_t.to(DEV), sin_t.to(DEV)
    hip.check(L.fh_qknorm_rope_f32(qkv.data_ptr(), gq.data_ptr(), gk.data_ptr(), cd.data_ptr(), sn.data_ptr(), B, n, H,
                                   hip.stream()), "qknorm_rope")
    torch.cuda.synchronize()
    return sd, p, x, qkv


# ---- the project's tolerances ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 1000, 3000])
def test_attention_block_bf16x6(n):
    """test_attention_block with fh_attention_bf16x6_f32, same bar."""
    B = 1 if n > 1000 else 2
    sd, p, x, qkv = post_rope_qkv(n, B)
    ref = ref_cpu.attention(sd, p, x, ref_cpu.rotary_table(sd, n))
    att = attn(qkv, B, n)
    out = torch.empty(B * n, D, device=DEV)
    hip.gemm(att, sd[p + "to_out.weight"].to(DEV), out, B * n, D, D)
    err = maxdiff(out.view(B, n, D), ref)
    print(f"attention block n={n}: max |error| {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16x6"])
@pytest.mark.parametrize("B,n,t", [(1, 25, 0.0), (2, 200, 0.3), (1, 3000, 0.5)])
def test_flow_forward_attn_bf16x6(B, n, t, bf):
    """test_flow_forward with attn_form='bf16x6', both forms of the linears, same bar."""
    from flowhigh_amd.flow import FlowNet
    sd = synth.make_flow_state_dict(seed=0)
    x, cond = rnd(B, n, 256, seed=160), rnd(B, n, 256, seed=161, scale=3.0) - 4.0
    ref = ref_cpu.flow_forward(sd, x, cond, t)
    net = FlowNet(sd, DEV, bf=bf, attn_form="bf16x6")
    xd, cd = x.view(B * n, 256).to(DEV), cond.view(B * n, 256).to(DEV)
    net.set_cond(cd, B, n)
    out = torch.empty(B * n, 256, device=DEV)
    net.forward(xd, t, out, B, n)
    err = maxdiff(out.view(B, n, 256), ref)
    print(f"flow forward B={B} n={n} linears {'bf16x6' if bf else 'f32'}: max |error| {err:.3e}")
    assert err <= 5e-5
    out2 = torch.empty(B * n, 256, device=DEV)
    net.forward(xd, t, out2, B, n, alpha=0.5, res=xd)
    assert maxdiff(out2.view(B, n, 256), x + 0.5 * ref) <= 5e-5


@pytest.mark.parametrize("name", E2E_CASES)
def test_generate_matches_reference_golden_attn_bf16x6(name):
    g = load_golden(name)
    m, _ = model_for(g["cfg"], g["seed"], g["method"], g["cfm_method"], g["sigma"])
    out, st = m.generate_batch([g["audio"]], g["sr_in"], 48000, g["steps"], noise=torch.from_numpy(g["noise"]),
                               return_stages=True)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == g["out"].shape
    assert int(st["cr"][0].item()) == g["cr"]
    assert np.abs(st["wav"].cpu().numpy() - g["wav"]).max() <= TOL_WAVEFORM
    assert np.abs(out.cpu().numpy() - g["out"]).max() <= TOL_WAVEFORM


def test_generate_synth_cfg_vs_oracle_attn_bf16x6():
    """Full-width vocoder (SYNTH-CFG) against the CPU oracle: test_generate_synth_cfg_vs_oracle's midpoint case."""
    cfg, sr_in, secs, steps = synth.SYNTH_CFG, 24000, 0.5, 2
    m, sd = model_for(cfg, 0, "midpoint")
    audio = synth.lowres_clip(7, secs, sr_in)
    noise = synth.prior_noise(7, int(round(secs * sr_in)) * (48000 // sr_in) // 480)
    ref, st = ref_cpu.generate(sd, cfg, audio, sr_in, noise, steps, "midpoint", return_stages=True)
    out, got = m.generate_batch([audio], sr_in, 48000, steps, noise=noise, return_stages=True)
    assert int(got["cr"][0].item()) == st["cr"]
    assert (got["wav"].cpu() - st["wav"]).abs().max().item() <= TOL_WAVEFORM
    assert (out.cpu() - ref).abs().max().item() <= TOL_WAVEFORM


def test_baseline_config5_mel_level_vs_oracle_attn_bf16x6():
    """configs[4] at the mel level (N = 3000, midpoint x 4: 8 transformer evaluations), the bar of
    test_baseline_config5_mel_level_vs_oracle."""
    cfg = synth.SYNTH_CFG
    m, sd = model_for(cfg, 0, "midpoint")
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    cond = ref_cpu.preprocess(synth.lowres_clip(510, 30.0, 24000), 24000)
    noise = synth.prior_noise(510, 3000)
    ref = ref_cpu.sample(sd, cfg, cond, noise, 4, "midpoint", decode=False)
    mel = m.sample(cond=cond, time_steps=4, decode_to_audio=False, noise=noise)
    assert tuple(mel.shape) == tuple(ref.shape) == (1, 3000, 256)
    err = (mel.cpu() - ref).abs().max().item()
    print(f"configs[4] mel level, attn_form='bf16x6': max |error| {err:.3e}")
    assert err <= 2e-4


# ---- bitwise invariants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,big", [(50, 32), (50, 33), (1000, 4), (1000, 5), (130, 40), (3000, 2)])
def test_attention_bf16x6_bits_do_not_depend_on_batch(n, big):
    """The two kernel shapes (SPLIT = 1 / 2, picked from the grid size by attention.hip's rule) run the same arithmetic: a clip
    gives the same bits alone and inside a batch on the other side of the threshold; and two runs of one call are equal."""
    assert -(-n // 128) * H * 1 < 512 <= -(-n // 128) * H * big
    qkv = rnd(big * n, 3 * D, seed=155 + n, scale=2.0).to(DEV)
    att = attn(qkv, big, n)
    assert torch.equal(att, attn(qkv, big, n))
    assert torch.isfinite(att).all()
    for b in (0, big - 1):
        q1 = qkv[b * n:(b + 1) * n].contiguous()
        assert torch.equal(attn(q1, 1, n), att[b * n:(b + 1) * n])


def test_ragged_attention_bf16x6_equals_per_clip_calls_bitwise():
    frames = [50, 333, 1, 64, 129, 1000]
    M, max_n = sum(frames), max(frames)
    starts = np.concatenate([[0], np.cumsum(frames)[:-1]])
    seg = torch.tensor(np.stack([starts, frames], 1), dtype=torch.int32).to(DEV)
    qkv = rnd(M, 3 * D, seed=157, scale=2.0).to(DEV)
    att = torch.full((M, D), float("nan"), device=DEV)
    hip.check(hip.lib().fh_attention_bf16x6_seg_f32(qkv.data_ptr(), att.data_ptr(), seg.data_ptr(), len(frames), max_n, H, 10.0,
                                                    hip.stream()), "fh_attention_bf16x6_seg_f32")
    assert torch.isfinite(att).all()
    for s0, n in zip(starts.tolist(), frames):
        assert torch.equal(attn(qkv[s0:s0 + n].clone(), 1, n), att[s0:s0 + n]), f"clip of {n} frames"


@pytest.mark.parametrize("cfgname,method,cfm", [("TINY_CFG", "euler", "basic_cfm"), ("SYNTH_CFG", "midpoint", "basic_cfm")])
def test_generate_many_ragged_equals_generate_per_clip_attn_bf16x6(cfgname, method, cfm):
    cfg = getattr(synth, cfgname)
    m, _ = model_for(cfg, 0, method, cfm)
    secs = [0.5, 1.31, 0.2, 0.5, 2.2, 0.7713, 0.05]
    clips = [synth.lowres_clip(140 + i, s_, 12000) for i, s_ in enumerate(secs)]
    clips[2] = (clips[2] * 20000).astype(np.int16)
    noise = [synth.prior_noise(140 + i, (len(c) * 4) // 480) for i, c in enumerate(clips)]
    many = m.generate_many(clips, 12000, 48000, 2, noise=noise, ragged=True)
    for i, c in enumerate(clips):
        one = m.generate(c, 12000, 48000, 2, noise=noise[i])
        assert tuple(many[i].shape) == tuple(one.shape) == (1, len(c) * 4)
        assert torch.equal(many[i], one), f"clip {i} ({secs[i]} s) differs from generate() alone"
    # the keyword reaches the kernels: the fp32-attention model of the same weights gives other bits
    m32, _ = model_for(cfg, 0, method, cfm, attn_form="f32")
    one32 = m32.generate(clips[4], 12000, 48000, 2, noise=noise[4])
    assert not torch.equal(one32, many[4])


def test_batch_and_guided_ragged_sampling_attn_bf16x6():
    """generate_batch rows = generate alone; sample_many with cond_scale != 1 (the null-condition pass) = sample per clip."""
    m, _ = model_for(synth.TINY_CFG, 0, "midpoint", cfm_method="independent_cfm_mix", sigma=0.3)
    secs = [0.5, 0.21, 1.0, 0.5]
    conds = [torch.from_numpy(ref_cpu.preprocess(synth.lowres_clip(60 + i, s, 12000), 12000).numpy()[0]) for i, s in enumerate(secs)]
    noise = [synth.prior_noise(60 + i, c.shape[0] // 480) for i, c in enumerate(conds)]
    many = m.sample_many(conds, time_steps=2, cond_scale=1.3, mel_pp=True, cfm_method="independent_cfm_mix", noise=noise)
    for c, z, got in zip(conds, noise, many):
        one = m.sample(cond=c[None], time_steps=2, cond_scale=1.3, mel_pp=True, cfm_method="independent_cfm_mix", noise=z)
        assert got.shape == one.shape and torch.equal(got, one)
    m, _ = model_for(synth.TINY_CFG, 0)
    clips = [synth.lowres_clip(240 + i, 0.5, 12000) for i in range(2)]
    z = [synth.prior_noise(240 + i, 50) for i in range(2)]
    both = m.generate_batch(clips, 12000, 48000, 1, noise=torch.cat(z, 0))
    for i in range(2):
        assert torch.equal(both[i:i + 1], m.generate(clips[i], 12000, 48000, 1, noise=z[i]))


def test_graph_capture_replays_bit_identical_attn_bf16x6():
    m, _ = model_for(synth.TINY_CFG, 0, upsampling="hip")
    n_in = 6000
    g = m.capture(2, n_in, 12000, 1)
    for seed in (50, 51):
        x = torch.from_numpy(np.stack([synth.lowres_clip(seed + i, n_in / 12000, 12000) for i in range(2)])).cuda()
        noise = torch.cat([synth.prior_noise(seed + i, 50) for i in range(2)], 0).cuda().reshape(100, -1).contiguous()
        g.x.copy_(x)
        g.noise.copy_(noise)
        got = g.replay().clone()
        ref = m.generate_from_device(x, 12000, 1, noise=noise)
        assert torch.equal(got, ref)


# ---- accuracy, the fp32 kernel as yardstick ------------------------------------------------------------------------------------
def attention_f64(qkv, B, n, scale=AP.SCALE):
    """float64 attention of the tensor the kernels read (on the device, one head at a time: [n, n] scores)."""
    x = qkv.view(B, n, 3, H, 64)
    out = torch.empty(B, n, H, 64, dtype=torch.float64, device=qkv.device)
    for b in range(B):
        for h in range(H):
            q, k, v = (x[b, :, i, h].double() for i in range(3))
            out[b, :, h] = torch.softmax(q @ k.t() * scale, dim=-1) @ v
    return out.view(B * n, D)


@pytest.mark.parametrize("kind,n", [("post-rope", 1000), ("post-rope", 3000), ("random", 1000), ("random", 3000)])
def test_rms_error_to_float64_is_within_a_quarter_of_the_fp32_kernels(kind, n):
    """RMS over all outputs of (kernel - float64 attention of the same tensor): bf16 x 6 <= 1.25 x fp32 MFMA.  The margin: the
    project's bf16 x 6 forms sit within +-15 % of the fp32-MFMA forms' error (profiles/r06_regime_sweep.txt), plus slack."""
    qkv = post_rope_qkv(n, 1)[3] if kind == "post-rope" else rnd(n, 3 * D, seed=155 + n, scale=2.0).to(DEV)
    ref = attention_f64(qkv, 1, n)
    e32 = attn(qkv, 1, n, "f32").double() - ref
    e16 = attn(qkv, 1, n, "bf16x6").double() - ref
    rms32, rms16 = e32.pow(2).mean().sqrt().item(), e16.pow(2).mean().sqrt().item()
    print(f"{kind} n={n}: rms error fp32 {rms32:.3e} bf16x6 {rms16:.3e} ratio {rms16 / rms32:.3f}; "
          f"max error fp32 {e32.abs().max().item():.3e} bf16x6 {e16.abs().max().item():.3e} ratio {e16.abs().max().item() / e32.abs().max().item():.3f}")
    assert rms16 <= RMS_RATIO_MAX * rms32


# ---- every piece pair --------------------------------------------------------------------------------------------------------
PIN_SHAPES = [(1, 200), (40, 130)]            # SPLIT = 2 (small grid) with a masked last tile; SPLIT = 1 (2 x 16 x 40 >= 512)


@pytest.mark.parametrize("B,n", PIN_SHAPES)
def test_pairs_qk_every_pair(B, n):
    """The six (K piece, Q piece) MFMAs: designed q, k whose six-pair logit is an exact fp32 number against the fp32 kernel fed
    that number: torch.equal.  (attn_pins.qk_case)"""
    assert (-(-n // 128) * H * B >= 512) == (B > 1)
    case = AP.qk_case(B, n, seed=20 + n)
    got = attn(case["bf"].to(DEV), B, n, "bf16x6")
    ref = attn(case["f32"].to(DEV), B, n, "f32")
    # (sanity of the construction itself: both are the two-key softmax of the designed logits.  s = L c has |s| <= 34: the
    # rounding of c moves it by 2e-6, its own two roundings by 4e-6 (ulp 2^-18), so exp2 by 4e-6 relative; v_exp_f32 and the
    # normalisation add a few 1e-7.  2e-5 of max |V| = 8)
    exp = AP.qk_expected(case)
    assert (ref.cpu().double() - exp).abs().max().item() <= 1.6e-4
    assert_same(got, ref.cpu(), f"K Q^T pairs B={B} n={n}")


@pytest.mark.parametrize("B,n", [(1, 64), (40, 128), (1, 1024)])
def test_pairs_v_pieces_against_p_h(B, n):
    """(V.h, V.m, V.l) x P.h: q = 0, P = 1, one non-zero V per output column, n a power of two: out = v / n exactly."""
    v = designed_values(B * H * 64, 30 + n)[0].view(B, H, 64)
    qkv, exp = AP.v_case(B, n, 0, v)
    assert_same(attn(qkv.to(DEV), B, n), exp, f"V pieces x P.h B={B} n={n}")


@pytest.mark.parametrize("B,n", PIN_SHAPES)
def test_pairs_p_pieces_against_v_h(B, n):
    """V.h x (P.h, P.m, P.l): exact logits in both kernels, V a power of two on one key per column: torch.equal."""
    qkv, logits, key_of, vpow = AP.p_case(B, n, seed=40 + n)
    qd = qkv.to(DEV)
    got, ref = attn(qd, B, n, "bf16x6"), attn(qd, B, n, "f32")
    exp = AP.p_expected(logits, key_of, vpow)
    assert (ref.cpu().double() - exp).abs().max().item() <= 1.6e-4        # (sanity, as in test_pairs_qk_every_pair)
    assert float((ref != 0).float().mean()) > 0.99
    assert_same(got, ref.cpu(), f"V.h x P pieces B={B} n={n}")


@pytest.mark.parametrize("B,n", PIN_SHAPES)
def test_pairs_v_m_p_m(B, n):
    """(V.m, P.m): column 0 carries p V with V = 2^e (1 + 2^-8 - 2^-16), column 1 the exact p 2^e of the same row:
    |col0 - (1 + 2^-8 - 2^-16) col1| <= VM_PM_ULPS ulps of col0 (attn_pins.VM_PM_ULPS says why)."""
    qkv, exps = AP.vm_pm_case(B, n, seed=50 + n)
    out = attn(qkv.to(DEV), B, n).cpu().double().view(B * n, H, 64)
    c1 = out[:, :, 1:2]
    cols = torch.cat([out[:, :, 0:1], out[:, :, 2:]], -1)
    assert bool((c1 > 0).all()) and torch.isfinite(out).all()
    miss = (cols - AP.VM_FACTOR * c1).abs() / AP.ulp(cols)
    print(f"(V.m, P.m) B={B} n={n}: largest miss {miss.max().item():.2f} ulps")
    assert miss.max().item() <= AP.VM_PM_ULPS
    # column 1 / 2^e = p / (1 + p) with p the second key's weight relative to the row maximum: general, neither 0 nor 1
    share = c1[..., 0] / torch.pow(2.0, exps).repeat_interleave(n, 0)
    assert 0.02 < float(share.min()) and float(share.max()) < 0.5
