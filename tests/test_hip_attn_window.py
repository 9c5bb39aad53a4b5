"""GPU: banded attention (attn_window=; fh_attention_band_f32 / _band_seg_f32 and their bf16x6 forms; attention_softmax.h: AttnBand).
Query i of a clip of n rows reads the keys j with 0 <= j < n and |i - j| <= R.
  * which keys a row reads, pinned exactly at every edge of the tile range and of the mask (an all-zero Q K, V[j] = j + 1);
  * the three bit properties: a band that spans the clip = the full kernel; a clip alone = the clip in a batch on the other side of
    the SPLIT threshold; the segment form = the batched form per clip;
  * the numbers against the oracle's attention with the band restated as a mask (attention_banded below), at the project's bars:
    the attention block, the flow forward, the whole path; generate_many / capture / the device prior through a windowed model."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import FLowHigh, FlowHighSR, hip, synth, tables      # noqa: E402
from oracle import ref_cpu                                   # noqa: E402

DEV = "cuda"
H, D = 16, 1024
TOL_WAVEFORM = 1e-4
INT_MAX = 2 ** 31 - 1
FORMS = ["f32", "bf16x6"]
_MODELS, _REFS = {}, {}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def maxdiff(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def _name(form, band, seg=False):
    return "fh_attention_" + ("bf16x6_" if form == "bf16x6" else "") + ("band_" if band else "") + ("seg_" if seg else "") + "f32"


def full(qkv, B, n, form, scale=10.0):
    out = torch.full((B * n, D), float("nan"), device=DEV)
    hip.check(getattr(hip.lib(), _name(form, False))(qkv.data_ptr(), out.data_ptr(), B, n, H, scale, hip.stream()), _name(form, False))
    return out


def band(qkv, B, n, R, form, scale=10.0):
    out = torch.full((B * n, D), float("nan"), device=DEV)
    hip.check(getattr(hip.lib(), _name(form, True))(qkv.data_ptr(), out.data_ptr(), B, n, H, R, scale, hip.stream()), _name(form, True))
    return out


def attention_banded(W):
    """The oracle's attention (oracle/ref_cpu.py: attention) with the band as a mask on the scores before the softmax."""
    def attention(sd, prefix, x, rot, heads=16):
        b, n, _ = x.shape
        qkv = F.linear(x, sd[prefix + "to_qkv.weight"])
        q, k, v = qkv.chunk(3, dim=-1)
        q, k, v = (t.reshape(b, n, heads, -1).permute(0, 2, 1, 3) for t in (q, k, v))
        dh = q.shape[-1]
        q = ref_cpu._rmsnorm_dir(q) * sd[prefix + "q_norm.gamma"] * (dh ** 0.5)
        k = ref_cpu._rmsnorm_dir(k) * sd[prefix + "k_norm.gamma"] * (dh ** 0.5)
        q = q * rot.cos() + ref_cpu._rotate_half(q) * rot.sin()
        k = k * rot.cos() + ref_cpu._rotate_half(k) * rot.sin()
        sim = torch.einsum("bhid,bhjd->bhij", q, k) * 10.0
        i = torch.arange(n)
        sim = sim.masked_fill((i[:, None] - i[None, :]).abs() > W, -torch.finfo(sim.dtype).max)
        attn = sim.softmax(dim=-1)
        out = torch.einsum("bhij,bhjd->bhid", attn, v)
        out = out.permute(0, 2, 1, 3).reshape(b, n, heads * dh)
        return F.linear(out, sd[prefix + "to_out.weight"])
    return attention


def test_the_restatement_without_a_band_is_the_oracles_attention():
    sd = synth.make_flow_state_dict(seed=3)
    p = "flowhigh.transformer.layers.0.3."
    x = rnd(2, 40, D, seed=150)
    rot = ref_cpu.rotary_table(sd, 40)
    assert torch.equal(attention_banded(39)(sd, p, x, rot), ref_cpu.attention(sd, p, x, rot))
    assert not torch.equal(attention_banded(3)(sd, p, x, rot), ref_cpu.attention(sd, p, x, rot))


# ---- 1. which keys a row reads -------------------------------------------------------------------------------------------------
def radii(n):
    return sorted({r for r in (0, 1, 5, 31, 32, 33, 63, 64, 100, n - 2, n - 1, n, INT_MAX) if r >= 0})


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 31, 33, 64, 65, 130, 257])
def test_band_membership_is_exact(n, B, form):
    """Q = K = 0: every score is 0, every valid key weighs 1 / |band(i)|.  V[b, j] = j + 1 + 1000 b in every column: the row is
    fl(fl(sum over the band) * fl(1 / |band|)), sums of integers below 2^24 (exact in fp32 and in three bf16 pieces).  A key too
    many or too few at either edge moves a row by about 0.5.  R = 0 and 1 at n >= 65 walk tiles that are masked whole for most
    lanes, a lane's first tile too: no NaN."""
    qkv = torch.zeros(B, n, 3, D)
    j = torch.arange(n, dtype=torch.float32)
    for b in range(B):
        qkv[b, :, 2] = (j + 1 + 1000 * b)[:, None]
    qkv = qkv.view(B * n, 3 * D).to(DEV)
    i = np.arange(n, dtype=np.int64)
    for R in radii(n):
        got = band(qkv, B, n, R, form).cpu().numpy().reshape(B, n, D)
        assert not np.isnan(got).any(), f"R={R}"
        lo, hi = np.maximum(0, i - R), np.minimum(n - 1, i + R)
        cnt = hi - lo + 1
        for b in range(B):
            total = cnt * (lo + hi + 2) // 2 + 1000 * b * cnt
            assert total.max() < 2 ** 24
            want = total.astype(np.float32) * (np.float32(1) / cnt.astype(np.float32))
            assert want.dtype == np.float32
            np.testing.assert_allclose(got[b], np.broadcast_to(want[:, None], (n, D)), rtol=1e-6, atol=0, err_msg=f"R={R} b={b}")


# ---- 2. - 4. bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,n", [(2, 50), (1, 333), (16, 200)])
def test_a_band_that_spans_the_clip_gives_the_full_kernels_bits(B, n, form):
    qkv = rnd(B * n, 3 * D, seed=155 + n, scale=2.0).to(DEV)
    want = full(qkv, B, n, form)
    assert torch.isfinite(want).all()
    for R in (n - 1, n, INT_MAX):
        assert torch.equal(band(qkv, B, n, R, form), want), f"R={R}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,big", [(50, 32), (130, 16), (200, 16)])
def test_band_bits_do_not_depend_on_batch(n, big, form):
    """A clip alone runs the SPLIT = 2 shape (64 queries per block), in the batch the SPLIT = 1 shape (128 per block, a wider tile
    range): the tiles one shape walks and the other does not are masked whole for the row."""
    assert -(-n // 128) * H * 1 < 512 <= -(-n // 128) * H * big
    qkv = rnd(big * n, 3 * D, seed=155 + n, scale=2.0).to(DEV)
    for R in (0, 7, 40, 100):
        att = band(qkv, big, n, R, form)
        assert torch.isfinite(att).all()
        for b in (0, big - 1):
            q1 = qkv[b * n:(b + 1) * n].contiguous()
            assert torch.equal(band(q1, 1, n, R, form), att[b * n:(b + 1) * n]), f"R={R} row {b}"


@pytest.mark.parametrize("form", FORMS)
def test_banded_seg_entry_equals_the_batched_entry_per_clip(form):
    frames = [50, 333, 1, 64, 129]
    M, max_n = sum(frames), max(frames)
    starts = np.concatenate([[0], np.cumsum(frames)[:-1]])
    seg = torch.tensor(np.stack([starts, frames], 1), dtype=torch.int32).to(DEV)
    qkv = rnd(M, 3 * D, seed=157, scale=2.0).to(DEV)
    name = _name(form, True, seg=True)
    for R in (0, 33, 200):
        att = torch.full((M, D), float("nan"), device=DEV)
        hip.check(getattr(hip.lib(), name)(qkv.data_ptr(), att.data_ptr(), seg.data_ptr(), len(frames), max_n, H, R, 10.0, hip.stream()), name)
        assert torch.isfinite(att).all()
        for s0, n in zip(starts.tolist(), frames):
            assert torch.equal(band(qkv[s0:s0 + n].clone(), 1, n, R, form), att[s0:s0 + n]), f"R={R}, clip of {n} frames"


# ---- 5. numbers: the attention block -------------------------------------------------------------------------------------------
def post_rope_qkv(n, B):
    """The qkv tensor of tests/test_hip_ops.py::test_attention_block after fh_qknorm_rope_f32, and what is needed to finish the block."""
    key = ("qkv", n, B)
    if key not in _REFS:
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
        _REFS[key] = (sd, p, x, qkv)
    return _REFS[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("R", [3, 40])
@pytest.mark.parametrize("n", [33, 200])
def test_attention_block_banded(n, R, form):
    """test_attention_block with the banded entry against the banded restatement, same inputs, same scale, same bar."""
    B = 2
    sd, p, x, qkv = post_rope_qkv(n, B)
    if ("block", n, R) not in _REFS:
        _REFS[("block", n, R)] = attention_banded(R)(sd, p, x, ref_cpu.rotary_table(sd, n))
    ref = _REFS[("block", n, R)]
    att = band(qkv, B, n, R, form)
    out = torch.empty(B * n, D, device=DEV)
    hip.gemm(att, sd[p + "to_out.weight"].to(DEV), out, B * n, D, D)
    err = maxdiff(out.view(B, n, D), ref)
    print(f"banded attention block n={n} R={R} {form}: max |error| {err:.3e}")
    assert err <= 1e-4


# ---- 6. the flow forward ---------------------------------------------------------------------------------------------------------
FLOW_CASE = (2, 200, 0.3)


def flow_inputs():
    B, n, t = FLOW_CASE
    return rnd(B, n, 256, seed=160), rnd(B, n, 256, seed=161, scale=3.0) - 4.0


def flow_out(sd, bf, form, W):
    from flowhigh_amd.flow import FlowNet
    B, n, t = FLOW_CASE
    x, cond = flow_inputs()
    net = FlowNet(sd, DEV, bf=bf, attn_form=form, attn_window=W)
    assert net.attn_window == W
    xd, cd = x.view(B * n, 256).to(DEV), cond.view(B * n, 256).to(DEV)
    net.set_cond(cd, B, n)
    out = torch.empty(B * n, 256, device=DEV)
    net.forward(xd, t, out, B, n)
    return out.view(B, n, 256)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf", [False, True], ids=["lin_f32", "lin_bf16x6"])
@pytest.mark.parametrize("W", [10, 64])
def test_flow_forward_with_a_window(W, bf, form, monkeypatch):
    """test_flow_forward's (2, 200, 0.3) case through a windowed net against the oracle with the restatement patched in, same bar."""
    B, n, t = FLOW_CASE
    sd = synth.make_flow_state_dict(seed=0)
    if ("flow", W) not in _REFS:
        monkeypatch.setattr(ref_cpu, "attention", attention_banded(W))
        x, cond = flow_inputs()
        _REFS[("flow", W)] = ref_cpu.flow_forward(sd, x, cond, t)
        monkeypatch.undo()
        assert maxdiff(_REFS[("flow", W)], ref_cpu.flow_forward(sd, x, cond, t)) > 5e-4       # (the band matters at this shape: ten times the bar)
    err = maxdiff(flow_out(sd, bf, form, W), _REFS[("flow", W)])
    print(f"flow forward W={W} linears {'bf16x6' if bf else 'f32'} attention {form}: max |error| {err:.3e}")
    assert err <= 5e-5


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf", [False, True], ids=["lin_f32", "lin_bf16x6"])
def test_flow_forward_with_a_window_wider_than_the_clip_is_the_net_without_one(bf, form):
    sd = synth.make_flow_state_dict(seed=0)
    assert torch.equal(flow_out(sd, bf, form, 1000), flow_out(sd, bf, form, None))


# ---- 7. the whole path, TINY_CFG ---------------------------------------------------------------------------------------------------
def model_for(form, window, **kw):
    key = (form, window)
    if key not in _MODELS:
        if "sd" not in _MODELS:
            _MODELS["sd"] = synth.make_state_dict(synth.TINY_CFG, 0)
        _MODELS[key] = FLowHigh(_MODELS["sd"], synth.TINY_CFG, "cuda", attn_form=form, attn_window=window)
    fh = _MODELS[key]
    assert fh.attn_window == window and fh.net.attn_window == window and fh.attn_form == form
    return FlowHighSR(fh, **{**dict(torchdiffeq_ode_method="euler"), **kw}), _MODELS["sd"]


@pytest.mark.parametrize("form", FORMS)
def test_generate_with_a_window_wider_than_the_clip_is_generate_without_one(form):
    clip, noise = synth.lowres_clip(7, 0.25, 12000), synth.prior_noise(7, 25)
    wide, _ = model_for(form, 25)               # (N = 25 frames: the window spans the clip)
    none, _ = model_for(form, None)
    assert torch.equal(wide.generate(clip, 12000, 48000, 1, noise=noise), none.generate(clip, 12000, 48000, 1, noise=noise))


@pytest.mark.parametrize("form", FORMS)
def test_generate_with_a_window_vs_oracle(form, monkeypatch):
    cfg, sr_in, secs, W = synth.TINY_CFG, 12000, 0.5, 8
    m, sd = model_for(form, W)
    audio, noise = synth.lowres_clip(7, secs, sr_in), synth.prior_noise(7, 50)
    if "gen" not in _REFS:
        monkeypatch.setattr(ref_cpu, "attention", attention_banded(W))
        _REFS["gen"] = ref_cpu.generate(sd, cfg, audio, sr_in, noise, 1, "euler", return_stages=True)
        monkeypatch.undo()
    ref, st = _REFS["gen"]
    out, got = m.generate_batch([audio], sr_in, 48000, 1, noise=noise, return_stages=True)
    assert int(got["cr"][0].item()) == st["cr"]
    assert (got["wav"].cpu() - st["wav"]).abs().max().item() <= TOL_WAVEFORM
    assert (out.cpu() - ref).abs().max().item() <= TOL_WAVEFORM
    # the keyword reaches the kernels: the same weights without a window give another waveform
    none, _ = model_for(form, None)
    assert not torch.equal(none.generate(audio, sr_in, 48000, 1, noise=noise), out)


@pytest.mark.parametrize("ends", ["per_clip", "ragged"])
@pytest.mark.parametrize("form", FORMS)
def test_generate_many_ragged_with_a_window_equals_generate_per_clip(form, ends):
    m, _ = model_for(form, 8)
    secs = [0.5, 1.31, 0.2]
    clips = [synth.lowres_clip(140 + i, s_, 12000) for i, s_ in enumerate(secs)]
    noise = [synth.prior_noise(140 + i, (len(c) * 4) // 480) for i, c in enumerate(clips)]
    many = m.generate_many(clips, 12000, 48000, 1, noise=noise, ragged=True, ends=ends)
    for i, c in enumerate(clips):
        one = m.generate(c, 12000, 48000, 1, noise=noise[i])
        assert tuple(many[i].shape) == tuple(one.shape) == (1, len(c) * 4)
        assert torch.equal(many[i], one), f"clip {i} ({secs[i]} s) differs from generate() alone"


def test_generate_many_with_a_window_and_the_device_prior():
    m, _ = model_for("f32", 8, prior="device", upsampling_method="hip")
    clips = [synth.lowres_clip(150 + i, s_, 12000) for i, s_ in enumerate([0.5, 0.9, 0.23])]
    many = m.generate_many(clips, 12000, 48000, 1, seed=31, ragged=True, ends="ragged")
    for i, c in enumerate(clips):
        assert torch.equal(many[i], m.generate(c, 12000, 48000, 1, seed=[(31, i)])), f"clip {i}"


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_replays_bit_identical_with_a_window(form):
    m, _ = model_for(form, 8, upsampling_method="hip")
    n_in = 6000
    g = m.capture(2, n_in, 12000, 1)
    x = torch.from_numpy(np.stack([synth.lowres_clip(50 + i, n_in / 12000, 12000) for i in range(2)])).cuda()
    noise = torch.cat([synth.prior_noise(50 + i, 50) for i in range(2)], 0).cuda().reshape(100, -1).contiguous()
    g.x.copy_(x)
    g.noise.copy_(noise)
    got = g.replay().clone()
    ref = m.generate_from_device(x, 12000, 1, noise=noise)
    assert torch.equal(got, ref)
    none, _ = model_for(form, None, upsampling_method="hip")
    assert not torch.equal(none.generate_from_device(x, 12000, 1, noise=noise), ref)
