"""GPU: fh_conv_grouped_bf16x6_f32 (conv_mfma_bf.hip), the grouped implicit-GEMM conv in the bf16 x 6 form, on the helper shapes of
test_hip_ops.py: run_conv with the new packer and entry.

"fp32-grade" is asserted, not assumed: every random-input case is compared with a float64 reference and, on the same inputs, so
is the fp32 kernel (fh_conv_grouped_f32, 16-channel chunks).  The new kernel has to stay inside the fp32 test's bar for the shape
AND inside twice the fp32 kernel's own error + 1e-7: the two forms are equal on average (bf16x6.h: 4.17e-7 against 4.19e-7 of
sum |a b|), the factor 2 covers the maxima of two different summation orders over ~1e5 outputs.  A lost piece pair lands right on
that bound; the exact-pair test at the end pins all six pairs and the device split with equality."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from flowhigh_amd import hip                                                                     # noqa: E402
from flowhigh_amd import vocoder as V                                                            # noqa: E402
from test_hip_bf16x6_pairs import assert_same, designed_values, slot_planes, slot_sum, weight_values   # noqa: E402

DEV = "cuda"
TILES = list(range(7))
PLAIN = [(16, 24, 7, 3, 300), (48, 40, 11, 5, 1111), (32, 200, 3, 1, 33)]          # (cin, cout, k, d, L), B = 2


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def err(got, ref64):
    return (got.detach().cpu().double() - ref64).abs().max().item()


def cpad_of(cout, tile_cfg):
    bm = hip.lib().fh_conv_tile_m(tile_cfg)
    return -(-cout // bm) * bm


def pack(w, cpad, bf):
    return (V.pack_conv_bf_weight(w, cpad) if bf else V.pack_conv_weight(w, cpad, 16)).to(DEV)


def run_conv(x, w, bias, dilation, tile_cfg, bf, res=None, scale=1.0):
    """test_hip_ops.run_conv; bf: three-piece weights and the bf16 x 6 entry, else the fp32 kernel with 16-channel chunks."""
    B, cin, L = x.shape
    cout, _, k = w.shape
    cpad = cpad_of(cout, tile_cfg)
    xd, out = x.to(DEV), torch.full((B, cout, L), float("nan"), device=DEV)
    wp = pack(w, cpad, bf)
    bd = bias.to(DEV) if bias is not None else None
    rd = [r.to(DEV) for r in (res or [])]
    offs = [(t - (k - 1) // 2) * dilation for t in range(k)]
    g = V.make_conv_group([V.make_conv_seg(xd, wp, cin, offs)], bd, rd, out, cout, cpad, L, L, L, scale=scale)
    keep = V.conv_grouped([g], B, cpad, L, tile_cfg, DEV, 16, bf=bf)
    torch.cuda.synchronize()
    del keep
    return out.cpu()


def assert_fp32_grade(got_bf, got_32, ref64, bar, what):
    e_bf, e32 = err(got_bf, ref64), err(got_32, ref64)
    print(f"{what}: bf16 x 6 {e_bf:.3e}, fp32 MFMA {e32:.3e} against float64 (bar {bar:.0e})")
    assert e_bf <= bar, what
    assert e_bf <= 2.0 * e32 + 1e-7, what


# ---- plain convs: every tile shape -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_case(case):
    cin, cout, k, d, L = case
    x, w, b = rnd(2, cin, L, seed=1), rnd(cout, cin, k, seed=2, scale=0.2), rnd(cout, seed=3)
    ref = F.conv1d(x.double(), w.double(), b.double(), dilation=d, padding=(k * d - d) // 2)
    return x, w, b, ref


@functools.lru_cache(maxsize=None)
def plain_out(case, tile_cfg):
    x, w, b, _ = plain_case(case)
    return run_conv(x, w, b, case[3], tile_cfg, bf=True)


@pytest.mark.parametrize("tile_cfg", TILES)
@pytest.mark.parametrize("case", PLAIN)
def test_conv_plain_is_fp32_grade(case, tile_cfg):
    x, w, b, ref = plain_case(case)
    got32 = run_conv(x, w, b, case[3], tile_cfg, bf=False)
    assert_fp32_grade(plain_out(case, tile_cfg), got32, ref, 5e-5, f"{case} tile {tile_cfg}")      # the fp32 test's bar on these shapes


@pytest.mark.parametrize("case", PLAIN)
def test_bits_do_not_depend_on_the_tile(case):
    outs = [plain_out(case, t) for t in TILES]
    assert not bool(torch.isnan(outs[0]).any())
    for t in TILES[1:]:
        assert torch.equal(outs[t], outs[0]), f"{case}: tile {t} against tile 0"


# ---- residuals, scale, K segments ------------------------------------------------------------------------------------------
def test_conv_large_k_residual_scale():
    cin = cout = 256
    x, w, b = rnd(1, cin, 700, seed=4), rnd(cout, cin, 11, seed=5, scale=0.02), rnd(cout, seed=6)
    r1, r2 = rnd(1, cout, 700, seed=7), rnd(1, cout, 700, seed=8)
    ref = (F.conv1d(x.double(), w.double(), b.double(), dilation=5, padding=25) + r1.double() + r2.double()) * 0.5
    got = run_conv(x, w, b, 5, 0, bf=True, res=[r1, r2], scale=0.5)
    got32 = run_conv(x, w, b, 5, 0, bf=False, res=[r1, r2], scale=0.5)
    assert_fp32_grade(got, got32, ref, 2e-5, "256 channels, k 11, d 5, two residuals, scale 0.5")


def test_conv_three_segments_fused_average_and_batch_invariance():
    """Last conv2 of a stage: one accumulator over the three AMP blocks + residuals, / 3; a clip of the batch alone: same bits."""
    c, L, B = 48, 400, 2
    ks = [11, 7, 3]
    xs = [rnd(B, c, L, seed=20 + i) for i in range(3)]
    ws = [rnd(c, c, k, seed=30 + i, scale=0.1) for i, k in enumerate(ks)]
    bs = [rnd(c, seed=40 + i) for i in range(3)]
    rs = [rnd(B, c, L, seed=50 + i) for i in range(3)]
    ref = sum(F.conv1d(x.double(), w.double(), b.double(), padding=(k - 1) // 2) + r.double() for x, w, b, r, k in zip(xs, ws, bs, rs, ks)) / 3
    tile_cfg, _, cpad = V.pick_tile_cfg(c)
    bsum = sum(bs).to(DEV)

    def run(bf, items):
        n = len(items)
        out = torch.full((n, c, L), float("nan"), device=DEV)
        xd, rd = [x[items].contiguous().to(DEV) for x in xs], [r[items].contiguous().to(DEV) for r in rs]
        wp = [pack(w, cpad, bf) for w in ws]
        segs = [V.make_conv_seg(xd[i], wp[i], c, [t - (k - 1) // 2 for t in range(k)]) for i, k in enumerate(ks)]
        g = V.make_conv_group(segs, bsum, rd, out, c, cpad, L, L, L, scale=1.0 / 3)
        keep = V.conv_grouped([g], n, cpad, L, tile_cfg, DEV, 16, bf=bf)
        torch.cuda.synchronize()
        del keep
        return out.cpu()
    got = run(True, [0, 1])
    assert_fp32_grade(got, run(False, [0, 1]), ref, 1e-5, "three K segments, three residuals, scale 1/3")
    assert torch.equal(run(True, [1]), got[1:2])


# ---- transposed conv as phase groups: out_stride, out_phase, k - u odd ---------------------------------------------------------
@pytest.mark.parametrize("u,k", [(5, 11), (4, 8), (2, 3), (3, 3), (6, 13)])
def test_conv_transpose_as_phase_groups(u, k):
    cin, cout, L, B = 32, 16, 157, 2
    x, wt, b = rnd(B, cin, L, seed=11), rnd(cin, cout, k, seed=12, scale=0.2), rnd(cout, seed=13)
    ref = F.conv_transpose1d(x.double(), wt.double(), b.double(), stride=u, padding=(k - u) // 2)
    extra = V.transposed_conv_extra(k, u)
    lout = u * L + extra
    assert ref.shape[-1] == lout
    tile_cfg, _, cpad = V.pick_tile_cfg(cout)
    xd, bd = x.to(DEV), b.to(DEV)

    def run(bf):
        out = torch.full((B, cout, lout), float("nan"), device=DEV)
        groups, keep = [], []
        for r, taps in enumerate(V.transposed_conv_phases(k, u)):
            wp = pack(torch.stack([wt[:, :, j] for j, _ in taps], dim=-1).permute(1, 0, 2), cpad, bf)
            keep.append(wp)
            groups.append(V.make_conv_group([V.make_conv_seg(xd, wp, cin, [o for _, o in taps])], bd, [], out,
                                            cout, cpad, L, lout, L + (extra if r == 0 else 0), stride=u, phase=r))
        keep.append(V.conv_grouped(groups, B, cpad, L + extra, tile_cfg, DEV, 16, bf=bf))
        torch.cuda.synchronize()
        return out.cpu()
    assert_fp32_grade(run(True), run(False), ref, 1e-5, f"ConvTranspose1d(k {k}, u {u})")


# ---- ragged: groups of different length in one launch --------------------------------------------------------------------------
@pytest.mark.parametrize("tile_cfg", [0, 4])
def test_ragged_groups_equal_their_own_launches(tile_cfg):
    cin, cout, k, d = 32, 40, 7, 3
    lens = [300, 33, 1111]
    cpad = cpad_of(cout, tile_cfg)
    w, b = rnd(cout, cin, k, seed=60, scale=0.2), rnd(cout, seed=61)
    wp, bd = pack(w, cpad, True), b.to(DEV)
    offs = [(t - (k - 1) // 2) * d for t in range(k)]
    xs = [rnd(1, cin, L, seed=62 + i).to(DEV) for i, L in enumerate(lens)]
    group = lambda x, out: V.make_conv_group([V.make_conv_seg(x, wp, cin, offs)], bd, [], out, cout, cpad, x.shape[-1], x.shape[-1], x.shape[-1])
    together = [torch.full((1, cout, L), float("nan"), device=DEV) for L in lens]
    keep = V.conv_grouped([group(x, o) for x, o in zip(xs, together)], 1, cpad, max(lens), tile_cfg, DEV, 16, bf=True)
    torch.cuda.synchronize()
    for x, o in zip(xs, together):
        alone = torch.full_like(o, float("nan"))
        keep = V.conv_grouped([group(x, alone)], 1, cpad, x.shape[-1], tile_cfg, DEV, 16, bf=True)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(alone).any()) and torch.equal(o, alone)
    del keep


# ---- argument errors: a negative code and a message, nothing launched ----------------------------------------------------------
def test_argument_errors():
    L = hip.lib()
    cin, cout, n = 32, 24, 100
    cpad = cpad_of(cout, 0)
    x, out = rnd(1, cin, n, seed=70).to(DEV), torch.full((1, cout, n), float("nan"), device=DEV)
    wp = pack(rnd(cout, cin, 3, seed=71), cpad, True)
    good = V.make_conv_group([V.make_conv_seg(x, wp, cin, [-1, 0, 1])], None, [], out, cout, cpad, n, n, n)
    d = hip.to_device_struct_array([good], DEV)
    msg = lambda: L.fh_last_error().decode()
    assert L.fh_conv_grouped_bf16x6_f32(d.data_ptr(), 1, 1, cpad, n, 7, hip.stream()) < 0 and "tile_cfg 7" in msg()
    assert L.fh_conv_grouped_bf16x6_f32(None, 1, 1, cpad, n, 0, hip.stream()) < 0 and "fh_conv_grouped_bf16x6_f32" in msg()
    assert L.fh_conv_grouped_bf16x6_f32(d.data_ptr(), 1, 1, cpad + 1, n, 0, hip.stream()) < 0 and "cout_pad" in msg()
    assert L.fh_conv_grouped_bf16x6_f32(d.data_ptr(), 1, 0, cpad, n, 0, hip.stream()) < 0 and "bad sizes" in msg()
    # cin = 24: the launcher sees a descriptor array that lives in pinned host memory (the kernel reads it there just as well)
    bad = V.make_conv_group([V.make_conv_seg(x, wp, 24, [-1, 0, 1])], None, [], out, cout, cpad, n, n, n)
    pinned = lambda g: torch.frombuffer(bytearray(bytes(g)), dtype=torch.uint8).pin_memory()
    hb = pinned(bad)
    assert L.fh_conv_grouped_bf16x6_f32(hb.data_ptr(), 1, 1, cpad, n, 0, hip.stream()) < 0
    assert "24 input channels" in msg() and "multiple of 16" in msg()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                     # nothing ran
    # ... and the same array with cin = 32 runs, with the bits of the device-resident descriptors
    hg = pinned(good)
    hip.check(L.fh_conv_grouped_bf16x6_f32(hg.data_ptr(), 1, 1, cpad, n, 0, hip.stream()), "pinned descriptors")
    torch.cuda.synchronize()
    first = out.clone()
    out.fill_(float("nan"))
    hip.check(L.fh_conv_grouped_bf16x6_f32(d.data_ptr(), 1, 1, cpad, n, 0, hip.stream()), "device descriptors")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and torch.equal(out, first)


# ---- the six piece pairs and the device split, by equality (tests/test_hip_bf16x6_pairs.py's construction) ---------------------
@pytest.mark.parametrize("tile_cfg", [0, 4])
def test_direct_bf16x6_every_pair(tile_cfg):
    """One nonzero bf16-exact weight per output channel co (input channel (7 co + 3) % 32: both 16-channel chunks, both octets =
    both lane halves of the K dimension; tap co % 3; output rows over both halves of the MFMA tile), placed in ONE piece slot:
    out[co, t] = x[ci, t + (tap - 1) d] (the slot's pieces) v_co exactly.  Slot h keeps the pairs h h, m h, l h; m: h m, m m; l: h l."""
    C, k, d, L, B = 32, 3, 2, 200, 2
    x, pieces = designed_values(B * C * L, 90 + tile_cfg)
    x, pieces = x.view(B, C, L), [p.view(B, C, L) for p in pieces]
    co = torch.arange(C)
    ci, tap = (7 * co + 3) % C, co % k
    assert sorted(ci.tolist()) == list(range(C))
    v = weight_values(C, 91)
    w = torch.zeros(C, C, k)
    w[co, ci, tap] = v
    cpad = cpad_of(C, tile_cfg)
    xd = x.to(DEV)
    offs = [(t - 1) * d for t in range(k)]
    for slot in (0, 1, 2):
        wd = slot_planes(V.pack_conv_weight(w, cpad, 16), slot).to(DEV)
        assert wd.shape == V.pack_conv_bf_weight(w, cpad).shape
        out = torch.full((B, C, L), float("nan"), device=DEV)
        g = V.make_conv_group([V.make_conv_seg(xd, wd, C, offs)], None, [], out, C, cpad, L, L, L)
        keep = V.conv_grouped([g], B, cpad, L, tile_cfg, DEV, 16, bf=True)
        torch.cuda.synchronize()
        del keep
        src = F.pad(slot_sum(pieces, slot), (d, d))                                         # [B, C, L + 2 d]
        exp = torch.stack([src[:, ci[o], tap[o] * d:tap[o] * d + L] for o in range(C)], dim=1) * v.double()[None, :, None]
        assert_same(out, exp.float(), f"direct bf16 x 6, tile {tile_cfg}, weight slot {'hml'[slot]}")
