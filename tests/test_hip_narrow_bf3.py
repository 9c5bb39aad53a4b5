"""GPU: fh_narrow_conv_bf16x3_f32 (narrow_bf.hip with two pieces per operand), the narrow stages' direct conv in the bf16 x 3 form:
every slab split (24 and 48 channels: even slabs; 32 and 40: uneven), the model's kernel sizes and dilations, rows that end inside
the first tile, just behind it and on a 16-byte boundary (the vector loader).  The rules are test_hip_direct_bf3.py's: fp32-grade
against the form's own definition (tests/ref_bf16x3.conv_bf16x3_ref), |y - float64| <= 2^-16 S + 2 e32 pointwise, with e32 from the
fp32 direct kernel (fh_conv_grouped_f32) on the same inputs; then every kept pair and the device split with equality."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from flowhigh_amd import hip, packing                                                             # noqa: E402
from flowhigh_amd import vocoder as V                                                            # noqa: E402
from ref_bf16x3 import BOUND, abs_sum, conv_bf16x3_ref                                           # noqa: E402
from test_hip_bf16x6_pairs import assert_same, designed_values, slot_split, slot_sum, weight_values    # noqa: E402
from test_hip_direct_bf import err, rnd                                                          # noqa: E402

DEV = "cuda"
ENTRY = "fh_narrow_conv_bf16x3_f32"


def run_narrow(x, w, bias, d, res=(), scale=1.0, pack=None):
    B, C, L = x.shape
    k = w.shape[-1]
    xd, out = x.to(DEV), torch.full((B, C, L), float("nan"), device=DEV)
    ud = (pack or packing.pack_narrow_bf3_weight)(w, C).to(DEV)
    bd, rd = bias.to(DEV) if bias is not None else None, [r.to(DEV) for r in res]       # (descriptors hold raw pointers: keep these alive)
    g = V.make_amp_group([V.make_amp_seg(xd, ud, k, direct=True)], bd, rd, out, L, scale=scale, direct=True)
    keep = V.amp_actconv([g], B, C, d, DEV, direct=True, bf3=True)
    torch.cuda.synchronize()
    del keep
    return out.cpu()


def run_fp32_direct(x, w, bias, d, res=(), scale=1.0):
    """The fp32 direct kernel on the same conv (the source of e32)."""
    B, C, L = x.shape
    k = w.shape[-1]
    ck = V.pick_ck(C)
    tile_cfg, _, cpad = V.pick_tile_cfg(C)
    xd, out = x.to(DEV), torch.full((B, C, L), float("nan"), device=DEV)
    wp = V.pack_conv_weight(w, cpad, ck).to(DEV)
    offs = [(t - (k - 1) // 2) * d for t in range(k)]
    bd, rd = bias.to(DEV), [r.to(DEV) for r in res]                                      # (kept alive until the launch has run)
    g = V.make_conv_group([V.make_conv_seg(xd, wp, C, offs)], bd, rd, out, C, cpad, L, L, L, scale=scale)
    keep = V.conv_grouped([g], B, cpad, L, tile_cfg, DEV, ck)
    torch.cuda.synchronize()
    del keep
    return out.cpu()


@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("C", [24, 48, 32, 40])
def test_narrow_conv_against_its_definition_and_float64(C, k, d):
    tile = hip.lib().fh_narrow_tile_len()
    assert tile == 256
    # one tile minus 1, one tile plus 17 (both unaligned rows), and two tiles (rows 16-byte aligned: the vector loader and stores)
    for L in (tile - 1, tile + 17, 2 * tile):
        B = 2
        x, w, b = rnd(B, C, L, seed=C + k), rnd(C, C, k, seed=C + k + 1, scale=0.2), rnd(C, seed=C + k + 2)
        r = rnd(B, C, L, seed=C + k + 3)
        kw = dict(dilation=d, padding=(k * d - d) // 2)
        ref64 = (F.conv1d(x.double(), w.double(), b.double(), **kw) + r.double()) * 0.5
        ref3 = (conv_bf16x3_ref(x, w, b, **kw) + r.double()) * 0.5
        S = 0.5 * abs_sum(x, w, **kw)
        got = run_narrow(x, w, b, d, res=[r], scale=0.5)
        got32 = run_fp32_direct(x, w, b, d, res=[r], scale=0.5)
        what = f"narrow C={C} k={k} d={d} L={L}"
        assert not bool(torch.isnan(got).any()), what
        e32, e_def = err(got32, ref64), err(got, ref3)
        miss = ((got.double() - ref64).abs() - (BOUND * S + 2.0 * e32)).max().item()
        print(f"{what}: |y - bf16x3 definition| {e_def:.3e} (fp32 MFMA against float64: {e32:.3e}); |y - float64| {err(got, ref64):.3e}, "
              f"at most {((got.double() - ref64).abs() / (BOUND * S)).max().item():.3f} of 2^-16 S")
        assert e_def <= 2.0 * e32 + 1e-7, what
        assert miss <= 0.0, what


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("C", [8, 16, 24, 32, 40, 48])
def test_narrow_bf16x3_every_pair(C, k, d, monkeypatch):
    """test_narrow_bf16x6_every_pair with two piece planes: one nonzero weight per output channel co (input channel (7 co + 3) % C,
    tap co % k) in ONE slot.  Slot h keeps the pairs h h and m h (sample piece first) -> (a_h + a_m) v; slot m keeps h m -> a_h v:
    the three kept pairs are each present and (m, m) is absent; the device split's h and m are pinned."""
    L = 300 + 37 * (C // 8) + k + d
    B = 2 if C in (24, 40) else 1
    x, pieces = designed_values(B * C * L, 20 + C + k + d)
    x, pieces = x.view(B, C, L), [p.view(B, C, L) for p in pieces]
    co = torch.arange(C)
    ci, tap = (7 * co + 3) % C, co % k
    assert sorted(ci.tolist()) == list(range(C))
    v = weight_values(C, 21 + C)
    w = torch.zeros(C, C, k)
    w[co, ci, tap] = v
    c = (k - 1) // 2
    for slot in (0, 1):
        monkeypatch.setattr(packing, "split_pieces", slot_split(slot))       # three planes with one filled; the packer keeps two
        out = run_narrow(x, w, None, d)
        src = F.pad(slot_sum(pieces, slot + 1), (c * d, c * d))               # weight slot h: a_h + a_m; slot m: a_h
        exp = torch.stack([src[:, ci[o], tap[o] * d:tap[o] * d + L] for o in range(C)], dim=1) * v.double()[None, :, None]
        assert_same(out, exp.float(), f"narrow bf16 x 3 C={C} k={k} d={d} L={L} weight slot {'hm'[slot]}")


def test_argument_refusals():
    """The three refusals tests/test_layout.py pins for fh_narrow_conv_bf16x6_f32, from the new entry under its own name."""
    fn = getattr(hip.lib(), ENTRY)
    msg = lambda: hip.lib().fh_last_error()
    assert fn(16, 1, 16, 1, 50, 1, 1, 0) == -1 and b"channels" in msg() and ENTRY.encode() in msg()
    assert fn(16, 1, 16, 1, 24, 7, 1, 0) == -1 and b"dilation" in msg() and ENTRY.encode() in msg()
    assert fn(16, 1, 16, 1, 24, 1, 2, 0) == -1 and b"flags" in msg() and ENTRY.encode() in msg()
