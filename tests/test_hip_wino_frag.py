"""GPU: the bf16 x 6 F(5,4) conv on weights in fragment order (tile_cfg | FH_WINO_FRAG_ORDER, packing.pack_wino54_weight_frag)
gives the bits of the same launch on 96-byte rows (packing.split_bf3 of pack_wino54_weight): same values, same MFMA order,
only the addresses of the weight loads differ.  The row form is held to float64 by test_hip_ops.py and
the bf16 x 6 suites; here the shapes are the smallest at which the new loader can go wrong: one chunk (no refill, the last request past
the end) and three (refill across chunks and tap groups), a padded co tile and two co tiles (third granule of a 96-row block),
both block heights, k = 3 / 7 / 11 as one three-segment group (tap-group counts 3, 2, 1), two blocks with a ragged tail and
whole blocks, plain rows and phase-major rows of dilation 3, 0 and 1 residual, batch 2."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from flowhigh_amd import hip              # noqa: E402
from flowhigh_amd import vocoder as V     # noqa: E402

DEV = "cuda"
KS = (3, 7, 11)
FILL = -7.0                                # outputs are prefilled with it: what a launch does not write compares equal
FLAGS_ROW = V.WINO_BF16X6
FLAGS_FRAG = V.WINO_BF16X6 | V.WINO_FRAG_ORDER


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def weights(cin, cout, cpad):
    """(row-form, fragment-order) device weights of the three kernel sizes, from the same fp32 weights."""
    ws = [rnd(cout, cin, k, seed=300 + k, scale=1.0 / (cin * k) ** 0.5) for k in KS]
    return ([V.split_bf3(V.pack_wino54_weight(w, cpad)).to(DEV) for w in ws], [V.pack_wino54_weight_frag(w, cpad).to(DEV) for w in ws])


def tile_pad(tile, cout):
    bm = hip.lib().fh_wino54_tile_m(tile | FLAGS_FRAG)
    assert bm == hip.lib().fh_wino54_tile_m(tile | FLAGS_ROW) == {1: 96, 2: 64}[tile]
    return -(-cout // bm) * bm


def make_groups(us, xs, bias, res, outs, cin, cout, cpad, lengths):
    """One three-segment group per clip: out = (sum_k conv_k(x_k) + bias + res) / 3."""
    return [V.make_wino_group([V.make_wino_seg(xs[c][i], us[i], cin, k, taps=4) for i, k in enumerate(KS)], bias,
                              [res[c]] if res is not None else [], outs[c], cout, cpad, n, scale=1.0 / 3) for c, n in enumerate(lengths)]


@pytest.mark.parametrize("nres", [0, 1])
@pytest.mark.parametrize("d,pm", [(1, False), (3, True)])
@pytest.mark.parametrize("L", [327, 640])
@pytest.mark.parametrize("cout", [80, 192])
@pytest.mark.parametrize("cin", [16, 48])
@pytest.mark.parametrize("tile", [1, 2])
def test_wino54_fragment_order_gives_the_rows_bits(tile, cin, cout, L, d, pm, nres):
    B = 2
    cpad = tile_pad(tile, cout)                           # (80 -> 96 in the 96-row block, 128 in the 64-row one; 192 -> 192)
    u_row, u_frag = weights(cin, cout, cpad)
    lay = (lambda t: V.to_phase_major(t, d)) if pm else (lambda t: t)
    xs = [lay(rnd(B, cin, L, seed=310 + i)).to(DEV) for i in range(len(KS))]
    res = lay(rnd(B, cout, L, seed=320)).to(DEV) if nres else None
    bias = rnd(cout, seed=321).to(DEV)
    outs = []
    for us, flags in ((u_row, FLAGS_ROW), (u_frag, FLAGS_FRAG)):
        out = torch.full_like(lay(torch.empty(B, cout, L)), FILL).to(DEV)
        g = make_groups(us, [xs], bias, [res] if nres else None, [out], cin, cout, cpad, [L])
        keep = V.conv_wino(g, B, cpad, L, d, DEV, V.WINO_F54 | tile | flags, phase_major=pm)
        torch.cuda.synchronize()
        del keep
        outs.append(out.cpu())
    assert torch.isfinite(outs[0]).all() and (outs[0] != FILL).float().mean().item() > 0.9
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("d,pm", [(1, False), (3, True)])
@pytest.mark.parametrize("tile", [1, 2])
def test_wino54_fragment_order_ragged_launch(tile, d, pm):
    """The ragged entry shares the dispatch: two clips of 327 and 640 samples in one launch."""
    cin, cout, lengths = 48, 80, [640, 327]
    cpad = tile_pad(tile, cout)
    u_row, u_frag = weights(cin, cout, cpad)
    lay = (lambda t: V.to_phase_major(t, d)) if pm else (lambda t: t)
    xs = [[lay(rnd(1, cin, n, seed=330 + 10 * c + i)).to(DEV) for i in range(len(KS))] for c, n in enumerate(lengths)]
    res = [lay(rnd(1, cout, n, seed=350 + c)).to(DEV) for c, n in enumerate(lengths)]
    bias = rnd(cout, seed=351).to(DEV)
    got = []
    for us, flags in ((u_row, FLAGS_ROW), (u_frag, FLAGS_FRAG)):
        outs = [torch.full_like(lay(torch.empty(1, cout, n)), FILL).to(DEV) for n in lengths]
        g = make_groups(us, xs, bias, res, outs, cin, cout, cpad, lengths)
        keep = V.conv_wino_ragged(g, lengths, cpad, d, DEV, V.WINO_F54 | tile | flags, phase_major=pm)
        torch.cuda.synchronize()
        del keep
        got.append([o.cpu() for o in outs])
    for a, b in zip(*got):
        assert torch.isfinite(a).all() and (a != FILL).float().mean().item() > 0.9
        assert torch.equal(a, b)


@pytest.mark.parametrize("entry,tile", [("fh_conv_wino54_f32", 1), ("fh_conv_wino54_f32", 2), ("fh_conv_wino54_f32", 0),
                                        ("fh_conv_wino_f32", 1), ("fh_conv_wino_f32", 16 | 1)])
def test_fragment_order_bit_needs_the_bf16x6_form(entry, tile):
    """FH_WINO_FRAG_ORDER without FH_WINO_BF16X6 (fp32 weights have no fragment order), or on the F(4,3) entry (96-byte rows only),
    is the argument error and launches nothing."""
    cin, cout, L = 16, 96, 320
    f54 = entry == "fh_conv_wino54_f32"
    w = rnd(cout, cin, 3, seed=360)
    u = (V.pack_wino54_weight_frag(w, cout) if f54 else V.frag_order(V.pack_wino_weight(w, cout))).to(DEV)
    x, out = rnd(1, cin, L, seed=361).to(DEV), torch.full((1, cout, L), FILL, device=DEV)
    bias = torch.zeros(cout, device=DEV)
    g = V.make_wino_group([V.make_wino_seg(x, u, cin, 3, taps=4 if f54 else 3)], bias, [], out, cout, cout, L)
    d = hip.to_device_struct_array([g], DEV)
    rc = getattr(hip.lib(), entry)(d.data_ptr(), 1, 1, cout, L, 1, 0, tile | V.WINO_FRAG_ORDER, hip.stream())
    torch.cuda.synchronize()
    assert rc == -1 and hip.lib().fh_last_error()                  # FH_E_ARG
    assert (out == FILL).all()
