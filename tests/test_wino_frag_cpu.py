"""CPU: the fragment-order packer of the bf16 x 6 F(5,4) weights (packing.pack_wino54_weight_frag, over packing.frag_order) is the
index permutation of the row form they replace -- [cin/16][G][points][cout_pad/32 granules][3 pieces][64 lanes][8 bf16], lane
32 lh + r of granule q, piece p = split_bf3(u)[..., 32 q + r, p, 8 lh : 8 lh + 8] -- element for element; the planner names the
layout of every launch, and a weight blob packed before the layout changed is refused."""
import json

import pytest
import torch

from flowhigh_amd import packing as P
from flowhigh_amd import planner, weights


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def permuted_rows(rows):
    """The permutation written out index by index: rows = split_bf3(u), [..., cout_pad, 3, 16] -> [..., cout_pad/32, 3, 64, 8]."""
    lead, cpad = rows.shape[:-3], rows.shape[-3]
    out = torch.empty(*lead, cpad // 32, 3, 64, 8, dtype=rows.dtype)
    for q in range(cpad // 32):
        for p in range(3):
            for lh in range(2):
                out[..., q, p, 32 * lh:32 * lh + 32, :] = rows[..., 32 * q:32 * q + 32, p, 8 * lh:8 * lh + 8]
    return out


@pytest.mark.parametrize("cout,cout_pad", [(80, 96), (192, 192)])
@pytest.mark.parametrize("cin", [16, 48])
@pytest.mark.parametrize("k", [3, 7, 11])
def test_wino54_fragment_order_is_the_permuted_row_form(k, cin, cout, cout_pad):
    w = rnd(cout, cin, k, seed=k + cin + cout)
    rows = P.split_bf3(P.pack_wino54_weight(w, cout_pad))
    frag = P.pack_wino54_weight_frag(w, cout_pad)
    assert frag.dtype == torch.int16 and frag.is_contiguous()
    assert tuple(frag.shape) == (cin // 16, -(-k // 4), 8, cout_pad // 32, 3, 64, 8) and frag.numel() == rows.numel()
    assert torch.equal(frag, permuted_rows(rows))
    assert torch.equal(rows, P.pack_wino54_weight_any(w, cout_pad, True))          # (the row form itself is what it was)


@pytest.mark.parametrize("cout,cout_pad", [(80, 96), (192, 192)])
@pytest.mark.parametrize("cin", [16, 48])
@pytest.mark.parametrize("k", [3, 10])
def test_frag_order_of_f43_weights_is_the_permuted_row_form(k, cin, cout, cout_pad):
    """The permutation itself does not depend on the transform: the same check on the F(4,3) kernel's six-point weights (no kernel
    reads those in fragment order: planner.wino_weight_flags)."""
    u = P.pack_wino_weight(rnd(cout, cin, k, seed=100 + k + cin + cout), cout_pad)
    frag = P.frag_order(u)
    assert tuple(frag.shape) == (cin // 16, -(-k // 3), 6, cout_pad // 32, 3, 64, 8)
    assert torch.equal(frag, permuted_rows(P.split_bf3(u)))


def test_fragment_order_needs_whole_granules():
    with pytest.raises(ValueError, match="granules of 32"):
        P.frag_order(torch.zeros(1, 1, 8, 48, 16))


def test_planner_names_the_weight_layout_of_a_launch():
    f54 = planner.WINO_F54
    assert planner.WINO_FRAG_ORDER == 128 and planner.WINO_BF16X6 == 16
    for tile in (1, 2):
        assert planner.wino_weight_flags(f54 | tile, True) == planner.WINO_BF16X6 | planner.WINO_FRAG_ORDER
        assert planner.wino_weight_flags(f54 | tile, False) == 0
    # (the F(4,3) kernel reads 96-byte rows)
    for tile in (0, 1, 4, 5, 6):
        assert planner.wino_weight_flags(tile, True) == planner.WINO_BF16X6 and planner.wino_weight_flags(tile, False) == 0
    w = rnd(80, 16, 7, seed=5)
    assert torch.equal(planner.wino_packer(f54 | 1, True)(w, 96), P.pack_wino54_weight_frag(w, 96))
    assert torch.equal(planner.wino_packer(f54 | 1, False)(w, 96), P.pack_wino54_weight(w, 96))
    assert torch.equal(planner.wino_packer(1, True)(w, 96), P.split_bf3(P.pack_wino_weight(w, 96)))


@pytest.mark.parametrize("form", ["bf16x6", "direct_bf16x6"])
def test_format_tag_refuses_blobs_of_the_row_layout(form):
    """Blobs packed with the bf16 x 6 weights in rows carry layout 4 in their tag: the tag of this layout is another one."""
    tag = json.loads(weights.format_tag(form))
    assert tag["form"] == form and tag["layout"] > 4
    parent = dict(tag, layout=4)
    assert weights.format_tag(form) != json.dumps(parent, sort_keys=True)
