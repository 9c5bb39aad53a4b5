"""The bf16 x 3 form's definition on the CPU (conv_form='direct_bf16x3'; csrc/bf16x6.h: kBf16x3SmallFirst), shared by the tests of
the two-piece direct kernels: every fp32 operand keeps the first two pieces of the exact split, h = bf16(x) and m = bf16(x - h), and
a product is the sum of the three pairs h h, h m, m h -- here summed in float64, so that what is left between a kernel and this
reference is the kernel's fp32 accumulation alone."""
import torch
import torch.nn.functional as F

from flowhigh_amd.packing import split_pieces

PAIRS = ((1, 0), (0, 1), (0, 0))            # (piece of x, piece of w): m h, h m, h h -- every pair with i + j <= 1
BOUND = 2.0 ** -16                          # |conv_bf16x3_ref - float64 conv| <= BOUND * abs_sum, pointwise (test_direct_bf3_cpu.py)


def two_pieces(t):
    """fp32 tensor -> (h, m) in float64."""
    return tuple(p.double() for p in split_pieces(t.float())[:2])


def conv_bf16x3_ref(x, w, bias=None, conv=F.conv1d, **conv_kwargs):
    """The float64 sum of the three pair-convs over split_pieces(.)[:2] of x and w (+ bias, in float64).  conv: F.conv1d or
    F.conv_transpose1d; conv_kwargs: its stride / padding / dilation."""
    xs, ws = two_pieces(x), two_pieces(w)
    y = sum(conv(xs[i], ws[j], None, **conv_kwargs) for i, j in PAIRS)
    return y if bias is None else y + bias.double().view(1, -1, 1)


def abs_sum(x, w, conv=F.conv1d, **conv_kwargs):
    """S = conv(|x|, |w|) in float64: the sum of |a b| over the products of each output."""
    return conv(x.double().abs(), w.double().abs(), None, **conv_kwargs)
