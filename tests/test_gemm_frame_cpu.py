"""The design behind tests/test_hip_gemm_frame.py, checked without a GPU.

That file tests the GEMM frame (gemm_common.h: tile variants, XCD block order, grid rounded up to 8, epilogues, strides) with
inputs for which fp32 arithmetic is exact, so that it can assert equality and every miss is a misplaced element:

  * A and W hold k/16, bias and R hold k/4, k an integer in [-8, 8]; alpha = 0.5; K <= 96.  A product is a multiple of 2^-8 of
    magnitude <= 1/4, a sum of K of them a multiple of 2^-8 below 24; with the bias (multiples of 2^-2, <= 2), alpha (exact
    halving) and R every intermediate is a multiple of 2^-9 below 2^5: 14 significant bits, whatever the order of addition.
  * k/16 with |k| <= 8 has at most 4 significant bits: one bf16 piece, so the bf16 x 6 form's six piece-pair products hold the
    same exact values (five of them zero).

Here: the designed operands give the same bits in fp32 F.linear as in float64; packing.split_pieces puts each value into its
high piece; gemm_variant restates launch_gemm's rule and gives the variant, block count and grid of every case; the LOGCLAMP
inputs lie on both sides of the clamp and the pair inputs keep GELU unsaturated.  The cases, the designed operands and
gemm_variant live here (this file runs everywhere) and test_hip_gemm_frame.py imports them."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import packing          # noqa: E402

ALPHA = 0.5
K_MAX = 96


# ---- launch_gemm's choice, restated -----------------------------------------------------------------------------------------
def gemm_variant(M, N, plain=True):
    """(variant, blocks, grid) of launch_gemm (gemm_common.h) for C[M, N]: plain = LINEAR / LOGCLAMP epilogue (the pair epilogues
    need NT = 2 and never take <1,1>); blocks = tiles of the variant, grid = blocks rounded up to a multiple of 8."""
    cd = lambda a, b: -(-a // b)
    if plain and cd(M, 64) * cd(N, 128) < 200:
        v, bm, bn = "<1,1>", 64, 64
    elif cd(M, 128) * cd(N, 128) < 512:
        v, bm, bn = "<1,2>", 64, 128
    else:
        v, bm, bn = "<2,2>", 128, 128
    blocks = cd(M, bm) * cd(N, bn)
    return v, blocks, cd(blocks, 8) * 8


def xcd_order(grid, m_tiles, bn):
    """gemm_block's remap: block id -> (m tile, n0) for a grid that is a multiple of 8."""
    per_xcd = grid >> 3
    work = [(bid & 7) * per_xcd + (bid >> 3) for bid in range(grid)]
    return work, [(w % m_tiles, (w // m_tiles) * bn) for w in work]


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _cd(a, b):
    return -(-a // b)


# (M, N, K, variant, blocks, grid)
LINEAR_CASES = [(M, N, K, "<1,1>", _cd(M, 64) * _cd(N, 64), _cd(_cd(M, 64) * _cd(N, 64), 8) * 8)
                for M in (1, 63, 64, 65, 129) for N in (64, 100, 192) for K in (32, 64, 96)]
LINEAR_CASES += [(1601, 1000, 32, "<1,2>", 208, 208), (1601, 1000, 64, "<1,2>", 208, 208),
                 (1601, 1100, 32, "<1,2>", 234, 240), (1601, 1100, 64, "<1,2>", 234, 240),
                 (4097, 2000, 32, "<2,2>", 528, 528), (4097, 2100, 32, "<2,2>", 561, 568)]
# (M, N packed, variant): GEGLU and MAG; K = 32
PAIR_CASES = [(65, 192, "<1,2>"), (333, 448, "<1,2>"), (4100, 2112, "<2,2>"), (4100, 2176, "<2,2>")]
# (M, N, variant): LOGCLAMP; K = 32
LOG_CASES = [(65, 100, "<1,1>"), (1601, 1000, "<1,2>")]
EPI_K = 32


def case_id(c):
    return "-".join(str(v) for v in c[:3])


# ---- designed operands ------------------------------------------------------------------------------------------------------
def _ints(shape, g, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def design(M, N, K, seed=0):
    """float64 (A [M, K], W [n_pad, K], bias [N], R [M, N]) of exact values: A, W = k/16 and bias, R = k/4 with integer |k| <= 8.
    W's pad rows N .. n_pad hold nonzero values (a column past N that reached C would not be zero)."""
    assert K <= K_MAX and K % 32 == 0
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * N + K)
    n_pad = -(-N // 128) * 128
    a = _ints((M, K), g) / 16
    w = _ints((n_pad, K), g) / 16
    pad = w[N:]
    pad[pad == 0] = 0.5
    return a, w, _ints((N,), g) / 4, _ints((M, N), g) / 4


def expected_linear(a, w, bias, r, N):
    """float64 alpha (A W^T + bias) + R cast to fp32; bias / r may be None; r [M, N] or one row [N] (ldr = 0)."""
    acc = a @ w[:N].t()
    if bias is not None:
        acc = acc + bias
    acc = ALPHA * acc
    if r is not None:
        acc = acc + r
    return acc.float()


def preact(a, w, bias, N):
    """The exact pre-activations A W^T + bias of the GEGLU / MAG / LOGCLAMP epilogues, float64."""
    return a @ w[:N].t() + bias


def pair_halves(pre):
    """Packed columns [M, N] -> (first, second) [M, N / 2] each: block blk of 64 packed columns holds first (32) then second (32);
    the pair (blk, j) lands in output column blk * 32 + j."""
    M, N = pre.shape
    p = pre.view(M, N // 64, 2, 32)
    return p[:, :, 0].reshape(M, N // 2), p[:, :, 1].reshape(M, N // 2)


SQRT_HALF = 0.70710678118654752440
MAG_EPS = float(torch.tensor(1e-9, dtype=torch.float32))
LOG_FLOOR = float(torch.tensor(1e-5, dtype=torch.float32))


def epilogue_formula(pre, mode):
    """The epilogue's formula (gemm_common.h) in the dtype of `pre`: float64 is the reference, float32 torch's own evaluation."""
    if mode == "logclamp":
        return torch.log(pre.clamp_min(LOG_FLOOR))
    first, second = pair_halves(pre)
    if mode == "geglu":
        return 0.5 * second * (1.0 + torch.erf(second * SQRT_HALF)) * first
    return torch.sqrt(first * first + second * second + MAG_EPS)


def ulp32(x):
    """One fp32 ulp at magnitude x > 0."""
    return float(2.0 ** (torch.frexp(torch.tensor(float(x), dtype=torch.float64))[1].item() - 24))


def epilogue_bar(pre, mode):
    """(bar, own, ref64): own = the largest distance of torch's fp32 CPU evaluation of the formula from the float64 one on these
    pre-activations; bar = 4 own + one fp32 ulp of the largest output."""
    ref64 = epilogue_formula(pre, mode)
    own = float((epilogue_formula(pre.float(), mode).double() - ref64).abs().max())
    return 4 * own + ulp32(ref64.abs().max()), own, ref64


# ---- the tests --------------------------------------------------------------------------------------------------------------
ALL_SHAPES = sorted({c[:3] for c in LINEAR_CASES} | {(M, N, EPI_K) for M, N, _ in PAIR_CASES + LOG_CASES})


@pytest.mark.parametrize("M,N,K", ALL_SHAPES)
def test_designed_operands_are_exact_in_fp32(M, N, K):
    """fp32 F.linear (any order of addition the CPU BLAS picks) gives the bits of float64 cast to fp32, with and without bias and
    R, and every value and every result is a multiple of its grid below the stated magnitude."""
    a, w, bias, r = design(M, N, K)
    for t, unit, lim in ((a, 16, 8), (w, 16, 8), (bias, 4, 8), (r, 4, 8)):
        k = t * unit
        assert torch.equal(k, k.round()) and float(k.abs().max()) <= lim
    assert bool((w[N:] != 0).all())
    acc32 = F.linear(a.float(), w[:N].float())
    assert torch.equal(acc32, (a @ w[:N].t()).float())
    assert torch.equal(acc32.double() * 256, (acc32.double() * 256).round()) and float(acc32.abs().max()) * 256 < 2 ** 16
    f = lambda t: None if t is None else t.float()
    for b in (None, bias):
        for rr in (None, r, r[0]):
            got = F.linear(a.float(), w[:N].float(), f(b)) * ALPHA
            got = got if rr is None else got + rr.float()
            assert torch.equal(got, expected_linear(a, w, b, rr, N))


def test_designed_values_are_one_bf16_piece():
    """Every designed A / W value k/16 is its own high piece: the bf16 x 6 form computes the same exact products."""
    v = torch.arange(-8, 9).float() / 16
    h, m, lo = packing.split_pieces(v)
    assert torch.equal(h.float(), v) and not bool(m.float().any()) and not bool(lo.float().any())
    a, w, _, _ = design(65, 100, 96)
    for t in (a, w):
        h, m, lo = packing.split_pieces(t.float())
        assert torch.equal(h.double(), t) and not bool(m.float().any()) and not bool(lo.float().any())


@pytest.mark.parametrize("case", LINEAR_CASES, ids=case_id)
def test_gemm_variant_of_the_linear_cases(case):
    M, N, K, variant, blocks, grid = case
    assert gemm_variant(M, N) == (variant, blocks, grid)


def test_the_linear_cases_cover_the_table():
    """Block counts 1, 4, 9 (grids 8, 8, 16) under <1,1>; 208 -> 208 and 234 -> 240 under <1,2>; 528 -> 528 and 561 -> 568 under
    <2,2>: grids with and without rounded-up blocks in every variant."""
    seen = {(c[3], c[4], c[5]) for c in LINEAR_CASES}
    assert {("<1,1>", 1, 8), ("<1,1>", 4, 8), ("<1,1>", 9, 16), ("<1,2>", 208, 208), ("<1,2>", 234, 240),
            ("<2,2>", 528, 528), ("<2,2>", 561, 568)} <= seen
    assert {c[2] for c in LINEAR_CASES if c[3] == "<1,1>"} == {32, 64, 96}


def test_gemm_variant_of_the_epilogue_cases():
    for M, N, variant in PAIR_CASES:
        assert N % 64 == 0 and gemm_variant(M, N, plain=False)[0] == variant
    assert [(N // 64) % 2 for _, N, _ in PAIR_CASES] == [1, 1, 1, 0]      # odd packed block counts: 3, 7, 33 (the MAG width)
    for M, N, variant in LOG_CASES:
        assert gemm_variant(M, N)[0] == variant
    # the variants match the bf16 x 6 tests' statement of the rule for LINEAR
    from test_hip_bf16x6_pairs import gemm_variant as linear_variant
    for c in LINEAR_CASES:
        assert linear_variant(c[0], c[1]) == c[3]


@pytest.mark.parametrize("grid,m_tiles,bn,n_tiles", [(8, 1, 64, 1), (8, 2, 64, 2), (16, 3, 64, 3), (208, 26, 128, 8),
                                                     (240, 26, 128, 9), (528, 33, 128, 16), (568, 33, 128, 17)])
def test_xcd_remap_is_a_bijection_onto_the_tiles(grid, m_tiles, bn, n_tiles):
    """(bid & 7) per_xcd + (bid >> 3) permutes 0 .. grid - 1, so every tile gets one block and the rounded-up blocks are exactly
    those with n0 >= n_tiles bn (the kernels return there)."""
    work, tiles = xcd_order(grid, m_tiles, bn)
    assert sorted(work) == list(range(grid))
    live = [t for t in tiles if t[1] < n_tiles * bn]
    assert sorted(live) == [(m, n * bn) for m in range(m_tiles) for n in range(n_tiles)]
    assert len(tiles) - len(live) == grid - m_tiles * n_tiles


@pytest.mark.parametrize("M,N,variant", LOG_CASES)
def test_logclamp_inputs_lie_on_both_sides_of_the_clamp(M, N, variant):
    a, w, bias, _ = design(M, N, EPI_K)
    pre = preact(a, w, bias, N)
    below = float((pre <= LOG_FLOOR).double().mean())
    assert 0.3 < below < 0.7
    assert float(pre[pre > LOG_FLOOR].min()) >= 2.0 ** -8          # the next value above the clamp is far from it


@pytest.mark.parametrize("M,N,variant", PAIR_CASES)
def test_pair_inputs_keep_gelu_unsaturated(M, N, variant):
    a, w, bias, _ = design(M, N, EPI_K)
    pre = preact(a, w, bias, N)
    assert float(pre.abs().max()) < 6.0
    assert torch.equal(pre.float().double(), pre)                                  # exact in fp32
    first, second = pair_halves(pre)
    assert first.shape == (M, N // 2) and torch.equal(first[:, 32:64], pre[:, 64:96]) and torch.equal(second[:, :32], pre[:, 32:64])
