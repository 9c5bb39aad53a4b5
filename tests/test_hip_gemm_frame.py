"""GPU: the frame of the two GEMM kernels (gemm_common.h under gemm_mfma.hip and gemm_bf.hip) at its edges, with inputs for which
fp32 is exact (tests/test_gemm_frame_cpu.py holds the design and proves it): the frame's job is placement -- which tile a block
takes, which element a lane stores, which row of A / R / C a stride reaches -- so the LINEAR cases assert equality with the float64
result, in both forms, and that nothing outside C[0:M, 0:N] is written.  The pair and log epilogues add one inexact fp32 function
to exact pre-activations; their bar is derived from torch's own fp32 evaluation of the same formula."""
import math
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from flowhigh_amd import hip, packing                                                                  # noqa: E402
from test_gemm_frame_cpu import (ALPHA, EPI_K, LINEAR_CASES, LOG_CASES, LOG_FLOOR, PAIR_CASES, case_id, design,   # noqa: E402
                                 epilogue_bar, expected_linear, gemm_variant, preact)
from test_hip_bf16x6_pairs import assert_same                                                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC5A5A5                                     # a quiet NaN with a payload no kernel produces
FORMS = pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16x6"])


def sentinel_buffer(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def assert_untouched_outside(c, M, out_w, what):
    """Every element of the C buffer outside [0:M, 0:out_w] still holds the sentinel's bits."""
    bits = c.view(torch.int32).clone()
    bits[:M, :out_w] = SENTINEL
    bad = bits != SENTINEL
    if bool(bad.any()):
        i = tuple(int(t) for t in bad.nonzero()[0])
        pytest.fail(f"{what}: {int(bad.sum())} elements outside C[0:{M}, 0:{out_w}] were written (first at {i})")


def strided(t, ld, fill=float("nan")):
    """[rows, cols] float64 -> device fp32 [rows, ld] with the pad columns cols .. ld holding `fill` (never to be read)."""
    rows, cols = t.shape
    out = torch.full((rows, ld), fill, dtype=torch.float32)
    out[:, :cols] = t.float()
    return out.to(DEV)


def device_weight(w, bf):
    w = w.float()
    return (packing.pack_gemm_bf_weight(w) if bf else w).to(DEV)


@FORMS
@pytest.mark.parametrize("case", LINEAR_CASES, ids=case_id)
def test_gemm_frame_linear_exact(case, bf):
    """C = alpha (A W^T + bias) + R bitwise, for every combination of {no bias, bias} x {no R, R with ldr = N + 5, one R row with
    ldr = 0}, A rows lda = K + 4 or K + 8 apart with NaN between them, C rows ldc = N + 3 apart inside a sentinel-filled
    [M + 2, ldc] buffer, W's pad rows nonzero."""
    M, N, K, variant, blocks, grid = case
    assert gemm_variant(M, N) == (variant, blocks, grid)
    a, w, bias, r = design(M, N, K)
    wd, bd = device_weight(w, bf), bias.float().to(DEV)
    ad = {lda: strided(a, lda) for lda in (K + 4, K + 8)}
    ldc = N + 3
    r_forms = {"none": (None, None, 0), "ldr": (strided(r, N + 5), r, N + 5), "row": (r[0].float().to(DEV), r[0], 0)}
    combo = 0
    for with_bias in (False, True):
        for r_name, (rd, r_ref, ldr) in r_forms.items():
            lda = (K + 4, K + 8)[combo % 2]
            combo += 1
            what = f"gemm {variant} {'bf16x6' if bf else 'f32'} M={M} N={N} K={K} bias={with_bias} R={r_name} lda={lda}"
            c = sentinel_buffer(M + 2, ldc)
            hip.gemm(ad[lda], wd, c, M, N, K, bias=bd if with_bias else None, R=rd, alpha=ALPHA, lda=lda, ldc=ldc, ldr=ldr, bf=bf)
            torch.cuda.synchronize()
            assert_untouched_outside(c, M, N, what)
            assert_same(c[:M, :N], expected_linear(a, w, bias if with_bias else None, r_ref, N), what)


def run_epilogue(M, N, mode, bf):
    """(device output [M, out_w], pre-activations float64 [M, N]) of one epilogue launch on the exact inputs, after checking that
    C's pad columns and guard rows keep the sentinel."""
    K = EPI_K
    a, w, bias, _ = design(M, N, K)
    out_w = N if mode == "logclamp" else N // 2
    ldc, lda = out_w + 3, K + 4
    c = sentinel_buffer(M + 2, ldc)
    epi = {"geglu": hip.EPI_GEGLU, "mag": hip.EPI_MAG, "logclamp": hip.EPI_LOGCLAMP}[mode]
    hip.gemm(strided(a, lda), device_weight(w, bf), c, M, N, K, bias=bias.float().to(DEV), epilogue=epi, lda=lda, ldc=ldc, bf=bf)
    torch.cuda.synchronize()
    assert_untouched_outside(c, M, out_w, f"gemm {mode} M={M} N={N}")
    return c[:M, :out_w].cpu(), preact(a, w, bias, N)


@FORMS
@pytest.mark.parametrize("mode", ["geglu", "mag"])
@pytest.mark.parametrize("M,N,variant", PAIR_CASES)
def test_gemm_frame_pair_epilogues(M, N, variant, mode, bf):
    """GEGLU and MAG on exact pre-activations: pair (blk, j) of the packed columns lands in output column blk * 32 + j (the float64
    reference is laid out so: a misplaced pair misses by the size of the values, not by rounding), for odd packed block counts
    (3, 7, 33: the NT = 2 wave column past N stores nothing) and an even one, under <1,2> and <2,2>.

    Bar = 4 x (largest distance of torch's fp32 CPU evaluation of the formula from float64) + one fp32 ulp of the largest output.
    Measured on an MI355X, at the shape where each is largest, (4100, 2112); both forms give the same figures (the
    pre-activations are the same bits):
      GEGLU  reference's own fp32 distance 1.155e-06  device distance 1.155e-06  bar 5.574e-06
      MAG    reference's own fp32 distance 3.534e-07  device distance 2.381e-07  bar 1.891e-06
    (at (65, 192): GEGLU 6.201e-07 / 6.201e-07 / 3.434e-06, MAG 3.079e-07 / 2.174e-07 / 1.708e-06)."""
    assert gemm_variant(M, N, plain=False)[0] == variant
    got, pre = run_epilogue(M, N, mode, bf)
    bar, own, ref64 = epilogue_bar(pre, mode)
    dist = float((got.double() - ref64).abs().max())
    print(f"{mode} {variant} M={M} N={N} bf={bf}: reference's own fp32 distance {own:.3e}, device distance {dist:.3e}, bar {bar:.3e}")
    assert bool(torch.isfinite(got).all())
    assert dist <= bar


@FORMS
@pytest.mark.parametrize("M,N,variant", LOG_CASES)
def test_gemm_frame_logclamp(M, N, variant, bf):
    """log(max(A W^T + bias, 1e-5)) on exact pre-activations, about half of them <= 0: those outputs all hold one bit pattern, the
    device's logf(1e-5f), and no other output does (the smallest pre-activation above the clamp is 2^-8).

    Bar as for the pair epilogues.  Measured on an MI355X, the same at both shapes and in both forms:
      LOGCLAMP  reference's own fp32 distance 3.422e-07  device distance 1.565e-06  bar 2.323e-06
    The device's distance is that of the clamp value itself: the device's logf(1e-5f) is -11.512927055 where the exact
    -11.512925490 rounds to -11.512925148 (torch's CPU value), 1.6 ulp away.  So the clamp value is taken from the device (one
    value at every clamped output) and held to the bar, not compared with the host's logf."""
    assert gemm_variant(M, N)[0] == variant
    got, pre = run_epilogue(M, N, "logclamp", bf)
    bar, own, ref64 = epilogue_bar(pre, "logclamp")
    dist = float((got.double() - ref64).abs().max())
    clamped = pre <= LOG_FLOOR
    floor = got[clamped][0]
    host = float(torch.log(torch.tensor(LOG_FLOOR, dtype=torch.float32)))
    print(f"logclamp {variant} M={M} N={N} bf={bf}: reference's own fp32 distance {own:.3e}, device distance {dist:.3e}, "
          f"bar {bar:.3e}; clamp value {float(floor)!r} against the host's logf(1e-5f) = {host!r}")
    assert 0.3 < float(clamped.double().mean()) < 0.7
    assert abs(float(floor) - math.log(LOG_FLOOR)) <= bar
    assert bool((got[clamped].view(torch.int32) == floor.view(torch.int32)).all())
    assert not bool((got[~clamped] == floor).any())
    assert dist <= bar
