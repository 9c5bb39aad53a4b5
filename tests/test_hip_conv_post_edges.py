"""GPU: both kernels of fh_conv_post_tanh_f32 (conv_mfma.hip) against tanh(conv1d) in float64.  The vectorised kernel (ksz = 7,
len % 4 == 0, aligned pointers: 4 outputs per thread from 3 float4 loads per channel) at the lengths where its `t >= 4` and
`t + 4 < len` guards decide; the scalar kernel (every other call), which no other test runs directly, at every kernel size and
around its 256-output block; the two against each other bit for bit -- they accumulate in the same order (channel outer, tap
inner, fmaf onto the bias), and a pointer one float into a larger buffer sends the same data through the scalar kernel.

The bar is not taken from the kernel: max and RMS of (kernel - float64) <= max(3 x the same of (fp32 torch F.conv1d + tanh -
float64), 4 ulps of 1) -- the output lies in [-1, 1]; three times the reference's own noise is the project's margin for a
different order of summation (tests/test_hip_regimes.py).  out sits between sentinels; for batch = 2 the two rows are adjacent,
so the float64 comparison of row 0's last and row 1's first outputs is the check that each is its own."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import hip                   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC5A5A5                          # a quiet NaN with a payload no kernel produces
GUARD = 64                                     # sentinel floats in front of and behind out (a multiple of 4: keeps out aligned)
BAR_FACTOR = 3.0
FLOOR = 4 * 2.0 ** -24
CINS = [1, 24, 48]
BATCHES = [1, 2]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def is_sentinel(t):
    return bool((t.view(torch.int32) == SENTINEL).all())


def conv_post(x, w, b, ksz, shift=0):
    """x [B, cin, len], w [cin, ksz], b [1] (host) -> out [B, len] (host), through out's interior between sentinels.  shift = 1: x
    and out start one float into their buffers (pointers that are not 16-byte aligned: the scalar kernel whatever ksz and len)."""
    B, cin, L = x.shape
    xbuf = torch.zeros(x.numel() + 4, device=DEV)
    xbuf[shift:shift + x.numel()] = x.reshape(-1).to(DEV)
    obuf = sentinel(2 * GUARD + B * L + 4)
    wd, bd = w.contiguous().to(DEV), b.to(DEV)
    xp, op = xbuf[shift:].data_ptr(), obuf[GUARD + shift:].data_ptr()
    assert (xp % 16 == 0 and op % 16 == 0) == (shift == 0)
    hip.check(hip.lib().fh_conv_post_tanh_f32(xp, wd.data_ptr(), bd.data_ptr(), op, B, cin, L, ksz, hip.stream()), "fh_conv_post_tanh_f32")
    torch.cuda.synchronize()
    lo, hi = GUARD + shift, GUARD + shift + B * L
    assert is_sentinel(obuf[:lo]), "a store in front of out"
    assert is_sentinel(obuf[hi:]), "a store behind out"
    got = obuf[lo:hi].cpu().view(B, L)
    assert bool(torch.isfinite(got).all()), "an output not written, or not finite"
    return got


def references(x, w, b, ksz):
    ref = torch.tanh(F.conv1d(x.double(), w.double()[None], b.double(), padding=ksz // 2)).squeeze(1)
    plain = torch.tanh(F.conv1d(x, w[None], b, padding=ksz // 2)).squeeze(1).double()
    return ref, plain


def assert_within_bar(got, ref, plain, what):
    ek, ep = got.double() - ref, plain - ref
    mk, mp = ek.abs().max().item(), ep.abs().max().item()
    rk, rp = ek.pow(2).mean().sqrt().item(), ep.pow(2).mean().sqrt().item()
    print(f"conv-post-edges {what}: max err kernel {mk:.3e} plain {mp:.3e}; rms kernel {rk:.3e} plain {rp:.3e}")
    assert mk <= max(BAR_FACTOR * mp, FLOOR), f"{what}: max error {mk:.3e}, plain fp32 {mp:.3e}"
    assert rk <= max(BAR_FACTOR * rp, FLOOR), f"{what}: rms error {rk:.3e}, plain fp32 {rp:.3e}"


def operands(B, cin, L, ksz):
    seed = 7000 + 97 * ksz + 13 * cin + B
    return rnd(B, cin, L, seed=seed + L), rnd(cin, ksz, seed=seed + 1, scale=0.1), rnd(1, seed=seed + 2, scale=0.1)


@pytest.mark.parametrize("L", [1, 2, 3, 5, 7, 255, 256, 257, 1025])
@pytest.mark.parametrize("ksz", [1, 3, 5, 7, 15])
def test_scalar_kernel_against_float64(ksz, L):
    """Every kernel size the entry takes, clips shorter than the halo, either side of the 256-output block, several blocks.
    (None of these lengths is a multiple of 4 except 256, and ksz = 7 at L = 256 is run from an unaligned pointer.)"""
    for cin in CINS:
        for B in BATCHES:
            x, w, b = operands(B, cin, L, ksz)
            shift = 1 if (ksz == 7 and L % 4 == 0) else 0
            got = conv_post(x, w, b, ksz, shift)
            assert_within_bar(got, *references(x, w, b, ksz), f"scalar ksz={ksz} L={L} cin={cin} B={B}")


@pytest.mark.parametrize("L", [4, 8, 12, 1020, 1024, 1028])
def test_vector_kernel_against_float64_and_the_scalar_kernel_bitwise(L):
    """One thread (len = 4: neither neighbour vector), two (len = 8: each has one), three, and either side of the 1024-output
    block.  The same call from pointers one float into larger buffers takes the scalar kernel: torch.equal."""
    for cin in CINS:
        for B in BATCHES:
            x, w, b = operands(B, cin, L, 7)
            got = conv_post(x, w, b, 7)
            assert_within_bar(got, *references(x, w, b, 7), f"vector L={L} cin={cin} B={B}")
            assert torch.equal(conv_post(x, w, b, 7, shift=1), got), f"L={L} cin={cin} B={B}: the two kernels differ"


@pytest.mark.parametrize("ksz,L,shift", [(7, 8, 0), (7, 1024, 0), (7, 8, 1), (7, 257, 0), (15, 1025, 0), (1, 5, 0)])
def test_saturation_gives_exactly_one(ksz, L, shift):
    """Pre-activations beyond +-20 (here +-25 to +-3e6): tanh is exactly +-1 in fp32, and nothing is NaN."""
    for cin in (1, 48):
        x = torch.ones(2, cin, L)
        x[1] = -1.0
        x[:, :, L // 2:] *= 1e4
        w = torch.full((cin, ksz), 1.0)
        for bias in (25.0, -25.0):
            b = torch.tensor([bias])
            pre = F.conv1d(x.double(), w.double()[None], b.double(), padding=ksz // 2).squeeze(1)
            sat = pre.abs() > 20
            assert bool(sat.any())
            got = conv_post(x, w, b, ksz, shift)
            assert torch.equal(got[sat], torch.sign(pre[sat]).float()), f"cin={cin} bias={bias}"


def test_argument_errors_write_nothing():
    L = hip.lib()
    x, w, b = torch.zeros(2 * 8, device=DEV), torch.zeros(2 * 17, device=DEV), torch.zeros(1, device=DEV)
    out = sentinel(16)
    xp, wp, bp, op, st = x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), hip.stream()
    bad = [(xp, wp, bp, op, 1, 2, 8, 4, st), (xp, wp, bp, op, 1, 2, 8, 0, st), (xp, wp, bp, op, 1, 2, 8, 17, st),
           (xp, wp, bp, op, 1, 2, 0, 7, st), (xp, wp, bp, op, 1, 0, 8, 7, st), (xp, wp, bp, op, 0, 2, 8, 7, st),
           (None, wp, bp, op, 1, 2, 8, 7, st), (xp, None, bp, op, 1, 2, 8, 7, st), (xp, wp, None, op, 1, 2, 8, 7, st),
           (xp, wp, bp, None, 1, 2, 8, 7, st)]
    for args in bad:
        rc = L.fh_conv_post_tanh_f32(*args)
        assert rc != 0, str(args[4:8])
        assert L.fh_last_error().decode().startswith("fh_conv_post_tanh_f32:"), L.fh_last_error().decode()
    torch.cuda.synchronize()
    assert is_sentinel(out)
    hip.check(L.fh_conv_post_tanh_f32(xp, wp, bp, op, 1, 2, 8, 7, st), "fh_conv_post_tanh_f32")
    torch.cuda.synchronize()
    assert torch.equal(out[:8].cpu(), torch.zeros(8)) and is_sentinel(out[8:])
