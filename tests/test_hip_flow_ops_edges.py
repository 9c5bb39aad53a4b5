"""GPU: the transformer's small kernels (flow_ops.hip, gemm_mfma.hip's gemv, sum_ops.hip) at the sizes where they change path --
a clip shorter than the conv's halo, the 32-token block edge, one row, a K that is not a multiple of the wave's 256-wide step,
a tail block of the sums -- each against float64 torch (the sums: against the fixed order of addition they promise, bitwise).
The segment forms are compared with float64 per clip, not with the plain kernels, and every buffer carries guard rows or a
sentinel so that a read or a write across an edge shows."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import hip, tables          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC5A5A5                          # a quiet NaN with a payload no kernel produces
GUARD = 1e3                                    # what the guard rows of an input hold: a leak is far above every bar here


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def maxdiff(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def is_sentinel(t):
    return bool((t.view(torch.int32) == SENTINEL).all())


def ulp32(x):
    return float(2.0 ** (torch.frexp(torch.tensor(float(x), dtype=torch.float64))[1].item() - 24))


# ---- depthwise conv + GELU + residual -----------------------------------------------------------------------------------------
DW_GUARD = 40            # guard rows: more than the widest halo (31)


def dwconv_ref(x, w, b):
    """float64 ConvPositionEmbed + residual of one clip: x [n, D], w [D, k], b [D]."""
    D, k = w.shape
    y = F.conv1d(x.double().t()[None], w.double()[:, None, :], b.double(), padding=k // 2, groups=D)
    return F.gelu(y)[0].t() + x.double()


def dwconv_operands(D, k, seed):
    w, b = rnd(D, k, seed=seed, scale=0.2), rnd(D, seed=seed + 1)
    return w, b, w.t().contiguous().to(DEV), b.to(DEV)                   # device weights tap-major [k, D]


@pytest.mark.parametrize("ksz", [1, 31, 63])
@pytest.mark.parametrize("n", [1, 2, 15, 16, 31, 32, 33, 65])
def test_dwconv_gelu_res_edges(n, ksz):
    """fh_dwconv_gelu_res_f32, B = 2, dim 128 and 384: clips shorter than the halo, either side of the 32-token block, no halo
    (ksz = 1) and the largest (63).  The rows before and after the batch hold 1e3 in x and a sentinel in y."""
    B = 2
    for D in (128, 384):
        w, b, wd, bd = dwconv_operands(D, ksz, 200 + ksz)
        x = rnd(B, n, D, seed=210 + n)
        xbuf = torch.full((B * n + 2 * DW_GUARD, D), GUARD)
        xbuf[DW_GUARD:DW_GUARD + B * n] = x.view(B * n, D)
        xd, yd = xbuf.to(DEV), sentinel(B * n + 2 * DW_GUARD, D)
        hip.check(hip.lib().fh_dwconv_gelu_res_f32(xd[DW_GUARD:].data_ptr(), wd.data_ptr(), bd.data_ptr(), yd[DW_GUARD:].data_ptr(),
                                                   B, n, D, ksz, hip.stream()), "dwconv")
        torch.cuda.synchronize()
        ref = torch.stack([dwconv_ref(x[i], w, b) for i in range(B)]).view(B * n, D)
        assert is_sentinel(yd[:DW_GUARD]) and is_sentinel(yd[DW_GUARD + B * n:])
        assert maxdiff(yd[DW_GUARD:DW_GUARD + B * n], ref) <= 5e-6


@pytest.mark.parametrize("D", [128, 384])
@pytest.mark.parametrize("ksz", [1, 31, 63])
def test_dwconv_gelu_res_seg_edges(ksz, D):
    """fh_dwconv_gelu_res_seg_f32 on clips of 1, 33, 2 and 64 tokens against float64 PER CLIP, with 1e3 guard rows before, between
    and after the clips: each clip is padded with zeros at its own ends, and y's guard rows keep their sentinel."""
    frames = [1, 33, 2, 64]
    w, b, wd, bd = dwconv_operands(D, ksz, 220 + ksz)
    starts, row = [], DW_GUARD
    for n in frames:
        starts.append(row)
        row += n + DW_GUARD
    xbuf = torch.full((row, D), GUARD)
    clips = [rnd(n, D, seed=230 + i) for i, n in enumerate(frames)]
    for s0, c in zip(starts, clips):
        xbuf[s0:s0 + c.shape[0]] = c
    seg = torch.tensor([[s0, n] for s0, n in zip(starts, frames)], dtype=torch.int32).to(DEV)
    xd, yd = xbuf.to(DEV), sentinel(row, D)
    hip.check(hip.lib().fh_dwconv_gelu_res_seg_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(), seg.data_ptr(),
                                                   len(frames), max(frames), D, ksz, hip.stream()), "dwconv seg")
    torch.cuda.synchronize()
    keep = torch.ones(row, dtype=torch.bool)
    for s0, c in zip(starts, clips):
        n = c.shape[0]
        keep[s0:s0 + n] = False
        assert maxdiff(yd[s0:s0 + n], dwconv_ref(c, w, b)) <= 5e-6, f"clip of {n} tokens"
    assert is_sentinel(yd[keep.to(DEV)])


# ---- RMSNorm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
@pytest.mark.parametrize("D", [256, 1024, 4096])
def test_rmsnorm_edges(D, rows):
    """fh_rmsnorm_f32: the smallest and the largest dim (1 and 16 vectors per lane), rows either side of the 4-row block, with and
    without beta, one all-zero row (F.normalize's eps), a sentinel row after the last."""
    x, g, b = rnd(rows, D, seed=240 + rows, scale=3.0), rnd(D, seed=241), rnd(D, seed=242)
    if rows > 1:
        x[rows // 2] = 0.0
    base = F.normalize(x.double(), dim=-1) * float(D) ** 0.5 * g.double()
    xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
    for beta, ref in ((bd, base + b.double()), (None, base)):
        y = sentinel(rows + 1, D)
        hip.check(hip.lib().fh_rmsnorm_f32(xd.data_ptr(), gd.data_ptr(), None if beta is None else beta.data_ptr(), y.data_ptr(),
                                           rows, D, hip.stream()), "rmsnorm")
        torch.cuda.synchronize()
        assert is_sentinel(y[rows:])
        assert maxdiff(y[:rows], ref) <= 5e-6
    if rows > 1:
        assert float(base[rows // 2].abs().max()) == 0.0


# ---- qk-norm + RoPE -----------------------------------------------------------------------------------------------------------
def rope_tables(n):
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))
    return tables.rotary_tables(inv_freq, n)


def qknorm_rope_ref(qkv, gq, gk, cos_t, sin_t, heads, dtype):
    """One clip, positions from 0: qkv [n, 3 inner] -> (q, k) [n, inner] each: F.normalize(x) * gamma * 8 per 64-wide head, then
    x cos + rotate_half(x) sin with the [n, 32] tables on both halves.  dtype float64: the reference; float32: torch's own."""
    n, inner = qkv.shape[0], heads * 64
    cs = torch.cat([cos_t, cos_t], -1).to(dtype)[:, None, :]
    sn = torch.cat([sin_t, sin_t], -1).to(dtype)[:, None, :]
    out = []
    for i, gam in enumerate((gq, gk)):
        x = qkv[:, i * inner:(i + 1) * inner].to(dtype).view(n, heads, 64)
        t = F.normalize(x, dim=-1) * gam.to(dtype) * 8.0
        rot = torch.cat([-t[..., 32:], t[..., :32]], -1)
        out.append((t * cs + rot * sn).reshape(n, inner))
    return out


def check_qknorm_rope(got, qkv0, clips, gq, gk, heads):
    """got / qkv0: the buffer after / before the launch (CPU), clips: [(first row, n)].  Returns (device distance, own, bar)."""
    inner = heads * 64
    assert torch.equal(got[:, 2 * inner:].view(torch.int32), qkv0[:, 2 * inner:].view(torch.int32))       # v: bitwise unchanged
    keep = torch.ones(qkv0.shape[0], dtype=torch.bool)
    dist = own = top = 0.0
    for s0, n in clips:
        keep[s0:s0 + n] = False
        cos_t, sin_t = rope_tables(n)
        ref = torch.cat(qknorm_rope_ref(qkv0[s0:s0 + n], gq, gk, cos_t, sin_t, heads, torch.float64), -1)
        r32 = torch.cat(qknorm_rope_ref(qkv0[s0:s0 + n], gq, gk, cos_t, sin_t, heads, torch.float32), -1)
        dist = max(dist, float((got[s0:s0 + n, :2 * inner].double() - ref).abs().max()))
        own = max(own, float((r32.double() - ref).abs().max()))
        top = max(top, float(ref.abs().max()))
    assert torch.equal(got[keep].view(torch.int32), qkv0[keep].view(torch.int32))                       # rows of no clip: unchanged
    return dist, own, 4 * own + ulp32(top)


def qknorm_operands(rows, heads, seed):
    qkv = rnd(rows, 3 * heads * 64, seed=seed, scale=2.0)
    return qkv, rnd(heads, 64, seed=seed + 1), rnd(heads, 64, seed=seed + 2)


@pytest.mark.parametrize("B,n,heads", [(1, 1, 1), (2, 3, 16), (1, 130, 16)])
def test_qknorm_rope_edges(B, n, heads):
    """fh_qknorm_rope_f32 against float64 F.normalize(x) * gamma * 8 and rotate-half with tables.rotary_tables; q head 0 of the
    first token is all zero (the eps path: its output is zero), v is bitwise unchanged.

    Bar = 4 x (largest distance of torch's fp32 CPU evaluation from float64 on these inputs) + one fp32 ulp of the largest output.
    Measured on an MI355X (reference's own fp32 distance / device distance / bar):
      (1, 1, 1)     3.642e-07 / 8.294e-07 / 1.934e-06
      (2, 3, 16)    9.144e-07 / 7.849e-07 / 4.134e-06
      (1, 130, 16)  1.402e-06 / 1.402e-06 / 6.560e-06"""
    qkv0, gq, gk = qknorm_operands(B * n, heads, 250 + n)
    if heads > 1:
        qkv0[0, :64] = 0.0
    qkv = qkv0.to(DEV)
    cos_t, sin_t = rope_tables(n)
    cd, sd, gqd, gkd = cos_t.to(DEV), sin_t.to(DEV), gq.to(DEV), gk.to(DEV)
    hip.check(hip.lib().fh_qknorm_rope_f32(qkv.data_ptr(), gqd.data_ptr(), gkd.data_ptr(), cd.data_ptr(), sd.data_ptr(), B, n, heads,
                                           hip.stream()), "qknorm_rope")
    torch.cuda.synchronize()
    got = qkv.cpu()
    dist, own, bar = check_qknorm_rope(got, qkv0, [(b * n, n) for b in range(B)], gq, gk, heads)
    print(f"qknorm_rope B={B} n={n} heads={heads}: reference's own fp32 distance {own:.3e}, device distance {dist:.3e}, bar {bar:.3e}")
    if heads > 1:
        assert float(got[0, :64].abs().max()) == 0.0
    assert dist <= bar


def test_qknorm_rope_seg_edges():
    """fh_qknorm_rope_seg_f32 on clips of 1, 5 and 130 tokens with rows of no clip before, between and after them: positions
    restart at 0 in every clip (float64 per clip), and v and the rows of no clip are bitwise unchanged.

    Bar as in test_qknorm_rope_edges.  Measured on an MI355X: reference's own fp32 distance 1.151e-06, device distance 1.035e-06,
    bar 5.558e-06."""
    heads, frames, gap = 16, [1, 5, 130], 3
    clips, row = [], gap
    for n in frames:
        clips.append((row, n))
        row += n + gap
    qkv0, gq, gk = qknorm_operands(row, heads, 260)
    qkv0[clips[1][0] + 2, 64 * heads + 128:64 * heads + 192] = 0.0                      # k head 2 of a token: the eps path
    qkv = qkv0.to(DEV)
    cos_t, sin_t = rope_tables(max(frames))
    cd, sd, gqd, gkd = cos_t.to(DEV), sin_t.to(DEV), gq.to(DEV), gk.to(DEV)
    seg = torch.tensor(clips, dtype=torch.int32).to(DEV)
    hip.check(hip.lib().fh_qknorm_rope_seg_f32(qkv.data_ptr(), gqd.data_ptr(), gkd.data_ptr(), cd.data_ptr(), sd.data_ptr(),
                                               seg.data_ptr(), len(frames), max(frames), heads, hip.stream()), "qknorm_rope seg")
    torch.cuda.synchronize()
    dist, own, bar = check_qknorm_rope(qkv.cpu(), qkv0, clips, gq, gk, heads)
    print(f"qknorm_rope seg {frames}: reference's own fp32 distance {own:.3e}, device distance {dist:.3e}, bar {bar:.3e}")
    assert dist <= bar


# ---- GEMV -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 252, 256, 260, 1024])
@pytest.mark.parametrize("N", [1, 3, 5, 1027])
def test_gemv_edges(N, K):
    """fh_gemv_f32: rows either side of the 4-row block, K of one lane, either side of the wave's 256-wide step and several steps;
    act 0 and 1 (SiLU), with and without bias, a sentinel after y[N - 1]."""
    w, x, b = rnd(N, K, seed=270 + K, scale=K ** -0.5), rnd(K, seed=271), rnd(N, seed=272)
    wd, xd, bd = w.to(DEV), x.to(DEV), b.to(DEV)
    for bias in (None, b):
        lin = F.linear(x.double(), w.double(), None if bias is None else bias.double())
        for act, ref in ((0, lin), (1, F.silu(lin))):
            y = sentinel(N + 5)
            hip.check(hip.lib().fh_gemv_f32(wd.data_ptr(), xd.data_ptr(), None if bias is None else bd.data_ptr(), y.data_ptr(), N, K,
                                            act, hip.stream()), "gemv")
            torch.cuda.synchronize()
            assert is_sentinel(y[N:])
            assert maxdiff(y[:N], ref) <= 5e-6


# ---- sums in a fixed order ----------------------------------------------------------------------------------------------------
SUM_NS = [4, 1020, 1024, 1028, 4100]


def mixed(n, seed):
    """Values of magnitudes 1e-3 .. 1e4: (a + b) + c depends on the order at almost every element."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 7 - 3)


def ordered_sum(srcs, scale):
    """fp32 (((s0 + s1) + s2) + ...) * scale, left to right."""
    v = srcs[0].clone()
    for s in srcs[1:]:
        v = v + s
    return v * torch.tensor(scale, dtype=torch.float32)


def assert_bits(got, exp, what):
    assert torch.equal(got.cpu().view(torch.int32), exp.view(torch.int32)), what


def test_the_sum_inputs_depend_on_the_order():
    """The design of the three tests below: with these values another order of addition changes bits."""
    s = [mixed(4100, 280 + i) for i in range(3)]
    assert not torch.equal(ordered_sum(s, 1.0), ordered_sum(s[::-1], 1.0))
    assert not torch.equal(ordered_sum(s, 1.0), s[0] + (s[1] + s[2]))


@pytest.mark.parametrize("n", SUM_NS)
def test_mean_is_the_fixed_order_sum(n):
    """fh_mean_f32 = ((a + b) + c) * scale bitwise, two and three sources, a sentinel after the output."""
    s = [mixed(n, 280 + i) for i in range(3)]
    d = [t.to(DEV) for t in s]
    for k in (2, 3):
        scale = 1.0 / k
        out = sentinel(n + 8)
        hip.check(hip.lib().fh_mean_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if k == 3 else None, out.data_ptr(), n, scale,
                                        hip.stream()), "mean")
        torch.cuda.synchronize()
        assert is_sentinel(out[n:])
        assert_bits(out[:n], ordered_sum(s[:k], scale), f"mean of {k}, n={n}")


@pytest.mark.parametrize("n", SUM_NS)
def test_sum_is_the_fixed_order_sum(n):
    """fh_sum_f32 = (((s0 + s1) + s2) + ...) * scale bitwise for 1, 2 and 12 sources."""
    s = [mixed(n, 300 + i) for i in range(12)]
    d = [t.to(DEV) for t in s]
    for k, scale in ((1, 1.0), (2, 0.5), (12, 1.0 / 3)):
        arr = (C.c_void_p * k)(*[t.data_ptr() for t in d[:k]])
        out = sentinel(n + 8)
        hip.check(hip.lib().fh_sum_f32(arr, k, out.data_ptr(), n, scale, hip.stream()), "sum")
        torch.cuda.synchronize()
        assert is_sentinel(out[n:])
        assert_bits(out[:n], ordered_sum(s[:k], scale), f"sum of {k}, n={n}")


def test_sum_multi_is_the_fixed_order_sum_per_job():
    """fh_sum_multi_f32: jobs of different n and source counts in one launch (max_n the longest), each its own scale and its
    own sentinel-guarded output."""
    shapes = [(4, 1, 1.0), (1020, 3, 1.0 / 3), (4100, 12, 0.25), (1028, 2, 0.5), (1024, 5, 1.0 / 7)]
    jobs, keep, exp, outs = [], [], [], []
    for i, (n, k, scale) in enumerate(shapes):
        s = [mixed(n, 320 + 12 * i + j) for j in range(k)]
        d = [t.to(DEV) for t in s]
        out = sentinel(n + 8)
        j = hip.SumJob()
        for q, t in enumerate(d):
            j.src[q] = t.data_ptr()
        j.out, j.n, j.n_src, j.scale = out.data_ptr(), n, k, scale
        jobs.append(j)
        keep.append(d)
        outs.append(out)
        exp.append(ordered_sum(s, scale))
    desc = hip.to_device_struct_array(jobs, DEV)
    hip.check(hip.lib().fh_sum_multi_f32(desc.data_ptr(), len(jobs), max(n for n, _, _ in shapes), hip.stream()), "sum_multi")
    torch.cuda.synchronize()
    for (n, k, _), out, e in zip(shapes, outs, exp):
        assert is_sentinel(out[n:])
        assert_bits(out[:n], e, f"job of {k} sources, n={n}")
