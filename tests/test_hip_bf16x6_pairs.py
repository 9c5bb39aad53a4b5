"""The bf16 x 6 property, by construction: every fp32 operand is split exactly into h + m + l (round to nearest even) and every
product is the sum of the six piece-pair MFMAs h h, h m, m h, h l, l h, m m.  The four kernels that implement it share one device
split and two pair schedules (bf16x6.h) but each feeds them its own way (gemm_bf.hip, narrow_bf.hip, conv_wino.hip's BF path,
conv_wino54_kernel.h <BF>), and their random-input tests sit at tolerances a lost small pair (2^-16 .. 2^-18 of a product) lands
right on.  Here every output is one exact product chain, so each test asserts equality:

  * the weights' three piece planes are written by the test with ONE slot filled (the others zero).  With an activation
    a = a_h + a_m + a_l the kept pairs make the result sum a v (slot h: pairs h h, m h, l h), sum (a_h + a_m) v (slot m: h m, m m)
    or sum a_h v (slot l: h l) -- each of the six pairs decides a known part of some output, and the slot m / l results pin the
    device split's a_h and a_m themselves (a truncating split gives other pieces for negative residuals);
  * activations are designed (designed_values: known pieces in 20 significant bits, both signs, both residual signs, binades
    2^-60 .. 2^60), weights have one or two significant bits;
  * direct kernels (GEMM, narrow-stage conv): one nonzero weight per output row / channel;
    Winograd kernels: a single power-of-two transform-domain weight U per output channel (one input channel, tap group and
    transform point) and input impulses spaced so that every tile's window holds exactly one: B^T d = b a, y = A^T U b a, with
    the float64 emulation of the kernel's own A^T, B^T and tile grid (wino_emulate; tests/tools/winograd_numerics.py's
    transforms) as the expected value.
The CPU tests check the construction itself: the packers' one split (packing.split_pieces) keeps every byte, the designed values
split as intended, and the emulation is the conv for U = G w."""
import sys
from fractions import Fraction
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
from flowhigh_amd import hip, packing          # noqa: E402
from flowhigh_amd import vocoder as V          # noqa: E402
from winograd_numerics import toom_cook        # noqa: E402

DEV = "cuda:0"
SLOTS = (0, 1, 2)                              # the weight piece that holds the value: h, m, l
H_ = Fraction(1, 2)
F43 = (4, 3, toom_cook(4, 3, [0, 1, -1, 2, -2]))                 # (outputs m, taps r, (A^T, G, B^T)) of conv_wino.hip
F54 = (5, 4, toom_cook(5, 4, [0, 1, -1, 2, -2, H_, -H_]))         # ... of conv_wino54_kernel.h


# ---- designed operands ---------------------------------------------------------------------------------------------------
def designed_values(n, seed):
    """(a, (a_h, a_m, a_l)) float32 [n]: a = s 2^e [(1 + i/128) + t_m 2^-9 (1 + j/128) + t_l 2^-18 (1 + k/2)], i in 1..127,
    j in 1..126, k in 0..1, signs s, t_m, t_l = +-1, e in {-60, -30, -1, 0, 3, 30, 60}.  The three terms are the round-to-nearest-even
    pieces with no tie on the way (|m + l| < half an ulp of h, |l| < half an ulp of m, neither h nor m a power of two), and a is
    exact in 20 bits.  t_m = -1 or t_l = -1 is a negative residual: a truncating split gives other pieces."""
    g = torch.Generator().manual_seed(seed)
    ex = torch.tensor([-60, -30, -1, 0, 3, 30, 60], dtype=torch.float64)
    e = ex[torch.randint(len(ex), (n,), generator=g)]
    sgn = lambda: torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    s, tm, tl = sgn(), sgn(), sgn()
    i = torch.randint(1, 128, (n,), generator=g).double()
    j = torch.randint(1, 127, (n,), generator=g).double()
    k = torch.randint(0, 2, (n,), generator=g).double()
    p2 = torch.pow(2.0, e)
    h = s * p2 * (1 + i / 128)
    m = s * tm * p2 * 2.0 ** -9 * (1 + j / 128)
    lo = s * tl * p2 * 2.0 ** -18 * (1 + k / 2)
    return (h + m + lo).float(), (h.float(), m.float(), lo.float())


def weight_values(n, seed):
    """+-2^t {1, 1.5}, t in -3 .. 3: one or two significant bits (bf16-exact, products with designed values stay exact)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-3, 4, (n,), generator=g).double()
    mant = torch.where(torch.rand(n, generator=g) < 0.5, 1.0, 1.5)
    s = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (s * mant * torch.pow(2.0, t)).float()


def pow2_values(n, seed):
    """+-2^t, t in -2 .. 2 (the transform-domain weights of the Winograd tests)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-2, 3, (n,), generator=g).double()
    s = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (s * torch.pow(2.0, t)).float()


def slot_sum(pieces, slot):
    """What the kept pairs make of an activation against a weight in `slot`: h -> a_h + a_m + a_l, m -> a_h + a_m, l -> a_h."""
    h, m, lo = (p.double() for p in pieces)
    return (h + m + lo, h + m, h)[slot]


def slot_split(slot):
    """Stand-in for packing.split_pieces: the (bf16-exact) value in piece `slot`, zero in the other two."""
    def split(x):
        v = x.float().to(torch.bfloat16)
        assert torch.equal(v.float(), x.float()), "slot weights must be bf16-exact"
        z = torch.zeros_like(v)
        return tuple(v if i == slot else z for i in SLOTS)
    return split


def slot_planes(u, slot):
    """fp32 [..., 16] of bf16-exact values -> the three-piece int16 tensor [..., 3, 16] with only `slot` filled."""
    return torch.stack(slot_split(slot)(u), dim=-2).contiguous().view(torch.int16)


def trunc_split(x):
    """The split a kernel that truncates instead of rounding would make (for the CPU test of the designed values)."""
    cut = lambda v: (v.float().view(torch.int32) & -65536).view(torch.float32)
    h = cut(x)
    r = x.float() - h
    m = cut(r)
    return h, m, cut(r - m)


def assert_same(got, exp, what):
    got = got.detach().cpu()
    if not torch.equal(got, exp):
        bad = (got != exp) | (torch.isnan(got) != torch.isnan(exp))
        i = tuple(int(t) for t in bad.nonzero()[0])
        err = (got.double() - exp.double()).abs()
        rel = float((err / exp.double().abs().clamp_min(1e-300))[bad].nan_to_num(float("inf")).min())
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ (first at {i}: {float(got[i])!r} against "
                    f"{float(exp[i])!r}; smallest relative miss {rel:.2e})")


# ---- the Winograd kernels' arithmetic, emulated --------------------------------------------------------------------------
def wino_emulate(x, U, d, form, center, slot=None):
    """float64 model of a Winograd launch: x [B, Ci, L] (float64), U [G, n, Co, Ci] transform-domain weights -> y [B, Co, L].
    Per phase p of the dilation, tile t holds outputs m t .. m t + m - 1 of the decimated row; tap group g reads samples
    m t + r g - center + j (zero outside the row), V = B^T d.  slot None: V in float64 (the conv itself for U = G w); else V is
    the kernel's fp32 value, split into the host pieces, and only the pairs of `slot` are kept (slot_sum)."""
    m, r, (at, _, bt) = form
    n = m + r - 1
    B, Ci, L = x.shape
    G = U.shape[0]
    y = torch.zeros(B, U.shape[2], L, dtype=torch.float64)
    for p in range(d):
        xp = x[..., p::d]
        lp = xp.shape[-1]
        T = -(-lp // m)
        xq = F.pad(xp, (center, m * T + r * G + n))
        M = 0
        for g in range(G):
            win = xq[..., r * g:].unfold(-1, n, m)[:, :, :T, :]                    # [B, Ci, T, n]
            v = torch.einsum("xj,bctj->xbct", bt, win)
            if slot is not None:
                assert int((win != 0).sum(-1).max()) <= 1, "a window with more than one impulse: V would not be one rounding"
                v = slot_sum(packing.split_pieces(v.float()), slot)
            M = M + torch.einsum("xoc,xbct->xbot", U[g], v)
        y[..., p::d] = torch.einsum("ix,xbot->boti", at, M).reshape(B, -1, m * T)[..., :lp]
    return y


def impulses(B, C, L, d, form, start_of, seed):
    """Input [B, C, L]: per channel and phase of the dilation, one designed value every 2 m samples, in the overlap of two
    neighbouring tile windows (offset m .. n - 1 from the even tile's window start start_of[ci] = r g - center): every window
    of that tap group holds exactly one (any window of n <= 2 m samples holds at most one)."""
    m, r, _ = form
    n = m + r - 1
    x = torch.zeros(B, C, L, dtype=torch.float64)
    vals = designed_values(B * C * L, seed)[0].double().view(B, C, L)
    for ci in range(C):
        o = start_of.get(ci, 0) + m + ci % (n - m)
        for p in range(d):
            pos = torch.arange(p, L, d)
            hit = pos[(torch.arange(pos.numel()) - o) % (2 * m) == 0]
            x[:, ci, hit] = vals[:, ci, hit]
    return x


def designed_u(C, G, n, center, r, seed, owns=lambda co: True):
    """Transform-domain weights [G, n, C, C]: per output channel co that `owns` ONE power-of-two entry at input channel
    (7 co + 3) % C, tap group co % G, transform point co % n; returns (U, start_of: the window start r g - center of each
    input channel's group)."""
    assert C % 7, "(7 co + 3) % C must reach every input channel"
    vals = pow2_values(C, seed).double()
    U = torch.zeros(G, n, C, C, dtype=torch.float64)
    start_of = {}
    for co in range(C):
        if owns(co):
            ci, g, xi = (7 * co + 3) % C, co % G, co % n
            U[g, xi, co, ci] = vals[co]
            start_of[ci] = r * g - center
    return U, start_of


def wino_planes(U, cpad, slot):
    """[G, n, C, C] -> the kernels' three-piece layout [C/16, G, n, cpad, 3, 16] with the values in piece `slot`."""
    G, n, co, ci = U.shape
    u = torch.zeros(ci // 16, G, n, cpad, 16, dtype=torch.float32)
    u[:, :, :, :co] = U.float().reshape(G, n, co, ci // 16, 16).permute(3, 0, 1, 2, 4)
    return slot_planes(u, slot)


# ---- CPU: the construction --------------------------------------------------------------------------------------------------
def _old_split(x):
    x = x.float()
    h = x.to(torch.bfloat16)
    r = x - h.float()
    m = r.to(torch.bfloat16)
    return h, m, (r - m.float()).to(torch.bfloat16)


def _split_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-100, 101, shape, generator=g).float())
    flat = x.view(-1)
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -100, 2.0 ** 100, -(2.0 ** 37), 2.0 ** -126,
                         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -24,
                         1 - 2.0 ** -9, (1 + 2.0 ** -8) * 2.0 ** 50, 3.0, 0.1, -1e-30])
    flat[:edge.numel()] = edge
    bits = torch.randint(0x0100, 0x7e00, (64,), generator=g).int() | (torch.randint(0, 2, (64,), generator=g).int() << 15)
    ties = (bits << 16 | 0x8000).view(torch.float32)                                  # halfway between two bf16 values
    flat[edge.numel():edge.numel() + 64] = ties
    return x


def test_packers_are_byte_identical_to_the_three_split_formulas():
    """packing.split_pieces replaced the split written out in pack_gemm_bf_weight, pack_narrow_bf_weight and split_bf3: every
    packer's output keeps its bytes (the weight blob layout, weights.format_tag, is unchanged)."""
    w = _split_inputs((128, 96), 1)
    h, m, lo = _old_split(w)
    old = torch.stack([h, m, lo], dim=0).view(3, 2, 64, 3, 4, 8).permute(1, 3, 0, 4, 2, 5).contiguous().view(torch.int16)
    assert torch.equal(packing.pack_gemm_bf_weight(w).view(torch.int16), old.reshape(-1))
    u = _split_inputs((4, 3, 6, 96, 16), 2)
    assert torch.equal(packing.split_bf3(u), torch.stack(_old_split(u), dim=-2).contiguous().view(torch.int16))
    for C, k in ((24, 11), (48, 7), (40, 3), (8, 5)):
        w = _split_inputs((C, C, k), 3 + C)
        new = packing.pack_narrow_bf_weight(w, C)
        saved = packing.split_pieces
        try:
            packing.split_pieces = _old_split
            ref = packing.pack_narrow_bf_weight(w, C)
        finally:
            packing.split_pieces = saved
        assert torch.equal(new.view(torch.int16), ref.view(torch.int16))
    x = _split_inputs((4096,), 4)
    for a, b in zip(packing.split_pieces(x), _old_split(x)):
        assert a.dtype == torch.bfloat16 and torch.equal(a.view(torch.int16), b.view(torch.int16))
    h, m, lo = packing.split_pieces(x)
    assert torch.equal(h.double() + m.double() + lo.double(), x.double())


def test_designed_values_split_as_intended():
    a, pieces = designed_values(20000, 5)
    assert torch.equal(sum(p.double() for p in pieces), a.double())                  # exact in fp32
    got = packing.split_pieces(a)
    for gp, p in zip(got, pieces):
        assert torch.equal(gp.float(), p)
    r = a - pieces[0]
    for v in (a, r, r - pieces[1]):                                                    # no value on the way is a bf16 tie
        assert not bool(((v.view(torch.int32) & 0xFFFF) == 0x8000).any())
    th, tm, _ = trunc_split(a)
    neg = (pieces[1] * pieces[0] < 0) | (pieces[2] * pieces[1] < 0)
    differs = (th != pieces[0]) | (tm != pieces[1])
    assert torch.equal(differs, neg) and 0.4 < float(neg.double().mean()) < 0.9
    assert all(bool((p != 0).all()) for p in pieces)
    e = torch.frexp(a)[1]
    assert {int(v) for v in e.unique()} == {-59, -29, 0, 1, 4, 31, 61}
    w = weight_values(1000, 6)
    assert torch.equal(w.to(torch.bfloat16).float(), w) and bool((w != 0).all())


@pytest.mark.parametrize("form,G_pack", [(F43, packing._WINO_G), (F54, packing._WINO54_G)], ids=["F43", "F54"])
@pytest.mark.parametrize("k,d", [(3, 1), (7, 3), (11, 5), (11, 1), (4, 1)])
def test_wino_emulation_is_the_conv_for_U_of_the_packers_G(form, G_pack, k, d):
    """wino_emulate with U = G w (G: the packer's, pack_wino_weight / pack_wino54_weight) is F.conv1d: the emulation's A^T, B^T
    and tile grid are a Winograd conv with the kernel's transform scaling."""
    m, r, (at, gm, bt) = form
    assert torch.allclose(gm, torch.tensor(G_pack, dtype=torch.float64), rtol=0, atol=1e-15)
    G = -(-k // r)
    g = torch.Generator().manual_seed(k * 10 + d)
    x, w = torch.randn(2, 16, 203, generator=g, dtype=torch.float64), torch.randn(8, 16, k, generator=g, dtype=torch.float64)
    wp = F.pad(w, (0, r * G - k))
    U = torch.stack([torch.einsum("xj,ocj->xoc", gm, wp[:, :, r * gg:r * gg + r]) for gg in range(G)])
    for center in {(k - 1) // 2, 0, k - 1}:
        got = wino_emulate(x, U, d, form, center)
        ref = F.conv1d(F.pad(x, (center * d, (k - 1 - center) * d)), w, dilation=d)
        assert (got - ref).abs().max() < 1e-11


@pytest.mark.parametrize("form", [F43, F54], ids=["F43", "F54"])
@pytest.mark.parametrize("G,center,d", [(3, 5, 1), (2, 3, 3), (1, 0, 1), (3, 6, 5)])
def test_wino_impulses_put_one_value_in_every_window(form, G, center, d):
    """Every window of the owning tap group that lies inside the row holds exactly one designed value, so B^T d = b a exactly."""
    m, r, _ = form
    C, n, L = 16, m + r - 1, 301
    U, start_of = designed_u(C, G, n, center, r, 1)
    assert len(start_of) == C
    x = impulses(1, C, L, d, form, start_of, 2)
    for ci, s0 in start_of.items():
        for p in range(d):
            xp = x[0, ci, p::d]
            T = -(-xp.numel() // m)
            start = torch.arange(T) * m + s0
            inside = (start >= 0) & (start + n <= xp.numel())
            win = F.pad(xp, (n, m * T + n)).unfold(-1, n, 1)[start[inside] + n]
            assert bool(inside.any()) and torch.equal((win != 0).sum(-1), torch.ones(int(inside.sum()), dtype=torch.long))


# ---- GPU: the bf16 x 6 GEMM (gemm_bf.hip) ----------------------------------------------------------------------------------
def gemm_variant(M, N):
    """The tile variant fh_gemm_bf16x6_f32 launches for the LINEAR epilogue (gemm_bf.hip)."""
    cd = lambda a, b: -(-a // b)
    return "<1,1>" if cd(M, 64) * cd(N, 128) < 200 else "<1,2>" if cd(M, 128) * cd(N, 128) < 512 else "<2,2>"


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,variant", [(100, 192, 64, "<1,1>"), (1000, 2048, 96, "<1,2>"), (4100, 2048, 64, "<2,2>"),
                                           (37, 128, 32, "<1,1>")])
def test_gemm_bf16x6_every_pair(M, N, K, variant, monkeypatch):
    """C = A W^T with one nonzero weight per output column (at k = (37 n + 5) % K: every k position of the K loop's lanes), the
    weight in one piece slot at a time: C = A[:, k(n)] (the slot's pieces) v_n exactly."""
    assert gemm_variant(M, N) == variant
    a, pieces = designed_values(M * K, 10 + M)
    a, pieces = a.view(M, K), [p.view(M, K) for p in pieces]
    kap = (torch.arange(N) * 37 + 5) % K
    v = weight_values(N, 11 + N)
    n_pad = -(-N // 128) * 128
    w = torch.zeros(n_pad, K)
    w[torch.arange(N), kap] = v
    ad = a.to(DEV)
    for slot in SLOTS:
        monkeypatch.setattr(packing, "split_pieces", slot_split(slot))
        wd = packing.pack_gemm_bf_weight(w).to(DEV)
        out = torch.full((M, N), float("nan"), device=DEV)
        hip.gemm(ad, wd, out, M, N, K, bf=True)
        torch.cuda.synchronize()
        exp = (slot_sum(pieces, slot)[:, kap] * v.double()[None, :]).float()
        assert_same(out, exp, f"gemm {variant} M={M} N={N} K={K} weight slot {'hml'[slot]}")


# ---- GPU: the bf16 x 6 narrow-stage conv (narrow_bf.hip) -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("C", [8, 16, 24, 32, 40, 48])
def test_narrow_bf16x6_every_pair(C, k, d, monkeypatch):
    """Direct conv with one nonzero weight per output channel co (input channel (7 co + 3) % C, tap co % k): out[co, t] =
    x[ci, t + (tap - center) d] v_co exactly, every slab split of narrow_slabs, aligned (L % 4 == 0) and unaligned rows."""
    L = 300 + 37 * (C // 8) + k + d
    B = 2 if C in (24, 40) else 1
    x, pieces = designed_values(B * C * L, 20 + C + k + d)
    x, pieces = x.view(B, C, L), [p.view(B, C, L) for p in pieces]
    co = torch.arange(C)
    ci, tap = (7 * co + 3) % C, co % k
    assert sorted(ci.tolist()) == list(range(C))            # (7 is prime to every C here: each input channel carries one weight)
    v = weight_values(C, 21 + C)
    w = torch.zeros(C, C, k)
    w[co, ci, tap] = v
    c = (k - 1) // 2
    xd = x.to(DEV)
    for slot in SLOTS:
        monkeypatch.setattr(packing, "split_pieces", slot_split(slot))
        ud = packing.pack_narrow_bf_weight(w, C).to(DEV)
        out = torch.full_like(xd, float("nan"))
        g = V.make_amp_group([V.make_amp_seg(xd, ud, k, direct=True)], None, [], out, L, direct=True)
        keep = V.amp_actconv([g], B, C, d, DEV, direct=True)
        torch.cuda.synchronize()
        del keep
        src = F.pad(slot_sum(pieces, slot), (c * d, c * d))                                  # [B, C, L + 2 c d]
        exp = torch.stack([src[:, ci[o], tap[o] * d:tap[o] * d + L] for o in range(C)], dim=1) * v.double()[None, :, None]
        assert_same(out, exp.float(), f"narrow C={C} k={k} d={d} L={L} weight slot {'hml'[slot]}")


# ---- GPU: the Winograd kernels' BF paths -----------------------------------------------------------------------------------
def run_wino(form, cfg, C, ks, d, L, B, pm, seed):
    """One launch per weight slot against wino_emulate.  ks: taps of each K segment; output channel co's weight entry lives in
    segment co % len(ks) (the other segments meet it with zero weights)."""
    m, r, _ = form
    n = m + r - 1
    nseg = len(ks)
    Us, xs = [], []
    for s, k in enumerate(ks):
        U, start_of = designed_u(C, -(-k // r), n, (k - 1) // 2, r, seed + s, owns=lambda co, s=s: co % nseg == s)
        Us.append(U)
        xs.append(impulses(B, C, L, d, form, start_of, seed + 100 + s))
    to_dev = lambda t: (V.to_phase_major(t.float(), d) if pm else t.float()).to(DEV)
    xd = [to_dev(x) for x in xs]
    flag = V.WINO_BF16X6 | (V.WINO_F54 if form is F54 else 0)
    name = "F(5,4)" if form is F54 else "F(4,3)"
    for slot in SLOTS:
        exp = sum(wino_emulate(x, U, d, form, (k - 1) // 2, slot) for x, U, k in zip(xs, Us, ks)).float()
        ud = [wino_planes(U, C, slot).to(DEV) for U in Us]
        out = torch.full_like(xd[0], float("nan"))
        segs = [V.make_wino_seg(xd[s], ud[s], C, k, taps=r) for s, k in enumerate(ks)]
        keep = V.conv_wino([V.make_wino_group(segs, None, [], out, C, C, L)], B, C, L, d, DEV, cfg | flag, phase_major=pm)
        torch.cuda.synchronize()
        del keep
        got = V.from_phase_major(out.cpu(), d, L) if pm else out.cpu()
        assert_same(got, exp, f"{name} cfg {cfg & 15} C={C} ks={ks} d={d} L={L} B={B} pm={pm} weight slot {'hml'[slot]}")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,C,k,d,L,B,pm", [(0, 128, 11, 1, 1000, 1, False), (1, 96, 7, 3, 777, 2, True),
                                              (4, 64, 3, 1, 1203, 1, False), (5, 32, 11, 5, 901, 1, True),
                                              (6, 128, 7, 1, 640, 2, False), (0, 64, 7, 3, 500, 1, False),
                                              (4, 64, 11, 1, 64, 1, False)])
def test_wino43_bf16x6_every_pair(cfg, C, k, d, L, B, pm):
    """F(4,3) BF path (conv_wino.hip): the tile shapes the planner picks from (64 x 512, 96 x 256, 64 x 256, 32 x 256,
    128 x 256), plain and phase-major layouts, 16-byte and 4-byte loaders."""
    run_wino(F43, cfg, C, [k], d, L, B, pm, seed=cfg * 7 + k)


@pytest.mark.gpu
@pytest.mark.parametrize("u,k,lin,cfg", [(2, 8, 300, 0), (3, 7, 257, 4), (4, 8, 160, 0)])
def test_wino43_bf16x6_transposed_phase_groups(u, k, lin, cfg):
    """The upsamplers' Winograd phase groups (ConvTranspose1d(k, stride u) as u groups of one launch with strided stores
    u n + r), each with its phase's taps and center (transposed_conv_phases)."""
    C, B, form = 64, 1, F43
    m, r, _ = form
    n = m + r - 1
    phases = []
    for ph, taps in enumerate(V.transposed_conv_phases(k, u)):
        offs = sorted(o for _, o in taps)
        kr, center = len(offs), -offs[0]
        U, start_of = designed_u(C, -(-kr // r), n, center, r, 40 + ph)
        phases.append((kr, center, U, impulses(B, C, lin, 1, form, start_of, 50 + ph)))
    assert V.transposed_conv_extra(k, u) == 0
    for slot in SLOTS:
        X = torch.full((B, C, u * lin), float("nan"), device=DEV)
        exp = torch.zeros(B, C, u * lin, dtype=torch.float64)
        groups, keep = [], []
        for ph, (kr, center, U, x) in enumerate(phases):
            exp[..., ph::u] = wino_emulate(x, U, 1, form, center, slot)
            xd, ud = x.float().to(DEV), wino_planes(U, C, slot).to(DEV)
            keep += [xd, ud]
            groups.append(V.make_wino_group([V.make_wino_seg(xd, ud, C, kr, center)], None, [], X, C, C, lin, stride=u, phase=ph))
        keep.append(V.conv_wino(groups, B, C, lin, 1, DEV, cfg | V.WINO_BF16X6))
        torch.cuda.synchronize()
        assert_same(X, exp.float(), f"F(4,3) phase groups u={u} k={k} cfg {cfg} weight slot {'hml'[slot]}")
        del keep


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,C,ks,d,L,B,pm", [(1, 192, (11,), 1, 1000, 1, False), (2, 128, (7,), 3, 777, 2, True),
                                               (1, 96, (3, 11), 1, 1203, 1, False), (2, 64, (11,), 5, 1500, 1, False),
                                               (2, 192, (7, 3, 11), 1, 640, 2, False), (1, 96, (7,), 5, 333, 1, True),
                                               (2, 64, (3,), 1, 17, 1, False)])
def test_wino54_bf16x6_every_pair(cfg, C, ks, d, L, B, pm):
    """F(5,4) BF path (conv_wino54_kernel.h <BF>): 96- and 64-row blocks (the tile heights that have a bf16 x 6 form), plain
    and phase-major layouts, aligned and unaligned rows, one to three K segments."""
    run_wino(F54, V.WINO_F54 | cfg, C, list(ks), d, L, B, pm, seed=cfg * 11 + sum(ks))
