"""Exact constructions that pin the twelve piece-pair MFMAs of the bf16 x 6 attention kernel (attention_bf.hip), and their host
emulation.  Used by tests/test_attn_form_cpu.py (the constructions themselves) and tests/test_hip_attention_bf.py (the kernels).

Pairs are written (first MFMA operand's piece, second's): (K, Q) for S^T = K Q^T and (V, P) for O^T = V^T P^T; kept pairs are
those with i + j <= 2.  All inputs are token-major qkv [B n, 3 H 64] as the entries take them (H = 16).

  qk_case     one non-zero d per q and k row, values whose pieces have one or two significant bits: the six kept products and
              all their partial sums are exact in fp32, so the logit L is a known fp32 number whatever the accumulation order.  Two
              live keys per (clip, head); all other keys carry -64 against a 1 of q on another d, and exp2 of their logit is 0.
              The fp32 kernel fed q' = (L_1, L_2) on two d and unit keys has the same logits bit for bit, hence (same softmax code,
              one live key per output column, V a power of two) the same output: torch.equal between the kernels.
  v_case      q = 0: every P is exactly 1 (pieces 1, 0, 0); one non-zero V per output column, n a power of two: out = v / n.
  p_case      q, k small integers / 4 on a few d (one bf16 piece each: logits exact in both kernels), every key live, V a power of
              two on one key per column: both kernels see the same general P and p v is exact in both: torch.equal.
  vm_pm_case  two live keys with logits 0 and -a c (a in (0.005, 0.3): p of the second key general in (0.05, 0.95)); on that key
              V = 2^e (1 + 2^-8 - 2^-16) in one column (pieces 2^e, 2^e (2^-8 - 2^-16), 0), 2^e in the next: the second column
              is exact (p 2^e / l), so column 0 = (1 + 2^-8 - 2^-16) x column 1 up to the roundings listed at VM_PM_ULPS.
"""
import torch

H, DH = 16, 64
INNER = H * DH
DEAD = -64.0                     # k of a dead key on the marker d (q there is 1): logit -64 scale log2(e) <= -900 at scale 10
SCALE = 10.0                     # the model's (attend.py: qk-norm attention scale)
# vm_pm_case: |col0 - V col1| in ulps of col0.  col1 = fl(p fl(1/l)) is one rounding from p / l x (1 + the error of inv), col0 =
# fl(o fl(1/l)) with o the six-pair sum of p V: its dropped pair V.m p.l is < 2^-8 2^-16 = 2^-24 of p V (half an ulp), the
# accumulation of the five small pairs rounds at their own size (< 2^-8 of the result: nothing), the last addition rounds once
# (half an ulp), and the two final multiplications by inv round once each (half an ulp each; inv's own error cancels).  2 ulps
# in all, 3 with the product V col1 taken in float64 from a rounded col1.  Without the (V.m, P.m) pair the miss is p.m V.m, up to
# 2^-16 of the result = 128 ulps.
VM_PM_ULPS = 3.0
C_LOG2E = 1.44269504088896340736


def split3(x):
    """The device split (bf16x6.h: round to nearest even, exact residuals), on the host: float32 pieces h, m, l."""
    x = x.float()
    h = x.to(torch.bfloat16).float()
    r = x - h
    m = r.to(torch.bfloat16).float()
    return h, m, (r - m).to(torch.bfloat16).float()


def split3_trunc(x):
    cut = lambda v: (v.float().view(torch.int32) & -65536).view(torch.float32)
    h = cut(x)
    r = x.float() - h
    m = cut(r)
    return h, m, cut(r - m)


def split3_l0(x):
    h, m, _ = split3(x)
    return h, m, torch.zeros_like(h)


KEPT = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]


def six(a_pieces, b_pieces, drop=None):
    """float64 sum of the kept piece products (every product is exact in float64; so is the sum for the designed values)."""
    tot = 0.0
    for i, j in KEPT:
        if (i, j) != drop:
            tot = tot + a_pieces[i].double() * b_pieces[j].double()
    return tot


def two_bit_values(n, seed, signed=True):
    """float32 [n] values s (h0 + t_m 2^-9 m0 + t_l 2^-18 l0), h0, m0, l0 in {1, 1.5}, s, t_m, t_l = +-1, kept only where the
    round-to-nearest-even split gives exactly those three pieces (a negative residual under a power-of-two piece would not).
    Products of two such values' pieces have <= 4 significant bits between 2^1 and 2^-38: the six kept ones sum exactly."""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(0)
    while out.numel() < n:
        k = 4 * n + 64
        pick = lambda: torch.where(torch.rand(k, generator=g) < 0.5, 1.0, 1.5).double()
        sgn = lambda: torch.randint(0, 2, (k,), generator=g).double() * 2 - 1
        s = sgn() if signed else torch.ones(k, dtype=torch.float64)
        h, m, lo = s * pick(), s * sgn() * pick() * 2.0 ** -9, s * sgn() * pick() * 2.0 ** -18
        a = (h + m + lo).float()
        ph, pm, pl = split3(a)
        ok = (ph.double() == h) & (pm.double() == m) & (pl.double() == lo)
        out = torch.cat([out, a[ok]])
    return out[:n]


def qk_case(B, n, seed):
    """-> dict(bf=qkv for the bf16 x 6 kernel, f32=qkv for the fp32 kernel, L=float64 [B, H, n, 2] logits before the scale,
    live=[B, H, 2] key positions, vcol=float64 [B, H, 2] the V values of the two keys (even / odd columns))."""
    g = torch.Generator().manual_seed(seed)
    bf = torch.zeros(B, n, 3, H, DH)
    f32 = torch.zeros(B, n, 3, H, DH)
    a = two_bit_values(B * n * H, seed + 1).view(B, n, H)
    bk = two_bit_values(B * H * 2, seed + 2, signed=False).view(B, H, 2)
    # the second key at half / a quarter of the first's size: a pair lost on both keys must not cancel in L_1 - L_2
    bk[:, :, 1] *= torch.where(torch.rand(B, H, generator=g) < 0.5, 0.5, 0.25)
    live = torch.stack([torch.randperm(n, generator=g)[:2] for _ in range(B * H)]).view(B, H, 2)
    d0 = torch.randint(0, DH, (B, H), generator=g)
    d1, d2 = (d0 + 1 + torch.randint(0, 20, (B, H), generator=g)) % DH, (d0 + 30 + torch.randint(0, 20, (B, H), generator=g)) % DH
    ve = torch.randint(-3, 4, (B, H, 2), generator=g).double()
    vcol = torch.pow(2.0, ve)
    L = torch.zeros(B, H, n, 2, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            ap = split3(a[b, :, h])
            for j in range(2):
                L[b, h, :, j] = six(split3(bk[b, h, j].expand(n)), ap)            # (K piece, Q piece)
            e0, e1, e2 = int(d0[b, h]), int(d1[b, h]), int(d2[b, h])
            bf[b, :, 0, h, e0] = a[b, :, h]
            bf[b, :, 0, h, e2] = 1.0
            f32[b, :, 0, h, e0] = L[b, h, :, 0].float()
            f32[b, :, 0, h, e1] = L[b, h, :, 1].float()
            f32[b, :, 0, h, e2] = 1.0
            junk = torch.randn(n, DH, generator=g)                                # dead keys' V: their P is exactly 0
            for t in (bf, f32):
                t[b, :, 1, h, e2] = DEAD
                t[b, :, 2, h, :] = junk
            for j in range(2):
                kj = int(live[b, h, j])
                bf[b, kj, 1, h, :] = 0.0
                f32[b, kj, 1, h, :] = 0.0
                bf[b, kj, 1, h, e0] = bk[b, h, j]
                f32[b, kj, 1, h, (e0, e1)[j]] = 1.0
                for t in (bf, f32):
                    t[b, kj, 2, h, :] = 0.0
                    t[b, kj, 2, h, j::2] = vcol[b, h, j].float()
    assert torch.equal(L.float().double(), L), "a designed logit is not an fp32 number"
    return dict(bf=bf.view(B * n, 3 * INNER), f32=f32.view(B * n, 3 * INNER), L=L, live=live, vcol=vcol)


def qk_expected(case, scale=SCALE):
    """float64 output [B, n, H, 64] of qk_case from its logits (softmax over the two live keys)."""
    L, vcol = case["L"], case["vcol"]
    p = torch.softmax(L * scale, dim=-1)                                          # [B, H, n, 2]
    B, Hh, n, _ = L.shape
    out = torch.zeros(B, n, Hh, DH, dtype=torch.float64)
    for j in range(2):
        out[..., j::2] = (p[..., j] * vcol[:, :, None, j]).permute(0, 2, 1)[..., None]
    return out.view(B * n, INNER)


def v_case(B, n, seed, values):
    """q = k = 0; column d of (clip b, head h) has its one non-zero V at key (7 d + 13 h + 5 b) % n.  values: float32 [B, H, 64].
    -> (qkv, expected float32 [B n, H 64] = v / n on every row)."""
    assert n & (n - 1) == 0, "n must be a power of two: 1 / n and v / n are exact"
    qkv = torch.zeros(B, n, 3, H, DH)
    d = torch.arange(DH)
    for b in range(B):
        for h in range(H):
            qkv[b, (7 * d + 13 * h + 5 * b) % n, 2, h, d] = values[b, h]
    exp = (values.double() / n).float().view(B, 1, INNER).expand(B, n, INNER).reshape(B * n, INNER)
    assert torch.equal(exp.double() * n, values.double().view(B, 1, INNER).expand(B, n, INNER).reshape(B * n, INNER))
    return qkv.view(B * n, 3 * INNER), exp


def p_case(B, n, seed):
    """-> (qkv, logits float64 [B, H, n, n] before the scale, key_of float [B, H, 64], vpow float64 [B, H, 64])."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.zeros(B, n, 3, H, DH)
    live_d = torch.rand(B, 1, H, DH, generator=g) < 0.125                       # ~8 of the 64 d carry the logits
    qkv[:, :, 0] = torch.randint(-1, 2, (B, n, H, DH), generator=g).float() * 0.25 * live_d
    qkv[:, :, 1] = torch.randint(-2, 3, (B, n, H, DH), generator=g).float() * 0.25 * live_d
    key_of = torch.randint(0, n, (B, H, DH), generator=g)
    vpow = torch.pow(2.0, torch.randint(-3, 4, (B, H, DH), generator=g).double())
    d = torch.arange(DH)
    for b in range(B):
        for h in range(H):
            qkv[b, key_of[b, h], 2, h, d] = vpow[b, h].float()
    q, k = qkv[:, :, 0].double().permute(0, 2, 1, 3), qkv[:, :, 1].double().permute(0, 2, 1, 3)
    logits = torch.einsum("bhid,bhjd->bhij", q, k)
    return qkv.view(B * n, 3 * INNER), logits, key_of, vpow


def p_expected(logits, key_of, vpow, scale=SCALE):
    p = torch.softmax(logits * scale, dim=-1)                                     # [B, H, n, n]
    B, Hh, n, _ = p.shape
    idx = key_of[:, :, None, :].expand(B, Hh, n, DH)
    return (torch.gather(p, 3, idx) * vpow[:, :, None, :]).permute(0, 2, 1, 3).reshape(B * n, INNER)


VM_FACTOR = 1.0 + 2.0 ** -8 - 2.0 ** -16


def vm_pm_case(B, n, seed):
    """-> (qkv, exps float64 [B, H]): per (clip, head) keys j1 (logit 0) and j2 (logit -a_i), V of j2 = 2^e VM_FACTOR in column
    0, 2^e in column 1, 2^e VM_FACTOR in columns 2.. (more samples of the same product); V of j1 = 0."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.zeros(B, n, 3, H, DH)
    a = (0.005 + 0.295 * torch.rand(B, n, H, generator=g)).float()
    exps = torch.randint(-3, 4, (B, H), generator=g).double()
    for b in range(B):
        for h in range(H):
            j1, j2 = torch.randperm(n, generator=g)[:2].tolist()
            d0, d2 = torch.randperm(DH, generator=g)[:2].tolist()
            qkv[b, :, 0, h, d0] = a[b, :, h]
            qkv[b, :, 0, h, d2] = 1.0
            qkv[b, :, 1, h, d2] = DEAD
            qkv[b, :, 2, h, :] = torch.randn(n, DH, generator=g)
            for j in (j1, j2):
                qkv[b, j, 1, h, :] = 0.0
                qkv[b, j, 2, h, :] = 0.0
            qkv[b, j2, 1, h, d0] = -1.0
            v = 2.0 ** float(exps[b, h])
            qkv[b, j2, 2, h, :] = v * VM_FACTOR
            qkv[b, j2, 2, h, 1] = v
    return qkv.view(B * n, 3 * INNER), exps


def ulp(x):
    """fp32 unit in the last place of |x| (float64 tensor in, float64 out)."""
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


# ---- host emulation of the row arithmetic the pins lean on -------------------------------------------------------------------
def emulate_pv(p, v, drop=None, split=split3):
    """fp32 emulation of one output of O^T = V^T P^T with one live key: the six (V piece, P piece) products added in the
    kernel's order (kBf16x6SmallFirst), one fp32 rounding per MFMA.  p, v float32 tensors -> float32."""
    vp, pp = split(v), split(p)
    acc = torch.zeros_like(p, dtype=torch.float32)
    for i, j in [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]:
        if (i, j) != drop:
            acc = (acc.double() + vp[i].double() * pp[j].double()).float()
    return acc
