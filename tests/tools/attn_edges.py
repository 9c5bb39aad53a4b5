"""The full attention kernels at their edges: input constructions, references, an fp32 host restatement of the kernels' frame that
takes named mutants, and the assertions tests/test_hip_attention_edges.py makes -- written once here so that
tests/test_attn_edges_cpu.py can show on the host that the unmutated restatement passes every one of them and that every mutant
fails one (the table: profiles/attention_edges.md).  Host only: torch and numpy.

A "runner" is what a check drives: an object with
    batched(qkv, out, row_off, B, n, heads, scale)   rows [row_off, row_off + B n) of `out` <- attention of qkv [B n, 3 heads 64]
    seg(qkv, out, clips, max_n, heads, scale)        clips = [(row0, n), ...]: rows of qkv AND of out
    device                                           where the tensors it is given live
The GPU tests' runners call the C entries; EmulatedRunner calls attention_emulated's core."""
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

DH = 64                                        # dim_head
N_EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 257]
N_F64 = [1, 33, 64, 65, 129, 193, 257]
HEADS = [1, 3, 16]
UNIFORM_C = [0, 64, -64]
F64_BUILDERS = ["ramp", "offset+", "offset-", "model_like", "soft"]
SEG_LENS = [65, 1, 0, 128, 33, 257, 64]
SEG_GAP = 37                                   # rows between two clips of the segment test (NaN in qkv, sentinel in out)
GUARD_ROWS = 128                               # sentinel rows in front of and behind out
SENTINEL = 0x7FC5A5A5                          # a quiet NaN with a payload no kernel produces
LAUNCH_THRESHOLD = 512                         # launch_attention: cdiv(n, 128) heads batch >= 512 -> SPLIT = 1 (128 queries per block)
MAX_LOGIT2 = 1000.0                            # the entries' contract here: |scale log2(e) q.k| <= 1000
GATHER_GAP2 = 200.0                            # base-2 logit gap below which exp2 is 0 in fp32, denormals included (2^-149)
BAR_FACTOR = 3.0                               # a kernel may be 3 x the plain fp32 reference's own error (test_hip_regimes.py's margin)
BAR_FLOOR_ULPS = 8.0                           # ... or 8 fp32 ulps of max |V| where that reference is (nearly) exact
MUTANTS = ("key_order", "mask_le", "whole_off_by_one", "skip_last_odd_tile", "drop_stream1", "no_corr", "corr_skip_any",
           "store_past_n", "head_pitch", "seg_reads_neighbour")
LOG2E = 1.44269504088896340736


def cdiv(a, b):
    return -(-a // b)


def is_large(n, heads, batch):
    """launch_attention's rule (attention_softmax.h)."""
    return cdiv(n, 128) * heads * batch >= LAUNCH_THRESHOLD


def batch_across_threshold(n, heads):
    """The smallest batch that takes the SPLIT = 1 shape."""
    return cdiv(LAUNCH_THRESHOLD, cdiv(n, 128) * heads)


def split_heads(qkv, B, n, heads):
    """qkv [B n, 3 heads 64] -> q, k, v [B, heads, n, 64] (views)."""
    x = qkv.view(B, n, 3, heads, DH)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


# ---- references ----------------------------------------------------------------------------------------------------------------
def _attention_plain(qkv, B, n, heads, scale, dtype):
    q, k, v = (t.to(dtype) for t in split_heads(qkv.cpu(), B, n, heads))
    out = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v                   # [B, heads, n, 64]
    return out.permute(0, 2, 1, 3).reshape(B * n, heads * DH)


def attention_f64(qkv, B, n, heads, scale):
    """float64 softmax attention of the tensor the kernel reads."""
    return _attention_plain(qkv, B, n, heads, scale, torch.float64)


def attention_fp32_plain(qkv, B, n, heads, scale):
    """The yardstick: softmax(q k^T scale) v in fp32 torch -- the noise an honest fp32 implementation has on that tensor."""
    return _attention_plain(qkv, B, n, heads, scale, torch.float32)


# ---- the kernels' frame in fp32 on the host (after attention_softmax.h) -----------------------------------------------------------
KEY_ORDER_PERM = torch.arange(32) ^ 4          # mutant key_order: the V rows of the two lane halves of a k-step exchanged


def _load(flat, rows, row0, ld, off, heads):
    """[heads, len(rows), 64] <- flat[(row0 + row) ld + off + 64 h + d]: the kernels' address, wrapped into the buffer (only the
    head_pitch mutant leaves it)."""
    idx = ((row0 + rows)[None, :, None] * ld + off + torch.arange(heads)[:, None, None] * DH + torch.arange(DH)[None, None, :])
    return flat[idx % flat.numel()]


def _emulate_clip(flat, row0, n, nk, heads, scale2, mutant, qb):
    """One clip: its queries padded to whole blocks of qb (rows past n hold q = 0, as in the kernel), keys [0, nk).
    Returns [padded queries, heads 64]."""
    inner = 1024 if mutant == "head_pitch" else heads * DH             # (the mutant: heads = 16 built into the pitches)
    ld = 3 * inner
    nq = cdiv(n, qb) * qb
    qrows = torch.arange(nq)
    q = _load(flat, qrows.clamp(max=n - 1), row0, ld, 0, heads)
    q = torch.where((qrows < n)[None, :, None], q, torch.zeros(()))
    m = [torch.full((heads, nq), -float("inf")) for _ in range(2)]
    l = [torch.zeros(heads, nq) for _ in range(2)]
    o = [torch.zeros(heads, nq, DH) for _ in range(2)]
    for k0 in range(0, nk, 32):
        kb, sp = k0 // 64 * 64, (k0 // 32) & 1
        if sp == 1 and mutant == "skip_last_odd_tile" and not kb + 64 <= nk:
            continue
        keys = k0 + torch.arange(32)
        staged = keys < nk                                                              # load_kv's guard: other rows are 0
        kt = torch.where(staged[None, :, None], _load(flat, keys.clamp(max=nk - 1), row0, ld, inner, heads), torch.zeros(()))
        vt = torch.where(staged[None, :, None], _load(flat, keys.clamp(max=nk - 1), row0, ld, 2 * inner, heads), torch.zeros(()))
        s = (q @ kt.transpose(-1, -2)) * scale2                                         # [heads, nq, 32]
        whole = k0 + 32 <= nk + (1 if mutant == "whole_off_by_one" else 0)
        if not whole:
            valid = keys <= nk if mutant == "mask_le" else keys < nk
            s = torch.where(valid[None, None, :], s, torch.full((), -float("inf")))
        m_new = torch.maximum(m[sp], s.max(-1).values)
        corr = torch.exp2(m[sp] - m_new)                                                # exp2(-inf) = 0 on the stream's first tile
        p = torch.exp2(s - m_new[..., None])
        l[sp] = l[sp] * corr + p.sum(-1)
        m[sp] = m_new
        if mutant == "no_corr":
            pass
        elif mutant == "corr_skip_any":                                                 # rescale a wave (32 queries) only if ALL lanes changed
            wave = (corr != 1).view(heads, nq // 32, 32).all(-1).repeat_interleave(32, dim=1)
            o[sp] = torch.where(wave[..., None], o[sp] * corr[..., None], o[sp])
        else:
            o[sp] = o[sp] * corr[..., None]                                             # (x * 1 is exact: the ballot skip changes no bit)
        if mutant == "key_order":
            vt = vt[:, KEY_ORDER_PERM]
        o[sp] = o[sp] + p @ vt
    if mutant == "drop_stream1":
        lsum, osum = l[0], o[0]
    else:                                                                               # merge_streams
        mm = torch.maximum(m[0], m[1])
        c0, c1 = torch.exp2(m[0] - mm), torch.exp2(m[1] - mm)                           # a stream that saw no key: exp2(-inf) = 0
        lsum = l[1] * c1 + l[0] * c0
        osum = o[1] * c1[..., None] + o[0] * c0[..., None]
    out = osum * (1.0 / lsum)[..., None]
    return out.permute(1, 0, 2).reshape(nq, heads * DH)


def emulate_into(qkv, out, clips, max_n, heads, scale, mutant=None, row_off=0, seg=False):
    """The launch: clips = [(row0, n)] of qkv; clip rows go to out[row_off + row0 + i].  A clip whose qkv rows are all NaN gives
    NaN rows without being computed (NaN in, NaN out: the batch tests fill the other clips with NaN)."""
    assert mutant is None or mutant in MUTANTS
    flat = qkv.reshape(-1)
    qb = 128 if is_large(max_n, heads, len(clips)) else 64
    scale2 = np.float32(scale) * np.float32(LOG2E)
    for row0, n in clips:
        if n <= 0:
            continue                                                                    # (every block of the clip: live == false)
        if bool(torch.isnan(qkv[row0:row0 + n]).all()):
            out[row_off + row0:row_off + row0 + n] = float("nan")
            continue
        nk = max_n if (seg and mutant == "seg_reads_neighbour") else n
        rows = _emulate_clip(flat, row0, n, nk, heads, float(scale2), mutant, qb)
        last = rows.shape[0] if mutant == "store_past_n" else n
        last = min(last, out.shape[0] - row_off - row0)
        out[row_off + row0:row_off + row0 + last] = rows[:last]


def attention_emulated(qkv, B, n, heads, scale, mutant=None):
    """fp32 host restatement of the kernels' frame: 32-key tiles, two base-2 online-softmax streams (even / odd tiles), the m, l,
    corr recurrences, merge_streams, the division at the end.  `mutant`: one of MUTANTS."""
    out = torch.full((B * n, heads * DH), float("nan"))
    emulate_into(qkv.cpu(), out, [(b * n, n) for b in range(B)], n, heads, scale, mutant)
    return out


class EmulatedRunner:
    device = "cpu"

    def __init__(self, mutant=None):
        self.mutant = mutant

    def batched(self, qkv, out, row_off, B, n, heads, scale):
        emulate_into(qkv, out, [(b * n, n) for b in range(B)], n, heads, scale, self.mutant, row_off=row_off)

    def seg(self, qkv, out, clips, max_n, heads, scale):
        emulate_into(qkv, out, clips, max_n, heads, scale, self.mutant, seg=True)


# ---- input builders ------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    qkv: torch.Tensor                           # [B n, 3 heads 64] fp32
    B: int
    n: int
    heads: int
    scale: float
    extra: dict = field(default_factory=dict)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _pack(q, k, v):
    """q, k, v [B, heads, n, 64] -> qkv [B n, 3 heads 64]."""
    B, heads, n, _ = q.shape
    x = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4)                # [B, n, 3, heads, 64]
    return x.reshape(B * n, 3 * heads * DH).float().contiguous()


def logits2_f64(case):
    """The base-2 logits of a case in float64, [B, heads, n, n]."""
    q, k, _ = (t.double() for t in split_heads(case.qkv, case.B, case.n, case.heads))
    return q @ k.transpose(-1, -2) * (case.scale * LOG2E)


def uniform(n, B, heads, c):
    """Every logit is c scale: K rows identical, Q rows identical.  V[b, j, :] = j + 1 + 1000 b, so a row is the mean of small
    integers: expected fl(fl(sum) fl(1 / n)) (extra['expected'], [B] fp32), the sum exact below 2^24."""
    q = torch.zeros(B, heads, n, DH)
    k = torch.zeros(B, heads, n, DH)
    q[..., 0] = 8.0
    k[..., 0] = c / 8.0
    j = torch.arange(n, dtype=torch.float32)
    v = (j[None, :] + 1 + 1000 * torch.arange(B, dtype=torch.float32)[:, None])[:, None, :, None].expand(B, heads, n, DH)
    total = n * (n + 1) // 2 + 1000 * np.arange(B, dtype=np.int64) * n
    assert total.max() < 2 ** 24
    expected = total.astype(np.float32) * (np.float32(1) / np.float32(n))
    assert expected.dtype == np.float32
    return Case("uniform", _pack(q, k, v), B, n, heads, 10.0, {"expected": expected, "c": c})


def gather(n, B, heads, seed):
    """k_j = 8 u_j (random unit vectors), q_i = 8 u_pi(i), pi a random permutation per clip and head (every key, so every tile and
    every register position, is some row's target), scale 10.  Asserted here in float64: the base-2 logit of key pi(i) is >= 200
    above every other key's, so every other probability is exactly 0 in fp32 and out[i] == V[pi(i)] bit for bit."""
    g = _gen(seed)
    u = torch.randn(B, heads, n, DH, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    k = (8.0 * u).float()
    pi = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(heads)]) for _ in range(B)])     # [B, heads, n]
    q = torch.gather(k, 2, pi[..., None].expand(B, heads, n, DH))
    v = torch.randn(B, heads, n, DH, generator=g)
    case = Case("gather", _pack(q, k, v), B, n, heads, 10.0, {"pi": pi})
    lg = logits2_f64(case)
    hit = torch.gather(lg, 3, pi[..., None])                                            # [B, heads, n, 1]
    others = lg.scatter(3, pi[..., None], -float("inf"))
    gap = (hit - others.max(-1, keepdim=True).values).min().item() if n > 1 else float("inf")
    assert gap >= GATHER_GAP2, f"gather n={n} heads={heads}: base-2 gap {gap:.1f} < {GATHER_GAP2}"
    assert lg.abs().max().item() <= MAX_LOGIT2
    case.extra["gap2"] = gap
    expected = torch.gather(v, 2, pi[..., None].expand(B, heads, n, DH))                # V[pi(i)]
    case.extra["expected"] = expected.permute(0, 2, 1, 3).reshape(B * n, heads * DH).contiguous()
    return case


def ramp(n, B, heads, seed):
    """A rank-one logit a_j b_i: a_j = 8 (j + 1) / n rises with the key, so every 32-key tile raises the running maximum of a row
    with b > 0 (corr < 1 at every tile) and never that of a row with b < 0 (corr == 1 from its second tile on); the sign of b
    alternates from row to row, so both kinds sit in every wave.  |b| in [2, 8], scale 10: |logit| <= 640 (+ noise of 0.03 from the
    other 63 dimensions)."""
    g = _gen(seed)
    q = torch.randn(B, heads, n, DH, generator=g) * 0.02
    k = torch.randn(B, heads, n, DH, generator=g) * 0.02
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
    q[..., 0] = sign * (2.0 + 6.0 * torch.rand(B, heads, n, generator=g))
    k[..., 0] = 8.0 * (torch.arange(n, dtype=torch.float32) + 1) / n
    v = torch.randn(B, heads, n, DH, generator=g)
    return Case("ramp", _pack(q, k, v), B, n, heads, 10.0)


def offset(n, B, heads, seed, sign):
    """Soft logits (a spread of a few nats) on a common offset of +-600 nats from one constant dimension of q and k."""
    g = _gen(seed)
    q = torch.randn(B, heads, n, DH, generator=g) * 0.16
    k = torch.randn(B, heads, n, DH, generator=g) * 0.16
    q[..., 0] = 8.0
    k[..., 0] = 7.5 * sign
    v = torch.randn(B, heads, n, DH, generator=g)
    return Case("offset+" if sign > 0 else "offset-", _pack(q, k, v), B, n, heads, 10.0)


def model_like(n, B, heads, seed):
    """q and k of length 8 (as after qk-norm), scale 10, v ~ N(0, 2^2)."""
    g = _gen(seed)
    q = torch.randn(B, heads, n, DH, generator=g)
    k = torch.randn(B, heads, n, DH, generator=g)
    q, k = 8.0 * q / q.norm(dim=-1, keepdim=True), 8.0 * k / k.norm(dim=-1, keepdim=True)
    v = torch.randn(B, heads, n, DH, generator=g) * 2.0
    return Case("model_like", _pack(q, k, v), B, n, heads, 10.0)


def soft(n, B, heads, seed):
    """q, k, v ~ N(0, 1), scale 0.125: logits about N(0, 1), where the yardstick's own noise is about 1e-6."""
    g = _gen(seed)
    q, k, v = (torch.randn(B, heads, n, DH, generator=g) for _ in range(3))
    return Case("soft", _pack(q, k, v), B, n, heads, 0.125)


def build(name, n, B, heads, seed):
    if name == "ramp":
        return ramp(n, B, heads, seed)
    if name in ("offset+", "offset-"):
        return offset(n, B, heads, seed, 1 if name == "offset+" else -1)
    return {"model_like": model_like, "soft": soft}[name](n, B, heads, seed)


@functools.lru_cache(maxsize=None)
def f64_case(name, n, heads):
    """A float64-comparison case with its two references, computed once and shared by every test that uses it (read only)."""
    case = build(name, n, 1, heads, 1000 + 7 * n + heads)
    assert logits2_f64(case).abs().max().item() <= MAX_LOGIT2
    ref = attention_f64(case.qkv, 1, n, heads, case.scale)
    plain = attention_fp32_plain(case.qkv, 1, n, heads, case.scale).double()
    vmax = split_heads(case.qkv, 1, n, heads)[2].abs().max().item()
    return case, ref, plain, vmax


# ---- sentinels -----------------------------------------------------------------------------------------------------------------
def sentinel(rows, cols, device):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def is_sentinel(t):
    return bool((t.view(torch.int32) == SENTINEL).all())


# ---- the assertions of tests/test_hip_attention_edges.py ------------------------------------------------------------------------
def run_guarded(runner, qkv, B, n, heads, scale):
    """One batched call into the interior of an out of sentinels: the 128 rows in front and behind keep them."""
    inner = heads * DH
    out = sentinel(2 * GUARD_ROWS + B * n, inner, runner.device)
    runner.batched(qkv, out, GUARD_ROWS, B, n, heads, scale)
    assert is_sentinel(out[:GUARD_ROWS]), "a store in front of out"
    assert is_sentinel(out[GUARD_ROWS + B * n:]), "a store behind out's last row"
    return out[GUARD_ROWS:GUARD_ROWS + B * n]


def run_shapes(runner, case, shapes=("alone", "batch")):
    """The clip alone (SPLIT = 2) and as the last clip of the smallest batch across the launch threshold (SPLIT = 1) whose other
    clips are NaN: every row written and finite, sentinels untouched, the two results equal bit for bit.  Returns the lone result."""
    assert case.B == 1
    n, heads = case.n, case.heads
    assert not is_large(n, heads, 1)
    qkv = case.qkv.to(runner.device)
    lone = run_guarded(runner, qkv, 1, n, heads, case.scale)
    assert bool(torch.isfinite(lone).all()), "alone: a row not written, or not finite"
    if "batch" in shapes:
        B = batch_across_threshold(n, heads)
        assert is_large(n, heads, B) and not is_large(n, heads, B - 1)
        big = torch.full((B * n, 3 * heads * DH), float("nan"), device=runner.device)
        big[(B - 1) * n:] = qkv
        last = run_guarded(runner, big, B, n, heads, case.scale)[(B - 1) * n:]
        assert bool(torch.isfinite(last).all()), "in the batch: a row not written, or not finite (NaN of a neighbouring clip?)"
        assert torch.equal(last, lone), "the clip in a batch across the threshold differs from the clip alone"
    return lone.cpu()


def check_uniform(runner, n, heads, c, shapes=("alone", "batch")):
    case = uniform(n, 1, heads, c)
    got = run_shapes(runner, case, shapes).numpy()
    want = np.full((n, heads * DH), case.extra["expected"][0], dtype=np.float32)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=f"uniform n={n} heads={heads} c={c}")


def check_gather(runner, n, heads, shapes=("alone", "batch")):
    case = gather(n, 1, heads, 2000 + 11 * n + heads)
    got = run_shapes(runner, case, shapes)
    want = case.extra["expected"]
    bad = int((got != want).any(-1).sum())
    assert torch.equal(got, want), f"gather n={n} heads={heads}: {bad} of {n} rows are not V[pi(i)] bit for bit"


def error_figures(got, ref, plain, vmax):
    ek, ep = got.double() - ref, plain - ref
    return {"max_kernel": ek.abs().max().item(), "max_plain": ep.abs().max().item(),
            "rms_kernel": ek.pow(2).mean().sqrt().item(), "rms_plain": ep.pow(2).mean().sqrt().item(),
            "floor": BAR_FLOOR_ULPS * 2.0 ** -24 * vmax}


def check_float64(runner, name, n, heads, shapes=("alone", "batch"), label=""):
    """max and RMS of (kernel - float64) <= max(3 x the same of (plain fp32 - float64), 8 ulps of max |V|), on the same tensor."""
    case, ref, plain, vmax = f64_case(name, n, heads)
    got = run_shapes(runner, case, shapes)
    f = error_figures(got, ref, plain, vmax)
    print(f"attn-edges {label} {name} n={n} heads={heads}: max err kernel {f['max_kernel']:.3e} plain {f['max_plain']:.3e} "
          f"ratio {f['max_kernel'] / max(f['max_plain'], 1e-300):.2f}; rms kernel {f['rms_kernel']:.3e} plain {f['rms_plain']:.3e} "
          f"ratio {f['rms_kernel'] / max(f['rms_plain'], 1e-300):.2f}; floor {f['floor']:.2e}")
    assert f["max_kernel"] <= max(BAR_FACTOR * f["max_plain"], f["floor"]), f"{name} n={n} heads={heads}: max error {f}"
    assert f["rms_kernel"] <= max(BAR_FACTOR * f["rms_plain"], f["floor"]), f"{name} n={n} heads={heads}: rms error {f}"
    return f


def segment_layout(repeat):
    """Rows of the segment test: 128 guard rows, then each clip followed by a gap, then 128 guard rows.  -> clips [(row0, n)], rows."""
    clips, row = [], GUARD_ROWS
    for n in SEG_LENS * repeat:
        clips.append((row, n))
        row += n + SEG_GAP
    return clips, row + GUARD_ROWS


def check_segment(runner, heads, repeat):
    """One segment launch over SEG_LENS (x repeat) packed with gaps: each clip equals its lone batched call bit for bit, the
    zero-row clip writes nothing, gaps and guard rows (NaN in qkv) keep their sentinel in out, every clip row is finite."""
    clips, rows = segment_layout(repeat)
    max_n = max(SEG_LENS)
    assert is_large(max_n, heads, len(clips)) == (repeat > 1), "repeat = 1: the small grid; more: across the threshold"
    inner = heads * DH
    qkv = torch.full((rows, 3 * inner), float("nan"))
    for i, (row0, n) in enumerate(clips):
        if n:
            qkv[row0:row0 + n] = model_like(n, 1, heads, 3000 + i).qkv
    qkv = qkv.to(runner.device)
    out = sentinel(rows, inner, runner.device)
    runner.seg(qkv, out, clips, max_n, heads, 10.0)
    keep = torch.ones(rows, dtype=torch.bool)
    for row0, n in clips:
        keep[row0:row0 + n] = False
    assert is_sentinel(out[keep.to(out.device)]), "a store outside the clips' rows"
    for i, (row0, n) in enumerate(clips):
        if n == 0:
            continue
        got = out[row0:row0 + n]
        assert bool(torch.isfinite(got).all()), f"clip {i} ({n} rows): not finite"
        lone = run_guarded(runner, qkv[row0:row0 + n].clone(), 1, n, heads, 10.0)
        assert torch.equal(got, lone), f"clip {i} ({n} rows) differs from its lone batched call"
