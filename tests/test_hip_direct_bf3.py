"""GPU: fh_conv_grouped_bf16x3_f32 (conv_mfma_bf.hip with two pieces per operand), the grouped implicit-GEMM conv in the bf16 x 3
form, on the shapes and helpers of test_hip_direct_bf.py with the two-piece packer and the new entry.

The form is NOT fp32-grade against float64, so two things are asserted on every random-input case:
  * against the form's own definition -- tests/ref_bf16x3.conv_bf16x3_ref, the float64 sum of the three pair-convs of the split
    operands -- the kernel is fp32-grade by the project's rule: |y - ref| <= 2 e32 + 1e-7, e32 being the fp32 kernel's
    (fh_conv_grouped_f32, 16-channel chunks) max-abs distance to float64 on the same inputs.  What is left between the kernel and
    that reference is fp32 accumulation of the same products in another order;
  * against float64, pointwise: |y - float64| <= 2^-16 S + 2 e32, S = conv(|x|, |w|) (tests/test_direct_bf3_cpu.py has the bound).
The exact-pair test at the end pins the three kept pairs, the absence of (m, m) and the device split's h and m with equality."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from flowhigh_amd import hip                                                                     # noqa: E402
from flowhigh_amd import vocoder as V                                                            # noqa: E402
from ref_bf16x3 import BOUND, abs_sum, conv_bf16x3_ref                                           # noqa: E402
from test_hip_bf16x6_pairs import assert_same, designed_values, slot_planes, slot_sum, weight_values   # noqa: E402
from test_hip_direct_bf import PLAIN, TILES, cpad_of, err, rnd                                   # noqa: E402

DEV = "cuda"
BF3 = 2                                             # the `bf` value of a conv step record that runs the bf16 x 3 entry
ENTRY = "fh_conv_grouped_bf16x3_f32"


def pack(w, cpad, bf):
    return (V.pack_conv_bf3_weight(w, cpad) if bf else V.pack_conv_weight(w, cpad, 16)).to(DEV)


def launch(groups, batch, cpad, n_len, tile_cfg, bf):
    keep = V.conv_grouped(groups, batch, cpad, n_len, tile_cfg, DEV, 16, bf=BF3 if bf else 0)
    torch.cuda.synchronize()
    del keep


def run_conv(x, w, bias, dilation, tile_cfg, bf, res=None, scale=1.0):
    """test_hip_direct_bf.run_conv; bf: two-piece weights and the bf16 x 3 entry, else the fp32 kernel with 16-channel chunks."""
    B, cin, L = x.shape
    cout, _, k = w.shape
    cpad = cpad_of(cout, tile_cfg)
    xd, out = x.to(DEV), torch.full((B, cout, L), float("nan"), device=DEV)
    wp = pack(w, cpad, bf)
    bd = bias.to(DEV) if bias is not None else None
    rd = [r.to(DEV) for r in (res or [])]
    offs = [(t - (k - 1) // 2) * dilation for t in range(k)]
    g = V.make_conv_group([V.make_conv_seg(xd, wp, cin, offs)], bd, rd, out, cout, cpad, L, L, L, scale=scale)
    launch([g], B, cpad, L, tile_cfg, bf)
    return out.cpu()


def assert_bf16x3(got, got32, ref3, ref64, S, what):
    """got: the kernel under test; got32: the fp32 kernel on the same inputs; ref3 / ref64: the form's definition and the float64
    conv, both with bias, residuals and scale; S: |scale| conv(|x|, |w|)."""
    assert not bool(torch.isnan(got).any()), what
    e32 = err(got32, ref64)
    e_def = err(got, ref3)
    miss = ((got.double() - ref64).abs() - (BOUND * S + 2.0 * e32)).max().item()
    worst = ((got.double() - ref64).abs() / (BOUND * S)).max().item()
    print(f"{what}: |y - bf16x3 definition| {e_def:.3e} (fp32 MFMA against float64: {e32:.3e}); |y - float64| {err(got, ref64):.3e}, "
          f"at most {worst:.3f} of 2^-16 S")
    assert e_def <= 2.0 * e32 + 1e-7, what
    assert miss <= 0.0, what


# ---- plain convs: every tile shape -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_case(case):
    cin, cout, k, d, L = case
    x, w, b = rnd(2, cin, L, seed=1), rnd(cout, cin, k, seed=2, scale=0.2), rnd(cout, seed=3)
    kw = dict(dilation=d, padding=(k * d - d) // 2)
    return x, w, b, F.conv1d(x.double(), w.double(), b.double(), **kw), conv_bf16x3_ref(x, w, b, **kw), abs_sum(x, w, **kw)


@functools.lru_cache(maxsize=None)
def plain_out(case, tile_cfg):
    x, w, b = plain_case(case)[:3]
    return run_conv(x, w, b, case[3], tile_cfg, bf=True)


@pytest.mark.parametrize("tile_cfg", TILES)
@pytest.mark.parametrize("case", PLAIN)
def test_conv_plain_against_its_definition_and_float64(case, tile_cfg):
    x, w, b, ref64, ref3, S = plain_case(case)
    got32 = run_conv(x, w, b, case[3], tile_cfg, bf=False)
    assert_bf16x3(plain_out(case, tile_cfg), got32, ref3, ref64, S, f"{case} tile {tile_cfg}")


@pytest.mark.parametrize("case", PLAIN)
def test_bits_do_not_depend_on_the_tile(case):
    outs = [plain_out(case, t) for t in TILES]
    assert not bool(torch.isnan(outs[0]).any())
    for t in TILES[1:]:
        assert torch.equal(outs[t], outs[0]), f"{case}: tile {t} against tile 0"


# ---- residuals, scale, K segments ------------------------------------------------------------------------------------------
def test_conv_large_k_residual_scale():
    cin = cout = 256
    x, w, b = rnd(1, cin, 700, seed=4), rnd(cout, cin, 11, seed=5, scale=0.02), rnd(cout, seed=6)
    r1, r2 = rnd(1, cout, 700, seed=7), rnd(1, cout, 700, seed=8)
    kw = dict(dilation=5, padding=25)
    rest = r1.double() + r2.double()
    ref64 = (F.conv1d(x.double(), w.double(), b.double(), **kw) + rest) * 0.5
    ref3 = (conv_bf16x3_ref(x, w, b, **kw) + rest) * 0.5
    got = run_conv(x, w, b, 5, 0, bf=True, res=[r1, r2], scale=0.5)
    got32 = run_conv(x, w, b, 5, 0, bf=False, res=[r1, r2], scale=0.5)
    assert_bf16x3(got, got32, ref3, ref64, 0.5 * abs_sum(x, w, **kw), "256 channels, k 11, d 5, two residuals, scale 0.5")


def test_conv_three_segments_fused_average_and_batch_invariance():
    """Last conv2 of a stage: one accumulator over the three AMP blocks + residuals, / 3; a clip of the batch alone: same bits."""
    c, L, B = 48, 400, 2
    ks = [11, 7, 3]
    xs = [rnd(B, c, L, seed=20 + i) for i in range(3)]
    ws = [rnd(c, c, k, seed=30 + i, scale=0.1) for i, k in enumerate(ks)]
    bs = [rnd(c, seed=40 + i) for i in range(3)]
    rs = [rnd(B, c, L, seed=50 + i) for i in range(3)]
    pads = [dict(padding=(k - 1) // 2) for k in ks]
    ref64 = sum(F.conv1d(x.double(), w.double(), b.double(), **p) + r.double() for x, w, b, r, p in zip(xs, ws, bs, rs, pads)) / 3
    ref3 = sum(conv_bf16x3_ref(x, w, b, **p) + r.double() for x, w, b, r, p in zip(xs, ws, bs, rs, pads)) / 3
    S = sum(abs_sum(x, w, **p) for x, w, p in zip(xs, ws, pads)) / 3
    tile_cfg, _, cpad = V.pick_tile_cfg(c)
    bsum = sum(bs).to(DEV)

    def run(bf, items):
        n = len(items)
        out = torch.full((n, c, L), float("nan"), device=DEV)
        xd, rd = [x[items].contiguous().to(DEV) for x in xs], [r[items].contiguous().to(DEV) for r in rs]
        wp = [pack(w, cpad, bf) for w in ws]
        segs = [V.make_conv_seg(xd[i], wp[i], c, [t - (k - 1) // 2 for t in range(k)]) for i, k in enumerate(ks)]
        g = V.make_conv_group(segs, bsum, rd, out, c, cpad, L, L, L, scale=1.0 / 3)
        launch([g], n, cpad, L, tile_cfg, bf)
        return out.cpu()
    got = run(True, [0, 1])
    assert_bf16x3(got, run(False, [0, 1]), ref3, ref64, S, "three K segments, three residuals, scale 1/3")
    assert torch.equal(run(True, [1]), got[1:2])


# ---- transposed conv as phase groups: out_stride, out_phase, k - u odd ---------------------------------------------------------
@pytest.mark.parametrize("u,k", [(5, 11), (2, 3), (6, 13)])
def test_conv_transpose_as_phase_groups(u, k):
    cin, cout, L, B = 32, 16, 157, 2
    x, wt, b = rnd(B, cin, L, seed=11), rnd(cin, cout, k, seed=12, scale=0.2), rnd(cout, seed=13)
    kw = dict(stride=u, padding=(k - u) // 2)
    ref64 = F.conv_transpose1d(x.double(), wt.double(), b.double(), **kw)
    ref3 = conv_bf16x3_ref(x, wt, b, conv=F.conv_transpose1d, **kw)
    S = abs_sum(x, wt, conv=F.conv_transpose1d, **kw)
    extra = V.transposed_conv_extra(k, u)
    lout = u * L + extra
    assert ref64.shape[-1] == lout
    tile_cfg, _, cpad = V.pick_tile_cfg(cout)
    xd, bd = x.to(DEV), b.to(DEV)

    def run(bf):
        out = torch.full((B, cout, lout), float("nan"), device=DEV)
        groups, keep = [], []
        for r, taps in enumerate(V.transposed_conv_phases(k, u)):
            wp = pack(torch.stack([wt[:, :, j] for j, _ in taps], dim=-1).permute(1, 0, 2), cpad, bf)
            keep.append(wp)
            groups.append(V.make_conv_group([V.make_conv_seg(xd, wp, cin, [o for _, o in taps])], bd, [], out,
                                            cout, cpad, L, lout, L + (extra if r == 0 else 0), stride=u, phase=r))
        launch(groups, B, cpad, L + extra, tile_cfg, bf)
        return out.cpu()
    assert_bf16x3(run(True), run(False), ref3, ref64, S, f"ConvTranspose1d(k {k}, u {u})")


# ---- the three kept pairs and the device split, by equality (tests/test_hip_bf16x6_pairs.py's construction) ----------------------
@pytest.mark.parametrize("tile_cfg", [0, 4])
def test_direct_bf16x3_every_pair(tile_cfg):
    """One nonzero bf16-exact weight per output channel co (input channel (7 co + 3) % 32: both 16-channel chunks, both octets =
    both lane halves of the K dimension; tap co % 3), placed in ONE of the two piece slots: out[co, t] = x[ci, t + (tap - 1) d]
    (the slot's pieces) v_co exactly.  Slot h keeps the pairs h h and h m -> (a_h + a_m) v; slot m keeps m h -> a_h v: the three
    kept pairs are each present, (m, m) is absent, and the device split's h and m are pinned, negative residuals included."""
    C, k, d, L, B = 32, 3, 2, 200, 2
    x, pieces = designed_values(B * C * L, 90 + tile_cfg)
    x, pieces = x.view(B, C, L), [p.view(B, C, L) for p in pieces]
    co = torch.arange(C)
    ci, tap = (7 * co + 3) % C, co % k
    assert sorted(ci.tolist()) == list(range(C))
    v = weight_values(C, 91)
    w = torch.zeros(C, C, k)
    w[co, ci, tap] = v
    cpad = cpad_of(C, tile_cfg)
    xd = x.to(DEV)
    offs = [(t - 1) * d for t in range(k)]
    for slot in (0, 1):
        wd = slot_planes(V.pack_conv_weight(w, cpad, 16), slot)[..., :2, :].contiguous().to(DEV)         # three planes, two kept
        assert wd.shape == V.pack_conv_bf3_weight(w, cpad).shape
        out = torch.full((B, C, L), float("nan"), device=DEV)
        g = V.make_conv_group([V.make_conv_seg(xd, wd, C, offs)], None, [], out, C, cpad, L, L, L)
        launch([g], B, cpad, L, tile_cfg, True)
        src = F.pad(slot_sum(pieces, slot + 1), (d, d))              # weight slot h: a_h + a_m; slot m: a_h   [B, C, L + 2 d]
        exp = torch.stack([src[:, ci[o], tap[o] * d:tap[o] * d + L] for o in range(C)], dim=1) * v.double()[None, :, None]
        assert_same(out, exp.float(), f"direct bf16 x 3, tile {tile_cfg}, weight slot {'hm'[slot]}")


# ---- argument errors: a negative code and a message with the entry's name, nothing launched ------------------------------------
def test_host_resident_descriptors_are_checked_by_the_launcher():
    L = hip.lib()
    fn = getattr(L, ENTRY)
    cin, cout, n = 32, 24, 100
    cpad = cpad_of(cout, 0)
    x, out = rnd(1, cin, n, seed=70).to(DEV), torch.full((1, cout, n), float("nan"), device=DEV)
    wp = pack(rnd(cout, cin, 3, seed=71), cpad, True)
    good = V.make_conv_group([V.make_conv_seg(x, wp, cin, [-1, 0, 1])], None, [], out, cout, cpad, n, n, n)
    d = hip.to_device_struct_array([good], DEV)
    msg = lambda: L.fh_last_error().decode()
    assert fn(d.data_ptr(), 1, 1, cpad, n, 7, hip.stream()) < 0 and "tile_cfg 7" in msg() and ENTRY in msg()
    assert fn(None, 1, 1, cpad, n, 0, hip.stream()) < 0 and ENTRY in msg()
    assert fn(d.data_ptr(), 1, 1, cpad + 1, n, 0, hip.stream()) < 0 and "cout_pad" in msg()
    pinned = lambda g: torch.frombuffer(bytearray(bytes(g)), dtype=torch.uint8).pin_memory()
    # cin = 24: the launcher sees a descriptor array that lives in pinned host memory
    bad = V.make_conv_group([V.make_conv_seg(x, wp, 24, [-1, 0, 1])], None, [], out, cout, cpad, n, n, n)
    hb = pinned(bad)
    assert fn(hb.data_ptr(), 1, 1, cpad, n, 0, hip.stream()) < 0
    assert ENTRY in msg() and "24 input channels" in msg() and "multiple of 16" in msg()
    # a segment count outside 1 .. 3
    many = hip.ConvGroup.from_buffer_copy(good)
    many.nseg = hip.CONV_MAX_SEG + 1
    hm = pinned(many)
    assert fn(hm.data_ptr(), 1, 1, cpad, n, 0, hip.stream()) < 0
    assert ENTRY in msg() and f"{hip.CONV_MAX_SEG + 1} segments" in msg()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                     # nothing ran
    # ... and the same array as it should be runs, with the bits of the device-resident descriptors
    hg = pinned(good)
    hip.check(fn(hg.data_ptr(), 1, 1, cpad, n, 0, hip.stream()), "pinned descriptors")
    torch.cuda.synchronize()
    first = out.clone()
    out.fill_(float("nan"))
    hip.check(fn(d.data_ptr(), 1, 1, cpad, n, 0, hip.stream()), "device descriptors")
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and torch.equal(out, first)
