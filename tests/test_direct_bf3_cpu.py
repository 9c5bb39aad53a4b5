"""conv_form='direct_bf16x3' on the host (no GPU): the two-piece weight packers, the form's name through the resolver, the
predicates and the blob tag, the launch plan -- the plan of 'direct_bf16x6', position for position, on the two new entries -- the
refusals, the bound of the three-pair arithmetic against float64, and the CPU estimate of what the form costs on the waveform.

The bound.  bf16 keeps 8 significant bits, so with h = bf16(x) and m = bf16(x - h), round to nearest even, |x - h| <= 2^-8 |x|,
|m| <= 2^-8 |x| and |x - h - m| <= 2^-8 |x - h| <= 2^-16 |x|.  A product a b against the kept pairs a_h b_h + a_h b_m + a_m b_h loses
a_m b_m + (a - a_h - a_m) b + (a_h + a_m) (b - b_h - b_m): at most 3 2^-16 (1 + 2^-16) |a b| in the worst case.  (The issue that
asked for this form derived 3 2^-18 from a unit roundoff of 2^-9; bf16's is 2^-8.)  The test below holds the float64 sum of the
three pair-convs to |conv_bf16x3_ref - float64| <= 2^-16 S, S = conv(|x|, |w|), pointwise: a third of the worst case.  It is the
bar the issue sets and it is kept: the three dropped terms of a product are roundings of independent sign and of rms size
~0.3 of their maxima, and an output sums >= 96 products, so the shapes here sit at 0.04 .. 0.21 of 2^-16 S (printed).  A lost
cross pair (h m or m h) is ~2^-9 S per product: 17 (2816 products per output) to 100 times the bar on these shapes."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent / "tools"))
from flowhigh_amd import hip, packing, planner, synth, weights          # noqa: E402
from flowhigh_amd.vocoder import Vocoder                                # noqa: E402
from ref_bf16x3 import BOUND, abs_sum, conv_bf16x3_ref, two_pieces      # noqa: E402

FORM = "direct_bf16x3"
FAMILIES = {"direct_bf16x3", "narrow_bf16x3", "direct"}
TWIN = {"direct_bf16x6": "direct_bf16x3", "narrow_bf16x6": "narrow_bf16x3", "direct": "direct"}
NEW_SYMBOLS = ("fh_conv_grouped_bf16x3_f32", "fh_narrow_conv_bf16x3_f32")
# the PLAIN shapes of test_hip_direct_bf.py (cin, cout, k, d, L; B = 2) and its 256-channel k 11 d 5 case
PLAIN = [(16, 24, 7, 3, 300), (48, 40, 11, 5, 1111), (32, 200, 3, 1, 33)]
WIDE = (256, 256, 11, 5, 700)


def _voc(cfgname, form):
    cfg = getattr(synth, cfgname)
    return Vocoder(cfg, synth.make_vocoder_state_dict(cfg, 1), "cpu", conv_form=form)


def _wide_range_weight(co, ci, k):
    g = torch.Generator().manual_seed(co + k)
    return torch.randn(co, ci, k, generator=g) * torch.exp2(torch.randint(-20, 21, (co, ci, k), generator=g).float())


# ---- packers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("co,ci,k", [(24, 16, 7), (200, 48, 11), (768, 32, 3)])
def test_pack_conv_bf3_weight(co, ci, k):
    w = _wide_range_weight(co, ci, k)
    cpad = -(-co // 32) * 32 + 32                                  # at least 32 padded rows
    p = packing.pack_conv_bf3_weight(w, cpad)
    assert p.dtype == torch.int16 and tuple(p.shape) == (ci // 16, k, cpad, 2, 16) and p.is_contiguous()         # 64-byte rows
    from flowhigh_amd import vocoder
    assert vocoder.pack_conv_bf3_weight is packing.pack_conv_bf3_weight
    ref = packing.pack_conv_weight(w, cpad, 16)
    assert torch.equal(p, packing.split_bf3(ref)[..., :2, :])       # h and m of the three-piece rows, bit for bit
    assert torch.equal(p, packing.pack_conv_bf_weight(w, cpad)[..., :2, :])
    h, m = packing.split_pieces(ref)[:2]
    assert torch.equal(p.view(torch.bfloat16).double().sum(dim=-2), h.double() + m.double())
    assert (p.view(torch.bfloat16).double().sum(dim=-2) - ref.double()).abs().le(2.0 ** -16 * ref.double().abs()).all()
    assert not bool(p[:, :, co:].any())                             # padded rows are zero
    wb = w.to(torch.bfloat16).float()                               # bf16-exact weights live in piece h alone
    pb = packing.pack_conv_bf3_weight(wb, cpad)
    assert not bool(pb[..., 1, :].any()) and torch.equal(pb[..., 0, :].view(torch.bfloat16).float(), packing.pack_conv_weight(wb, cpad, 16))
    with pytest.raises(ValueError):
        packing.pack_conv_bf3_weight(torch.zeros(8, 24, 3), 32)


@pytest.mark.parametrize("c,co,ci,k", [(24, 24, 24, 11), (48, 48, 48, 7), (40, 40, 40, 3), (32, 32, 32, 11), (8, 8, 8, 5), (24, 20, 17, 7)])
def test_pack_narrow_bf3_weight(c, co, ci, k):
    w = _wide_range_weight(co, ci, k)
    two, three = packing.pack_narrow_bf3_weight(w, c).view(torch.int16), packing.pack_narrow_bf_weight(w, c).view(torch.int16)
    from flowhigh_amd import vocoder
    assert vocoder.pack_narrow_bf3_weight is packing.pack_narrow_bf3_weight
    ma = -(-c // 16)
    o2 = o3 = 0
    for _, og in packing.narrow_slabs(c):                           # per slab: [k-block][N tile][piece][64 lanes][8]
        nb = -(-(k * og) // 4)
        n2, n3 = nb * ma * 2 * 512, nb * ma * 3 * 512
        assert torch.equal(two[o2:o2 + n2].view(nb, ma, 2, 64, 8), three[o3:o3 + n3].view(nb, ma, 3, 64, 8)[:, :, :2])
        o2, o3 = o2 + n2, o3 + n3
    assert o2 == two.numel() and o3 == three.numel() and 2 * three.numel() == 3 * two.numel()
    wb = w.to(torch.bfloat16).float()                               # bf16-exact weights: piece m is zero, piece h the three-piece h
    pb = packing.pack_narrow_bf3_weight(wb, c).view(torch.int16)
    assert not bool(pb.view(-1, 2, 512)[:, 1].any())
    assert torch.equal(pb.view(-1, 2, 512)[:, 0], packing.pack_narrow_bf_weight(wb, c).view(torch.int16).view(-1, 3, 512)[:, 0])
    with pytest.raises(ValueError):
        packing.pack_narrow_bf3_weight(torch.zeros(56, 56, 3))
    with pytest.raises(ValueError):
        packing.pack_narrow_bf3_weight(torch.zeros(24, 24, 13))


# ---- the name --------------------------------------------------------------------------------------------------------------------
def test_form_name_resolves_and_auto_is_unchanged(monkeypatch):
    for k in ("FH_CONV_FORM", "FH_WINO", "FH_CONV_BF16X6"):
        monkeypatch.delenv(k, raising=False)
    assert FORM in planner.CONV_FORMS and FORM in planner.DIRECT_FORMS
    assert planner.resolve_conv_form(FORM) == (FORM, False)
    assert planner.resolve_conv_form("auto") == ("bf16x6", True) and planner.DEFAULT_CONV_FORM == "bf16x6"
    assert planner.resolve_conv_form() == ("bf16x6", True)
    with pytest.raises(ValueError):
        planner.resolve_conv_form("direct_bf16")
    monkeypatch.setenv("FH_CONV_FORM", FORM)
    assert planner.resolve_conv_form() == (FORM, False)
    assert planner.use_direct_bf16x3() and not planner.use_direct_bf16x6() and not planner.use_bf16x6()
    assert planner.use_gemm_bf16x6() and planner.use_amp_bf16x6()
    assert not planner.use_wino(768, 1) and not planner.use_wino54(768)
    monkeypatch.delenv("FH_CONV_FORM")
    assert planner.use_direct_bf16x3(FORM) and not planner.use_direct_bf16x3("direct_bf16x6") and not planner.use_direct_bf16x3("direct")
    assert not planner.use_direct_bf16x6(FORM) and planner.use_gemm_bf16x6(FORM) and planner.use_amp_bf16x6(FORM)
    assert [planner.direct_bf_pieces(f) for f in ("winograd", "bf16x6", "direct", "direct_bf16x6", FORM)] == [0, 0, 0, 1, 2]
    assert planner.use_amp(24, [3, 7, 11], [[1, 3, 5]] * 3, FORM) and not planner.use_amp(96, [3, 7, 11], [[1, 3, 5]] * 3, FORM)
    tags = {f: weights.format_tag(f) for f in ("winograd", "bf16x6", "direct", "direct_bf16x6", FORM)}
    assert len(set(tags.values())) == 5
    assert hip.ABI_VERSION == 6 and all(s in hip.EXPORTS for s in NEW_SYMBOLS)
    assert hip._SIGS["fh_conv_grouped_bf16x3_f32"] == hip._SIGS["fh_conv_grouped_bf16x6_f32"]
    assert hip._SIGS["fh_narrow_conv_bf16x3_f32"] == hip._SIGS["fh_narrow_conv_bf16x6_f32"]
    header = (Path(__file__).resolve().parents[1] / "include" / "flowhigh_hip.h").read_text()
    assert all(f"int {s}(" in header for s in NEW_SYMBOLS) and "#define FH_ABI_VERSION 6" in header


# ---- plans -----------------------------------------------------------------------------------------------------------------------
def _conv_steps(p):
    """(step, family) of the conv-family launches of a plan, launch order."""
    steps = [s for s in p["steps"] if s.kind in ("conv", "convt", "wino", "amp")]
    assert len(steps) == len(p["conv_launches"])
    return list(zip(steps, [f for f, _, _ in p["conv_launches"]]))


def test_plan_is_the_direct_bf16x6_plan_on_the_new_entries():
    from flowhigh_amd import runtime
    new, old = _voc("SYNTH_CFG", FORM), _voc("SYNTH_CFG", "direct_bf16x6")
    assert new.form == FORM and new.direct_bf == 2 and old.direct_bf == 1 and new.amp_direct and not new.bf
    pn, po = new.plan(1, 100), old.plan(1, 100)
    got, ref = _conv_steps(pn), _conv_steps(po)
    assert {f for _, f in got} == FAMILIES
    assert len(pn["steps"]) == len(po["steps"]) and [m[0] for m in pn["meta"]] == [m[0] for m in po["meta"]]      # the same launch positions
    assert [s.kind for s in pn["steps"]] == [s.kind for s in po["steps"]]
    assert [(TWIN[f], ex, fl) for f, ex, fl in po["conv_launches"]] == pn["conv_launches"]                      # families mapped, FLOPs equal
    for (s, fam), (r, rfam) in zip(got, ref):
        assert fam == TWIN[rfam] and s.kind == r.kind
        if s.kind == "amp":
            assert fam == "narrow_bf16x3" and (s.ng, s.n_tiles, s.c, s.dil, s.cmax, s.flops) == (r.ng, r.n_tiles, r.c, r.dil, r.cmax, r.flops)
            assert s.flags == r.flags | planner.AMP_BF16X3 and r.flags & planner.AMP_DIRECT and not r.flags & planner.AMP_BF16X3
            assert runtime.narrow_entry(s.flags, s.cmax) == ("fh_narrow_conv_bf16x3_f32", (s.flags & 1,))
            assert runtime.narrow_entry(r.flags, r.cmax) == ("fh_narrow_conv_bf16x6_f32", (r.flags & 1,))
            continue
        assert (s.cpad, s.tcfg, s.ng, s.n_len, s.flops) == (r.cpad, r.tcfg, r.ng, r.n_len, r.flops)
        if s.kind == "conv":
            assert fam == "direct_bf16x3" and s.bf == 2 and s.ck == 16 and r.bf == 1 and r.ck == 16
            assert runtime.conv_entry(s.bf, s.ck) == ("fh_conv_grouped_bf16x3_f32", ())
            assert runtime.conv_entry(r.bf, r.ck) == ("fh_conv_grouped_bf16x6_f32", ())
        else:
            assert fam == "direct" and s.kind == "convt" and s.phases == r.phases
    assert [s.kind for s, f in got if f == "direct"] == ["convt"] * 3           # the three phase-fused transposed convs stay on fp32 MFMA
    # two-piece weights where the new entries run: 64-byte rows, two thirds of the narrow stages' bytes; fp32 under the fused upsamplers
    assert new.pre_w.dtype == torch.int16 and tuple(new.pre_w.shape[-2:]) == (2, 16) and tuple(old.pre_w.shape[-2:]) == (3, 16)
    nn_, on_ = [[e["ua"] for st in v.stages for b in st["blocks"] for e in b["c1"] + b["c2"] if "ua" in e] for v in (new, old)]
    assert nn_ and len(nn_) == len(on_) and all(3 * a.numel() == 2 * b.numel() for a, b in zip(nn_, on_))
    for st_n, st_o in zip(new.stages, old.stages):
        assert (st_n["conv_bf"], st_n["up_bf"]) == tuple(2 * v for v in (st_o["conv_bf"], st_o["up_bf"]))
        for ph_n, ph_o in zip(st_n["up_phases"], st_o["up_phases"]):
            assert ph_n["w"].dtype == ph_o["w"].dtype and (ph_n["w"].dtype == torch.float32) == (st_n["up_bf"] == 0)


def test_the_other_forms_keep_their_records():
    """bf stays 0 / 1 and the narrow flags stay 4 | aligned for the forms that were there before."""
    for form, bfs, fams in (("direct", {0}, {"direct"}), ("direct_bf16x6", {1}, {"direct_bf16x6", "narrow_bf16x6", "direct"}),
                            ("bf16x6", set(), None), ("winograd", set(), None)):
        p = _voc("SYNTH_CFG", form).plan(1, 100)
        assert {s.bf for s in p["steps"] if s.kind == "conv"} <= (bfs or {0})
        assert all(not s.flags & planner.AMP_BF16X3 for s in p["steps"] if s.kind == "amp")
        if fams:
            assert {f for f, _, _ in p["conv_launches"]} == fams
        else:
            assert not {f for f, _, _ in p["conv_launches"]} & {"direct_bf16x3", "narrow_bf16x3"}


def test_ragged_plan_carries_the_entry_choice():
    from flowhigh_amd import runtime
    voc = _voc("TINY_CFG", FORM)
    rp = voc.plan_ragged([40, 25])
    rc = [s for s in rp["steps"] if s.kind == "rconv"]
    ra = [s for s in rp["steps"] if s.kind == "ramp"]
    assert rc and all(s.bf == 2 and s.ck == 16 for s in rc)
    assert ra and all(s.flags & planner.AMP_DIRECT and s.flags & planner.AMP_BF16X3 for s in ra)
    assert all(runtime.narrow_entry(s.flags, s.cmax)[0] == "fh_narrow_conv_bf16x3_f32" for s in ra)
    old = _voc("TINY_CFG", "direct_bf16x6").plan_ragged([40, 25])["steps"]
    assert all(s.bf == 1 for s in old if s.kind == "rconv") and all(not s.flags & planner.AMP_BF16X3 for s in old if s.kind == "ramp")
    assert [s.kind for s in rp["steps"]] == [s.kind for s in old]


@pytest.mark.parametrize("cfgname", ["TINY_CFG", "ALT_CFG"])
def test_plan_builds_for_other_configurations(cfgname):
    p = _voc(cfgname, FORM).plan(1, 100)
    fams = {f for f, _, _ in p["conv_launches"]}
    assert fams <= FAMILIES and "direct_bf16x3" in fams
    for s in p["steps"]:
        if s.kind == "conv":
            assert s.bf == (2 if s.ck == 16 else 0)                 # 8-channel chunks stay on the fp32 entry


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_vocoder_refuses_a_store_of_another_form():
    cfg = synth.TINY_CFG
    sd = synth.make_vocoder_state_dict(cfg, 1)
    for other in ("direct_bf16x6", "direct"):
        store = weights.WeightStore("cpu")
        store.form = other
        with pytest.raises(ValueError, match=other):
            Vocoder(cfg, sd, "cpu", conv_form=FORM, store=store)
    store = weights.WeightStore("cpu")
    store.form = FORM
    with pytest.raises(ValueError, match=FORM):
        Vocoder(cfg, sd, "cpu", conv_form="direct_bf16x6", store=store)
    with pytest.raises(ValueError):
        Vocoder(cfg, sd, "cpu", conv_form="direct_bf16")


@pytest.mark.parametrize("symbol", NEW_SYMBOLS)
def test_a_library_without_a_new_symbol_is_refused_at_load(symbol, monkeypatch):
    """The entries are additive (the ABI version stays 6): a library built before them has the right version and not the symbols,
    and the load fails with a HipError that says to rebuild."""
    import ctypes as C
    real = C.CDLL(str(hip.LIB_PATH))
    assert hasattr(real, symbol)

    class Older:
        def __getattr__(self, name):
            if name == symbol:
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip.C, "CDLL", lambda path: Older())
    with pytest.raises(hip.HipError, match=symbol + ".*rebuild"):
        hip.lib()
    assert hip._lib is None
    monkeypatch.undo()
    assert hip.lib().fh_abi_version() == 6


def test_narrow_argument_checks_carry_over():
    """The three refusals tests/test_layout.py pins for fh_narrow_conv_bf16x6_f32, with the new entry's name (nothing is launched)."""
    lib = hip.lib()
    assert lib.fh_narrow_conv_bf16x3_f32(16, 1, 16, 1, 50, 1, 1, 0) == -1 and b"channels" in lib.fh_last_error()
    assert b"fh_narrow_conv_bf16x3_f32" in lib.fh_last_error()
    assert lib.fh_narrow_conv_bf16x3_f32(16, 1, 16, 1, 24, 7, 1, 0) == -1 and b"dilation" in lib.fh_last_error()
    assert lib.fh_narrow_conv_bf16x3_f32(16, 1, 16, 1, 24, 1, 2, 0) == -1 and b"flags" in lib.fh_last_error()
    assert lib.fh_conv_grouped_bf16x3_f32(16, 1, 1, 128, 10, 9, 0) == -1 and b"fh_conv_grouped_bf16x3_f32: unknown tile_cfg 9" in lib.fh_last_error()


# ---- the arithmetic's bound --------------------------------------------------------------------------------------------------
def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("case", PLAIN + [WIDE])
def test_three_pairs_stay_inside_the_derived_bound(case):
    cin, cout, k, d, L = case
    wide = case == WIDE
    x = _rnd(1 if wide else 2, cin, L, seed=4 if wide else 1)
    w = _rnd(cout, cin, k, seed=5 if wide else 2, scale=0.02 if wide else 0.2)
    kw = dict(dilation=d, padding=(k * d - d) // 2)
    # the pieces themselves
    for t in (x, w):
        h, m = two_pieces(t)
        assert (m.abs() <= 2.0 ** -8 * t.double().abs()).all() and ((t.double() - h - m).abs() <= 2.0 ** -16 * t.double().abs()).all()
    ref64 = F.conv1d(x.double(), w.double(), None, **kw)
    got = conv_bf16x3_ref(x, w, **kw)
    S = abs_sum(x, w, **kw)
    ratio = ((got - ref64).abs() / (BOUND * S)).max().item()
    print(f"{case}: max |bf16x3 - float64| / (2^-16 S) = {ratio:.3f}")
    assert ratio <= 1.0
    # a lost cross pair is more than ten times outside
    xs, ws = two_pieces(x), two_pieces(w)
    lost = F.conv1d(xs[0], ws[0], None, **kw) + F.conv1d(xs[1], ws[0], None, **kw)          # h m missing
    assert ((lost - ref64).abs() / (BOUND * S)).max().item() > 10.0


# ---- the estimate ------------------------------------------------------------------------------------------------------------------
def test_estimate_on_the_tiny_configuration_is_inside_half_the_parity_bar():
    """tests/tools/bf16x3_estimate.py: the oracle's BigVGAN with its convs in the three-pair arithmetic against its float64 run, TINY_CFG,
    a 20-frame random mel.  The project's bar on the waveform is 1e-4; the form has to be predicted inside half of it."""
    from bf16x3_estimate import estimate
    r = estimate("TINY_CFG", 20, modes=("bf16x3", "bf16"))
    print(f"TINY_CFG, 20 frames: bf16x3 max abs {r['bf16x3'][0]:.2e} rms {r['bf16x3'][1]:.2e}; one piece {r['bf16'][0]:.2e}")
    assert r["bf16x3"][0] <= 5e-5
    assert r["bf16"][0] > 1e-4                      # (one piece per operand is of no use: the emulation does tell the forms apart)
