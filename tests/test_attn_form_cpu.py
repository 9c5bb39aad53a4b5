"""attn_form (the arithmetic form of the two products of attention: 'f32' | 'bf16x6'), the parts that need no GPU: the keyword's
resolution, the two C entries' presence and argument errors, and the exact constructions tests/test_hip_attention_bf.py pins the
twelve piece-pair MFMAs with (tests/tools/attn_pins.py), each checked against a host emulation: the correct arithmetic passes,
every mutant (a dropped pair, l = 0, a truncating split) moves what the GPU test compares."""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import attn_pins as AP                                  # noqa: E402
from flowhigh_amd import hip, planner                   # noqa: E402

ENTRIES = ("fh_attention_bf16x6_f32", "fh_attention_bf16x6_seg_f32")


# ---- keyword ----------------------------------------------------------------------------------------------------------------
def test_resolve_attn_form():
    assert planner.resolve_attn_form() == planner.resolve_attn_form(None) == "f32" == planner.DEFAULT_ATTN_FORM
    assert planner.resolve_attn_form("f32") == "f32" and planner.resolve_attn_form("bf16x6") == "bf16x6"
    for bad in ("auto", "bf16", "BF16X6", "", 1, True):
        with pytest.raises(ValueError) as e:
            planner.resolve_attn_form(bad)
        assert "'f32'" in str(e.value) and "'bf16x6'" in str(e.value)


def test_attn_form_has_no_environment_switch(monkeypatch):
    for name in ("FH_ATTN_FORM", "FH_ATTENTION_FORM", "FH_ATTN_BF16X6"):
        monkeypatch.setenv(name, "bf16x6")
    assert planner.resolve_attn_form() == "f32"
    src = "".join(p.read_text() for p in (ROOT / "flowhigh_amd").glob("*.py"))
    assert "FH_ATTN" not in src


def test_public_constructors_refuse_an_unknown_attn_form_before_loading_anything(tmp_path):
    from flowhigh_amd import FLowHigh, FlowHighSR
    with pytest.raises(ValueError, match="bf16x6"):
        FLowHigh(None, {}, "cuda", attn_form="bf16")
    with pytest.raises(ValueError, match="f32"):
        FlowHighSR.from_local(tmp_path / "no_such_dir", attn_form="fp32")
    import inspect
    for fn in (FLowHigh.__init__, FlowHighSR.from_local.__func__, FlowHighSR.from_pretrained.__func__):
        assert inspect.signature(fn).parameters["attn_form"].default is None
    assert isinstance(FLowHigh.attn_form, property) and FLowHigh.attn_form.fset is None


def test_flownet_picks_the_entry_pair_once():
    from flowhigh_amd.flow import FlowNet
    sig = __import__("inspect").signature(FlowNet.__init__)
    assert sig.parameters["attn_form"].default == "f32"
    from flowhigh_amd import synth
    sd = synth.make_flow_state_dict(seed=0)
    for form, names in (("f32", ("fh_attention_f32", "fh_attention_seg_f32")), ("bf16x6", ENTRIES)):
        net = FlowNet(sd, "cpu", attn_form=form)
        assert net.attn_form == form and (net._attn, net._attn_seg) == names
    with pytest.raises(ValueError):
        FlowNet(sd, "cpu", attn_form="bf16x3")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_6_exports_the_two_entries():
    assert hip.ABI_VERSION == 6
    assert set(ENTRIES) <= set(hip.EXPORTS)
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert "#define FH_ABI_VERSION 6" in header
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert hip._SIGS[name] == hip._SIGS[name.replace("_bf16x6", "")]
    assert hip.lib().fh_abi_version() == 6


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_errors_are_returned_with_the_entrys_name(name):
    L = hip.lib()
    fn = getattr(L, name)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p -= p % 16                    # (never dereferenced: every call below is refused before a launch)
    seg = name.endswith("_seg_f32")
    good = dict(qkv=p, out=p, seg=p, count=1, n=8, heads=16)
    for bad in (dict(qkv=0), dict(out=0), dict(count=0), dict(n=0), dict(heads=0), dict(count=-3), dict(qkv=p + 4)) + \
            ((dict(seg=0),) if seg else ()):
        a = dict(good, **bad)
        args = (a["qkv"], a["out"]) + ((a["seg"],) if seg else ()) + (a["count"], a["n"], a["heads"], 10.0, 0)
        rc = fn(*args)
        assert rc != 0, bad
        assert L.fh_last_error().decode().startswith(name + ":"), (bad, L.fh_last_error())


# ---- the pin constructions ---------------------------------------------------------------------------------------------------
def test_two_bit_values_split_as_designed():
    a = AP.two_bit_values(20000, 1)
    h, m, lo = AP.split3(a)
    assert torch.equal(h.double() + m.double() + lo.double(), a.double())
    for p, scale in ((h, 1.0), (m, 2.0 ** 9), (lo, 2.0 ** 18)):
        assert set((p.abs() * scale).unique().tolist()) == {1.0, 1.5}
    assert bool((m * h < 0).any()) and bool((lo * m < 0).any())                 # negative residuals are in
    th, tm, tl = AP.split3_trunc(a)
    assert torch.equal(th.double() + tm.double() + tl.double(), a.double())      # (a truncating split is exact too ...)
    assert 0.3 < float(((th != h) | (tm != m)).double().mean())                  # (... with other pieces)
    from flowhigh_amd import packing
    for x, y in zip(packing.split_pieces(a), (h, m, lo)):
        assert torch.equal(x.float(), y)


def _logit_gap(Lpair, scale=AP.SCALE):
    """what decides the output of qk_case: the fp32 difference of the two live keys' scaled logits, as the kernels form it"""
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(AP.C_LOG2E, dtype=torch.float32)
    s = Lpair.float() * c
    return s[..., 0] - s[..., 1]


@pytest.mark.parametrize("B,n", [(1, 200), (3, 130)])
def test_qk_case_logits_are_exact_and_every_mutant_moves_them(B, n):
    case = AP.qk_case(B, n, seed=5)
    L = case["L"]                                             # [B, H, n, 2]
    assert torch.equal(L.float().double(), L)
    bf = case["bf"].view(B, n, 3, AP.H, AP.DH)
    q, k = bf[:, :, 0], bf[:, :, 1]
    a = q.abs().amax(-1)                                      # the designed q value sits beside a 1: recover it per row
    live = case["live"]
    # the accumulation in the kernel's order, one fp32 rounding per MFMA, reaches the same number: every partial sum is exact
    for b in range(B):
        for h in range(AP.H):
            qrow = q[b, :, h]
            d0 = int((k[b, int(live[b, h, 0]), h] != 0).nonzero()[0])
            av = qrow[:, d0]
            for j in range(2):
                bv = k[b, int(live[b, h, j]), h, d0].expand(n)
                assert torch.equal(AP.emulate_pv(av, bv).double(), L[b, h, :, j])       # (same schedule: (K piece, Q piece))
                for drop in AP.KEPT:
                    assert not torch.equal(AP.six(AP.split3(bv), AP.split3(av), drop), L[b, h, :, j])
            gap = _logit_gap(L[b, h])
            bs = [k[b, int(live[b, h, j]), h, d0].expand(n) for j in range(2)]
            for drop in AP.KEPT:                              # a lost pair: >= 2^-18 of a logit, never the same on both keys
                Lm = torch.stack([AP.six(AP.split3(bj), AP.split3(av), drop) for bj in bs], -1)
                assert float((_logit_gap(Lm) != gap).double().mean()) > 0.99, drop
            # l = 0 loses (l h) and (h l) together: where a_l b_h = -a_h b_l they cancel on a row, on a quarter of the rows
            Lm = torch.stack([AP.six(AP.split3_l0(bj), AP.split3_l0(av)) for bj in bs], -1)
            assert float((_logit_gap(Lm) != gap).double().mean()) > 0.5
    # dead keys: exp2 of their logit is exactly 0 whatever the row maximum
    assert AP.DEAD * AP.SCALE * AP.C_LOG2E + 3.0 * AP.SCALE * AP.C_LOG2E < -800
    assert float(L.abs().max()) <= 2.3
    # the fp32 kernel's input carries the logits themselves
    f32 = case["f32"].view(B, n, 3, AP.H, AP.DH)
    for b in range(B):
        for h in range(AP.H):
            for j in range(2):
                kj = f32[b, int(live[b, h, j]), 1, h]
                assert kj.abs().sum() == 1.0
                assert torch.equal((f32[b, :, 0, h] * kj).sum(-1).double(), L[b, h, :, j])
    assert torch.equal(case["bf"].view(B, n, 3, -1)[:, :, 2], case["f32"].view(B, n, 3, -1)[:, :, 2])      # same V
    assert a.min() >= 1.0 - 2.0 ** -8


def test_qk_case_truncating_split_moves_some_logits():
    """A truncating split is exact as well (h + m + l = x), its pieces are up to twice as large, so the three dropped pairs are:
    the logits move by about one fp32 ulp, on part of the rows."""
    a, b = AP.two_bit_values(20000, 7), AP.two_bit_values(20000, 8, signed=False)
    good = AP.six(AP.split3(b), AP.split3(a))
    t = AP.six(AP.split3_trunc(b), AP.split3_trunc(a)).float().double()
    assert 0.05 < float((t != good).double().mean())


def test_v_case_pins_the_three_v_pieces_against_p_h():
    from test_hip_bf16x6_pairs import designed_values
    v = designed_values(2 * AP.H * AP.DH, 3)[0].view(2, AP.H, AP.DH)
    qkv, exp = AP.v_case(2, 128, 0, v)
    x = qkv.view(2, 128, 3, AP.H, AP.DH)
    assert not x[:, :, :2].any() and torch.equal((x[:, :, 2] != 0).sum(1), torch.ones(2, AP.H, AP.DH, dtype=torch.long))
    assert torch.equal(x[:, :, 2].sum(1), v)
    one = torch.ones_like(v)
    assert torch.equal(AP.split3(one)[0], one) and not AP.split3(one)[1].any() and not AP.split3(one)[2].any()
    assert torch.equal(AP.emulate_pv(one, v), v)
    for drop in ((0, 0), (1, 0), (2, 0)):
        assert bool((AP.emulate_pv(one, v, drop) != v).all()), drop
    assert bool((AP.emulate_pv(one, v, split=AP.split3_l0) != v).all())


def test_p_case_pins_the_three_p_pieces_against_v_h():
    qkv, logits, key_of, vpow = AP.p_case(1, 96, 11)
    x = qkv.view(96, 3, AP.H, AP.DH)
    for t in (x[:, 0], x[:, 1]):                                   # one bf16 piece each
        h, m, lo = AP.split3(t)
        assert torch.equal(h, t) and not m.any() and not lo.any()
    assert torch.equal((logits * 16).round(), logits * 16) and float(logits.abs().max()) <= 2.0
    assert float(logits.std()) > 0.05                              # general P, not a flat softmax
    g = torch.Generator().manual_seed(1)
    p = torch.rand(50000, generator=g).float() * torch.exp2(-torch.randint(0, 20, (50000,), generator=g).float())
    v = torch.pow(2.0, torch.randint(-3, 4, (50000,), generator=g).float())
    assert torch.equal(AP.emulate_pv(p, v).double(), p.double() * v.double())
    assert torch.equal(AP.emulate_pv(p, v, split=AP.split3_trunc).double(), p.double() * v.double())
    for drop in ((0, 1), (0, 2)):           # (torch.rand draws multiples of 2^-24: some small p have no l piece)
        assert float((AP.emulate_pv(p, v, drop).double() != p.double() * v.double()).double().mean()) > 0.8, drop
    assert float((AP.emulate_pv(p, v, split=AP.split3_l0).double() != p.double() * v.double()).double().mean()) > 0.8


def _vm_pm_row(p, e, drop=None):
    """the kernel's row for vm_pm_case with second-key probability p: (column 0, column 1) in fp32"""
    f32 = lambda t: t.float()
    ell = f32(1.0 + p.double())                                                  # l = 1 + p, one rounding
    inv = f32(1.0 / ell.double())
    v0 = torch.full_like(p, 2.0 ** e * AP.VM_FACTOR)
    v1 = torch.full_like(p, 2.0 ** e)
    c0 = f32(AP.emulate_pv(p, v0, drop).double() * inv.double())
    c1 = f32(AP.emulate_pv(p, v1, drop).double() * inv.double())
    return c0, c1


def test_vm_pm_case_bound_holds_for_the_six_pairs_and_fails_without_m_m():
    h, m, lo = AP.split3(torch.tensor([AP.VM_FACTOR * 4.0]))
    assert (float(h), float(m), float(lo)) == (4.0, 4.0 * (2.0 ** -8 - 2.0 ** -16), 0.0)
    g = torch.Generator().manual_seed(2)
    p = (0.05 + 0.9 * torch.rand(100000, generator=g)).float()
    for e in (-3, 0, 3):
        c0, c1 = _vm_pm_row(p, e)
        miss = (c0.double() - AP.VM_FACTOR * c1.double()).abs() / AP.ulp(c0.double())
        assert float(miss.max()) <= AP.VM_PM_ULPS
        c0, c1 = _vm_pm_row(p, e, drop=(1, 1))
        miss = (c0.double() - AP.VM_FACTOR * c1.double()).abs() / AP.ulp(c0.double())
        assert float((miss > AP.VM_PM_ULPS).double().mean()) > 0.9
    qkv, exps = AP.vm_pm_case(1, 70, 3)
    x = qkv.view(70, 3, AP.H, AP.DH)
    logit = torch.einsum("ihd,jhd->hij", x[:, 0].double(), x[:, 1].double())
    live = logit > AP.DEAD / 2
    assert torch.equal(live.sum(-1), torch.full((AP.H, 70), 2))
    gap = torch.where(live, logit, torch.zeros_like(logit)).amin(-1)                 # the second key's logit, the first's is 0
    p2 = torch.exp(gap * AP.SCALE) / (1 + torch.exp(gap * AP.SCALE)) * 2            # ~ p of the second key relative to the row maximum
    assert float(gap.max()) < 0 and 0.04 < float(torch.exp(gap * AP.SCALE).min()) and float(torch.exp(gap * AP.SCALE).max()) < 0.96
    assert p2.isfinite().all()
