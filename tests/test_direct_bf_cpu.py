"""conv_form='direct_bf16x6' on the host (no GPU): the weight packer of the bf16 x 6 direct kernel (conv_mfma_bf.hip), the form's
name through the resolver and the blob tag, and the launch plan -- the plan of 'direct' with every 16-channel-chunk conv launch on
the new entry, the narrow stages on narrow_bf.hip and only the phase-fused transposed convs left on fp32 MFMA."""
import pytest
import torch

from flowhigh_amd import hip, packing, planner, synth, weights
from flowhigh_amd.vocoder import Vocoder

FORM = "direct_bf16x6"
FAMILIES = {"direct_bf16x6", "narrow_bf16x6", "direct"}


def _voc(cfgname, form):
    cfg = getattr(synth, cfgname)
    return Vocoder(cfg, synth.make_vocoder_state_dict(cfg, 1), "cpu", conv_form=form)


@pytest.mark.parametrize("co,ci,k", [(24, 16, 7), (200, 48, 11), (768, 32, 3)])
def test_pack_conv_bf_weight(co, ci, k):
    g = torch.Generator().manual_seed(co + k)
    w = torch.randn(co, ci, k, generator=g) * torch.exp2(torch.randint(-20, 21, (co, ci, k), generator=g).float())
    cpad = -(-co // 32) * 32 + 32                                  # at least 32 padded rows
    p = packing.pack_conv_bf_weight(w, cpad)
    assert p.dtype == torch.int16 and tuple(p.shape) == (ci // 16, k, cpad, 3, 16)
    from flowhigh_amd import vocoder
    assert vocoder.pack_conv_bf_weight is packing.pack_conv_bf_weight
    pieces = p.view(torch.bfloat16).double()
    ref = packing.pack_conv_weight(w, cpad, 16)
    assert torch.equal(pieces.sum(dim=-2), ref.double())            # h + m + l is the fp32 weight, exactly
    assert torch.equal(p, packing.split_bf3(ref))
    assert not bool(p[:, :, co:].any())                             # padded rows are zero
    wb = w.to(torch.bfloat16).float()                               # bf16-exact weights live in piece h alone
    pb = packing.pack_conv_bf_weight(wb, cpad)
    assert not bool(pb[..., 1:, :].any()) and torch.equal(pb[..., 0, :].view(torch.bfloat16).float(), packing.pack_conv_weight(wb, cpad, 16))
    with pytest.raises(ValueError):
        packing.pack_conv_bf_weight(torch.zeros(8, 24, 3), 32)


def test_form_name_resolves_and_auto_is_unchanged(monkeypatch):
    for k in ("FH_CONV_FORM", "FH_WINO", "FH_CONV_BF16X6"):
        monkeypatch.delenv(k, raising=False)
    assert FORM in planner.CONV_FORMS
    assert planner.resolve_conv_form(FORM) == (FORM, False)
    assert planner.resolve_conv_form("auto") == (planner.DEFAULT_CONV_FORM, True) and planner.DEFAULT_CONV_FORM == "bf16x6"
    assert planner.resolve_conv_form() == (planner.DEFAULT_CONV_FORM, True)
    monkeypatch.setenv("FH_CONV_FORM", FORM)
    assert planner.resolve_conv_form() == (FORM, False)
    assert planner.use_gemm_bf16x6() and planner.use_amp_bf16x6() and planner.use_direct_bf16x6() and not planner.use_bf16x6()
    assert not planner.use_wino(768, 1) and not planner.use_wino54(768)
    monkeypatch.delenv("FH_CONV_FORM")
    assert planner.use_gemm_bf16x6(FORM) and planner.use_amp_bf16x6(FORM) and not planner.use_direct_bf16x6("direct")
    assert not planner.use_gemm_bf16x6("direct") and not planner.use_amp(24, [3, 7, 11], [[1, 3, 5]] * 3, "direct")
    assert planner.use_amp(24, [3, 7, 11], [[1, 3, 5]] * 3, FORM) and not planner.use_amp(96, [3, 7, 11], [[1, 3, 5]] * 3, FORM)
    tags = {f: weights.format_tag(f) for f in ("winograd", "bf16x6", "direct", FORM)}
    assert len(set(tags.values())) == 4
    assert hip.ABI_VERSION == 6 and "fh_conv_grouped_bf16x6_f32" in hip.EXPORTS
    assert hip._SIGS["fh_conv_grouped_bf16x6_f32"] == hip._SIGS["fh_conv_grouped_f32"][:6] + [hip._P]      # no ck argument


def _conv_steps(p):
    """(step, family) of the conv-family launches of a plan, launch order."""
    steps = [s for s in p["steps"] if s.kind in ("conv", "convt", "wino", "amp")]
    assert len(steps) == len(p["conv_launches"])
    return list(zip(steps, [f for f, _, _ in p["conv_launches"]]))


def test_plan_is_the_direct_plan_on_the_new_entry():
    new, old = _voc("SYNTH_CFG", FORM), _voc("SYNTH_CFG", "direct")
    assert new.form == FORM and new.direct_bf and new.amp_direct and not new.bf
    pn, po = new.plan(1, 100), old.plan(1, 100)
    got, ref = _conv_steps(pn), _conv_steps(po)
    assert {f for _, f in got} == FAMILIES
    assert len(got) == len(ref) and [m[0] for m in pn["meta"]] == [m[0] for m in po["meta"]]          # the same launch positions
    flops = {f: sum(ex for ff, ex, _ in pn["conv_launches"] if ff == f) for f in FAMILIES}
    total = sum(flops.values())
    assert total == sum(ex for _, ex, _ in po["conv_launches"])
    for (s, fam), (r, rfam) in zip(got, ref):
        assert rfam == "direct"
        if s.kind == "amp":
            # narrow stages (<= 48 channels): narrow_bf.hip, whatever chunk the direct form walks them in
            assert fam == "narrow_bf16x6" and r.kind == "conv" and s.c <= 48 and s.flags & planner.AMP_DIRECT
            continue
        assert s.kind == r.kind and (s.cpad, s.tcfg, s.ng, s.n_len) == (r.cpad, r.tcfg, r.ng, r.n_len)
        if s.kind == "conv":
            assert fam == "direct_bf16x6" and s.bf == 1 and s.ck == 16 and r.bf == 0
        else:
            assert fam == "direct" and s.kind == "convt"
    # the fp32 entries keep the phase-fused transposed convs only: under 1 % of the plan's FLOPs
    assert [s.kind for s, f in got if f == "direct"] == ["convt"] * 3
    assert flops["direct"] <= 0.01 * total
    # every segment of a bf16 x 6 launch walks 16-channel chunks of three-piece weights (6 bytes per weight instead of 4)
    for s, (_, structs) in zip(pn["steps"], pn["meta"]):
        if s.kind == "conv":
            assert all(g.seg[i].cin % 16 == 0 for g in structs for i in range(g.nseg))
    assert new.pre_w.dtype == torch.int16 and tuple(new.pre_w.shape[-2:]) == (3, 16) and old.pre_w.dtype == torch.float32


def test_ragged_plan_carries_the_entry_choice():
    voc = _voc("TINY_CFG", FORM)
    rp = voc.plan_ragged([40, 25])
    rc = [s for s in rp["steps"] if s.kind == "rconv"]
    assert rc and all(s.bf == 1 and s.ck == 16 for s in rc)
    assert all(s.bf == 0 for s in _voc("TINY_CFG", "direct").plan_ragged([40, 25])["steps"] if s.kind == "rconv")


@pytest.mark.parametrize("cfgname", ["TINY_CFG", "ALT_CFG"])
def test_plan_builds_for_other_configurations(cfgname):
    p = _voc(cfgname, FORM).plan(1, 100)
    fams = {f for f, _, _ in p["conv_launches"]}
    assert fams <= FAMILIES and "direct_bf16x6" in fams
    for s in p["steps"]:
        if s.kind == "conv":
            assert s.bf == (s.ck == 16)                             # 8-channel chunks stay on the fp32 entry


def test_vocoder_refuses_a_store_of_another_form():
    cfg = synth.TINY_CFG
    sd = synth.make_vocoder_state_dict(cfg, 1)
    store = weights.WeightStore("cpu")
    store.form = "direct"
    with pytest.raises(ValueError, match="direct"):
        Vocoder(cfg, sd, "cpu", conv_form=FORM, store=store)
    with pytest.raises(ValueError):
        Vocoder(cfg, sd, "cpu", conv_form="direct_bf16")


def test_a_library_without_a_declared_symbol_is_refused_at_load(monkeypatch):
    """The entry is additive (the ABI version stays 6), so a library built before it has the right version and not the symbol: the
    load fails with a HipError that says to rebuild, not with an AttributeError at the first launch."""
    import ctypes as C
    real = C.CDLL(str(hip.LIB_PATH))

    class Older:
        def __getattr__(self, name):
            if name == "fh_conv_grouped_bf16x6_f32":
                raise AttributeError(name)
            return getattr(real, name)
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip.C, "CDLL", lambda path: Older())
    with pytest.raises(hip.HipError, match="fh_conv_grouped_bf16x6_f32.*rebuild"):
        hip.lib()
    assert hip._lib is None
    monkeypatch.undo()
    assert hip.lib().fh_abi_version() == 6
