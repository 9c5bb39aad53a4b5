"""attn_window (banded attention: frame i attends to the frames j of its clip with |i - j| <= W), the parts that need no GPU: the
keyword's resolution and its way through the constructors, the four banded C entries' presence, signatures and argument errors,
and which entry pair a FlowNet holds."""
import ctypes
import inspect
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from flowhigh_amd import hip, planner                   # noqa: E402

FULL = ("fh_attention_f32", "fh_attention_seg_f32", "fh_attention_bf16x6_f32", "fh_attention_bf16x6_seg_f32")
BAND = ("fh_attention_band_f32", "fh_attention_band_seg_f32", "fh_attention_bf16x6_band_f32", "fh_attention_bf16x6_band_seg_f32")


# ---- keyword ----------------------------------------------------------------------------------------------------------------
def test_resolve_attn_window():
    assert planner.resolve_attn_window() is None and planner.resolve_attn_window(None) is None
    for w in (0, 1, 500, 2 ** 31 - 1, 2 ** 40):
        got = planner.resolve_attn_window(w)
        assert got == w and type(got) is int
    for w in (np.int32(7), np.int64(7), np.uint8(7)):
        got = planner.resolve_attn_window(w)
        assert got == 7 and type(got) is int
    for bad in (-1, -500, np.int64(-3), True, False, 1.0, 500.0, np.float32(4), "500", "", (5,), [5]):
        with pytest.raises(ValueError, match="attn_window"):
            planner.resolve_attn_window(bad)


def test_attn_window_has_no_environment_switch(monkeypatch):
    for name in ("FH_ATTN_WINDOW", "FH_ATTENTION_WINDOW", "FH_ATTN_BAND"):
        monkeypatch.setenv(name, "7")
    assert planner.resolve_attn_window() is None
    src = "".join(p.read_text() for p in (ROOT / "flowhigh_amd").glob("*.py"))
    assert "FH_ATTN" not in src


def test_defaults_are_full_attention_and_the_property_is_read_only():
    from flowhigh_amd import FLowHigh, FlowHighSR
    from flowhigh_amd.flow import FlowNet
    for fn in (FLowHigh.__init__, FlowHighSR.from_local.__func__, FlowHighSR.from_pretrained.__func__, FlowNet.__init__):
        assert inspect.signature(fn).parameters["attn_window"].default is None
    assert isinstance(FLowHigh.attn_window, property) and FLowHigh.attn_window.fset is None
    for fn in (FLowHigh.__init__, FlowHighSR.from_local.__func__):
        assert "10 ms" in (inspect.getsource(fn))                 # the unit is said where the keyword is taken


def test_public_constructors_refuse_a_wrong_attn_window_before_loading_anything(tmp_path):
    from flowhigh_amd import FLowHigh, FlowHighSR
    with pytest.raises(ValueError, match="attn_window"):
        FlowHighSR.from_local(tmp_path / "no_such_dir", attn_window=-1)
    with pytest.raises(ValueError, match="attn_window"):
        FlowHighSR.from_local(tmp_path / "no_such_dir", attn_window=2.5)
    with pytest.raises(ValueError, match="attn_window"):
        FLowHigh(None, {}, "cuda", attn_window=True)
    with pytest.raises(ValueError, match="attn_window"):
        FlowHighSR.from_pretrained(attn_window="500")          # (before huggingface_hub is imported or asked)


@pytest.mark.parametrize("form", ["f32", "bf16x6"])
def test_flownet_holds_the_full_pair_and_the_banded_pair(form):
    from flowhigh_amd import synth
    from flowhigh_amd.flow import FlowNet
    sd = synth.make_flow_state_dict(seed=0)
    full = {"f32": FULL[:2], "bf16x6": FULL[2:]}[form]
    band = {"f32": BAND[:2], "bf16x6": BAND[2:]}[form]
    net = FlowNet(sd, "cpu", attn_form=form, attn_window=None)
    assert net.attn_window is None and net._radius is None
    assert (net._attn, net._attn_seg) == full                  # what a model without the keyword calls: today's pair
    net = FlowNet(sd, "cpu", attn_form=form, attn_window=7)
    assert net.attn_window == 7 and net._radius == 7
    assert (net._attn, net._attn_seg) == full and (net._attn_band, net._attn_band_seg) == band
    assert FlowNet(sd, "cpu", attn_form=form, attn_window=2 ** 40)._radius == 2 ** 31 - 1        # (the entries take a C int)
    assert FlowNet(sd, "cpu", attn_form=form, attn_window=0)._radius == 0                        # (0 is a band, not "off")
    with pytest.raises(ValueError, match="attn_window"):
        FlowNet(sd, "cpu", attn_form=form, attn_window=-2)


def test_the_window_is_no_part_of_a_weight_blobs_format_tag():
    from flowhigh_amd import weights
    assert "window" not in inspect.getsource(weights.format_tag)
    assert "attn_window" not in inspect.signature(weights.format_tag).parameters


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_6_exports_the_four_banded_entries():
    assert hip.ABI_VERSION == 6 == hip.lib().fh_abi_version()
    assert set(BAND) <= set(hip.EXPORTS) and set(FULL) <= set(hip.EXPORTS)
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert "#define FH_ABI_VERSION 6" in header
    for name in BAND:
        assert f"int {name}(" in header
        assert hasattr(hip.lib(), name)
    assert "|i - j| <= radius" in header


@pytest.mark.parametrize("full,band", list(zip(FULL, BAND)))
def test_a_banded_signature_is_its_full_counterparts_plus_one_int(full, band):
    a, b = hip._SIGS[full], hip._SIGS[band]
    assert len(b) == len(a) + 1
    at = b.index(ctypes.c_float)                           # radius sits in front of scale
    assert b[at - 1] is ctypes.c_int and b[:at - 1] + b[at:] == a
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    decl = header[header.index(f"int {band}("):]
    decl = decl[:decl.index(";")]
    assert "int radius, float scale" in " ".join(decl.split())


@pytest.mark.parametrize("name", BAND)
def test_argument_errors_are_returned_with_the_entrys_name(name):
    L = hip.lib()
    fn = getattr(L, name)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p -= p % 16                    # (never dereferenced: every call below is refused before a launch)
    seg = name.endswith("_seg_f32")
    good = dict(qkv=p, out=p, seg=p, count=1, n=8, heads=16, radius=3)
    for bad in (dict(qkv=0), dict(out=0), dict(count=0), dict(n=0), dict(heads=0), dict(count=-3), dict(n=-1), dict(qkv=p + 4),
                dict(radius=-1), dict(radius=-2 ** 31)) + ((dict(seg=0),) if seg else ()):
        a = dict(good, **bad)
        args = (a["qkv"], a["out"]) + ((a["seg"],) if seg else ()) + (a["count"], a["n"], a["heads"], a["radius"], 10.0, 0)
        rc = fn(*args)
        assert rc != 0, bad
        assert L.fh_last_error().decode().startswith(name + ":"), (bad, L.fh_last_error())
