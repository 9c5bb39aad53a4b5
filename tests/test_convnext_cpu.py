"""CPU: the ConvNeXt vector field's host side -- the restatement (tests/ref_convnext.py) against the live reference, the
state-dict contract, architecture detection and its errors, the C ABI's three new entries, the gamma fold."""
import re
from pathlib import Path

import pytest
import torch

import ref_convnext as rc
from flowhigh_amd import FLowHigh, FlowHighSR, convnext, flowhighsr, hip, synth
from oracle import ref_shim

ROOT = Path(__file__).resolve().parents[1]
FH, VOC = "flowhigh.", "flowhigh.audio_enc_dec.vocoder."
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")


@pytest.fixture(scope="module")
def flow_sd():
    return synth.make_convnext_state_dict(5)


PIN_SHAPES = [(2, 9), (1, 40)]
PIN_T = 0.37


def pin_inputs(batch, n):
    g = torch.Generator().manual_seed(100 * batch + n)
    return torch.randn(batch, n, 256, generator=g), torch.randn(batch, n, 256, generator=g) * 2.0 - 3.0


_REF_CHILD = """
import json, sys
import numpy as np
import torch
sys.path[:0] = [{root!r}, {tests!r}]
from flowhigh_amd import synth
from oracle import ref_shim
from test_convnext_cpu import FH, PIN_SHAPES, PIN_T, pin_inputs
ref_shim.load_reference()
from flowhigh.models.flow import FLowHigh
m = FLowHigh(dim_in=256, depth=2, architecture="convnext").eval()
sd = synth.make_convnext_state_dict(5)
m.load_state_dict({{k[len(FH):]: v for k, v in sd.items()}}, strict=True)          # pins the key names and shapes
out = dict(keys=json.dumps(sorted(m.state_dict())))
with torch.no_grad():
    for batch, n in PIN_SHAPES:
        x, cond = pin_inputs(batch, n)
        out[f"v_{{batch}}_{{n}}"] = m(x, times=torch.tensor(PIN_T), cond=cond, cond_drop_prob=0.).numpy()
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def ref_run(tmp_path_factory):
    """The reference's own FLowHigh(dim_in=256, depth=2, architecture='convnext') under the oracle's import stand-ins, the
    synthetic tensors loaded with strict=True, run on the pin inputs.  In a child process: the stand-ins replace torch.load,
    Tensor.cuda and six third-party modules for the whole interpreter."""
    import subprocess
    import sys
    import numpy as np
    out = str(tmp_path_factory.mktemp("convnext_pin") / "ref.npz")
    code = _REF_CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), out=out)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(out, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@needs_reference
@pytest.mark.parametrize("batch,n", PIN_SHAPES)
def test_restatement_equals_live_reference(ref_run, flow_sd, batch, n):
    x, cond = pin_inputs(batch, n)
    ref = torch.from_numpy(ref_run[f"v_{batch}_{n}"])
    with torch.no_grad():
        got = rc.convnext_forward(flow_sd, x, cond, PIN_T)
    err = (got - ref).abs().max().item()
    print(f"restatement vs reference at (B, n) = ({batch}, {n}): {err:.3e}")
    assert got.shape == ref.shape and err <= 2e-6          # the bar of test_reference_pin.py


@needs_reference
def test_expected_keys_equal_the_reference_modules(ref_run):
    import json
    want = {k for k in flowhighsr.expected_state_keys(synth.TINY_CFG, architecture="convnext") if not k.startswith(VOC)}
    assert want == {FH + k for k in json.loads(str(ref_run["keys"]))}


def test_expected_keys_and_synthetic_checkpoint_agree(flow_sd):
    cfg = synth.TINY_CFG
    sd = dict(flow_sd, **synth.make_vocoder_state_dict(cfg, 5))
    assert set(flowhighsr.expected_state_keys(cfg, architecture="convnext")) == set(sd)
    flowhighsr.check_state_dict_keys(sd, cfg, architecture="convnext")
    assert not any(k.startswith(FH + "transformer.") for k in sd)
    assert flow_sd[FH + "convnext.7.dwconv.weight"].shape == (1024, 1, 7) and flow_sd[FH + "convnext.0.pwconv1.weight"].shape == (3072, 1024)
    assert float(flow_sd[FH + "convnext.0.norm.scale.weight"].abs().max()) > 0          # the time path reaches the output
    gam = flow_sd[FH + "convnext.3.gamma"]
    assert gam.shape == (1024,) and 0.5 <= float(gam.min()) and float(gam.max()) <= 1.5
    # every existing call keeps its result: the defaults are the transformer's
    tsd = synth.make_state_dict(cfg, 0)
    assert set(flowhighsr.expected_state_keys(cfg)) == set(flowhighsr.expected_state_keys(cfg, 2, "transformer")) == set(tsd)
    flowhighsr.check_state_dict_keys(tsd, cfg)
    with pytest.raises(RuntimeError, match="Unexpected key"):          # what a convnext checkpoint met before this keyword
        flowhighsr.check_state_dict_keys(sd, cfg)


def test_detection_contradiction_and_keyword_errors(flow_sd):
    cfg = synth.TINY_CFG
    sd = dict(flow_sd, **synth.make_vocoder_state_dict(cfg, 5))
    tsd = synth.make_state_dict(cfg, 0)
    assert flowhighsr.detect_architecture(sd) == "convnext" and flowhighsr.detect_architecture(tsd) == "transformer"
    assert flowhighsr.resolve_architecture(None, sd) == "convnext" and flowhighsr.resolve_architecture(None) == "transformer"
    assert convnext.n_blocks(sd) == 8 and convnext.is_convnext_state_dict(sd) and not convnext.is_convnext_state_dict(tsd)
    # a named architecture the keys contradict: the strict-load error, before any device is touched
    with pytest.raises(RuntimeError, match=r"Error\(s\) in loading state_dict"):
        FLowHigh(sd, cfg, "cpu", architecture="transformer")
    with pytest.raises(RuntimeError, match=r"Missing key\(s\).*convnext\.0\.dwconv"):
        FLowHigh(tsd, cfg, "cpu", architecture="convnext")
    with pytest.raises(ValueError, match="architecture"):
        FLowHigh(sd, cfg, "cpu", architecture="resnet")
    # attention keywords with a backbone that has no attention
    for kw in (dict(attn_window=500), dict(attn_form="bf16x6"), dict(attn_window=0)):
        with pytest.raises(ValueError, match="convnext"):
            FLowHigh(sd, cfg, "cpu", **kw)
        with pytest.raises(ValueError, match="convnext"):
            FlowHighSR.from_local("/nonexistent", architecture="convnext", **kw)
    # detected or named consistently, the constructor gets as far as the device check (there is no CPU path)
    for arch in (None, "convnext"):
        with pytest.raises(hip.HipError):
            FLowHigh(sd, cfg, "cpu", architecture=arch)
    with pytest.raises(hip.HipError):
        FLowHigh(tsd, cfg, "cpu", architecture="transformer")
    with pytest.raises(ValueError, match="state dict"):
        FLowHigh(None, cfg, "cpu", architecture="convnext", store=object())


def test_checkpoint_files_are_read_and_convert_declines(tmp_path, flow_sd):
    """from_local's reader takes a convnext checkpoint (detected, or named); the weight-blob converter says that blobs are made
    for the transformer backbone only, and its command exits non-zero."""
    import subprocess
    import sys
    cfg = synth.TINY_CFG
    tsd = synth.write_checkpoint_dir(tmp_path, cfg, seed=5)
    model = dict({k: v for k, v in tsd.items() if k.startswith(VOC)}, **flow_sd)
    torch.save({"model": model}, tmp_path / "FLowHigh_basic_400k.pt")
    sd, got_cfg = flowhighsr.read_checkpoints(tmp_path)
    assert got_cfg == cfg and set(sd) == set(model) and flowhighsr.detect_architecture(sd) == "convnext"
    flowhighsr.read_checkpoints(tmp_path, "convnext")
    with pytest.raises(RuntimeError, match="Missing key"):
        flowhighsr.read_checkpoints(tmp_path, "transformer")
    from flowhigh_amd import convert, weights
    with pytest.raises(NotImplementedError, match="transformer backbone only"):
        convert.convert(tmp_path)
    r = subprocess.run([sys.executable, "-m", "flowhigh_amd.convert", str(tmp_path)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "transformer backbone only" in r.stderr and not (tmp_path / weights.BLOB_NAME).exists()


def test_header_exports_and_abi_are_consistent():
    header = (ROOT / "include" / "flowhigh_hip.h").read_text()
    assert re.search(r"#define FH_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    for name in ("fh_dwconv_ln_f32", "fh_dwconv_ln_seg_f32", "fh_gelu_f32"):
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/flowhigh_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert name in hip.EXPORTS and len(hip._SIGS[name]) == len(params), name
        for p, ctype in zip(params, hip._SIGS[name]):          # pointer / int / float / long long, in the header's order
            kind = hip._P if "*" in p else hip._F if p.startswith("float") else hip.C.c_longlong if p.startswith("long long") else hip._I
            assert ctype is kind, (name, p)
    assert "convnext.hip" in __import__("flowhigh_amd.build", fromlist=["SOURCES"]).SOURCES


def test_library_exports_the_entries_and_checks_their_arguments():
    """The argument checks run on the host before anything is launched, so they can be called without a GPU."""
    from flowhigh_amd import build
    build.build(verbose=False)
    L = hip.lib()
    ok = (256, 0, 0, 256, 256, 256)           # x, w (none), bias, scale, shift, y: fake aligned pointers, never dereferenced here
    assert L.fh_dwconv_ln_f32(*ok, 1, 4, 200, 7, 1e-6, 0) == -1 and b"dim 200" in L.fh_last_error()
    assert L.fh_dwconv_ln_f32(256, 256, 256, 256, 256, 256, 1, 4, 256, 4, 1e-6, 0) == -1 and b"ksz 4" in L.fh_last_error()
    assert L.fh_dwconv_ln_f32(256, 256, 256, 256, 256, 256, 1, 4, 256, 9, 1e-6, 0) == -1 and b"ksz 9" in L.fh_last_error()
    assert L.fh_dwconv_ln_f32(*ok, 1, 0, 256, 7, 1e-6, 0) == -1
    assert L.fh_dwconv_ln_f32(260, 0, 0, 256, 256, 256, 1, 4, 256, 7, 1e-6, 0) == -1 and b"aligned" in L.fh_last_error()
    assert L.fh_dwconv_ln_seg_f32(*ok, 0, 1, 4, 256, 7, 1e-6, 0) == -1          # no segment table
    assert L.fh_dwconv_ln_seg_f32(*ok, 256, 1, 4, 200, 7, 1e-6, 0) == -1 and b"fh_dwconv_ln_seg_f32" in L.fh_last_error()
    assert L.fh_gelu_f32(256, 256, 0, 0) == -1 and L.fh_gelu_f32(0, 256, 4, 0) == -1


def test_gamma_fold_in_float64_is_the_unfolded_product():
    g = torch.Generator().manual_seed(3)
    w2, b2 = torch.randn(256, 768, generator=g) / 28.0, torch.randn(256, generator=g)
    gamma = torch.rand(256, generator=g) + 0.5
    h = torch.randn(5, 768, generator=g, dtype=torch.float64)
    w64, b64 = convnext.fold_gamma64(w2, b2, gamma)
    assert w64.dtype == torch.float64 and b64.dtype == torch.float64
    unfolded = gamma.double() * (h @ w2.double().T + b2.double())
    folded = h @ w64.T + b64
    assert ((folded - unfolded).abs() / unfolded.abs().clamp_min(1.0)).max().item() <= 1e-12
    w32, b32 = convnext.fold_gamma(w2, b2, gamma)                    # rounded once
    assert torch.equal(w32, w64.float()) and torch.equal(b32, b64.float()) and w32.dtype == torch.float32


def test_restatement_in_float32_stays_close_to_float64(flow_sd):
    g = torch.Generator().manual_seed(9)
    x, cond = torch.randn(1, 12, 256, generator=g), torch.randn(1, 12, 256, generator=g) * 2.0 - 3.0
    with torch.no_grad():
        a = rc.convnext_forward(flow_sd, x, cond, 0.5)
        b = rc.convnext_forward(rc.cast(flow_sd, torch.float64), x.double(), cond.double(), 0.5)
        other_t = rc.convnext_forward(flow_sd, x, cond, 0.1)
    assert (a.double() - b).abs().max().item() < 1e-4
    assert (a - other_t).abs().max().item() > 1e-2            # the time embedding reaches the output
