"""GPU: the four full attention entries (fh_attention_f32, fh_attention_bf16x6_f32 and their _seg_ forms) value by value at their
edges -- the 32-key tile, the stream pair (64), the query blocks (64 and 128), a stream with no key, a last block with one live
query -- against exact expectations and float64, in both kernel shapes: alone (SPLIT = 2) and as the last clip of the smallest
batch across the launch threshold (SPLIT = 1) whose other clips are NaN.  out always sits between 128 sentinel rows.

The constructions, the references and the assertions themselves are tests/tools/attn_edges.py's; tests/test_attn_edges_cpu.py
runs the same assertions on an fp32 host restatement of the kernels' frame and on its ten mutants (each fails one).  No bar here
is taken from a kernel's output: a check is exact (uniform rows at rtol 1e-6 of a closed form, gather and the invariances bit for
bit) or 3 x the error of plain fp32 torch attention on the same tensor, with a floor of 8 ulps of max |V|.  The measured ratios:
profiles/attention_edges.md."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import attn_edges as AE                                  # noqa: E402
from flowhigh_amd import hip                             # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORMS = ["f32", "bf16x6"]
ENTRY = {"f32": ("fh_attention_f32", "fh_attention_seg_f32"), "bf16x6": ("fh_attention_bf16x6_f32", "fh_attention_bf16x6_seg_f32")}


class HipRunner:
    device = DEV

    def __init__(self, form):
        self.name, self.seg_name = ENTRY[form]

    def batched(self, qkv, out, row_off, B, n, heads, scale):
        assert qkv.is_contiguous() and out.is_contiguous() and tuple(qkv.shape) == (B * n, 3 * heads * AE.DH)
        assert out.shape[0] >= row_off + B * n and out.shape[1] == heads * AE.DH
        hip.check(getattr(hip.lib(), self.name)(qkv.data_ptr(), out[row_off:].data_ptr(), B, n, heads, scale, hip.stream()), self.name)
        torch.cuda.synchronize()

    def seg(self, qkv, out, clips, max_n, heads, scale):
        assert qkv.is_contiguous() and out.is_contiguous() and qkv.shape[0] == out.shape[0]
        assert all(0 <= r0 and r0 + n <= qkv.shape[0] and 0 <= n <= max_n for r0, n in clips)
        seg = torch.tensor(clips, dtype=torch.int32).to(DEV)
        hip.check(getattr(hip.lib(), self.seg_name)(qkv.data_ptr(), out.data_ptr(), seg.data_ptr(), len(clips), max_n, heads, scale,
                                                    hip.stream()), self.seg_name)
        torch.cuda.synchronize()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("heads", AE.HEADS)
@pytest.mark.parametrize("c", AE.UNIFORM_C)
@pytest.mark.parametrize("n", AE.N_EDGES)
def test_uniform_rows(n, c, heads, form):
    """Every logit is c scale (c = 0, +64, -64: base-2 logits 0 and +-923), V[j] = j + 1: each row is fl(fl(sum) fl(1 / n)), sums
    of integers below 2^24 (exact in fp32 and in three bf16 pieces).  A key too many or too few moves a row by about 0.5."""
    AE.check_uniform(HipRunner(form), n, heads, c)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("heads", AE.HEADS)
@pytest.mark.parametrize("n", AE.N_EDGES)
def test_gather_is_exact(n, heads, form):
    """q_i = k_pi(i) with every other key >= 200 base-2 logits below: p is exactly one-hot, out[i] == V[pi(i)] bit for bit (n = 1:
    out == V[0]).  The fp32 kernel has p = 1, l = 1, corr = 0 or 1; the bf16x6 kernel's three V pieces against P.h = 1 sum exactly."""
    AE.check_gather(HipRunner(form), n, heads)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", AE.N_F64)
@pytest.mark.parametrize("name,heads", [(b, 16) for b in AE.F64_BUILDERS] + [("soft", 3)])
def test_against_float64(name, heads, n, form):
    """max and RMS of (kernel - float64 attention) <= max(3 x the same of (plain fp32 torch attention - float64), 8 ulps of
    max |V|), both on the tensor the kernel reads.  ramp: a maximum that arrives late in half the rows of every wave and first in
    the other half; offset: soft logits on +-600 nats; model_like; soft (where the yardstick's noise is about 1e-6)."""
    AE.check_float64(HipRunner(form), name, n, heads, label=form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("repeat", [1, 2])
def test_segment_form_at_the_edges(repeat, form):
    """One _seg_ launch over clips of 65, 1, 0, 128, 33, 257 and 64 rows packed with gaps (NaN in qkv, sentinels in out): every
    clip equals its lone batched call bit for bit and is finite, the zero-row clip writes nothing, every other row of out keeps
    its sentinel.  repeat = 1: the small grid (SPLIT = 2); repeat = 2: 14 clips, across the threshold (SPLIT = 1)."""
    AE.check_segment(HipRunner(form), 16, repeat)


@pytest.mark.parametrize("form", FORMS)
def test_argument_errors_write_nothing(form):
    L = hip.lib()
    name, seg_name = ENTRY[form]
    qkv = torch.zeros(4, 3 * 64, device=DEV)
    out = AE.sentinel(4, 64, DEV)
    seg = torch.tensor([[0, 4]], dtype=torch.int32).to(DEV)
    q, o, s, st = qkv.data_ptr(), out.data_ptr(), seg.data_ptr(), hip.stream()
    bad = [(name, (q, o, 1, 0, 1, 1.0, st)), (name, (q, o, 0, 4, 1, 1.0, st)), (name, (q, o, 1, 4, 0, 1.0, st)),
           (name, (None, o, 1, 4, 1, 1.0, st)), (name, (q, None, 1, 4, 1, 1.0, st)),
           (seg_name, (q, o, s, 1, 0, 1, 1.0, st)), (seg_name, (q, o, s, 0, 4, 1, 1.0, st)), (seg_name, (q, o, s, 1, 4, 0, 1.0, st)),
           (seg_name, (None, o, s, 1, 4, 1, 1.0, st)), (seg_name, (q, None, s, 1, 4, 1, 1.0, st)), (seg_name, (q, o, None, 1, 4, 1, 1.0, st))]
    for entry, args in bad:
        rc = getattr(L, entry)(*args)
        assert rc != 0, f"{entry}{args[2:-1]}"
        assert L.fh_last_error().decode().startswith(entry + ":"), L.fh_last_error().decode()
        with pytest.raises(hip.HipError):
            hip.check(rc, entry)
    torch.cuda.synchronize()
    assert AE.is_sentinel(out)
    # (and the same buffers are a valid call)
    hip.check(getattr(L, name)(q, o, 1, 4, 1, 1.0, st), name)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
