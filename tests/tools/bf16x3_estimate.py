"""`python tests/tools/bf16x3_estimate.py [configuration ...] [--frames=N] [--seed=S]`: what conv_form='direct_bf16x3' costs in accuracy,
estimated on the CPU before any kernel runs.

The oracle's BigVGAN (oracle/ref_cpu.bigvgan_forward) is run in float64 with F.conv1d / F.conv_transpose1d wrapped: every unit-group
conv with at least 16 input channels has its input and weight rounded to fp32 and then evaluated in one of the forms below;
everything else (the activations' depthwise filters, snake, tanh, sums) stays float64.  The input is a random mel of `frames` frames;
the figures are the distances of the waveform to the all-float64 run.

  bf16x3   two pieces per operand, the three pairs h h, h m, m h summed in float64 (tests/ref_bf16x3.conv_bf16x3_ref's arithmetic)
  fp32     the conv in fp32 (torch's CPU kernels)
  bf16     one piece per operand: plain bf16 products

A configuration is the name of a golden (tests/golden/<name>.npz: its vocoder JSON and seed) or of a constant of flowhigh_amd.synth
(SYNTH_CFG, TINY_CFG, ALT_CFG, ...).  Without names: every golden and SYNTH_CFG, as a markdown table."""
import contextlib
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from flowhigh_amd import synth                       # noqa: E402
from flowhigh_amd.packing import split_pieces       # noqa: E402
from oracle import ref_cpu                           # noqa: E402
from ref_bf16x3 import PAIRS                         # noqa: E402

MODES = ("bf16x3", "fp32", "bf16")
MIN_CIN = 16


def _emulated(fn, mode):
    def conv(x, w, bias=None, *args, **kw):
        if kw.get("groups", 1) != 1 or x.shape[1] < MIN_CIN:
            return fn(x, w, bias, *args, **kw)
        x32, w32 = x.float(), w.float()
        if mode == "fp32":
            return fn(x32, w32, None if bias is None else bias.float(), *args, **kw).double()
        xs, ws = ([p.double() for p in split_pieces(t)] for t in (x32, w32))
        pairs = PAIRS if mode == "bf16x3" else ((0, 0),)
        y = sum(fn(xs[i], ws[j], None, *args, **kw) for i, j in pairs)
        return y if bias is None else y + bias.double().view(1, -1, 1)
    return conv


@contextlib.contextmanager
def conv_mode(mode):
    """Inside: the oracle's convs run in `mode` (None: untouched)."""
    saved = F.conv1d, F.conv_transpose1d
    if mode is not None:
        F.conv1d, F.conv_transpose1d = _emulated(saved[0], mode), _emulated(saved[1], mode)
    try:
        yield
    finally:
        F.conv1d, F.conv_transpose1d = saved


def resolve(name):
    """-> (vocoder JSON dict, seed of the synthetic weights)."""
    if hasattr(synth, name):
        return getattr(synth, name), 0
    sys.path.insert(0, str(ROOT / "tests"))
    from conftest import load_golden
    g = load_golden(name)
    return g["cfg"], g["seed"]


def estimate(name, frames=20, seed=0, modes=("bf16x3",)):
    """{mode: (max abs, rms)} of the vocoder's waveform against its float64 run, configuration `name`, a random mel of `frames` frames."""
    cfg, wseed = resolve(name) if isinstance(name, str) else (name, 0)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in synth.make_vocoder_state_dict(cfg, wseed).items()}
    mel = (torch.randn(1, int(cfg["num_mels"]), frames, generator=torch.Generator().manual_seed(seed)) * 2.0 - 3.0).double()
    ref = ref_cpu.bigvgan_forward(sd, cfg, mel)
    out = {}
    for mode in modes:
        with conv_mode(mode):
            got = ref_cpu.bigvgan_forward(sd, cfg, mel)
        d = got - ref
        out[mode] = (d.abs().max().item(), d.pow(2).mean().sqrt().item())
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    frames, seed = int(opt.get("frames", 20)), int(opt.get("seed", 0))
    if not args:
        from conftest import E2E_CASES
        args = list(E2E_CASES) + ["SYNTH_CFG"]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    print(f"| configuration | {' | '.join(f'{m} max abs | {m} rms' for m in MODES)} |")
    print("|---|" + "---|" * (2 * len(MODES)))
    for name in args:
        r = estimate(name, frames, seed, MODES)
        print(f"| {name} | " + " | ".join(f"{r[m][0]:.2e} | {r[m][1]:.2e}" for m in MODES) + " |", flush=True)
